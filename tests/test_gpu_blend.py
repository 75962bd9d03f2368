"""The bias-aware blend of the denoised and the raw frame on the GPU (rtpbr_denoise_blend, Renderer.denoise_blend).  Every comparison
is ``==`` on bit patterns against the CPU restatement (tests/post_ref/blend.h) fed with the GPU's own image_buffer, half A and
features; plus the buffer lifetime, state and error rules of include/rtpbr.h."""
import ctypes as C

import numpy as np
import pytest

import blend_ref_lib as bl
import checks as ck
import hostile as hz
import present_ref_lib as pr
from checks import EINVAL, ESTATE
from raytracingpbr_amd import Camera, Renderer
from raytracingpbr_amd.dataclass import BlendParams, NoiseStats
from raytracingpbr_amd.renderer import (BUF_BLEND_WEIGHT, BUF_DENOISED_ERROR, BUF_DENOISED_PIXELS, BUF_HALF_BUFFER, BUF_IMAGE_BUFFER,
                                        BUF_IMAGE_PIXELS, BUF_MOMENTS, BUF_NOISE, BUF_SELECTION)

pytestmark = pytest.mark.gpu

FRAMES = [(7, 5), (33, 17), (64, 48)]      # smaller than a tile and than the radius-3 window; partial tiles both ways; whole tiles
NEVER = 16777216                           # min_half_samples above every count: t = 1 everywhere


def _dealt(name, w, h, per_sample=False):
    """three unequal batches (2, 2, 3 spp: A, B, A), or the same 7 samples dealt one by one by the sample calls (4 + 3)"""
    scene, cfg = ck.scene(name, w, h)
    r = Renderer(scene, cfg)
    if per_sample:
        r.set_half_mode(per_sample=True)
    for n in (2, 2, 3):
        r.sample(n)
        if not per_sample:
            r.half_update()
    a = r.half_buffer[..., 3]
    assert np.all(a == (4 if per_sample else 5)) and np.all(r.image_buffer[..., 3] == 7)
    return cfg, r


def _want(r, cfg, radius, z, m, **denoise):
    return bl.denoise_blend(cfg, r.image_buffer, r.half_buffer, ck.feats(r), radius, z, m, **denoise)


def _check(r, cfg, radius=None, z=None, m=None, what="", **denoise):
    """one denoise_blend against the restatement: both buffers and the statistics; returns (denoised, weight, stats) of the restatement"""
    stats = r.denoise_blend(radius, z, m, **denoise)
    out, t, st = _want(r, cfg, radius, z, m, **denoise)
    what = f"{what} radius {radius} z {z} min_half_samples {m} {denoise}"
    ck.same(r.blend_weight, t, "blend_weight " + what)
    ck.same(r.denoised_pixels, out, "denoised_pixels " + what)
    assert (stats.pixels_estimated, stats.pixels_above) == st[:2], (what, stats, st)
    assert np.float32(stats.max_noise).view(np.uint32) == np.float32(st[2]).view(np.uint32), (what, stats, st)
    return out, t, st


def _varied(t, what):
    """the condition of a bit-identity case, on the restatement's weight: the kernel's blend branch and its t = 1 branch both run"""
    between = float(((t > 0) & (t < 1)).mean())
    assert between >= 0.05 and (t == 1).any(), f"{what}: {between:.1%} of the weights lie strictly between 0 and 1, {int((t == 1).sum())} are 1"


def _sweep(r, cfg, what):
    """radius 1..3, 0 and 4 levels, with and without demodulation; min_half_samples = 1 and z = 0 so that the weight varies.
    With no level the filter is the identity: filtered - raw is 0 (demodulate = 0: exactly; the rule gives t = 1 everywhere) or
    the rounding of c / a * a, so the weight-variety condition is asserted on the cases that filter."""
    for radius in (1, 2, 3):
        for iterations in (0, 4):
            for demodulate in (0, 1):
                p = dict(iterations=iterations, demodulate=demodulate)
                if iterations:
                    _varied(_want(r, cfg, radius, 0.0, 1, **p)[1], f"{what} radius {radius} {p}")
                _, t, st = _check(r, cfg, radius, 0.0, 1, what, **p)
                if not iterations and not demodulate:
                    assert np.all(t == 1) and st[1] == 0
    assert st[0] == cfg.width * cfg.height


# ------------------------------------------------------------------ 1. bit for bit against the restatement
@pytest.mark.parametrize("name", ["cornell_v3", "scene_demo"])
@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
def test_weight_and_blended_frame_bit_identical_to_restatement(frame, name):
    w, h = frame
    cfg, r = _dealt(name, w, h)
    _sweep(r, cfg, f"{name} {w}x{h}")
    if name == "scene_demo" and w * h > 100:
        obj = r.feature_object
        assert (obj == -1).any() and len(np.unique(obj)) > 2      # misses, and more than one object in a window
    # the defaults: both parameter structs NULL (7 samples: below min_half_samples, t = 1)
    out, t, st = _check(r, cfg, what="defaults")
    assert st == (0, 0, 0.0) and np.all(t == 1)
    _check(r, cfg, 3, 2.0, 2, "the gate on")


def test_halves_dealt_per_sample():
    cfg, r = _dealt("cornell_v3", 33, 17, per_sample=True)
    _sweep(r, cfg, "per-sample dealing 33x17")


# ------------------------------------------------------------------ 2. equality with rtpbr_denoise, and what the call leaves alone
@pytest.mark.parametrize("name", ["cornell_v3", "scene_demo"])
def test_with_every_half_too_small_the_call_writes_rtpbr_denoises_bytes(name):
    cfg, r = _dealt(name, 33, 17)
    for holes in (False, True):
        if holes:                                         # a row and a pixel without samples (written data: A is zeroed, and stays)
            ib = r.image_buffer
            ib[:, 3] = 0.0
            ib[5, 9] = 0.0
            r.image_buffer = ib
        for p in ({}, dict(iterations=0), dict(iterations=1, demodulate=1), dict(iterations=3, sigma_color=0.5)):
            r.denoise(**p)
            want = r.denoised_pixels
            stats = r.denoise_blend(2, 0.0, NEVER, **p)
            ck.same(r.denoised_pixels, want, f"denoised_pixels {p}")
            assert np.all(r.blend_weight == 1) and (stats.pixels_estimated, stats.pixels_above, stats.max_noise) == (0, 0, 0.0)
    r.post_process()
    ck.same(r.denoised_pixels[:, 3], r.image_pixels[:, 3], "pixels without samples show what post_process shows")


def test_denoise_blend_writes_nothing_else():
    cfg, r = _dealt("cornell_v3", 33, 17)
    r.noise_update()
    r.noise_estimate(0.0)
    r.denoise_error(0.01)
    r.select_error(0.01, 1)
    r.post_process()
    others = (BUF_IMAGE_BUFFER, BUF_IMAGE_PIXELS, BUF_HALF_BUFFER, BUF_MOMENTS, BUF_NOISE, BUF_DENOISED_ERROR, BUF_SELECTION)
    before = {b: r._read(b) for b in others}
    counters = ck.counters(r)
    for iterations in (0, 1, 4):
        r.denoise_blend(3, 0.0, 1, iterations=iterations, demodulate=1)
        for b, a in before.items():
            ck.same(r._read(b), a, f"buffer {b} after denoise_blend")
        assert ck.counters(r) == counters
    # the snapshot: the next half_update deals exactly what came since the last one
    r.sample(2)
    r.half_update()
    assert np.all(r.half_buffer[..., 3] == 5) and np.all(r.image_buffer[..., 3] == 9)      # A 5 > B 2: the batch went to B
    assert ck.code(lambda: r._write(BUF_BLEND_WEIGHT, before[BUF_NOISE])) == EINVAL      # output only


def test_present_serves_the_blended_frame():
    cfg, r = _dealt("scene_demo", 33, 17)
    out, t, _ = _check(r, cfg, 2, 0.0, 1)
    assert ((t > 0) & (t < 1)).any()
    for fmt, f in (("rgb8", pr.FORMAT_RGB8), ("rgba8", pr.FORMAT_RGBA8)):
        for dither in (False, True):
            r.present("denoised", fmt, dither)
            got = r.presented
            want = pr.present(out, f, dither)
            assert got.shape == want.shape and np.array_equal(got, want), (fmt, dither)
    # ... and an asynchronous read of either output is ordered before the next call overwrites it
    hw, hd = r.host_array(BUF_BLEND_WEIGHT), r.host_array(BUF_DENOISED_PIXELS)
    tw, td = r.read_async(BUF_BLEND_WEIGHT, hw), r.read_async(BUF_DENOISED_PIXELS, hd)
    r.denoise_blend(2, 0.0, NEVER)
    r.read_wait(tw)
    r.read_wait(td)
    ck.same(hw, t, "the asynchronous read holds the earlier weight")
    ck.same(hd, out, "the asynchronous read holds the earlier frame")
    assert np.all(r.blend_weight == 1)


# ------------------------------------------------------------------ 3. refusals and the buffer's lifetime
def test_refusals_change_nothing():
    cfg, r = _dealt("cornell_v3", 33, 17)
    api, ctx = r.api, r._ctx
    nan, inf = float("nan"), float("inf")
    assert ck.code(lambda: r.blend_weight) == ESTATE               # before the first call
    r.denoise_blend(2, 0.0, 1)
    watched = (BUF_BLEND_WEIGHT, BUF_DENOISED_PIXELS, BUF_HALF_BUFFER, BUF_IMAGE_BUFFER)
    before = {b: r._read(b) for b in watched}
    s = NoiseStats()
    assert api.fn["denoise_blend"](None, None, None, C.byref(s)) == EINVAL
    for bad in ({"iterations": 9}, {"iterations": -1}, {"demodulate": 2}, {"sigma_color": 0.0}, {"sigma_normal": nan}, {"sigma_depth": -1.0},
                {"sigma_albedo": inf}, {"iterations": 8, "sigma_color": 1e-18}):
        assert ck.code(lambda: r.denoise_blend(**bad)) == EINVAL, bad
        assert ck.code(lambda: r.denoise(**bad)) == EINVAL, bad      # exactly rtpbr_denoise's checks
    for radius in (0, 4, -1):
        assert ck.code(lambda: r.denoise_blend(radius)) == EINVAL
    for z in (-1.0, nan, inf, float("-inf"), -1e-30):
        assert ck.code(lambda: r.denoise_blend(z=z)) == EINVAL
    for m in (0, -1, NEVER + 1):
        assert ck.code(lambda: r.denoise_blend(min_half_samples=m)) == EINVAL
    r.set_tiles(16, 16, 0, 2)
    assert ck.code(lambda: r.denoise_blend()) == ESTATE
    r.set_tiles(0, 0, 0, 1)
    for b, a in before.items():
        ck.same(r._read(b), a, f"buffer {b} after the refused calls")
    # a NULL statistics pointer is allowed, as in rtpbr_denoise_error; -0 is a z >= 0
    e = BlendParams(2, -0.0, 1)
    assert api.fn["denoise_blend"](ctx, None, C.byref(e), None) == 0
    for b, a in before.items():
        ck.same(r._read(b), a, f"buffer {b} after the same call again")


def test_refusals_before_the_context_is_set_up_and_before_half_a_exists():
    scene, cfg = ck.scene("cornell_v3", 16, 12)
    api = Renderer(scene, cfg).api
    ctx = C.c_void_p()
    api.call("create", 0, C.byref(ctx))
    try:
        assert api.fn["denoise_blend"](ctx, None, None, None) == ESTATE      # no configuration
        c = cfg.copy()
        api.call("set_config", ctx, C.byref(c))
        assert api.fn["half_update"](ctx) == 0
        assert api.fn["denoise_blend"](ctx, None, None, None) == ESTATE      # no scene, no camera
    finally:
        api.call("destroy", ctx)
    r = Renderer(scene, cfg)
    r.sample(2)
    assert ck.code(lambda: r.denoise_blend()) == ESTATE and ck.code(lambda: r.blend_weight) == ESTATE      # before half A exists
    assert ck.code(lambda: r.denoise_blend(iterations=9)) == EINVAL and ck.code(lambda: r.denoise_blend(radius=4)) == EINVAL      # parameters come first
    assert ck.code(lambda: r.denoised_pixels) == ESTATE                      # nothing was allocated on the way
    r.set_half_mode(per_sample=True)                                       # a dealing call makes A: everything so far is one batch
    r.sample(2)
    assert r.denoise_blend(1, 0.0, 1).pixels_estimated == 16 * 12


def test_a_new_resolution_frees_the_weight_buffer():
    cfg, r = _dealt("cornell_v3", 33, 17)
    r.denoise_blend(1, 0.0, 1)
    assert r.blend_weight.shape == (33, 17)
    cfg2 = cfg.copy(width=17, height=9)
    r.set_config(cfg2)
    assert ck.code(lambda: r.blend_weight) == ESTATE and ck.code(lambda: r.denoise_blend()) == ESTATE
    for n in (2, 2):
        r.sample(n)
        r.half_update()
    _check(r, cfg2, 3, 0.0, 1, "the new frame")
    r.set_config(cfg2.copy(exposure=cfg2.exposure * 0.5))                  # the same resolution: the buffer stays
    assert r.blend_weight.shape == (17, 9)


# ------------------------------------------------------------------ 4. hostile image buffers
@pytest.mark.parametrize("frame,family", [("97x61", "F"), ("97x61", "N"), ("7x5", "F")])      # (family N needs an object of 40 pixels)
def test_hostile_image_buffer(frame, family):
    """the hostile buffer lands in A (the first batch of a fresh context), rtpbr_sample(2) in B"""
    w, h = hz.FRAMES[frame]
    scene, cfg = hz.scene_cfg("v3", w, h)
    r = Renderer(scene, cfg)
    r.render_features()
    ib = hz.buffer_for(family, r.feature_object)
    r.image_buffer = ib
    r.half_update()
    r.sample(2)
    r.half_update()
    ib2, a, feats = r.image_buffer, r.half_buffer, ck.feats(r)
    for radius, z, denoise in ((1, 0.0, {}), (3, 0.0, dict(iterations=2, demodulate=1, **hz.SIGMAS)), (3, 2.0, {}), (2, 0.0, dict(iterations=0))):
        stats = r.denoise_blend(radius, z, 1, **denoise)
        out, t, st = bl.denoise_blend(cfg, ib2, a, feats, radius, z, 1, **denoise)
        stage = f"denoise_blend {frame} {family} radius {radius} z {z} {'defaults' if not denoise else denoise}"
        hz.guard(stage, out)
        hz.compare(stage, r.denoised_pixels, out, ib2)
        hz.compare(stage.replace("denoise_blend", "blend_weight"), r.blend_weight, t, ib2)
        hz.compare_stats(stage, stats, st)
        assert not np.isnan(t).any() and np.all((t >= 0) & (t <= 1)) and st[0] > 0.5 * w * h


# ------------------------------------------------------------------ 5. one scripted sequence
def test_scripted_sequence_against_the_restatement():
    """sample, half_update, blend; selected batches, half_update, blend; a reprojection that carries half A, blend (the warped
    counts are fractional: min_half_samples decides which pixels are usable); refresh; a second size, where the call is refused
    until halves exist again."""
    w, h = 33, 17
    scene, cfg = ck.scene("cornell_v3", w, h)
    r = Renderer(scene, cfg)
    r.refresh()                                            # (reproject wants one since set_config)
    r.set_half_mode(warp=True)
    p = dict(iterations=2)
    for n in (3, 3):
        r.sample(n)
        r.half_update()
    _, t, st = _check(r, cfg, 2, 0.0, 3, "two batches", **p)
    assert st[0] == w * h and st[1] > 0
    mask = np.zeros((w, h), np.uint8)
    mask[w // 3: w // 3 + 8] = 1
    r.select_mask(mask)
    for _ in range(2):                                     # A (a tie), then B
        r.sample_selected(2)
        r.half_update()
    _, t, st = _check(r, cfg, 3, 0.0, 4, "after the selected batches", **p)      # 5 + 5 on the stripe, 3 + 3 elsewhere
    assert st[0] == int(mask.sum()) and np.all(t[mask == 0] == 1)
    c = scene.camera
    cam = Camera((c.lookfrom[0] + 1.5, c.lookfrom[1] + 0.5, c.lookfrom[2]), tuple(c.lookat), tuple(c.vup), c.vfov, c.aspect, c.aperture, c.focus)
    r.reproject(cam)
    a, ib = r.half_buffer, r.image_buffer
    assert (a[..., 3] > 0).any() and (ib[..., 3] - a[..., 3] > 0).any()         # history carried in both halves
    _, t, st = _check(r, cfg, 2, 0.0, 3, "after the reprojection", **p)
    usable = (a[..., 3] >= 3) & (ib[..., 3] - a[..., 3] >= 3)
    assert st[0] == int(usable.sum()) and st[0] > 0 and np.all(t[~usable] == 1)
    r.refresh()
    stats = r.denoise_blend(2, 0.0, 1, **p)
    assert stats.pixels_estimated == 0 and np.all(r.blend_weight == 1)
    r.post_process()
    ck.same(r.denoised_pixels, r.image_pixels, "an empty frame shows what post_process shows")
    r.set_config(cfg.copy(width=20, height=13))
    assert ck.code(lambda: r.denoise_blend(2, 0.0, 1, **p)) == ESTATE and ck.code(lambda: r.blend_weight) == ESTATE


# ------------------------------------------------------------------ 6. the loop
def test_render_adaptive_denoised_ends_with_the_blend():
    w = h = 32
    scene, cfg = ck.scene("cornell_v3", w, h)
    r, s = Renderer(scene, cfg), Renderer(scene, cfg)
    args = (0.02, 40, 8, 1)
    traced, stats = r.render_adaptive_denoised(*args, blend=True, iterations=3)
    traced_s, stats_s = s.render_adaptive_denoised(*args, iterations=3)
    assert traced == traced_s and stats.pixels_above == stats_s.pixels_above      # the stop rule is unchanged
    ck.same(r.image_buffer, s.image_buffer, "image_buffer")
    ck.same(r.half_buffer, s.half_buffer, "half_buffer")
    out, t, _ = _want(r, cfg, None, None, None, iterations=3)
    ck.same(r.denoised_pixels, out, "denoised_pixels")
    ck.same(r.blend_weight, t, "blend_weight")
    assert ck.code(lambda: s.blend_weight) == ESTATE
