"""The error estimate of the level-blended frame with the bias in display space per tap, on the GPU (rtpbr_blend_error_display,
Renderer.blend_error(bias="display"), Renderer.render_adaptive_denoised(stop="blend", bias="display")).  Every comparison is
``==`` on bit patterns against the CPU restatement (tests/post_ref/blend.h with display set) fed with the GPU's
own image_buffer, half A and features; plus what the call shares with rtpbr_blend_error (the plane) and what it does not
(anything else), and the state and error rules of include/rtpbr.h.  Shapes and states are those of
tests/test_gpu_blend_error.py (tests/blend_error_states.py)."""
import ctypes as C

import numpy as np
import pytest

import blend_error_ref_lib as be
import blend_error_states as states
import checks as ck
import feature_ref_lib as fr
import half_ref_lib as hl
import levels_ref_lib as lv
from checks import EINVAL, ESTATE
from oracle_backend import OracleRenderer
from raytracingpbr_amd import Camera, Renderer
from raytracingpbr_amd.dataclass import BlendParams, ErrorParams, NoiseStats
from raytracingpbr_amd.renderer import (BUF_BLEND_DEPTH, BUF_BLEND_ERROR, BUF_BLEND_WEIGHT, BUF_DENOISED_ERROR, BUF_DENOISED_PIXELS,
                                        BUF_HALF_BUFFER, BUF_IMAGE_BUFFER, BUF_IMAGE_PIXELS, BUF_MOMENTS, BUF_NOISE, BUF_SELECTION)

pytestmark = pytest.mark.gpu

FRAMES = [(16, 16), (17, 33), (37, 21)]    # one tile; ragged both ways, more than one tile either way: the halo crosses tiles and the frame border
NEVER = 16777216                           # min_half_samples above every count
M = 5                                      # min_half_samples of the dealt states: the stripe (6 + 6) is usable, the rest (4 + 4) only valid
THR = 0.02


def _check(r, cfg, threshold=THR, radius=None, z=None, m=None, window=None, what="", **denoise):
    stats = r.blend_error(threshold, radius, z, m, window, bias="display", **denoise)
    want = be.blend_error(cfg, r.image_buffer, r.half_buffer, ck.feats(r), threshold, radius, z, m, window, display=True, **denoise)
    states.compare(r, stats, want, f"{what} threshold {threshold} radius {radius} z {z} min_half_samples {m} window {window} {denoise}")
    return want


def _sweep(r, cfg, what):
    """window 1..3, 0 / 1 / 4 levels, with and without demodulation; the blend's radius goes 1, 2, 3 with the window and z is 0
    (windows refuse levels: T_K < 1).  The ladders of a (levels, demodulation) pair are filtered once.  The old call runs on the
    same state: unless the two planes differ and a bias term is there, the comparison shows nothing of the new rule."""
    ib, a, feats = r.image_buffer, r.half_buffer, ck.feats(r)
    seen_bias = seen_refused = seen_other = False
    for iterations in (0, 1, 4):
        for demodulate in (0, 1):
            p = dict(iterations=iterations, demodulate=demodulate)
            f = lv.Filtered(cfg, ib, a, feats, **p)
            for window in (1, 2, 3):
                want = be.from_ladders(f, THR, window, 0.0, M, window, display=True)
                states.compare(r, r.blend_error(THR, window, 0.0, M, window, bias="display", **p), want, f"{what} window {window} {p}")
                assert want.stats[0] == cfg.width * cfg.height and 0 < want.stats[1]
                usable = (a[..., 3] >= M) & (ib[..., 3] - a[..., 3] >= M)
                assert usable.any() and not usable.all()
                seen_bias |= bool((want.bias2 > 0).any()) and iterations > 0
                seen_refused |= bool((want.weight < 1).any())
                r.blend_error(THR, window, 0.0, M, window, **p)
                seen_other |= not np.array_equal(ck.bits(r.blend_error_map), ck.bits(want.error))
    assert seen_bias and seen_refused and seen_other


# ------------------------------------------------------------------ 1. bit for bit against the restatement
@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
def test_error_plane_frame_and_statistics_bit_identical_to_restatement(frame):
    w, h = frame
    cfg, r = states.dealt_4_4_stripe_6_6(w, h)
    assert len(np.unique(r.feature_object)) > 2                          # windows straddle objects
    _sweep(r, cfg, f"{w}x{h}")
    # the defaults: every parameter struct NULL (below min_half_samples = 16: nothing usable, no bias term)
    want = _check(r, cfg, what="defaults")
    assert not want.bias2.any() and np.all(want.weight == 1)
    # a gate that is not 0, and the blend's radius apart from the window's
    _check(r, cfg, 0.05, 3, 2.0, 4, 1, "z 2", iterations=2)


# ------------------------------------------------------------------ 2. what the restatement must meet
def test_halves_dealt_per_sample():
    cfg, r = states.dealt_4_4_stripe_6_6(17, 33, per_sample=True)
    _sweep(r, cfg, "per-sample dealing 17x33")


def test_after_a_reprojection_pixels_with_an_empty_half_and_without_samples_are_not_estimated():
    w, h = 37, 21
    scene, cfg = states.cornell(w, h)
    r = Renderer(scene, cfg)
    r.refresh()                                                          # (reproject wants one since set_config)
    for _ in range(2):
        r.sample(4)
        r.half_update()
    c = scene.camera
    cam = Camera((c.lookfrom[0] + 1.5, c.lookfrom[1] + 0.5, c.lookfrom[2]), tuple(c.lookat), tuple(c.vup), c.vfov, c.aspect, c.aperture, c.focus)
    r.reproject(cam)                                                     # A = 0: the history lies in B
    assert not r.half_buffer.any() and (r.image_buffer[..., 3] == 0).any()
    want = _check(r, cfg, m=1, what="right after the reprojection", iterations=2)
    assert want.stats == (0, 0, 0.0) and not want.error.any()
    r.select_mask(states.stripe(w, h))
    r.sample_selected(2)                                                 # the stripe's batch goes to A
    r.half_update()
    a, ib = r.half_buffer[..., 3], r.image_buffer[..., 3]
    valid = (a > 0) & (ib - a > 0)
    assert valid.any() and (~valid & (ib > 0)).any() and (ib == 0).any()
    for window in (1, 3):
        want = _check(r, cfg, 0.01, 2, 0.0, 1, window, "after the reprojection", iterations=2)
        assert want.stats[0] == int(valid.sum()) and not want.error[~valid].any()
        assert not want.slope[ib == 0].any()                             # a pixel without samples has slope 0 (and is no tap)
        assert (want.bias2 > 0).any()


# ------------------------------------------------------------------ 3. the two calls share the plane and nothing else
def test_nothing_else_moves_and_the_old_call_restores_its_plane():
    w, h = 37, 21
    cfg, r = states.dealt_4_4_stripe_6_6(w, h)
    r.noise_update()
    r.noise_estimate(0.0)
    r.denoise_error(0.01)
    r.select_error(0.01, 1)
    r.post_process()
    others = (BUF_IMAGE_BUFFER, BUF_IMAGE_PIXELS, BUF_HALF_BUFFER, BUF_MOMENTS, BUF_NOISE, BUF_DENOISED_ERROR, BUF_SELECTION)
    before = {b: r._read(b) for b in others}
    counters = ck.counters(r)
    for p in (dict(iterations=0), dict(iterations=1, demodulate=1), dict(iterations=4)):
        for radius, z in ((1, 0.0), (3, 2.0)):
            st_l = r.denoise_blend_levels(radius, z, M, **p)
            frame = {b: r._read(b) for b in (BUF_DENOISED_PIXELS, BUF_BLEND_WEIGHT, BUF_BLEND_DEPTH)}
            r.blend_error(THR, radius, z, M, 2, **p)
            old = r.blend_error_map
            r.denoise()                                                  # (something else in the frame buffer in between)
            st_e = r.blend_error(THR, radius, z, M, 2, bias="display", **p)
            new = r.blend_error_map
            for b, a in frame.items():
                ck.same(r._read(b), a, f"buffer {b} of the display call against denoise_blend_levels {p} radius {radius} z {z}")
            assert st_e.pixels_estimated == w * h and st_l.pixels_estimated == int((states.stripe(w, h) != 0).sum())
            for b, a in before.items():
                ck.same(r._read(b), a, f"buffer {b} after the display call")
            assert ck.counters(r) == counters
            # the last of the two calls wins the plane, either way round
            r.blend_error(THR, radius, z, M, 2, **p)
            ck.same(r.blend_error_map, old, f"the old call's plane after the display call {p} radius {radius} z {z}")
            for b, a in frame.items():
                ck.same(r._read(b), a, f"buffer {b} of the old call after the display call")
            r.blend_error(THR, radius, z, M, 2, bias="display", **p)
            ck.same(r.blend_error_map, new, f"the display call's plane after the old call {p} radius {radius} z {z}")
            assert p["iterations"] == 0 or not np.array_equal(ck.bits(old), ck.bits(new))
    assert ck.code(lambda: r._write(BUF_BLEND_ERROR, before[BUF_NOISE])) == EINVAL        # an output only


def test_with_nothing_usable_the_plane_is_rtpbr_denoise_errors():
    w, h = 37, 21
    cfg, r = states.dealt_4_4_stripe_6_6(w, h)
    for p in ({}, dict(iterations=0), dict(iterations=1, demodulate=1), dict(iterations=3, sigma_color=0.5)):
        for window in (1, 2, 3):
            want = r.denoise_error(THR, window, **p)
            plane = r.denoised_error
            got = r.blend_error(THR, 2, 0.0, NEVER, window, bias="display", **p)
            ck.same(r.blend_error_map, plane, f"blend_error_map against denoised_error {p} window {window}")
            assert (got.pixels_estimated, got.pixels_above, got.max_noise) == (want.pixels_estimated, want.pixels_above, want.max_noise)
    # no levels, no demodulation: the raw halves' variance and no bias, usable or not
    r.denoise_error(THR, 2, iterations=0, demodulate=0)
    plane = r.denoised_error
    r.blend_error(THR, 2, 0.0, 1, 2, bias="display", iterations=0, demodulate=0)
    ck.same(r.blend_error_map, plane, "K = 0")


def test_select_blend_error_is_the_numpy_rule_on_the_new_plane():
    w, h = 37, 21
    cfg, r = states.dealt_4_4_stripe_6_6(w, h)
    r.blend_error(THR, 2, 0.0, M, 2, iterations=2)                       # the old call's plane first: the selection must not see it
    old = r.blend_error_map
    want = _check(r, cfg, THR, 2, 0.0, M, 2, iterations=2)
    err = want.error
    thr = float(np.median(err))
    assert not np.array_equal(hl.select(r.image_buffer, r.half_buffer, err, thr, 0, 0), hl.select(r.image_buffer, r.half_buffer, old, thr, 0, 0))
    for dilate in (0, 1, 3):
        n = r.select_blend_error(thr, dilate)
        mask = hl.select(r.image_buffer, r.half_buffer, err, thr, dilate, 0)
        got = r.selection
        assert got.dtype == np.uint8 and np.array_equal(got, mask), f"dilate {dilate}: {int((got != mask).sum())} pixels differ"
        assert n == int(mask.sum()) and 0 < n < w * h
    ck.same(r.blend_error_map, err, "the plane after the selections")
    # every way out serves it
    into = np.empty((w, h), np.float32)
    r.read_into(BUF_BLEND_ERROR, into)
    ck.same(into, err, "read_into")
    assert r.device_ptr(BUF_BLEND_ERROR)[1] == w * h * 4


# ------------------------------------------------------------------ 4. refusals and the buffer's lifetime
def test_refusals_change_nothing():
    cfg, r = states.dealt_4_4_stripe_6_6(17, 33)
    api, ctx = r.api, r._ctx
    nan, inf = float("nan"), float("inf")
    show = lambda **k: r.blend_error(bias="display", **k)      # noqa: E731
    assert ck.code(lambda: r.blend_error_map) == ESTATE and ck.code(lambda: r.select_blend_error(0.0)) == ESTATE      # before the first call
    r.denoise_blend_levels(2, 0.0, M)
    assert ck.code(lambda: r.blend_error_map) == ESTATE and ck.code(lambda: r.select_blend_error(0.0)) == ESTATE      # ... of either estimate
    r.blend_error(THR, 2, 0.0, M, 2, bias="display")                     # the first call makes the plane: the old one never ran here
    r.select_blend_error(THR, 1)
    watched = (BUF_BLEND_ERROR, BUF_BLEND_WEIGHT, BUF_BLEND_DEPTH, BUF_DENOISED_PIXELS, BUF_HALF_BUFFER, BUF_IMAGE_BUFFER, BUF_SELECTION)
    before = {b: r._read(b) for b in watched}
    s = NoiseStats()
    assert api.fn["blend_error_display"](None, None, None, None, 0.0, C.byref(s)) == EINVAL
    for bad in ({"iterations": 9}, {"iterations": -1}, {"demodulate": 2}, {"sigma_color": 0.0}, {"sigma_normal": nan}, {"sigma_depth": -1.0},
                {"sigma_albedo": inf}, {"iterations": 8, "sigma_color": 1e-18}):
        assert ck.code(lambda: show(**bad)) == EINVAL, bad
    for radius in (0, 4, -1):
        assert ck.code(lambda: show(radius=radius)) == EINVAL and ck.code(lambda: show(window=radius)) == EINVAL
    for z in (-1.0, nan, inf, float("-inf")):
        assert ck.code(lambda: show(z=z)) == EINVAL
    for m in (0, -1, NEVER + 1):
        assert ck.code(lambda: show(min_half_samples=m)) == EINVAL
    for thr in (-1.0, nan):
        assert ck.code(lambda: show(threshold=thr)) == EINVAL
    r.set_tiles(16, 16, 0, 2)
    assert ck.code(lambda: show()) == ESTATE
    r.set_tiles(0, 0, 0, 1)
    for b, a in before.items():
        ck.same(r._read(b), a, f"buffer {b} after the refused calls")
    with pytest.raises(ValueError):
        r.blend_error(bias="tap")
    # NULL for every parameter struct and the statistics is allowed
    e, w = BlendParams(2, 0.0, M), ErrorParams(2)
    assert api.fn["blend_error_display"](ctx, None, C.byref(e), C.byref(w), THR, None) == 0
    for b, a in before.items():
        ck.same(r._read(b), a, f"buffer {b} after the same call again")


def test_refusals_before_the_context_is_set_up_and_before_half_a_exists():
    scene, cfg = states.cornell(16, 12)
    api = Renderer(scene, cfg).api
    ctx = C.c_void_p()
    api.call("create", 0, C.byref(ctx))
    try:
        assert api.fn["blend_error_display"](ctx, None, None, None, 0.0, None) == ESTATE      # no configuration
        c = cfg.copy()
        api.call("set_config", ctx, C.byref(c))
        assert api.fn["half_update"](ctx) == 0
        assert api.fn["blend_error_display"](ctx, None, None, None, 0.0, None) == ESTATE      # no scene, no camera
    finally:
        api.call("destroy", ctx)
    r = Renderer(scene, cfg)
    r.sample(2)
    show = lambda **k: r.blend_error(bias="display", **k)      # noqa: E731
    assert ck.code(lambda: show()) == ESTATE and ck.code(lambda: r.blend_error_map) == ESTATE      # before half A exists
    assert ck.code(lambda: show(iterations=9)) == EINVAL and ck.code(lambda: show(window=4)) == EINVAL      # parameters come first
    assert ck.code(lambda: r.denoised_pixels) == ESTATE and ck.code(lambda: r.blend_weight) == ESTATE      # nothing was allocated on the way


def test_a_new_resolution_frees_the_planes_and_a_larger_frame_gets_its_own():
    cfg, r = states.dealt_4_4_stripe_6_6(16, 16)
    _check(r, cfg, THR, 3, 0.0, M, 3, "the first frame")
    assert r.blend_error_map.shape == (16, 16)
    cfg2 = cfg.copy(width=37, height=21)
    r.set_config(cfg2)
    for b in (lambda: r.blend_error_map, lambda: r.blend_error(bias="display"), lambda: r.select_blend_error(0.0)):
        assert ck.code(b) == ESTATE
    for _ in range(2):
        r.sample(4)
        r.half_update()
    want = _check(r, cfg2, THR, 3, 0.0, 4, 3, "the larger frame")        # (a slope plane kept from 16 x 16 would be overrun here)
    assert (want.bias2 > 0).any()
    _check(r, cfg2, THR, 2, 2.0, 4, 1, "the larger frame again", iterations=2, demodulate=1)
    r.set_config(cfg2.copy(exposure=cfg2.exposure * 0.5))                # the same resolution: the plane stays
    assert r.blend_error_map.shape == (37, 21)


# ------------------------------------------------------------------ 5. the loop
def _loop_on_the_restatements(scene, cfg, display, error, max_spp, batch, dilate, **params):
    """render_adaptive_denoised(stop="blend") with the oracle's samples, half_ref's dealing and selection and the estimate of
    blend_error_ref_lib under the rule ``display`` selects; (traced, used, the last BlendError, image_buffer, half A)"""
    w, h = cfg.width, cfg.height
    feats = fr.features(scene, cfg)
    o = OracleRenderer(scene, cfg)
    hv = hl.Halves(w, h)
    traced = used = 0
    for _ in range(2):
        o.sample(batch)
        hv.update(o.image_buffer)
        traced, used = traced + w * h * batch, used + batch
    while True:
        got = be.blend_error(cfg, o.image_buffer, hv.a, feats, error, display=display, **params)
        if got.stats[1] == 0 or used + batch > max_spp:
            break
        mask = hl.select(o.image_buffer, hv.a, got.error, error, dilate, 0)
        before = o.image_buffer
        o.sample(batch)                                                  # the full frame at the same sample index ...
        o.image_buffer = np.where((mask != 0)[..., None], o.image_buffer, before)      # ... kept where selected
        hv.update(o.image_buffer)
        traced, used = traced + int(mask.sum()) * batch, used + batch
    ib = o.image_buffer
    o.close()
    return traced, used, got, ib, hv.a


def test_render_adaptive_denoised_with_the_display_bias_ends_on_the_threshold_and_with_the_linear_on_the_budget():
    """32 x 32, error 0.3, at most 64 spp in batches of 8, dilate 1, three levels, min_half_samples 8: the bias term is active
    from the first estimate on.  The per-tap rule ends on the threshold after adaptive rounds (the restatements: 48 spp, 17 200
    pixel-samples); the per-window rule keeps the pixels beside the light above any such threshold and runs into the budget
    (DESIGN.md sections 6n and 6o).  Both loops equal the same loop on the oracle and the restatements."""
    w = h = 32
    scene, cfg = states.cornell(w, h)
    args, params = (0.3, 64, 8, 1), dict(iterations=3, min_half_samples=8)
    r = Renderer(scene, cfg)
    traced, stats = r.render_adaptive_denoised(*args, blend="levels", stop="blend", bias="display", **params)
    want_traced, used, want, ib, a = _loop_on_the_restatements(scene, cfg, True, *args, **params)
    assert want.stats[1] == 0 and used + 8 <= 64 and 16 < used           # the restatement loop: the threshold, after adaptive rounds
    assert stats.pixels_above == 0 and traced == want_traced
    ck.same(r.image_buffer, ib, "image_buffer")
    ck.same(r.half_buffer, a, "half_buffer")
    states.compare(r, stats, want, "the frame and the estimate the loop ends with")
    assert (want.bias2 > 0).any()
    # the same arguments with the per-window rule
    r = Renderer(scene, cfg)
    traced, stats = r.render_adaptive_denoised(*args, blend="levels", stop="blend", bias="linear", **params)
    want_traced, used, want, ib, a = _loop_on_the_restatements(scene, cfg, False, *args, **params)
    assert want.stats[1] > 0 and used + 8 > 64                           # the restatement loop: the budget, with pixels above
    assert stats.pixels_above == want.stats[1] > 0 and traced == want_traced
    ck.same(r.image_buffer, ib, "image_buffer, linear")
    ck.same(r.blend_error_map, want.error, "blend_error_map, linear")
    with pytest.raises(ValueError):
        r.render_adaptive_denoised(*args, blend="levels", bias="display", **params)      # not without stop="blend"


# ------------------------------------------------------------------ 6. random call sequences against a state model
@pytest.mark.parametrize("seed", [0, 8, 9])      # (0 and 8 draw the pair of calls both ways round, 9 RTPBR_ESTATE for the display call)
def test_random_call_sequences(seed):
    """~30 random operations of tests/blend_display_sequences.py on 33 x 17 / 20 x 13 frames: the two estimate calls,
    select_blend_error, sample, sample_selected, half_update, reproject, refresh and set_config to a new size between the draws
    of the existing sequences — every call refused or accepted as include/rtpbr.h says, every value it returns or leaves behind
    bit for bit the model's"""
    import blend_display_sequences as ds
    import call_sequences as cs
    s = ds.display_script(seed)
    a, b = cs.new_renderer(s, Renderer), ds.model(s)
    try:
        seen, events = ds.run(s, a, b)
    finally:
        a.close()
        b.close()
    assert any(k == "blend_error_map" for _, k, _ in seen) and any(k == "half_buffer" for _, k, _ in seen)
    assert any(e[0] == ds.DISPLAY for e in events)
