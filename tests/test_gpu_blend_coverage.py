"""rtpbr_denoise_blend_levels, rtpbr_blend_error and rtpbr_blend_error_display with option blend_coverage = 1 on the GPU
(atrous_level's COVER form, level_blend's LIN instances, cover_weights, cover_resolve), held bit for bit to the CPU restatement
(tests/blend_coverage_ref_lib.py, tests/blend_coverage_ref) fed with the GPU's own image_buffer, half A and features: the frame,
the weight, the depth, the error plane in both bias modes, the returned statistics and counter blend_resolved; plus the two
identities, the calls that ignore the option, the option-off bytes afterwards and the refusals of include/rtpbr.h.  jit = 0."""
import itertools

import numpy as np
import pytest

import blend_coverage_ref_lib as bc
import blend_error_ref_lib as be
import checks as ck
import coverage_ref_lib as cl
import feature_ref_lib as fl
import levels_ref_lib as lv
from raytracingpbr_amd import Config, Renderer, cornell_box, src_scene
from raytracingpbr_amd._capi import RtpbrError
from raytracingpbr_amd.ibl import synthetic_env

pytestmark = pytest.mark.gpu

SHARP = dict(sigma_color=0.5, sigma_normal=0.3, sigma_depth=0.05, sigma_albedo=0.1)      # sigmas at which every term of e matters
NEVER = 16777216                           # min_half_samples above every count: t_k = 1 everywhere
MODES = ("levels", "linear", "display")
OUT_OF_RANGE = "coverage: grid x resolution out of range (1..65535)"


def _cornell(w, h):
    return cornell_box("v3", aspect=w / h), Config.cornell_v3(w, h, 0, 3)


def _dealt(sc, cfg, each=16):
    """two batches of ``each`` samples with a half_update after either: halves each + each; the features exist"""
    r = Renderer(sc, cfg)
    r.set_option("jit", 0)
    for _ in range(2):
        r.sample(each)
        r.half_update()
    r.render_features()
    return r


def _call(r, mode, **p):
    """the call of ``mode`` through the new methods: (NoiseStats, blend_resolved)"""
    if mode == "levels":
        return r.denoise_blend_levels_coverage(**{k: v for k, v in p.items() if k not in ("window", "threshold")})
    return r.blend_error_coverage(bias=mode, **p)


def _compare(r, got, want, what):
    stats, resolved = got
    ck.same(r.denoised_pixels, want.denoised, "denoised_pixels " + what)
    ck.same(r.blend_weight, want.weight, "blend_weight " + what)
    ck.same(r.blend_depth, want.depth, "blend_depth " + what)
    if want.error is not None:
        ck.same(r.blend_error_map, want.error, "blend_error_map " + what)
    ck.stats_same(stats, want.stats, what)
    assert resolved == want.resolved == r.counter("blend_resolved"), (what, resolved, want.resolved)


def _sweep(r, cfg, cov_of, what, levels=(1, 2, 5), demodulates=(0, 1), covers=((4, 4), (0, 2), (8, 2)), sig=SHARP):
    """levels x demodulate x (power, grid): the three ladders are filtered once and shared by the rule settings — radius 1..3, both
    resolve settings, min_half_samples 8 and 16, the three calls, windows 1 and 3.  Returns the restatement's results."""
    ib, a, feats = r.image_buffer, r.half_buffer, ck.feats(r)
    seen = []
    rules = itertools.cycle([(1, 0.0, 8, 3), (2, 2.0, 16, 1), (3, 0.0, 16, 3), (3, 2.0, 8, 1), (2, 0.0, 16, 2)])
    for iterations, demodulate, (power, grid) in itertools.product(levels, demodulates, covers):
        d = dict(iterations=iterations, demodulate=demodulate, **sig)
        f = bc.Filtered(cfg, ib, a, feats, cov_of(grid), power, **d)
        for resolve, mode in itertools.product((0, 1), MODES):
            radius, z, m, window = next(rules)
            w = f"{what} {mode} {d} power {power} grid {grid} resolve {resolve} radius {radius} z {z} m {m} window {window}"
            want = f.run(mode, resolve, radius, z, m, window, 0.01)
            got = _call(r, mode, power=power, resolve=resolve, grid=grid, radius=radius, z=z, min_half_samples=m, window=window,
                        threshold=0.01, **d)
            _compare(r, got, want, w)
            seen.append(want)
    return seen


# ------------------------------------------------------------------ 1. bit for bit against the restatement
def test_cornell_every_plane_statistic_and_the_counter_bit_identical_to_the_restatement():
    """Cornell 48x40: not square, several 256-lane blocks, window tiles and 16 x 16 resolve tiles, partial ones both ways"""
    sc, cfg = _cornell(48, 40)
    r = _dealt(sc, cfg)
    assert r.counter("blend_resolved") == 0                    # before any such call
    feats = fl.features(sc, cfg)
    covs = {g: cl.coverage(sc, cfg, g, feats=feats) for g in (2, 4)}
    seen = _sweep(r, cfg, covs.get, "cornell 48x40")
    assert any(s.resolved > 0 for s in seen) and any((s.weight < 1).any() for s in seen) and any(s.stats[1] > 0 for s in seen)
    assert any(s.error is not None and (s.error > 0).any() for s in seen)
    ck.same(r.coverage, covs[4 if r.coverage[0, 0, 3] == 16 else 2], "the coverage plane after the calls")
    # the defaults of everything: 16 + 16 samples meet min_half_samples 16
    for mode in MODES:
        want = bc.blend_coverage(cfg, r.image_buffer, r.half_buffer, ck.feats(r), covs[4], mode=mode)
        _compare(r, _call(r, mode), want, f"defaults {mode}")
        assert want.resolved > 0 and want.stats[0] == 48 * 40
    ck.same(r.coverage, covs[4], "the coverage plane at the default grid")


def test_a_frame_smaller_than_any_window_tile_and_tap_footprint():
    """7x5: the window and the dilated taps leave the frame on every side, W * H is no multiple of 64"""
    sc, cfg = _cornell(7, 5)
    r = _dealt(sc, cfg)
    feats = fl.features(sc, cfg)
    covs = {g: cl.coverage(sc, cfg, g, feats=feats) for g in (2, 4)}
    _sweep(r, cfg, covs.get, "7x5", levels=(1, 2, 5), demodulates=(0, 1), covers=((4, 4), (8, 2)))
    _sweep(r, cfg, covs.get, "7x5 defaults", levels=(4,), demodulates=(0,), covers=((4, 4), (0, 4)), sig={})


def test_the_src_scene_with_sky_pixels_and_object_minus_1():
    """The src/ scene, persistent-ray form, 32x18: pixels of object -1 are taps of object -1 only and serve as second object -1"""
    W, H = 32, 18
    sc, cfg = src_scene(aspect=W / H), Config.src(W, H, 7, steps_per_launch=1)
    r = Renderer(sc, cfg)
    r.set_option("jit", 0)
    r.set_env(synthetic_env(192, 96, seed=0), 1.4, 2.2)
    for _ in range(2):
        r.sample(8)
        r.half_update()
    r.render_features()
    cov = cl.coverage(sc, cfg, 4)
    obj = r.feature_object
    assert (obj == -1).any() and (obj >= 0).any() and (cov[..., 1] == -1).any()
    usable = (r.half_buffer[..., 3] >= 1) & (r.image_buffer[..., 3] - r.half_buffer[..., 3] >= 1)
    assert usable.any()
    ib, a, feats = r.image_buffer, r.half_buffer, ck.feats(r)
    for d, power, resolve, m in ((dict(iterations=1), 4, 1, 1), (dict(iterations=3, demodulate=1, **SHARP), 8, 1, 1), (dict(), 4, 1, 2),
                                 (dict(iterations=2), 0, 0, 1), (dict(iterations=2, **SHARP), 4, 0, 1)):
        f = bc.Filtered(cfg, ib, a, feats, cov, power, **d)
        for mode, radius, window in (("levels", 3, 1), ("linear", 2, 3), ("display", 1, 1)):
            want = f.run(mode, resolve, radius, 0.0, m, window, 0.01)
            got = _call(r, mode, power=power, resolve=resolve, radius=radius, z=0.0, min_half_samples=m, window=window, threshold=0.01, **d)
            _compare(r, got, want, f"src {mode} {d} power {power} resolve {resolve} m {m}")
    ck.same(r.coverage, cov, "the coverage plane")


def test_a_frame_with_holes():
    """select_mask + sample_selected: a column next to nothing and one pixel stay without samples in all three buffers"""
    w, h = 33, 17
    sc, cfg = _cornell(w, h)
    r = Renderer(sc, cfg)
    r.set_option("jit", 0)
    holes = np.zeros((w, h), bool)
    holes[:, 3] = holes[5, 9] = holes[20:22, 8:11] = True
    r.select_mask((~holes).astype(np.uint8))
    r.refresh()
    for _ in range(2):
        r.sample_selected(8)
        r.half_update()
    r.render_features()
    a, b = r.half_buffer[..., 3], r.image_buffer[..., 3]
    assert np.all(a[~holes] == 8) and np.all(b[~holes] == 16) and np.all(b[holes] == 0) and np.all(a[holes] == 0)
    feats = fl.features(sc, cfg)
    cov = cl.coverage(sc, cfg, 4, feats=feats)
    assert (holes & (cov[..., 2] > 0)).any()                   # a hole on a silhouette
    for K, demodulate in ((1, 0), (3, 1), (4, 0)):
        for mode in MODES:
            d = dict(iterations=K, demodulate=demodulate)
            want = bc.blend_coverage(cfg, r.image_buffer, r.half_buffer, ck.feats(r), cov, mode=mode, radius=2, z=0.0, min_half_samples=8,
                                     window=2, **d)
            _compare(r, _call(r, mode, radius=2, z=0.0, min_half_samples=8, window=2, **d), want, f"holes {mode} {d}")
            assert want.resolved > 0 and np.all(want.weight[holes] == 1) and np.all(want.depth[holes] == K)
            r.post_process()
            ck.same(r.denoised_pixels[holes], r.image_pixels[holes], "pixels without samples")


# ------------------------------------------------------------------ 2. the identities, and who reads the option
def test_the_two_identities_on_the_device():
    sc, cfg = _cornell(48, 40)
    r = _dealt(sc, cfg)
    planes = lambda: [r.denoised_pixels, r.blend_weight, r.blend_depth]      # noqa: E731
    # power 0 without the resolve: every output of the option-off call
    for d in (dict(), dict(iterations=1, demodulate=1), dict(iterations=5, demodulate=1, **SHARP)):
        for radius, z, m in ((3, 2.0, 16), (1, 0.0, 8)):
            off = r.denoise_blend_levels(radius, z, m, **d)
            want = planes()
            on, resolved = r.denoise_blend_levels_coverage(0, 0, 4, radius, z, m, **d)
            for x, y, name in zip(planes(), want, ("denoised", "weight", "depth")):
                ck.same(x, y, f"power 0, no resolve: {name} {d}")
            assert resolved == 0 and bytes(on) == bytes(off)
            for bias in ("linear", "display"):
                off = r.blend_error(0.01, radius, z, m, 2, bias=bias, **d)
                want = planes() + [r.blend_error_map]
                on, resolved = r.blend_error_coverage(0.01, 0, 0, 2, radius, z, m, 2, bias=bias, **d)
                for x, y, name in zip(planes() + [r.blend_error_map], want, ("denoised", "weight", "depth", "error")):
                    ck.same(x, y, f"power 0, no resolve, {bias}: {name} {d}")
                assert resolved == 0 and bytes(on) == bytes(off)
    # no usable pixel: rtpbr_denoise_coverage's bytes, weight 1, depth K
    for p in (dict(), dict(iterations=1, demodulate=1, power=8, grid=2), dict(iterations=3, power=1, resolve=0, **SHARP)):
        cs = r.denoise_coverage(**p)
        want = r.denoised_pixels
        for mode in MODES:
            stats, resolved = _call(r, mode, radius=2, z=0.0, min_half_samples=NEVER, **p)
            ck.same(r.denoised_pixels, want, f"no usable pixel, {mode} {p}")
            assert np.all(r.blend_weight == 1) and np.all(r.blend_depth == p.get("iterations", 4)) and resolved == cs.pixels_estimated
            assert mode != "levels" or (stats.pixels_estimated, stats.pixels_above, stats.max_noise) == (0, 0, 0.0)


def test_no_level_does_not_read_the_option_and_an_option_off_call_afterwards_has_the_parents_bytes():
    sc, cfg = _cornell(48, 40)
    r = _dealt(sc, cfg)
    ib, a, feats = r.image_buffer, r.half_buffer, ck.feats(r)
    st, resolved = r.denoise_blend_levels_coverage(iterations=3, radius=2, z=0.0)
    assert resolved > 0
    on = r.denoised_pixels
    # iterations = 0: the bytes of option off; the counter keeps the last such call's value
    out, t, depth, want_st = lv.denoise_blend_levels(cfg, ib, a, feats, 2, 0.0, 16, iterations=0)
    st0, kept = r.denoise_blend_levels_coverage(iterations=0, radius=2, z=0.0, power=8, grid=2)
    ck.same(r.denoised_pixels, out, "no level: denoised")
    ck.same(r.blend_weight, t, "no level: weight")
    ck.same(r.blend_depth, depth, "no level: depth")
    ck.stats_same(st0, want_st, "no level")
    assert kept == resolved
    want = be.blend_error(cfg, ib, a, feats, 0.01, 2, 0.0, 16, 1, display=True, iterations=0)
    st0, kept = r.blend_error_coverage(0.01, radius=2, z=0.0, window=1, bias="display", iterations=0)
    ck.same(r.blend_error_map, want.error, "no level: the error plane")
    ck.stats_same(st0, want.stats, "no level, the error call")
    # the option is off again: the plain rule's bytes, as the restatement of the parent's call gives them
    for mode, display in (("levels", None), ("linear", False), ("display", True)):
        if mode == "levels":
            stats = r.denoise_blend_levels(2, 0.0, 16, iterations=3)
            want_out, want_t, want_d, want_st = lv.denoise_blend_levels(cfg, ib, a, feats, 2, 0.0, 16, iterations=3)
        else:
            stats = r.blend_error(0.01, 2, 0.0, 16, 1, bias=mode, iterations=3)
            w = be.blend_error(cfg, ib, a, feats, 0.01, 2, 0.0, 16, 1, display=display, iterations=3)
            want_out, want_t, want_d, want_st = w.denoised, w.weight, w.depth, w.stats
            ck.same(r.blend_error_map, w.error, f"option off after on, {mode}: the error plane")
        ck.same(r.denoised_pixels, want_out, f"option off after on, {mode}: denoised")
        ck.same(r.blend_weight, want_t, f"option off after on, {mode}: weight")
        ck.same(r.blend_depth, want_d, f"option off after on, {mode}: depth")
        ck.stats_same(stats, want_st, f"option off after on, {mode}")
        assert not np.array_equal(ck.bits(r.denoised_pixels), ck.bits(on))
    assert r.counter("blend_resolved") == resolved             # ... and the counter still describes the last such call
    r.denoise_coverage(iterations=3)                           # rtpbr_denoise_coverage's own count does not touch it
    assert r.counter("blend_resolved") == resolved


def test_every_other_display_call_ignores_the_option():
    sc, cfg = _cornell(48, 40)
    r = Renderer(sc, cfg)
    r.set_option("jit", 0)
    r.track_noise = r.track_halves = True
    for _ in range(2):
        r.sample(16)
    shots = {}
    for option in (0, 1, 0):
        r.set_option("blend_coverage", option)
        r.set_option("blend_coverage_power", 8 if option else 4)
        got = {}
        for name, call in (("denoise", lambda: r.denoise(iterations=3)), ("guided", lambda: r.denoise_guided(iterations=3)),
                           ("coverage", lambda: r.denoise_coverage(iterations=3)), ("error", lambda: r.denoise_error(iterations=3)),
                           ("blend", lambda: r.denoise_blend(iterations=3))):
            call()
            got[name] = r.denoised_pixels
        got["denoised_error"] = r.denoised_error
        got["blend weight of denoise_blend"] = r.blend_weight
        r.post_process()
        got["post_process"] = r.image_pixels
        r.present("pixels")
        got["present"] = r.presented
        for name, px in got.items():
            if name in shots:
                ck.same(px, shots[name], f"{name} with blend_coverage = {option}")
        shots.update(got)
    assert r.counter("blend_resolved") == 0                    # none of them is such a call
    # ... and the three calls do read it; denoise_fill and coverage_fill beside it change nothing in them
    r.denoise_blend_levels(iterations=3)
    off = r.denoised_pixels
    r.set_option("blend_coverage", 1)
    r.denoise_blend_levels(iterations=3)
    on = r.denoised_pixels
    assert not np.array_equal(ck.bits(on), ck.bits(off)) and r.counter("blend_resolved") > 0
    r.set_option("denoise_fill", 1)
    r.set_option("coverage_fill", 1)
    for call in (lambda: r.denoise_blend_levels(iterations=3), lambda: r.blend_error(iterations=3),
                 lambda: r.blend_error(iterations=3, bias="display")):
        call()
        ck.same(r.denoised_pixels, on, "the three calls write the same frame, with both fill options set")


def test_present_serves_the_new_frame():
    sc, cfg = _cornell(48, 40)
    r = _dealt(sc, cfg)
    r.denoise_blend_levels_coverage(radius=2, z=0.0)
    out = r.denoised_pixels
    r.present("denoised", "rgb8")
    shown = r.presented
    r.denoise_blend_levels(2, 0.0)
    assert not np.array_equal(ck.bits(r.denoised_pixels), ck.bits(out))
    r.present("denoised", "rgb8")
    assert not np.array_equal(shown, r.presented)
    r.denoise_blend_levels_coverage(radius=2, z=0.0)
    ck.same(r.denoised_pixels, out, "the same call again")
    r.present("denoised", "rgb8")
    assert np.array_equal(r.presented, shown)


# ------------------------------------------------------------------ 3. refusals
def test_refusals_leave_the_counter_the_option_and_the_frame_as_they_were():
    sc, cfg = _cornell(48, 40)
    r = _dealt(sc, cfg)
    st, resolved = r.denoise_blend_levels_coverage(iterations=2, radius=2, z=0.0)
    assert resolved > 0
    watched = lambda: [r.denoised_pixels, r.blend_weight, r.blend_depth, r.image_buffer, r.half_buffer]      # noqa: E731
    before = watched()
    for key, bad in (("blend_coverage", (-1, 2)), ("blend_coverage_grid", (1, 3, 5)), ("blend_coverage_power", (-1, 9)),
                     ("blend_coverage_resolve", (-1, 2))):
        for value in bad:
            assert ck.code(lambda: r.set_option(key, value)) == ck.EINVAL, (key, value)
    for bad in (dict(iterations=9), dict(iterations=-1), dict(demodulate=2), dict(sigma_color=0.0), dict(sigma_depth=float("nan")),
                dict(power=9), dict(power=-1), dict(resolve=2), dict(grid=3), dict(radius=0), dict(radius=4), dict(z=-1.0),
                dict(min_half_samples=0)):
        assert ck.code(lambda: r.denoise_blend_levels_coverage(**bad)) == ck.EINVAL, bad
        assert ck.code(lambda: r.blend_error_coverage(**bad)) == ck.EINVAL, bad
    for bad in (dict(window=0), dict(window=4), dict(threshold=-1.0)):
        assert ck.code(lambda: r.blend_error_coverage(**bad)) == ck.EINVAL, bad
    r.set_tiles(16, 16, 0, 2)
    for mode in MODES:
        assert ck.code(lambda: _call(r, mode)) == ck.ESTATE
    r.set_tiles(0, 0, 0, 1)
    assert r.counter("blend_resolved") == resolved
    for x, y in zip(watched(), before):
        ck.same(x, y, "a buffer after the refused calls")
    # the option was put back after every refusal: the plain rule's bytes
    r.denoise_blend_levels(2, 0.0, iterations=2)
    ck.same(r.denoised_pixels, lv.denoise_blend_levels(cfg, r.image_buffer, r.half_buffer, ck.feats(r), 2, 0.0, iterations=2)[0],
            "denoise_blend_levels after the refusals")
    # a new resolution frees the planes; the next such call makes them again
    cfg2 = cfg.copy(width=cfg.width + 4)
    r.set_config(cfg2)
    for _ in range(2):
        r.sample(16)
        r.half_update()
    feats2 = fl.features(sc, cfg2)
    want = bc.blend_coverage(cfg2, r.image_buffer, r.half_buffer, feats2, cl.coverage(sc, cfg2, 4, feats=feats2), iterations=2)
    _compare(r, r.denoise_blend_levels_coverage(iterations=2), want, "after a new resolution")


def test_grid_times_resolution_is_refused_in_denoise_coverages_words():
    """16384 x 2 at grid 4: 65536 sub-ray columns.  Nothing but the sample and the halves runs on this frame."""
    sc, cfg = _cornell(48, 40)
    cfg = cfg.copy(width=16384, height=2)
    r = Renderer(sc, cfg)
    r.set_option("jit", 0)
    for _ in range(2):
        r.sample(1)
        r.half_update()
    with pytest.raises(RtpbrError) as own:
        r.denoise_coverage(grid=4, iterations=1)
    assert own.value.code == ck.EINVAL and OUT_OF_RANGE in str(own.value)
    for mode in MODES:
        with pytest.raises(RtpbrError) as e:
            _call(r, mode, grid=4, iterations=1, min_half_samples=1)
        assert e.value.code == ck.EINVAL and str(e.value) == str(own.value), mode
    assert ck.code(lambda: r.blend_weight) == ck.ESTATE        # nothing was allocated on the way
    assert ck.code(lambda: _call(r, "levels", grid=4, radius=4)) == ck.EINVAL       # the calls' own checks come first ...
    with pytest.raises(RtpbrError) as e:
        r.denoise_blend_levels_coverage(grid=4, radius=4)
    assert OUT_OF_RANGE not in str(e.value)
    assert r.counter("blend_resolved") == 0


# ------------------------------------------------------------------ 4. the loop
@pytest.mark.parametrize("stop", ["filter", "blend"])
def test_render_adaptive_denoised_ends_with_the_new_calls_bytes(stop):
    w = h = 32
    sc, cfg = ck.scene("cornell_v3", w, h)
    r, s = Renderer(sc, cfg), Renderer(sc, cfg)
    for x in (r, s):
        x.set_option("jit", 0)
    args = (0.02, 40, 8, 1)
    cover = {"power": 8, "grid": 2}
    traced, stats = r.render_adaptive_denoised(*args, blend="levels", stop=stop, coverage=cover, iterations=3)
    assert traced >= 2 * 8 * w * h and r.counter("blend_resolved") > 0
    ib, a, feats = r.image_buffer, r.half_buffer, ck.feats(r)
    cov = cl.coverage(sc, cfg, 2)
    want = bc.blend_coverage(cfg, ib, a, feats, cov, mode="levels" if stop == "filter" else "linear", threshold=0.02, iterations=3,
                             power=cover["power"])
    ck.same(r.denoised_pixels, want.denoised, "denoised_pixels")
    ck.same(r.blend_weight, want.weight, "blend_weight")
    ck.same(r.blend_depth, want.depth, "blend_depth")
    if stop == "blend":
        ck.same(r.blend_error_map, want.error, "blend_error_map")
        ck.stats_same(stats, want.stats, "the last estimate")
    else:                                  # the stop rule is the plain loop's: the same samples
        traced_s, stats_s = s.render_adaptive_denoised(*args, blend="levels", iterations=3)
        assert traced == traced_s and stats.pixels_above == stats_s.pixels_above
        ck.same(ib, s.image_buffer, "image_buffer")
    with pytest.raises(ValueError):
        s.render_adaptive_denoised(*args, coverage=True)
    assert r.counter("blend_resolved") == want.resolved
    r.denoise_blend_levels(iterations=3)   # the option is off after the loop
    ck.same(r.denoised_pixels, lv.denoise_blend_levels(cfg, ib, a, feats, iterations=3)[0], "denoise_blend_levels after the loop")
