"""rtpbr_denoise with option denoise_fill = 1 on the GPU (atrous_level's FILL form), held bit for bit to the CPU restatement
(tests/fill_ref_lib.py, tests/fill_ref) with its three counters, plus the equalities with the option off, the calls that ignore the
option and the refusals of include/rtpbr.h."""
import itertools

import numpy as np
import pytest

import checks as ck
import feature_ref_lib as fl
import fill_ref_lib as fi
from raytracingpbr_amd import Camera, Config, Renderer, cornell_box, src_scene
from raytracingpbr_amd.ibl import synthetic_env

pytestmark = pytest.mark.gpu

SHARP = dict(sigma_color=0.5, sigma_normal=0.3, sigma_depth=0.05, sigma_albedo=0.1)      # sigmas at which every term of e matters
COUNTERS = ("fill_filled", "fill_empty", "fill_deepest")


def _cornell(w, h):
    return cornell_box("v3", aspect=w / h), Config.cornell_v3(w, h, 0, 3)


def _counters(r):
    return tuple(r.counter(k) for k in COUNTERS)


def _lattice_frame(r, period, phase, spp):
    """select_lattice + refresh + sample_selected: the sparse frame; (image_buffer, mask)"""
    cfg = r.config
    m = fi.lattice(cfg.width, cfg.height, period, phase)
    assert r.select_lattice(period, phase) == int(m.sum())
    r.refresh()
    r.sample_selected(spp)
    ib = r.image_buffer
    assert np.array_equal(ib[..., 3] > 0, m)
    return ib, m


def _check(r, cfg, ib, feats, what, **p):
    """one denoise_fill call against the restatement: the frame's bytes and the three counters"""
    before = _counters(r)
    got = r.denoise_fill(**p)
    want, counts = fi.denoise_fill(cfg, ib, feats, **p)
    ck.same(r.denoised_pixels, want, what)
    if p.get("iterations") == 0:           # no level: nothing is filled and the counters keep the last filling call's
        assert got == before, (what, got, before)
    else:
        assert got == counts, (what, got, counts)
    return counts


@pytest.mark.parametrize("period,phase", [((2, 2), (0, 0)), ((2, 2), (1, 1)), ((2, 2), (1, 0)), ((2, 2), (0, 1)), ((4, 4), (0, 0)), ((3, 2), (2, 0))])
def test_filled_frame_and_counters_bit_identical_to_the_restatement(period, phase):
    """Cornell 48x40: not square, several 256-lane blocks; iterations 0..5, both demodulate settings, sharp sigmas and the defaults"""
    sc, cfg = _cornell(48, 40)
    r = Renderer(sc, cfg)
    ib, m = _lattice_frame(r, period, phase, 4)
    feats = fl.features(sc, cfg)
    seen = set()
    for iterations, demodulate, sig in itertools.product(range(6), (0, 1), (SHARP, {})):
        seen.add(_check(r, cfg, ib, feats, f"{period} {phase} K={iterations} demodulate={demodulate} {sig}",
                        iterations=iterations, demodulate=demodulate, **sig))
    assert any(c[0] > 0 for c in seen)
    if period == (4, 4):
        assert any(c[2] > 0 for c in seen) and any(c[1] > 0 for c in seen)      # a deeper level filled something; one level leaves holes
    ck.same(r.image_buffer, ib, "image_buffer after the calls")


def test_a_frame_smaller_than_any_tap_footprint():
    sc, cfg = _cornell(7, 5)
    r = Renderer(sc, cfg)
    feats = fl.features(sc, cfg)
    for period, phase in (((2, 2), (1, 1)), ((4, 4), (0, 0)), ((8, 8), (6, 4))):
        ib, m = _lattice_frame(r, period, phase, 4)
        for iterations, demodulate in itertools.product((1, 2, 4), (0, 1)):
            _check(r, cfg, ib, feats, f"7x5 {period} K={iterations}", iterations=iterations, demodulate=demodulate, **SHARP)


def test_the_sky_is_filled_from_the_sky_only():
    """The src/ scene, persistent-ray form: sample_selected is refused there, so the sparse frame is a masked image_buffer written
    back.  Pixels of object -1 are filled from pixels of object -1: the restatement's rule, held bit for bit."""
    W, H = 32, 18
    sc, cfg = src_scene(aspect=W / H), Config.src(W, H, 7, steps_per_launch=1)
    r = Renderer(sc, cfg)
    r.set_env(synthetic_env(192, 96, seed=0), 1.4, 2.2)
    r.sample(8)
    full = r.image_buffer
    m = fi.lattice(W, H, (2, 2), (1, 0)) & (full[..., 3] > 0)
    ib = fi.masked(full, m)
    r.image_buffer = ib
    r.render_features()
    feats = ck.feats(r)
    sky = feats["object"] == -1
    assert (sky & ~m).any() and (sky & m).any() and (~sky & ~m).any()
    for p in (dict(iterations=1), dict(iterations=3, demodulate=1, **SHARP), dict()):
        counts = _check(r, cfg, ib, feats, f"src {p}", **p)
        assert counts == fi.reach(m, feats["object"], p.get("iterations", 4))[1]
    ck.same(r.image_buffer, ib, "image_buffer")


def test_the_holes_of_a_camera_move_are_filled():
    """Holes of arbitrary shape: sample, reproject to a moved camera, denoise_fill before any new sample — held to the restatement
    fed with the image_buffer and the features read back from the device."""
    sc, cfg = _cornell(48, 40)
    r = Renderer(sc, cfg)
    r.refresh()
    r.sample(4)
    cam = Camera(lookfrom=(6.0, 4.0, 33.0), lookat=(0.0, -1.0, 0.0), vup=(0, 1, 0), vfov=35.0, aspect=48 / 40, aperture=0.01, focus=4.0)
    r.reproject(cam)
    ib, feats = r.image_buffer, ck.feats(r)
    holes = int((ib[..., 3] == 0).sum())
    assert 0 < holes < 48 * 40
    for p in (dict(), dict(iterations=2, demodulate=1, **SHARP)):
        counts = _check(r, cfg, ib, feats, f"after reproject {p}", **p)
        assert counts[0] > 0 and counts[0] + counts[1] == holes


def test_sample_selected_on_a_lattice_traces_the_rays_sample_traces_there():
    sc, cfg = _cornell(48, 40)
    r = Renderer(sc, cfg)
    r.refresh()
    r.sample(2)
    dense = r.image_buffer
    for period, phase in (((2, 2), (1, 0)), ((4, 4), (3, 3))):
        r.set_option("sample_base", 0)     # (refresh keeps the sample index: the same two samples again)
        ib, m = _lattice_frame(r, period, phase, 2)
        ck.same(ib[m], dense[m], f"{period}: the lattice's pixels")
        assert not ib[~m].any()


def test_with_one_level_and_on_full_frames_the_option_changes_nothing_and_it_does_not_leak():
    sc, cfg = _cornell(48, 40)
    r = Renderer(sc, cfg)
    r.refresh()
    r.sample(4)
    c0 = ck.counters(r)
    for p in (dict(iterations=1), dict(iterations=4), dict(iterations=4, demodulate=1, **SHARP)):
        r.denoise(**p)
        den = r.denoised_pixels
        assert r.denoise_fill(**p) == (0, 0, 0)
        ck.same(r.denoised_pixels, den, f"a fully sampled frame, {p}")
    assert ck.counters(r) == c0
    ib, m = _lattice_frame(r, (2, 2), (0, 1), 4)
    for p in (dict(iterations=1), dict(iterations=1, demodulate=1, **SHARP)):
        r.denoise(**p)
        den = r.denoised_pixels
        filled, empty, deepest = r.denoise_fill(**p)
        out = r.denoised_pixels
        ck.same(out[m], den[m], f"one level, the sampled pixels, {p}")
        assert filled > 0 and filled + empty == int((~m).sum()) and deepest == 0
        assert not np.array_equal(ck.bits(out[~m]), ck.bits(den[~m]))
        r.denoise(**p)                     # the option is off again: the bytes denoise gave before
        ck.same(r.denoised_pixels, den, f"denoise after denoise_fill, {p}")
        assert _counters(r) == (filled, empty, deepest)      # ... and the counters still describe the filling call
    # present serves the filled frame
    r.denoise_fill()
    out = r.denoised_pixels
    r.present("denoised", "rgb8")
    shown = r.presented
    r.denoise()
    assert not np.array_equal(ck.bits(r.denoised_pixels), ck.bits(out))
    r.present("denoised", "rgb8")
    holes = r.presented
    assert not np.array_equal(shown, holes)
    r.denoise_fill()
    r.present("denoised", "rgb8")
    assert np.array_equal(r.presented, shown)


def test_the_other_display_calls_ignore_the_option():
    sc, cfg = _cornell(48, 40)
    r = Renderer(sc, cfg)
    r.track_noise = r.track_halves = True
    ib, m = _lattice_frame(r, (2, 2), (1, 1), 2)
    r.sample_selected(2)
    shots = {}
    for option in (0, 1, 0):
        r.set_option("denoise_fill", option)
        got = {}
        for name, call in (("guided", lambda: r.denoise_guided(iterations=3)), ("coverage", lambda: r.denoise_coverage(iterations=3)),
                           ("blend_levels", lambda: r.denoise_blend_levels(iterations=3)), ("blend", lambda: r.denoise_blend(iterations=3)),
                           ("error", lambda: r.denoise_error(iterations=3))):
            call()
            got[name] = r.denoised_pixels
        r.post_process()
        got["post_process"] = r.image_pixels
        r.present("pixels")
        got["present"] = r.presented
        for name, px in got.items():
            if name in shots:
                ck.same(px, shots[name], f"{name} with denoise_fill = {option}")
        shots.update(got)
    assert _counters(r) == (0, 0, 0)       # none of them is a filling call


def test_refusals_leave_the_counters_as_they_were():
    sc, cfg = _cornell(48, 40)
    r = Renderer(sc, cfg)
    assert _counters(r) == (0, 0, 0)       # before any filling call
    ib, m = _lattice_frame(r, (4, 4), (0, 0), 2)
    counts = r.denoise_fill(iterations=2)
    assert counts[0] > 0 and counts == fi.reach(m, fl.features(sc, cfg)["object"], 2)[1]
    den = r.denoised_pixels
    assert ck.code(lambda: r.counter("fill_nothing")) == ck.EINVAL
    assert ck.code(lambda: r.set_option("denoise_fill", 2)) == ck.EINVAL
    for bad in (dict(iterations=9), dict(iterations=-1), dict(demodulate=2), dict(sigma_color=0.0), dict(sigma_depth=float("nan"))):
        assert ck.code(lambda: r.denoise_fill(**bad)) == ck.EINVAL, bad
    r.set_tiles(16, 16, 0, 2)
    assert ck.code(lambda: r.denoise_fill()) == ck.ESTATE
    r.set_tiles(0, 0, 0, 1)
    assert _counters(r) == counts
    ck.same(r.denoised_pixels, den, "denoised after the refused calls")
    r.denoise(iterations=3)                # the option was put back after every refusal
    ck.same(r.denoised_pixels, fl.denoise(cfg, ib, fl.features(sc, cfg), iterations=3), "denoise after the refusals")
