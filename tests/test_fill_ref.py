"""CPU tier: the restatement of rtpbr_denoise with option denoise_fill = 1 (tests/fill_ref_lib.py, tests/fill_ref) that the GPU
tests hold the kernels to — known answers of the rule, its equalities with rtpbr_denoise, the reach rule against an independent
numpy computation, and the measurement of sparse lattice frames on the oracle."""
import numpy as np
import pytest

import checks as ck
import feature_ref_lib as fl
import fill_ref_lib as fi
from oracle_backend import OracleRenderer
from raytracingpbr_amd import Config, cornell_box

# ------------------------------------------------------------------ known answers
W0, H0 = 24, 16
L = np.array([[0.5, 0.25, 1.0], [2.0, 1.0, 0.5]], np.float32)      # the two objects' radiance: powers of two


def _two_objects():
    """Object 0 left of the middle, object 1 right of it, flat features, albedo 1/2; every pixel holds 4 samples of its object's
    radiance.  Every weight scales a power of two, so sx / sw is the radiance itself, bit for bit, whatever the weights are."""
    n = np.zeros((W0, H0, 3), np.float32)
    n[..., 2] = 1.0
    obj = np.zeros((W0, H0), np.int32)
    obj[W0 // 2:] = 1
    feats = {"albedo": np.full((W0, H0, 3), 0.5, np.float32), "normal": n, "depth": np.full((W0, H0), 3.0, np.float32), "object": obj}
    ib = np.empty((W0, H0, 4), np.float32)
    ib[..., :3] = L[obj] * np.float32(4)
    ib[..., 3] = 4
    return feats, ib, L[obj]


def _shown(cfg, linear, feats):
    """the configured tone map of a linear image, by the restatement of rtpbr_denoise's iterations = 0"""
    ib = np.concatenate([linear.astype(np.float32), np.ones(linear.shape[:2] + (1,), np.float32)], axis=2)
    return fl.denoise(cfg, ib, feats, iterations=0, demodulate=0)


@pytest.mark.parametrize("demodulate", [0, 1])
def test_a_hole_takes_exactly_its_own_objects_radiance_and_never_the_other_objects(demodulate):
    cfg = Config.cornell_v3(W0, H0, seed=0, max_raytrace=3)
    feats, ib, own = _two_objects()
    ib[3:5, 3:6] = 0.0                     # inside object 0
    ib[W0 // 2] = 0.0                      # object 1's whole border column: its nearest live pixels are object 0's
    ib[W0 // 2 - 1, 2:9] = 0.0             # ... and part of object 0's
    holes = int((ib[..., 3] == 0).sum())
    for iterations in (1, 3):
        out, counts = fi.denoise_fill(cfg, ib, feats, iterations=iterations, demodulate=demodulate)
        ck.same(out, _shown(cfg, own, feats), f"K={iterations}")
        assert counts == (holes, 0, 0)
    # with the option off the holes show what post_process shows
    den = fl.denoise(cfg, ib, feats, iterations=1, demodulate=demodulate)
    assert not np.array_equal(ck.bits(den), ck.bits(out))


def test_a_hole_out_of_reach_of_level_0_is_filled_at_level_1():
    """The centre of a 5x5 hole: none of its 25 taps at stride 1 is live; at stride 2 the taps at +-4 are."""
    cfg = Config.cornell_v3(W0, H0, seed=0, max_raytrace=3)
    feats, ib, own = _two_objects()
    ib[3:8, 5:10] = 0.0
    raw = fl.denoise(cfg, ib, feats, iterations=0, demodulate=0)
    out, counts = fi.denoise_fill(cfg, ib, feats, iterations=1)
    assert counts == (24, 1, 0)
    want = _shown(cfg, own, feats)
    want[5, 7] = raw[5, 7]                 # still empty after the only level: what post_process shows
    ck.same(out, want, "one level")
    out, counts = fi.denoise_fill(cfg, ib, feats, iterations=2)
    assert counts == (25, 0, 1)
    ck.same(out, _shown(cfg, own, feats), "two levels")
    # a hole that spans its object: object 1 has no live pixel at all, and object 0's never cross over
    ib[W0 // 2:] = 0.0
    out, counts = fi.denoise_fill(cfg, ib, feats, iterations=5)
    assert counts == (25, W0 // 2 * H0, 1)
    ck.same(out[W0 // 2:], fl.denoise(cfg, ib, feats, iterations=0, demodulate=0)[W0 // 2:], "an object without samples")


def test_a_frame_without_samples_comes_back_as_no_levels_show_it():
    cfg = Config.cornell_v3(W0, H0, seed=0, max_raytrace=3)
    feats, ib, _ = _two_objects()
    ib[:] = 0.0
    for demodulate in (0, 1):
        out, counts = fi.denoise_fill(cfg, ib, feats, iterations=4, demodulate=demodulate)
        ck.same(out, fl.denoise(cfg, ib, feats, iterations=0, demodulate=demodulate), "no samples")
        assert counts == (0, W0 * H0, 0)


# ------------------------------------------------------------------ the equalities with rtpbr_denoise
SHARP = dict(sigma_color=0.5, sigma_normal=0.3, sigma_depth=0.05, sigma_albedo=0.1)


@pytest.fixture(scope="module")
def cornell():
    W, H = 48, 40
    sc, cfg = cornell_box("v3", aspect=W / H), Config.cornell_v3(W, H, seed=0, max_raytrace=3)
    feats = fl.features(sc, cfg)
    o = OracleRenderer(sc, cfg)
    o.refresh()
    o.sample(4)
    ib = o.image_buffer
    o.close()
    return sc, cfg, feats, ib


def test_one_level_leaves_every_sampled_pixel_its_denoise_bytes(cornell):
    _, cfg, feats, ib = cornell
    for period, phase in (((2, 2), (1, 0)), ((4, 4), (3, 1)), ((3, 2), (0, 1))):
        m = fi.lattice(cfg.width, cfg.height, period, phase)
        sparse = fi.masked(ib, m)
        for p in (dict(), dict(demodulate=1, **SHARP)):
            out, counts = fi.denoise_fill(cfg, sparse, feats, iterations=1, **p)
            den = fl.denoise(cfg, sparse, feats, iterations=1, **p)
            ck.same(out[m], den[m], f"{period} {p}")
            assert counts[0] > 0 and not np.array_equal(ck.bits(out[~m]), ck.bits(den[~m]))


def test_a_fully_sampled_frame_has_denoise_bytes_at_every_depth(cornell):
    _, cfg, feats, ib = cornell
    for iterations in range(6):
        for p in (dict(), dict(demodulate=1, **SHARP)):
            out, counts = fi.denoise_fill(cfg, ib, feats, iterations=iterations, **p)
            ck.same(out, fl.denoise(cfg, ib, feats, iterations=iterations, **p), f"K={iterations} {p}")
            assert counts == (0, 0, 0)


def test_no_levels_is_denoise_with_no_levels(cornell):
    _, cfg, feats, ib = cornell
    m = fi.lattice(cfg.width, cfg.height, (2, 2), (0, 0))
    sparse = fi.masked(ib, m)
    for demodulate in (0, 1):
        out, counts = fi.denoise_fill(cfg, sparse, feats, iterations=0, demodulate=demodulate)
        ck.same(out, fl.denoise(cfg, sparse, feats, iterations=0, demodulate=demodulate), f"demodulate={demodulate}")
        assert counts == (0, int((~m).sum()), 0)


# ------------------------------------------------------------------ the reach rule
@pytest.mark.parametrize("period", [(2, 2), (4, 4)])
def test_a_pixel_is_filled_exactly_when_a_tap_of_the_level_is_live_on_its_object(cornell, period):
    """h >= 1/256 and exp_(-80) ~ 1.8e-35: every tap taken has a normal positive weight, so sw > 0 exactly when a tap was taken.
    The expected counts come from the live mask and the object plane alone (fill_ref_lib.reach), none of the filter's sums."""
    _, cfg, feats, ib = cornell
    m = fi.lattice(cfg.width, cfg.height, period, (period[0] - 1, 0))
    sparse = fi.masked(ib, m)
    raw = fl.denoise(cfg, sparse, feats, iterations=0, demodulate=0)
    for iterations in (1, 2, 4, 5):
        at, want = fi.reach(m, feats["object"], iterations)
        out, counts = fi.denoise_fill(cfg, sparse, feats, iterations=iterations, **SHARP)
        assert counts == want, (iterations, counts, want)
        assert counts[0] + counts[1] == int((~m).sum())
        ck.same(out[at == -2], raw[at == -2], f"never reached, K={iterations}")
        assert np.isfinite(out[at >= 0]).all()
    if period == (2, 2):
        assert want == (int((~m).sum()), 0, 0)      # every hole of the (2,2) lattice has a live neighbour on its object


# ------------------------------------------------------------------ the measurement
def test_filled_lattice_frames_beat_the_same_frames_shown_with_their_holes():
    """Cornell v3 at 64x64, seed 0, max_raytrace 4; 4 groups of samples with sample_base = g * 4096 at 1, 4 and 16 spp; truth: 1024
    spp at sample_base 2^20 shown with iterations = 0; score: RMSE of the display colour; a lattice frame is the full frame with the
    other pixels zeroed (what sample_selected leaves: tests/test_gpu_fill.py checks that on the device).  Asserted: in every group and
    at every sample count the filled (2,2) frame is closer to the truth than the same frame shown with its holes.  The table this
    restatement prints (means over the groups) is in DESIGN.md section 6q; cost in pixel-samples, N = W * H:
        1 spp dense, denoise N 0.1859 | 4 spp (2,2) filled N 0.1793 | 4 spp dense, denoise 4N 0.1118 | 16 spp (2,2) filled 4N 0.1068
        1 spp (2,2) filled N/4 0.2726 | (2,2) frames with their holes 0.3382 .. 0.3610 | (4,4): 16 spp filled N 0.2008, 36 of 4096
        pixels (0.88 %) still empty after four levels
    This measures the restatement, not the kernels."""
    W = H = 64
    sc, cfg = cornell_box("v3"), Config.cornell_v3(W, H, seed=0, max_raytrace=4)
    feats = fl.features(sc, cfg)
    m2, m4 = fi.lattice(W, H, (2, 2)), fi.lattice(W, H, (4, 4))
    shown = lambda ib: fl.denoise(cfg, ib, feats, iterations=0, demodulate=0).astype(np.float64)      # noqa: E731
    o = OracleRenderer(sc, cfg)
    o.refresh()
    o.set_sample_base(1 << 20)
    o.sample(1024)
    truth = shown(o.image_buffer)
    rmse = lambda px: float(np.sqrt(((px.astype(np.float64) - truth) ** 2).mean()))      # noqa: E731
    score, left = {}, None
    for g in range(4):
        o.refresh()
        o.set_sample_base(g * 4096)
        done = 0
        for spp in (1, 4, 16):
            o.sample(spp - done)
            done = spp
            ib = o.image_buffer
            score[("dense", spp, g)] = rmse(fl.denoise(cfg, ib, feats))
            score[("filled22", spp, g)] = rmse(fi.denoise_fill(cfg, fi.masked(ib, m2), feats)[0])
            score[("holes22", spp, g)] = rmse(fl.denoise(cfg, fi.masked(ib, m2), feats))
            out, counts = fi.denoise_fill(cfg, fi.masked(ib, m4), feats)
            score[("filled44", spp, g)], left = rmse(out), counts[1]
    o.close()
    mean = lambda who, spp: float(np.mean([score[(who, spp, g)] for g in range(4)]))      # noqa: E731
    for who in ("dense", "filled22", "holes22", "filled44"):
        print(who, {spp: round(mean(who, spp), 4) for spp in (1, 4, 16)}, "per group at 4 spp",
              [round(score[(who, 4, g)], 4) for g in range(4)])
    print("equal cost N: filled22@4 / dense@1 =", round(mean("filled22", 4) / mean("dense", 1), 3),
          "; 4N: filled22@16 / dense@4 =", round(mean("filled22", 16) / mean("dense", 4), 3))
    print(f"(4,4): {left} of {W * H} pixels still empty after four levels ({100.0 * left / (W * H):.2f} %)")
    for g in range(4):
        for spp in (1, 4, 16):
            assert score[("filled22", spp, g)] < score[("holes22", spp, g)], (g, spp, score[("filled22", spp, g)], score[("holes22", spp, g)])
