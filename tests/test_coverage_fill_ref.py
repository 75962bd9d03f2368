"""CPU tier: the restatement of rtpbr_denoise_coverage with option coverage_fill = 1 (tests/coverage_fill_ref_lib.py,
tests/coverage_fill_ref) that the GPU tests hold the kernels to — known answers of the rule, its equalities with the restatements of
rtpbr_denoise_coverage (coverage_ref_lib) and of the plain fill (fill_ref_lib), bit for bit, the counts against the reach rule at
power 0, and the precondition of the lattice cases: some pixel is both filled and resolved."""
import numpy as np
import pytest

import checks as ck
import coverage_fill_ref_lib as cf
import coverage_ref_lib as cl
import feature_ref_lib as fl
import fill_ref_lib as fi
from oracle_backend import OracleRenderer
from raytracingpbr_amd import Config, cornell_box

# ------------------------------------------------------------------ known answers
W0, H0 = 24, 16
L = np.array([[0.5, 0.25, 1.0], [2.0, 1.0, 0.5]], np.float32)      # the two objects' radiance: powers of two


def _two_objects():
    """Object 0 left of the middle, object 1 right of it, flat features, albedo 1/2; the two columns at the border are the
    candidates, each with 12 of 16 sub-rays on its own object and 4 on the other (a hand-made plane); every pixel holds 4 samples
    of its own object's radiance.  Every weight scales a power of two, so s / sw is the radiance itself, bit for bit, whatever the
    weights are — in the levels and in E2."""
    n = np.zeros((W0, H0, 3), np.float32)
    n[..., 2] = 1.0
    obj = np.zeros((W0, H0), np.int32)
    obj[W0 // 2:] = 1
    feats = {"albedo": np.full((W0, H0, 3), 0.5, np.float32), "normal": n, "depth": np.full((W0, H0), 3.0, np.float32), "object": obj}
    cov = np.empty((W0, H0, 4), np.int32)
    cov[:] = (16, -2, 0, 16)
    cov[W0 // 2 - 1] = (12, 1, 4, 16)
    cov[W0 // 2] = (12, 0, 4, 16)
    ib = np.empty((W0, H0, 4), np.float32)
    ib[..., :3] = L[obj] * np.float32(4)
    ib[..., 3] = 4
    # what a resolved border pixel holds: (12 L_own + 4 L_other) / 16, exact in f32
    mix = L[obj].copy()
    border = cov[..., 2] > 0
    mix[border] = ((np.float32(12) * L[obj] + np.float32(4) * L[1 - obj]) / np.float32(16))[border]
    return feats, cov, ib, L[obj], mix


def _shown(cfg, linear, feats):
    """the configured tone map of a linear image, by the restatement of rtpbr_denoise's iterations = 0"""
    ib = np.concatenate([linear.astype(np.float32), np.ones(linear.shape[:2] + (1,), np.float32)], axis=2)
    return fl.denoise(cfg, ib, feats, iterations=0, demodulate=0)


@pytest.mark.parametrize("demodulate", [0, 1])
@pytest.mark.parametrize("power", [0, 1, 4])
def test_a_hole_on_a_silhouette_takes_the_count_weighted_mix_of_the_two_objects(power, demodulate):
    """The hole at the border of object 0 is filled with object 0's radiance L0 (the weighted mean of pixels that all hold L0),
    its live neighbours on object 1 hold F = L1, and the resolve gives (12 L0 + 4 L1) / 16: exactly, as its sampled neighbours
    in the same column get.  A hole on object 1's side of the border and one in the interior ride along."""
    cfg = Config.cornell_v3(W0, H0, seed=0, max_raytrace=3)
    feats, cov, ib, own, mix = _two_objects()
    ib[W0 // 2 - 1, 5] = 0.0               # on the silhouette, object 0's side
    ib[W0 // 2, 9:11] = 0.0                # ... and object 1's
    ib[3:5, 3:6] = 0.0                     # interior
    holes = int((ib[..., 3] == 0).sum())
    for iterations in (1, 3):
        out, st, counts, both = cf.denoise_coverage_fill(cfg, ib, feats, cov, power=power, resolve=1, iterations=iterations,
                                                         demodulate=demodulate, both=True)
        ck.same(out, _shown(cfg, mix, feats), f"K={iterations}")
        assert counts == (holes, 0, 0) and both == 3
        assert st == (2 * H0, 2 * H0, 0.25)                      # every border pixel is resolved, the filled ones included
        # without the resolve a filled pixel shows its own object's radiance, and nobody is resolved
        out, st, counts = cf.denoise_coverage_fill(cfg, ib, feats, cov, power=power, resolve=0, iterations=iterations, demodulate=demodulate)
        ck.same(out, _shown(cfg, own, feats), f"K={iterations}, no resolve")
        assert counts == (holes, 0, 0) and st[0] == 0
    # with the option off the holes show what post_process shows and are nobody's E2 neighbour
    off, st_off = cl.denoise_coverage(cfg, ib, feats, cov, power=power, resolve=1, iterations=1, demodulate=demodulate)
    assert not np.array_equal(ck.bits(off), ck.bits(_shown(cfg, mix, feats))) and st_off[0] == 2 * H0 - 3


def test_a_hole_whose_only_live_neighbours_have_k_0_stays_empty_at_that_level():
    """The pixels around the hole (3, 3) hold no sub-ray of their own object: k = 0^power = 0 for power >= 1.  Every tap of level
    0 is live and on the hole's object, yet sw = 0: the hole stays empty — the reach rule of the plain fill would fill it.  Level
    1's taps at distance 4 have k = 1 and fill it; at power 0 every k is 1 and level 0 does."""
    cfg = Config.cornell_v3(W0, H0, seed=0, max_raytrace=3)
    feats, cov, ib, own, mix = _two_objects()
    cov[1:6, 1:6] = (0, 1, 16, 16)
    ib[3, 3] = 0.0
    raw = fl.denoise(cfg, ib, feats, iterations=0, demodulate=0)
    assert fi.reach(ib[..., 3] > 0, feats["object"], 1)[1] == (1, 0, 0)
    for power in (1, 4, 8):
        for resolve in (0, 1):             # (the k = 0 pixels name object 1 as their second: none of its pixels is next to them)
            out, st, counts = cf.denoise_coverage_fill(cfg, ib, feats, cov, power=power, resolve=resolve, iterations=1, demodulate=0)
            assert counts == (0, 1, 0)
            want = _shown(cfg, mix if resolve else own, feats)
            want[3, 3] = raw[3, 3]         # still empty: what post_process shows
            ck.same(out, want, f"power={power} resolve={resolve}, one level")
            out, st, counts = cf.denoise_coverage_fill(cfg, ib, feats, cov, power=power, resolve=resolve, iterations=2, demodulate=0)
            assert counts == (1, 0, 1)
            ck.same(out, _shown(cfg, mix if resolve else own, feats), f"power={power} resolve={resolve}, two levels")
    out, st, counts = cf.denoise_coverage_fill(cfg, ib, feats, cov, power=0, resolve=0, iterations=1, demodulate=0)
    assert counts == (1, 0, 0)
    ck.same(out, _shown(cfg, own, feats), "power 0")


def test_a_pixel_still_empty_is_nobodys_e2_neighbour_and_is_not_resolved():
    """Object 1 has no live pixel at all: none of its pixels is filled (taps never cross object indices), object 0's border pixels
    find no E2 neighbour and keep F, and nothing is resolved."""
    cfg = Config.cornell_v3(W0, H0, seed=0, max_raytrace=3)
    feats, cov, ib, own, mix = _two_objects()
    ib[W0 // 2:] = 0.0
    ib[4, 4] = 0.0
    out, st, counts = cf.denoise_coverage_fill(cfg, ib, feats, cov, iterations=3, demodulate=0)
    assert counts == (1, W0 // 2 * H0, 0) and st[0] == 0
    ck.same(out[:W0 // 2], _shown(cfg, own, feats)[:W0 // 2], "object 0")
    ck.same(out[W0 // 2:], fl.denoise(cfg, ib, feats, iterations=0, demodulate=0)[W0 // 2:], "object 1")


# ------------------------------------------------------------------ the equalities
SHARP = dict(sigma_color=0.5, sigma_normal=0.3, sigma_depth=0.05, sigma_albedo=0.1)
# the lattice frames of this file and of tests/test_gpu_coverage_fill.py
LATTICES = [((2, 2), (0, 0)), ((2, 2), (1, 1)), ((2, 2), (1, 0)), ((2, 2), (0, 1)), ((4, 4), (0, 0)), ((3, 2), (2, 0))]


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
    return sc, cfg, feats, ib, {g: cl.coverage(sc, cfg, g, feats=feats) for g in (2, 4)}


def test_a_frame_without_holes_has_denoise_coverage_bytes_and_statistics(cornell):
    _, cfg, feats, ib, covs = cornell
    for iterations in range(6):
        for p in (dict(), dict(demodulate=1, power=1, **SHARP), dict(power=8, resolve=0), dict(power=0, demodulate=1)):
            cov = covs[2 if p.get("power") == 1 else 4]
            out, st, counts = cf.denoise_coverage_fill(cfg, ib, feats, cov, iterations=iterations, **p)
            want, want_st = cl.denoise_coverage(cfg, ib, feats, cov, iterations=iterations, **p)
            ck.same(out, want, f"K={iterations} {p}")
            assert st == want_st and counts == (0, 0, 0), (iterations, p, st, want_st, counts)


@pytest.mark.parametrize("period,phase", LATTICES)
def test_power_0_without_resolve_is_the_plain_fill(cornell, period, phase):
    _, cfg, feats, ib, covs = cornell
    m = fi.lattice(cfg.width, cfg.height, period, phase)
    sparse = fi.masked(ib, m)
    for p in (dict(), dict(iterations=1, demodulate=1), dict(iterations=2, **SHARP), dict(iterations=5, demodulate=1, **SHARP), dict(iterations=0)):
        out, st, counts = cf.denoise_coverage_fill(cfg, sparse, feats, covs[4], power=0, resolve=0, **p)
        want, want_counts = fi.denoise_fill(cfg, sparse, feats, **p)
        ck.same(out, want, f"{period} {phase} {p}")
        assert counts == want_counts and st[0] == 0
        # ... and the counts are the reach rule's: k = 1 everywhere, every tap taken has a normal positive weight
        if p.get("iterations") != 0:
            assert counts == fi.reach(m, feats["object"], p.get("iterations", 4))[1]
    # with the resolve the counts are the same (the resolve fills nobody) and the bytes are not
    out, st, counts = cf.denoise_coverage_fill(cfg, sparse, feats, covs[4], power=0, resolve=1)
    assert counts == fi.reach(m, feats["object"], 4)[1] and st[0] > 0
    assert not np.array_equal(ck.bits(out), ck.bits(fi.denoise_fill(cfg, sparse, feats)[0]))


@pytest.mark.parametrize("period,phase", LATTICES)
def test_one_level_without_resolve_leaves_every_sampled_pixel_its_option_off_bytes(cornell, period, phase):
    _, cfg, feats, ib, covs = cornell
    m = fi.lattice(cfg.width, cfg.height, period, phase)
    sparse = fi.masked(ib, m)
    for p in (dict(), dict(power=1, demodulate=1, **SHARP), dict(power=8)):
        out, st, counts = cf.denoise_coverage_fill(cfg, sparse, feats, covs[4], resolve=0, iterations=1, **p)
        off = cl.denoise_coverage(cfg, sparse, feats, covs[4], resolve=0, iterations=1, **p)[0]
        ck.same(out[m], off[m], f"{period} {phase} {p}")
        assert counts[0] > 0 and counts[0] + counts[1] == int((~m).sum()) and counts[2] == 0
        assert not np.array_equal(ck.bits(out[~m]), ck.bits(off[~m]))


@pytest.mark.parametrize("period,phase", LATTICES)
def test_precondition_some_pixel_is_both_filled_and_resolved(cornell, period, phase):
    """What makes the lattice cases of the GPU tier cases of the composition: at the defaults, on each of their frames, at both
    grids.  Reported beside how the counts differ from the reach rule's (k = 0 taps, underflow)."""
    _, cfg, feats, ib, covs = cornell
    m = fi.lattice(cfg.width, cfg.height, period, phase)
    sparse = fi.masked(ib, m)
    for g in (2, 4):
        for p in (dict(), dict(power=8)):
            out, st, counts, both = cf.denoise_coverage_fill(cfg, sparse, feats, covs[g], both=True, **p)
            print(f"{period} {phase} grid {g} {p}: counts {counts} (reach rule {fi.reach(m, feats['object'], 4)[1]}), resolved {st[0]}, "
                  f"filled and resolved {both}")
            assert both >= 1 and counts[0] > 0
            assert counts[0] + counts[1] == int((~m).sum())
            reach = fi.reach(m, feats["object"], 4)[1]
            assert counts[0] <= reach[0]                         # the weights can only refuse what reach allows


# ------------------------------------------------------------------ the measurement
def test_coverage_filled_frames_beat_the_same_frames_shown_with_their_holes():
    """Section 6q's set-up: Cornell v3 at 64x64, seed 0, max_raytrace 4; 4 groups of samples with sample_base = g * 4096; truth: 1024
    spp at sample_base 2^20 shown with iterations = 0; score: RMSE of the display colour on the whole frame and on the pixels with
    coverage below 1 (grid 4).  Frames: the (2,2) lattice at 1, 4 and 16 spp (the full frame with the other pixels zeroed), and the
    frame examples/sparse_preview.py shows after its move (4 spp on every pixel, then the restatement of rtpbr_reproject to the
    camera moved by (4, 1, 0); truth from the moved camera).  Three things on each: the plain fill (fill_ref_lib), coverage_fill at
    the defaults, and — lattice frames only — denoise_coverage on every pixel at the same number of samples.  Asserted: in every
    group, on every one of these frames, the coverage-filled frame is closer to the truth than the same frame shown by
    denoise_coverage with its holes, on the whole frame.  Everything else is printed, and recorded in DESIGN.md section 6r; nothing
    of it is asserted.  What this restatement prints (means over the groups; plain fill / coverage fill / with holes):
        whole frame, lattice 1 spp 0.2726 / 0.2717 / 0.3613 | 4 spp 0.1793 / 0.1784 / 0.3459 | 16 spp 0.1068 / 0.1030 / 0.3383 |
        after the move 0.1196 / 0.1170 / 0.1217 (300 holes, 40 of them with coverage below 1, all filled, those 40 resolved)
        coverage below 1 (284 px; 308 after the move): 0.2950 / 0.2734 / 0.4154 | 0.2137 / 0.1923 / 0.3986 | 0.1708 / 0.1435 / 0.3920 |
        0.1714 / 0.1528 / 0.2158; coverage fill / plain fill there 0.927 / 0.900 / 0.840 / 0.891, below 1 in every group
        equal cost against dense denoise_coverage: whole frame 0.975 (4 spp lattice : 1 spp) and 0.949 (16 : 4), coverage below 1
        0.988 and 1.000 (plain fill: 1.098 and 1.191)
    The asserted margin per group: 4 spp 0.166-0.194 against 0.344-0.348; after the move 0.104-0.125 against 0.114-0.126.
    This measures the restatement, not the kernels."""
    import reproject_ref_lib as rr
    from raytracingpbr_amd import Camera
    W = H = 64
    sc, cfg = cornell_box("v3"), Config.cornell_v3(W, H, seed=0, max_raytrace=4)
    c = sc.camera
    moved = Camera(lookfrom=(c.lookfrom[0] + 4.0, c.lookfrom[1] + 1.0, c.lookfrom[2]), lookat=tuple(c.lookat), vup=tuple(c.vup), vfov=c.vfov,
                   aspect=1.0, aperture=c.aperture, focus=c.focus)
    views = {}
    for name, cam in (("first", None), ("moved", moved)):
        feats = fl.features(sc, cfg, cam)
        cov = cl.coverage(sc, cfg, 4, cam, feats=feats)
        views[name] = (feats, cov, cov[..., 0] < cov[..., 3])
    m2 = fi.lattice(W, H, (2, 2))
    o = OracleRenderer(sc, cfg)
    truth = {}
    for name, cam in (("first", c), ("moved", moved)):
        o.set_camera(cam)
        o.refresh()
        o.set_sample_base(1 << 20)
        o.sample(1024)
        truth[name] = fl.denoise(cfg, o.image_buffer, views[name][0], iterations=0, demodulate=0).astype(np.float64)
    score = {}

    def rate(key, view, px):
        se = (px.astype(np.float64) - truth[view]) ** 2
        score[key + ("frame",)] = float(np.sqrt(se.mean()))
        score[key + ("edge",)] = float(np.sqrt(se[views[view][2]].mean()))

    for g in range(4):
        o.set_camera(c)
        o.refresh()
        o.set_sample_base(g * 4096)
        done = 0
        feats, cov, _ = views["first"]
        for spp in (1, 4, 16):
            o.sample(spp - done)
            done = spp
            ib = o.image_buffer
            sparse = fi.masked(ib, m2)
            rate(("dense", spp, g), "first", cl.denoise_coverage(cfg, ib, feats, cov)[0])
            rate(("plain", spp, g), "first", fi.denoise_fill(cfg, sparse, feats)[0])
            rate(("cover", spp, g), "first", cf.denoise_coverage_fill(cfg, sparse, feats, cov)[0])
            rate(("holes", spp, g), "first", cl.denoise_coverage(cfg, sparse, feats, cov)[0])
            if spp == 4:
                ib4 = ib.copy()
        # the move: 4 spp on every pixel, warped to the moved camera; nothing new is sampled
        feats_m, cov_m, _ = views["moved"]
        warped = rr.reproject(cfg, c, moved, ib4, feats, feats_m)[0]
        holes = int((warped[..., 3] == 0).sum())
        out, st, counts, both = cf.denoise_coverage_fill(cfg, warped, feats_m, cov_m, both=True)
        rate(("cover", "moved", g), "moved", out)
        rate(("plain", "moved", g), "moved", fi.denoise_fill(cfg, warped, feats_m)[0])
        rate(("holes", "moved", g), "moved", cl.denoise_coverage(cfg, warped, feats_m, cov_m)[0])
        print(f"group {g}: the move leaves {holes} holes, {int((views['moved'][2] & (warped[..., 3] == 0)).sum())} of them with coverage below 1; "
              f"coverage fill: counts {counts}, filled and resolved {both}")
    o.close()
    mean = lambda who, f, s: float(np.mean([score[(who, f, g, s)] for g in range(4)]))      # noqa: E731
    print(f"pixels with coverage below 1: first view {int(views['first'][2].sum())}, moved view {int(views['moved'][2].sum())} of {W * H}")
    for s in ("frame", "edge"):
        for f in (1, 4, 16, "moved"):
            row = {who: round(mean(who, f, s), 4) for who in ("plain", "cover", "holes")}
            print(s, f, row, "cover / plain =", round(row["cover"] / row["plain"], 3), "per group",
                  [round(score[("cover", f, g, s)] / score[("plain", f, g, s)], 3) for g in range(4)])
        for lat, dense in ((4, 1), (16, 4)):
            print(s, f"equal cost: cover@{lat} on the lattice / dense denoise_coverage@{dense} =",
                  round(mean("cover", lat, s) / mean("dense", dense, s), 3), f"(dense {round(mean('dense', dense, s), 4)});",
                  "plain / dense =", round(mean("plain", lat, s) / mean("dense", dense, s), 3))
    for s in ("frame", "edge"):
        for f in (1, 4, 16, "moved"):
            print(s, f, "cover per group", [round(score[("cover", f, g, s)], 4) for g in range(4)], "holes per group",
                  [round(score[("holes", f, g, s)], 4) for g in range(4)])
    for g in range(4):
        for f in (1, 4, 16, "moved"):
            assert score[("cover", f, g, "frame")] < score[("holes", f, g, "frame")], (g, f)
