"""CPU tier: the restatement of rtpbr_denoise_blend_levels / rtpbr_blend_error / rtpbr_blend_error_display with option
blend_fill = 1 (tests/blend_fill_ref_lib.py, tests/blend_fill_ref) that the GPU tests hold the kernels to — known answers on a
hand-sized frame, the four identities of include/rtpbr.h with the restatements of the option-off calls (levels_ref_lib,
blend_error_ref_lib, blend_coverage_ref_lib) and of the two filling filters (fill_ref_lib, coverage_fill_ref_lib), bit for bit,
the reach of the levels, and the measurement behind the rule on the oracle."""
import numpy as np
import pytest

import blend_coverage_ref_lib as bc
import blend_error_ref_lib as be
import blend_fill_ref_lib as bf
import checks as ck
import coverage_fill_ref_lib as cf
import coverage_ref_lib as cl
import feature_ref_lib as fl
import fill_ref_lib as fi
import half_ref_lib as hl
import levels_ref_lib as lv
from oracle_backend import OracleRenderer
from raytracingpbr_amd import Config, cornell_box

SHARP = dict(sigma_color=0.5, sigma_normal=0.3, sigma_depth=0.05, sigma_albedo=0.1)      # sigmas at which every term of e matters
NEVER = 16777216                           # min_half_samples above every count: t_k = 1 everywhere
MODES = ("levels", "linear", "display")


def _lum(c):
    c = np.asarray(c, np.float32)
    return (np.float32(0.299) * c[..., 0] + np.float32(0.587) * c[..., 1]) + np.float32(0.114) * c[..., 2]


def _raw(cfg, ib, feats):
    """what post_process shows"""
    return fl.denoise(cfg, ib, feats, iterations=0, demodulate=0)


def _dealt_per_sample(o, hv, n):
    """n more samples, each dealt as a dealing sample call deals it: to the half with fewer samples, A on a tie"""
    for _ in range(n):
        o.sample(1)
        hv.update(o.image_buffer)


# ------------------------------------------------------------------ known answers
W0, H0 = 24, 16
L = np.array([[0.5, 0.25, 1.0], [2.0, 1.0, 0.5]], np.float32)      # the two objects' radiance: powers of two


def two_objects(count=8):
    """Object 0 left of the middle, object 1 right of it, flat features, albedo 1/2; the two columns at the border hold 12 of 16
    sub-rays on their own object and 4 on the other (a hand-made plane); every pixel holds ``count`` samples of its own object's
    radiance, half of them in A.  Every weight scales a power of two, so s / sw is the radiance itself, bit for bit, whatever the
    weights are: a filled pixel must show exactly its object's radiance, and the halves agree, so every t_k is 1."""
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
    ib[..., :3] = L[obj] * np.float32(count)
    ib[..., 3] = count
    mix = L[obj].copy()
    border = cov[..., 2] > 0
    mix[border] = ((np.float32(12) * L[obj] + np.float32(4) * L[1 - obj]) / np.float32(16))[border]
    return feats, cov, ib, L[obj], mix


def _shown(cfg, linear, feats):
    """the configured tone map of a linear image, by the restatement of rtpbr_denoise's iterations = 0"""
    ib = np.concatenate([linear.astype(np.float32), np.ones(linear.shape[:2] + (1,), np.float32)], axis=2)
    return fl.denoise(cfg, ib, feats, iterations=0, demodulate=0)


@pytest.mark.parametrize("demodulate", [0, 1])
def test_a_filled_pixel_shows_its_objects_radiance_with_weight_1_and_depth_K(demodulate):
    """Holes in the interior of both objects, one on either side of the border and a 5x5 block: on paper, every hole lies within two
    pixels of a sampled pixel of its object except the block's centre, which level 2 reaches: (filled, empty, deepest) = (n, 0, 1).
    Every pixel of the frame shows its object's radiance; with blend_coverage the border columns, filled ones included, show the
    (12 own + 4 other) / 16 mix."""
    cfg = Config.cornell_v3(W0, H0, seed=0, max_raytrace=3)
    feats, cov, ib, own, mix = two_objects()
    holes = np.zeros((W0, H0), bool)
    holes[W0 // 2 - 1, 5] = holes[W0 // 2, 9:11] = True
    holes[2:7, 3:8] = True
    holes[18, 2] = holes[20, 12] = True
    ib[holes] = 0.0
    a = ib * np.float32(0.5)
    n = int(holes.sum())
    for K in (2, 3):
        for mode in MODES:
            got = bf.blend_fill(cfg, ib, a, feats, mode=mode, iterations=K, demodulate=demodulate, radius=3, z=0.0, min_half_samples=4)
            ck.same(got.denoised, _shown(cfg, own, feats), f"{mode} K={K}")
            assert got.counts == (n, 0, 1) and got.resolved == 0
            assert np.all(got.weight == 1) and np.all(got.depth == K)
            assert got.stats[0] == W0 * H0 - n             # a filled pixel is usable in nobody's window, and is not estimated
            if mode != "levels":
                assert np.all(got.error == 0)
            got = bf.blend_fill(cfg, ib, a, feats, cov, mode=mode, iterations=K, demodulate=demodulate, radius=3, z=0.0, min_half_samples=4)
            ck.same(got.denoised, _shown(cfg, mix, feats), f"{mode} K={K}, blend_coverage")
            ck.same(got.before, _shown(cfg, own, feats), f"{mode} K={K}, blend_coverage, before the resolve")
            assert got.counts == (n, 0, 1) and got.resolved == 2 * H0
            assert np.all(got.weight == 1) and np.all(got.depth == K)
    # one level does not reach the block's centre: it stays what post_process shows, weight 1, depth 0
    got = bf.blend_fill(cfg, ib, a, feats, iterations=1, radius=3, z=0.0, min_half_samples=4)
    centre = np.zeros((W0, H0), bool)
    centre[4, 5] = True
    assert got.counts == (n - 1, 1, 0)
    ck.same(got.denoised[centre], _raw(cfg, ib, feats)[centre], "the centre of the block after one level")
    ck.same(got.denoised[~centre], _shown(cfg, own, feats)[~centre], "everybody else after one level")
    assert got.weight[4, 5] == 1 and got.depth[4, 5] == 0 and np.all(got.depth[~centre] == 1)


def test_an_object_without_any_sample_stays_empty_and_is_counted():
    """identity (d): object 1 has no sampled pixel; no level can fill it (a tap is on the centre's object), with and without
    blend_coverage, where its border column is nobody's second-object tap either"""
    cfg = Config.cornell_v3(W0, H0, seed=0, max_raytrace=3)
    feats, cov, ib, own, mix = two_objects()
    gone = feats["object"] == 1
    ib[gone] = 0.0
    ib[3, 3] = 0.0                         # and a hole that can be filled
    a = ib * np.float32(0.5)
    for mode in MODES:
        for c in (None, cov):
            got = bf.blend_fill(cfg, ib, a, feats, c, mode=mode, iterations=3, radius=2, z=0.0, min_half_samples=4)
            assert got.counts == (1, int(gone.sum()), 0)
            ck.same(got.denoised[gone], _raw(cfg, ib, feats)[gone], f"{mode}: the object without samples")
            ck.same(got.denoised[~gone], _shown(cfg, own, feats)[~gone], f"{mode}: the other object (nobody to resolve with)")
            assert np.all(got.weight == 1) and np.all(got.depth[gone] == 0) and np.all(got.depth[~gone] == 3) and got.resolved == 0


# ------------------------------------------------------------------ reach
def _one_object(W, H, live):
    n = np.zeros((W, H, 3), np.float32)
    n[..., 2] = 1.0
    feats = {"albedo": np.full((W, H, 3), 0.5, np.float32), "normal": n, "depth": np.full((W, H), 3.0, np.float32),
             "object": np.zeros((W, H), np.int32)}
    ib = np.zeros((W, H, 4), np.float32)
    ib[live] = (4.0, 2.0, 8.0, 8.0)
    return feats, ib


def test_a_7x7_hole_is_filled_at_level_2_and_a_hole_wider_than_three_levels_reach_keeps_its_centre():
    W, H = 32, 24
    cfg = Config.cornell_v3(W, H, seed=0, max_raytrace=3)
    live = np.ones((W, H), bool)
    live[10:17, 8:15] = False
    feats, ib = _one_object(W, H, live)
    a = ib * np.float32(0.5)
    for cov in (None, np.tile(np.array([16, -2, 0, 16], np.int32), (W, H, 1))):
        f = bf.Filtered(cfg, ib, a, feats, cov, iterations=3)
        at, counts = fi.reach(live, feats["object"], 3)
        assert f.counts == counts == (49, 0, 1)
        centre = np.zeros((W, H), bool)
        centre[12:15, 10:13] = True
        assert np.array_equal(f.live[0], live) and np.array_equal(f.live[1], ~centre) and f.live[2].all() and f.live[3].all()
        assert np.array_equal(f.live[1], (at == -1) | (at == 0))
        got = f.run("levels", radius=3, z=0.0, min_half_samples=4)
        assert np.all(got.depth == 3) and np.all(got.weight == 1)
    # one sampled column: level 1 reaches 2 pixels, level 2 four more, level 3 eight more
    live = np.zeros((W, H), bool)
    live[0] = True
    feats, ib = _one_object(W, H, live)
    a = ib * np.float32(0.5)
    f = bf.Filtered(cfg, ib, a, feats, iterations=3)
    at, counts = fi.reach(live, feats["object"], 3)
    assert f.counts == counts == (14 * H, 17 * H, 2)
    assert f.live[3][:15].all() and not f.live[3][15:].any()
    got = f.run("linear", radius=3, z=0.0, min_half_samples=4)
    ck.same(got.denoised[15:], _raw(cfg, ib, feats)[15:], "beyond three levels' reach")
    assert np.all(got.depth[:15] == 3) and np.all(got.depth[15:] == 0) and np.all(got.weight == 1) and np.all(got.error[1:] == 0)


# ------------------------------------------------------------------ the identities on a rendered frame
@pytest.fixture(scope="module")
def cornell():
    """Cornell 32x24, halves 4 + 4 dealt per sample"""
    W, H = 32, 24
    sc, cfg = cornell_box("v3", aspect=W / H), Config.cornell_v3(W, H, seed=0, max_raytrace=3)
    feats = fl.features(sc, cfg)
    o = OracleRenderer(sc, cfg)
    o.refresh()
    hv = hl.Halves(W, H)
    _dealt_per_sample(o, hv, 8)
    ib = o.image_buffer
    o.close()
    assert np.all(hv.a[..., 3] == 4) and np.all(ib[..., 3] == 8)
    return cfg, feats, ib, hv.a.copy(), cl.coverage(sc, cfg, 4, feats=feats)


def test_without_holes_the_option_changes_nothing(cornell):
    """identity (a): image_buffer and both halves have no empty pixel: ladders, frame, weight, depth, error plane and statistics
    are the option-off calls', with and without blend_coverage, in both bias modes"""
    cfg, feats, ib, a, cov = cornell
    for p in (dict(), dict(iterations=1, demodulate=1), dict(iterations=3, **SHARP)):
        plain, fill = lv.Filtered(cfg, ib, a, feats, **p), bf.Filtered(cfg, ib, a, feats, **p)
        cover, cfill = bc.Filtered(cfg, ib, a, feats, cov, **p), bf.Filtered(cfg, ib, a, feats, cov, **p)
        for x, y in ((fill, plain), (cfill, cover)):
            for name in ("fd", "fa", "fb"):
                ck.same(getattr(x, name), getattr(y, name), f"the ladder {name} {p}")
            assert x.counts == (0, 0, 0) and x.live.all() and x.live_a.all() and x.live_b.all()
        for radius, z, m, window in ((3, 2.0, 4, 1), (1, 0.0, 2, 3)):
            what = f"{p} radius {radius} z {z} m {m}"
            out, t, depth, st = plain.blend(radius, z, m)
            got = fill.run("levels", None, radius, z, m)
            for x, y, name in ((got.denoised, out, "denoised"), (got.weight, t, "weight"), (got.depth, depth, "depth")):
                ck.same(x, y, f"levels {name} {what}")
            assert got.stats == st
            assert z != 0.0 or (t < 1).any()                     # the rule was at work
            for mode in MODES[1:]:
                got = fill.run(mode, None, radius, z, m, window, 0.01)
                want = be.from_ladders(plain, 0.01, radius, z, m, window, display=mode == "display")
                for k in ("denoised", "weight", "depth", "error", "variance", "bias2", "slope"):
                    ck.same(getattr(got, k), getattr(want, k), f"{mode} {k} {what}")
                assert got.stats == want.stats
            for mode in MODES:
                got, want = cfill.run(mode, 1, radius, z, m, window, 0.01), cover.run(mode, 1, radius, z, m, window, 0.01)
                for k in ("denoised", "before", "weight", "depth") + (() if mode == "levels" else ("error", "variance", "bias2", "slope")):
                    ck.same(getattr(got, k), getattr(want, k), f"blend_coverage {mode} {k} {what}")
                assert got.stats == want.stats and got.resolved == want.resolved > 0


def _frames(cfg, feats, ib, a):
    """the sparse frames of the identities: name -> (image_buffer, half A, the pixels without samples)"""
    W, H = cfg.width, cfg.height
    out = {}
    m = fi.lattice(W, H, (2, 2))
    out["lattice"] = (fi.masked(ib, m), fi.masked(a, m), ~m)
    hole = np.zeros((W, H), bool)
    silhouette = np.argwhere(feats["object"][1:-1, 1:-1] != feats["object"][2:, 1:-1]) + 1
    x, y = (int(v) for v in silhouette[len(silhouette) // 2])
    hole[max(x - 4, 0):x + 5, max(y - 4, 0):y + 5] = True
    out["hole"] = (fi.masked(ib, ~hole), fi.masked(a, ~hole), hole)
    ids, n = np.unique(feats["object"], return_counts=True)
    gone = feats["object"] == ids[np.argmin(n)]
    out["object"] = (fi.masked(ib, ~gone & m), fi.masked(a, ~gone & m), ~(~gone & m))
    # one sample a pixel on the lattice: A = 1, B = 0 — half B's ladder is empty everywhere
    one = fi.masked(ib, m) * np.float32(0.125)
    out["one sample"] = (one, one.copy(), ~m)
    return out


def test_with_no_usable_pixel_the_frame_and_the_counters_are_the_filling_filters(cornell):
    """identity (b): min_half_samples above every count: every T is 1; the frame is rtpbr_denoise's with denoise_fill, under
    blend_coverage rtpbr_denoise_coverage's with coverage_fill, and so are the three counters"""
    cfg, feats, ib, a, cov = cornell
    for name, (sib, sa, empty) in _frames(cfg, feats, ib, a).items():
        for p in (dict(), dict(iterations=1, demodulate=1), dict(iterations=3, **SHARP)):
            K = p.get("iterations", 4)
            want, counts = fi.denoise_fill(cfg, sib, feats, **p)
            cwant, cst, ccounts = cf.denoise_coverage_fill(cfg, sib, feats, cov, **p)
            assert counts[0] > 0
            for mode in MODES:
                got = bf.blend_fill(cfg, sib, sa, feats, mode=mode, radius=2, z=0.0, min_half_samples=NEVER, **p)
                ck.same(got.denoised, want, f"{name} {mode} {p}")
                assert got.counts == counts and np.all(got.weight == 1)
                got = bf.blend_fill(cfg, sib, sa, feats, cov, mode=mode, radius=2, z=0.0, min_half_samples=NEVER, **p)
                ck.same(got.denoised, cwant, f"{name} blend_coverage {mode} {p}")
                assert got.counts == ccounts and got.resolved == cst[0] and np.all(got.weight == 1)
                assert set(np.unique(got.depth[empty])) <= {0.0, float(K)} and np.all(got.depth[~empty] == K)


def test_filled_and_unfillable_pixels_on_rendered_frames(cornell):
    """identities (c) and (d) with the rule at work (z = 0, min_half_samples 2): a pixel without samples that the whole ladder
    filled has weight 1 and depth K, one it did not reach shows post_process's colour with depth 0 and is counted in fill_empty;
    the pixels with samples still blend (some weight below 1), and the error calls estimate only them"""
    cfg, feats, ib, a, cov = cornell
    for name, (sib, sa, empty) in _frames(cfg, feats, ib, a).items():
        for c in (None, cov):
            f = bf.Filtered(cfg, sib, sa, feats, c, iterations=3, **SHARP)
            filled, still = empty & f.live[3], empty & ~f.live[3]
            assert f.counts[:2] == (int(filled.sum()), int(still.sum())) and filled.any()
            assert (name == "object") == bool(still.any())
            for mode in MODES:
                got = f.run(mode, radius=2, z=0.0, min_half_samples=2, window=2)
                assert np.all(got.weight[empty] == 1) and np.all(got.depth[filled] == 3) and np.all(got.depth[still] == 0)
                ck.same(got.before[still], _raw(cfg, sib, feats)[still], f"{name} {mode}: the pixels nobody reached")
                assert not np.array_equal(ck.bits(got.denoised[filled]), ck.bits(_raw(cfg, sib, feats)[filled]))
                assert name == "one sample" or (got.weight[~empty] < 1).any()
                if mode != "levels":
                    assert np.all(got.error[empty] == 0)
                    assert got.stats[0] == (0 if name == "one sample" else int((~empty).sum()))


# ------------------------------------------------------------------ the measurement behind the rule
def test_the_filling_blend_on_cornell_against_denoise_fill_and_the_blend_with_holes():
    """Cornell v3 at 64x64, seed 0, max_raytrace 4; 4 groups of samples with sample_base = g * 4096, halves dealt per sample; truth:
    1024 spp at sample_base 2^20 shown with iterations = 0; score: RMSE of the display colour over the groups, on the whole frame
    and on the pixels that had no samples.  Frames: the (2,2) lattice at 4 / 16 / 64 spp per traced pixel, and the frame right after
    the move of examples/sparse_preview.py (its 4 spp lattice frame, warped with warp on to the camera moved by (4, 1, 0); truth
    from the moved camera).  On each: rtpbr_denoise with denoise_fill, the option-off level blend (which shows the holes), and the
    new call at the blend's defaults (min_half_samples 16) and at min_half_samples 2.
    Asserted: on every lattice frame the new call's whole-frame RMSE is below the option-off level blend's — three pixels of four
    are black there.  Everything else is printed and recorded in DESIGN.md section 6t, worse rows included; no ratio is asserted.
    This measures the restatement, not the kernels."""
    import half_mode_ref_lib as hm
    from raytracingpbr_amd import Camera
    W = H = 64
    sc, cfg = cornell_box("v3"), Config.cornell_v3(W, H, seed=0, max_raytrace=4)
    c = sc.camera
    moved = Camera(lookfrom=(c.lookfrom[0] + 4.0, c.lookfrom[1] + 1.0, c.lookfrom[2]), lookat=tuple(c.lookat), vup=tuple(c.vup), vfov=c.vfov,
                   aspect=1.0, aperture=c.aperture, focus=c.focus)
    feats, feats_m = fl.features(sc, cfg), fl.features(sc, cfg, moved)
    m2 = fi.lattice(W, H, (2, 2))
    o = OracleRenderer(sc, cfg)
    truth = {}
    for name, cam, f in (("first", c, feats), ("moved", moved, feats_m)):
        o.set_camera(cam)
        o.refresh()
        o.set_sample_base(1 << 20)
        o.sample(1024)
        truth[name] = _raw(cfg, o.image_buffer, f).astype(np.float64)
    se = {}

    def rate(key, view, px, empty):
        e = (px.astype(np.float64) - truth[view]) ** 2
        se.setdefault(key + ("frame",), []).append(e.mean())
        se.setdefault(key + ("holes",), []).append(e[empty].mean())

    def all_of(frame, view, sib, sa, f):
        empty = sib[..., 3] == 0
        rate(("fill", frame), view, fi.denoise_fill(cfg, sib, f)[0], empty)
        rate(("off", frame), view, lv.denoise_blend_levels(cfg, sib, sa, f)[0], empty)
        ladders = bf.Filtered(cfg, sib, sa, f)
        rate(("new", frame), view, ladders.run("levels").denoised, empty)
        got = ladders.run("levels", min_half_samples=2)
        rate(("new m=2", frame), view, got.denoised, empty)
        return ladders.counts, int(empty.sum()), float((got.weight[~empty] < 1).mean())

    for g in range(4):
        o.set_camera(c)
        o.refresh()
        o.set_sample_base(g * 4096)
        hv = hl.Halves(W, H)
        done = 0
        for spp in (4, 16, 64):
            _dealt_per_sample(o, hv, spp - done)
            done = spp
            sib, sa = fi.masked(o.image_buffer, m2), fi.masked(hv.a, m2)
            info = all_of(spp, "first", sib, sa, feats)
            if spp == 4:
                wib, _, wa = hm.gather(cfg, sc, sc, c, moved, sib, sa, feats, feats_m)
                print(f"group {g}: after the move (counts, pixels without samples, share of sampled pixels with T < 1 at m = 2):",
                      all_of("moved", "moved", wib, wa, feats_m))
            print(f"group {g} lattice {spp} spp:", info)
    o.close()
    rmse = {k: float(np.sqrt(np.mean(v))) for k, v in se.items()}
    for s in ("frame", "holes"):
        for frame in (4, 16, 64, "moved"):
            x = {who: rmse[(who, frame, s)] for who in ("fill", "off", "new", "new m=2")}
            print(f"{s} {frame}: denoise_fill {x['fill']:.4f} blend with holes {x['off']:.4f} new {x['new']:.4f} new m=2 {x['new m=2']:.4f}; "
                  f"new / fill {x['new'] / x['fill']:.3f} new m=2 / fill {x['new m=2'] / x['fill']:.3f} new / holes {x['new'] / x['off']:.3f}")
    for frame in (4, 16, 64):
        assert rmse[("new", frame, "frame")] < rmse[("off", frame, "frame")], frame
