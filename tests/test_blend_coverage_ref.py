"""CPU tier: the restatement of rtpbr_denoise_blend_levels / rtpbr_blend_error / rtpbr_blend_error_display with option
blend_coverage = 1 (tests/blend_coverage_ref_lib.py, tests/blend_coverage_ref) that the GPU tests hold the kernels to — its two
identities with the restatements of the option-off calls (levels_ref_lib, blend_error_ref_lib) and of rtpbr_denoise_coverage
(coverage_ref_lib), bit for bit, known answers of the rule, and the measurement behind it on the oracle."""
import numpy as np
import pytest

import blend_coverage_ref_lib as bc
import blend_error_ref_lib as be
import checks as ck
import coverage_ref_lib as cl
import feature_ref_lib as fl
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


# ------------------------------------------------------------------ the two identities
@pytest.fixture(scope="module")
def cornell():
    """Cornell 48x40, halves 16 + 16 dealt by the rule from two equal batches"""
    W, H = 48, 40
    sc, cfg = cornell_box("v3", aspect=W / H), Config.cornell_v3(W, H, seed=0, max_raytrace=3)
    feats = fl.features(sc, cfg)
    o = OracleRenderer(sc, cfg)
    o.refresh()
    hv = hl.Halves(W, H)
    for _ in range(2):
        o.sample(16)
        hv.update(o.image_buffer)
    ib = o.image_buffer
    o.close()
    assert np.all(hv.a[..., 3] == 16) and np.all(ib[..., 3] == 32)
    return cfg, feats, ib, hv.a, {g: cl.coverage(sc, cfg, g, feats=feats) for g in (2, 4)}


def test_power_0_without_the_resolve_is_the_option_off_call(cornell):
    """every k is 1.0f and nothing is resolved: every output of the three calls equals the plain ladders', bit for bit"""
    cfg, feats, ib, a, covs = cornell
    for p in (dict(), dict(iterations=1, demodulate=1), dict(iterations=2, **SHARP), dict(iterations=5, demodulate=1, **SHARP)):
        plain = lv.Filtered(cfg, ib, a, feats, **p)
        cover = bc.Filtered(cfg, ib, a, feats, covs[4], power=0, **p)
        for x, y, name in ((cover.fd, plain.fd, "fd"), (cover.fa, plain.fa, "fa"), (cover.fb, plain.fb, "fb")):
            ck.same(x, y, f"the ladder {name} {p}")
        for radius, z, m, window in ((3, 2.0, 16, 1), (1, 0.0, 8, 3), (2, 0.0, 16, 2)):
            what = f"{p} radius {radius} z {z} m {m}"
            got = cover.run("levels", 0, radius, z, m)
            out, t, depth, st = plain.blend(radius, z, m)
            ck.same(got.denoised, out, "denoised " + what)
            ck.same(got.before, out, "before " + what)
            ck.same(got.weight, t, "weight " + what)
            ck.same(got.depth, depth, "depth " + what)
            assert got.stats == st and got.resolved == 0
            assert z != 0.0 or (t < 1).any()                     # the rule was at work
            for mode in MODES[1:]:
                got = cover.run(mode, 0, radius, z, m, window, 0.01)
                want = be.from_ladders(plain, 0.01, radius, z, m, window, display=mode == "display")
                for k in ("denoised", "weight", "depth", "error", "variance", "bias2", "slope"):
                    ck.same(getattr(got, k), getattr(want, k), f"{mode} {k} {what}")
                assert got.stats == want.stats and got.resolved == 0
    # ... and with either of the two the bytes are others
    plain = lv.Filtered(cfg, ib, a, feats).blend(3, 0.0, 16)[0]
    for power, resolve in ((0, 1), (4, 0)):
        got = bc.blend_coverage(cfg, ib, a, feats, covs[4], power=power, resolve=resolve, radius=3, z=0.0, min_half_samples=16)
        assert not np.array_equal(ck.bits(got.denoised), ck.bits(plain)) and (got.resolved > 0) == bool(resolve)


def test_with_no_usable_pixel_the_frame_is_denoise_coverages(cornell):
    """min_half_samples above every count: every T is 1, the frame is rtpbr_denoise_coverage's with the same parameters, weight 1
    and depth K — in all three calls, whose error plane then is the two-half estimate of that frame before the resolve"""
    cfg, feats, ib, a, covs = cornell
    for p in (dict(), dict(iterations=1, demodulate=1, power=8), dict(iterations=3, power=1, resolve=0, **SHARP),
              dict(iterations=2, power=0), dict(iterations=5, demodulate=1, power=4, resolve=1, **SHARP)):
        for g in (2, 4):
            want, want_st = cl.denoise_coverage(cfg, ib, feats, covs[g], **p)
            for mode in MODES:
                got = bc.blend_coverage(cfg, ib, a, feats, covs[g], mode=mode, radius=2, z=0.0, min_half_samples=NEVER, **p)
                ck.same(got.denoised, want, f"{mode} grid {g} {p}")
                assert np.all(got.weight == 1) and np.all(got.depth == p.get("iterations", 4)) and got.resolved == want_st[0]
                if mode == "levels":
                    assert got.stats == (0, 0, 0.0)
                else:
                    assert got.stats[0] == cfg.width * cfg.height and np.all(got.bias2 == 0)
            assert p.get("resolve") == 0 or want_st[0] > 0


# ------------------------------------------------------------------ known answers
W0, H0 = 24, 16
L = np.array([[0.5, 0.25, 1.0], [2.0, 1.0, 0.5]], np.float32)      # the two objects' radiance: powers of two


def two_objects(count=32):
    """Object 0 left of the middle, object 1 right of it, flat features, albedo 1/2; the two columns at the border are the
    candidates, each with 12 of 16 sub-rays on its own object and 4 on the other (a hand-made plane); every pixel holds ``count``
    samples of its own object's radiance, half of them in A.  Every weight scales a power of two, so s / sw is the radiance
    itself, bit for bit, whatever the weights are — in the levels of all three chains and in the resolve."""
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
    # what a resolved border pixel holds: (12 L_own + 4 L_other) / 16, exact in f32
    mix = L[obj].copy()
    border = cov[..., 2] > 0
    mix[border] = ((np.float32(12) * L[obj] + np.float32(4) * L[1 - obj]) / np.float32(16))[border]
    return feats, cov, ib, ib * np.float32(0.5), L[obj], mix


def _shown(cfg, linear, feats):
    """the configured tone map of a linear image, by the restatement of rtpbr_denoise's iterations = 0"""
    ib = np.concatenate([linear.astype(np.float32), np.ones(linear.shape[:2] + (1,), np.float32)], axis=2)
    return fl.denoise(cfg, ib, feats, iterations=0, demodulate=0)


@pytest.mark.parametrize("demodulate", [0, 1])
@pytest.mark.parametrize("power", [0, 1, 4])
def test_a_two_object_pixel_resolves_to_the_count_weighted_mix(power, demodulate):
    cfg = Config.cornell_v3(W0, H0, seed=0, max_raytrace=3)
    feats, cov, ib, a, own, mix = two_objects()
    for iterations in (1, 3):
        for mode in MODES:
            got = bc.blend_coverage(cfg, ib, a, feats, cov, mode=mode, power=power, resolve=1, iterations=iterations, demodulate=demodulate,
                                    radius=3, z=0.0, min_half_samples=16)
            ck.same(got.denoised, _shown(cfg, mix, feats), f"{mode} K={iterations}")
            ck.same(got.before, _shown(cfg, own, feats), f"{mode} K={iterations}, before the resolve")
            assert got.resolved == 2 * H0 and np.all(got.weight == 1) and np.all(got.depth == iterations)
            if mode != "levels":           # the halves agree and no level moves a pixel: no error is seen, before the resolve
                assert np.all(got.error == 0) and got.stats == (W0 * H0, 0, 0.0)
            got = bc.blend_coverage(cfg, ib, a, feats, cov, mode=mode, power=power, resolve=0, iterations=iterations, demodulate=demodulate,
                                    radius=3, z=0.0, min_half_samples=16)
            ck.same(got.denoised, _shown(cfg, own, feats), f"{mode} K={iterations}, no resolve")
            assert got.resolved == 0


def test_a_tap_of_share_0_weighs_nothing():
    """The pixel (4, 4) holds another radiance and no sub-ray of its own object: k = 0^power = 0 for power >= 1.  It is a tap of
    every pixel around it in all three chains, and none of them moves: every other pixel shows exactly what it shows without the
    outlier.  At power 0 the filter pulls its neighbours."""
    cfg = Config.cornell_v3(W0, H0, seed=0, max_raytrace=3)
    feats, cov, ib, a, own, mix = two_objects()
    cov[4, 4] = (0, 1, 16, 16)             # (its second object has no pixel next to it: not resolved)
    ib[4, 4, :3] = np.float32(8.0) * np.float32(32)
    a = ib * np.float32(0.5)
    others = np.ones((W0, H0), bool)
    others[4, 4] = False
    want = _shown(cfg, mix, feats)
    for power in (1, 4, 8):
        for mode in MODES:
            for m in (16, NEVER):          # (NEVER: every level is kept, so the frame is the filter's last level itself)
                got = bc.blend_coverage(cfg, ib, a, feats, cov, mode=mode, power=power, iterations=3, radius=3, z=0.0, min_half_samples=m)
                ck.same(got.denoised[others], want[others], f"{mode} power {power} m {m}")
                assert got.resolved == 2 * H0
    got = bc.blend_coverage(cfg, ib, a, feats, cov, power=0, iterations=3, radius=3, z=0.0, min_half_samples=NEVER)
    assert not np.array_equal(ck.bits(got.denoised[others]), ck.bits(want[others]))


def test_a_pixel_without_samples_shows_what_post_process_shows_and_is_nobodys_tap():
    """Holes in the interior and on either side of the silhouette: each shows the tone map of its own (0, 0, 0, 0), has weight 1
    and depth K, is not resolved, and neither the levels nor the resolve of its neighbours read it — the pixel across the border
    still gets the exact mix from its other neighbours."""
    cfg = Config.cornell_v3(W0, H0, seed=0, max_raytrace=3)
    feats, cov, ib, a, own, mix = two_objects()
    holes = np.zeros((W0, H0), bool)
    holes[W0 // 2 - 1, 5] = holes[W0 // 2, 9:11] = True
    holes[3:5, 3:6] = True
    ib[holes] = 0.0
    a = ib * np.float32(0.5)
    raw = fl.denoise(cfg, ib, feats, iterations=0, demodulate=0)
    for mode in MODES:
        for K in (1, 3):
            got = bc.blend_coverage(cfg, ib, a, feats, cov, mode=mode, iterations=K, radius=3, z=0.0, min_half_samples=16)
            ck.same(got.denoised[holes], raw[holes], f"{mode} K={K}: the holes")
            ck.same(got.denoised[~holes], _shown(cfg, mix, feats)[~holes], f"{mode} K={K}: everybody else")
            assert got.resolved == 2 * H0 - 3 and np.all(got.weight[holes] == 1) and np.all(got.depth[holes] == K)
            assert got.stats[0] == W0 * H0 - int(holes.sum())
            if mode != "levels":
                assert np.all(got.error[holes] == 0)


# ------------------------------------------------------------------ the measurement behind the rule
def test_the_coverage_aware_blend_beats_the_level_blend_on_cornell():
    """Cornell v3 at 64x64, seed 0, max_raytrace 4; 4 groups of samples with sample_base = g * 4096, halves 16+16 / 64+64 / 256+256
    dealt by the rule itself from two equal batches; truth: 2048 spp at sample_base 2^20 shown with iterations = 0; every
    default (4 levels, blend radius 3 / z 2 / min_half_samples 16, grid 4, power 4, resolve 1); score: RMSE of the display
    luminance over the pixels of a set and the groups; sets: coverage_ref_lib.error_sets.
    Asserted: the new frame's RMSE is below denoise_blend_levels' on the whole frame and on the pixels with coverage below 1, at
    64+64 and at 256+256 (the prototype's margins there: 6 to 11 %).  Everything else is printed, and recorded in DESIGN.md
    section 6s; nothing of it is asserted.  What this restatement prints is in the table there.
    This measures the restatement, not the kernels."""
    W = H = 64
    cfg, sc = Config.cornell_v3(W, H, seed=0, max_raytrace=4), cornell_box("v3")
    feats = fl.features(sc, cfg)
    cov = cl.coverage(sc, cfg, 4, feats=feats)
    sets = cl.error_sets(feats["object"], cov)
    shown = lambda ib: _lum(fl.denoise(cfg, ib, feats, iterations=0, demodulate=0)).astype(np.float64)      # noqa: E731
    o = OracleRenderer(sc, cfg)
    o.refresh()
    o.set_sample_base(1 << 20)
    o.sample(2048)
    truth = shown(o.image_buffer)
    halves = (16, 64, 256)
    who = ("denoise", "levels", "coverage", "new", "taps")
    se = {h: {k: [] for k in who} for h in halves}
    resolved = []
    for g in range(4):
        o.refresh()
        o.set_sample_base(g * 4096)
        done, snap = 0, {}
        for upto in (16, 32, 64, 128, 256, 512):
            o.sample(upto - done)
            done = upto
            snap[upto] = o.image_buffer
        for h in halves:
            hv = hl.Halves(W, H)
            hv.update(snap[h])
            hv.update(snap[2 * h])
            ib = snap[2 * h]
            assert np.all(hv.a[..., 3] == h) and np.all(ib[..., 3] == 2 * h)
            err = lambda px: (_lum(px).astype(np.float64) - truth) ** 2      # noqa: E731
            f = bc.Filtered(cfg, ib, hv.a, feats, cov)
            new = f.run("levels")
            resolved.append(new.resolved)
            se[h]["denoise"].append(err(fl.denoise(cfg, ib, feats)))
            se[h]["levels"].append(err(lv.denoise_blend_levels(cfg, ib, hv.a, feats)[0]))
            se[h]["coverage"].append(err(cl.denoise_coverage(cfg, ib, feats, cov)[0]))
            se[h]["new"].append(err(new.denoised))
            se[h]["taps"].append(err(f.run("levels", resolve=0).denoised))      # the weighted taps alone
    o.close()
    rmse = {(h, k, s): float(np.sqrt(np.mean([e[m] for e in se[h][k]]))) for h in halves for k in who for s, m in sets.items()}
    print("pixels:", {s: int(m.sum()) for s, m in sets.items()}, "resolved per frame:", resolved)
    for h in halves:
        for s in ("frame", "edge", "interior"):
            x = {k: rmse[(h, k, s)] for k in who}
            print(f"halves {h} + {h} {s}: denoise {x['denoise']:.4f} levels {x['levels']:.4f} coverage {x['coverage']:.4f} new {x['new']:.4f}; "
                  f"new / levels {x['new'] / x['levels']:.3f} new / coverage {x['new'] / x['coverage']:.3f}; "
                  f"taps alone / levels {x['taps'] / x['levels']:.3f}")
    for h in (64, 256):
        for s in ("frame", "edge"):
            assert rmse[(h, "new", s)] < rmse[(h, "levels", s)], (h, s, rmse[(h, "new", s)], rmse[(h, "levels", s)])
