"""CPU tier: the restatement of rtpbr_denoise_blend_levels (tests/post_ref/blend.h) that the GPU tests hold the kernels to —
its ladder of filters against blend_ref's filter, known answers of the rule, hostile buffers, and the measurement behind the rule
on the oracle."""
import os
import re

import numpy as np
import pytest

import blend_ref_lib as bl
import checks as ck
import feature_ref_lib as fr
import half_ref_lib as hl
import hostile as hz
import levels_ref_lib as lv
from oracle_backend import OracleRenderer
from raytracingpbr_amd import Config, cornell_box, src_scene
from raytracingpbr_amd.dataclass import BlendParams
from raytracingpbr_amd.ibl import synthetic_env


def _lum(c):
    c = np.asarray(c, np.float32)
    return (np.float32(0.299) * c[..., 0] + np.float32(0.587) * c[..., 1]) + np.float32(0.114) * c[..., 2]


def _image(W, H, colour, count):
    ib = np.empty((W, H, 4), np.float32)
    ib[..., :3] = np.asarray(colour, np.float32) * np.float32(count)
    ib[..., 3] = count
    return ib


def _flat_features(W, H):
    """one object facing the camera at one depth: nothing but the colour term stops the filter"""
    n = np.zeros((W, H, 3), np.float32)
    n[..., 2] = 1.0
    return {"albedo": np.full((W, H, 3), 0.5, np.float32), "normal": n, "depth": np.full((W, H), 3.0, np.float32),
            "object": np.zeros((W, H), np.int32)}


def _step(W, H, count):
    """luminance 0.5 left of the middle, 1 right of it (powers of two: test_blend_ref.py says why)"""
    ib = _image(W, H, (0.5, 0.5, 0.5), count)
    ib[W // 2:] = _image(W, H, (1.0, 1.0, 1.0), count)[W // 2:]
    return ib


# ------------------------------------------------------------------ the ladder of filters
def test_every_level_of_the_ladder_is_the_filter_with_that_many_iterations():
    W, H = 41, 33
    cfg, sc = Config.cornell_v3(W, H, seed=0, max_raytrace=3), cornell_box("v3")
    feats = fr.features(sc, cfg)
    ib, _ = hz.base_buffer(W, H)
    ib[3:6, 4:9] = 0.0                              # a block of pixels without samples
    for demodulate in (0, 1):
        ladder = lv.filter_levels(cfg, ib, feats, iterations=4, demodulate=demodulate)
        assert ladder.shape == (5, W, H, 3)
        for k in range(5):
            want = bl.filter(cfg, ib, feats, linear=True, iterations=k, demodulate=demodulate)
            assert np.array_equal(ck.bits(ladder[k]), ck.bits(want)), (k, demodulate)
            # ... and a shorter ladder is the head of a longer one
            assert np.array_equal(ck.bits(lv.filter_levels(cfg, ib, feats, iterations=k, demodulate=demodulate)), ck.bits(ladder[:k + 1]))
        assert not ladder[:, 3:6, 4:9].any()


# ------------------------------------------------------------------ known answers
def test_identical_constant_halves_keep_every_level_and_give_the_denoised_frame():
    """(channel values that are powers of two, no demodulation: every level is then exactly the constant)"""
    W, H = 41, 33
    cfg, sc = Config.cornell_v3(W, H, seed=0, max_raytrace=3), cornell_box("v3")
    feats = fr.features(sc, cfg)
    col = (0.5, 0.25, 1.0)
    ib, a = _image(W, H, col, 16), _image(W, H, col, 8)
    for K in (0, 1, 4):
        f = lv.Filtered(cfg, ib, a, feats, iterations=K)
        for radius in (1, 2, 3):
            for z in (0.0, 2.0):
                out, t, depth, st = f.blend(radius, z, 8)
                assert np.all(t == 1) and np.all(depth == K) and st == (W * H, 0, 0.0)
                assert np.array_equal(ck.bits(out), ck.bits(fr.denoise(cfg, ib, feats, iterations=K)))


@pytest.mark.parametrize("radius", [1, 2, 3])
def test_noise_free_step_keeps_as_many_levels_as_see_no_blur(radius):
    """Both halves equal and noise free: dp = 0, so SC = 0 and every significant window gives t_k = 0; z = 0 makes every window
    with a pixel that level k changed significant.  Level 1 reaches 2 pixels and level 2 another 4: depth 0 within 2 + radius
    columns of the step, 1 out to 6 + radius, 2 beyond.  Where level 1 is kept and level 2 refused the pixel itself is beyond
    level 1's reach, so FD_1 = FD_0 there and c = FD_0 + 1 * (FD_1 - FD_0) is the raw colour."""
    W, H = 40, 9
    cfg = Config.cornell_v3(W, H, seed=0, max_raytrace=3)
    feats = _flat_features(W, H)
    ib, a = _step(W, H, 16), _step(W, H, 8)
    p = dict(iterations=2, demodulate=0)
    out, t, depth, st = lv.denoise_blend_levels(cfg, ib, a, feats, radius, 0.0, 8, **p)
    mid = W // 2
    band0 = np.zeros((W, H), bool)
    band0[mid - 2 - radius: mid + 2 + radius] = True
    band01 = np.zeros((W, H), bool)
    band01[mid - 6 - radius: mid + 6 + radius] = True
    band1, band2 = band01 & ~band0, ~band01
    assert band1.any() and band2.any()
    assert np.all(depth[band0] == 0) and np.all(depth[band1] == 1) and np.all(depth[band2] == 2)
    assert np.all(t[band01] == 0) and np.all(t[band2] == 1)
    raw, den = fr.denoise(cfg, ib, feats, iterations=0, demodulate=0), fr.denoise(cfg, ib, feats, **p)
    assert np.array_equal(ck.bits(out)[band01], ck.bits(raw)[band01]) and np.array_equal(ck.bits(out)[band2], ck.bits(den)[band2])
    assert not np.array_equal(ck.bits(raw)[band0], ck.bits(den)[band0])
    assert st == (W * H, int(band01.sum()), 1.0)


def test_min_half_samples_gates_at_the_count_itself():
    W, H = 40, 9
    cfg = Config.cornell_v3(W, H, seed=0, max_raytrace=3)
    feats = _flat_features(W, H)
    p = dict(iterations=2, demodulate=0)
    m = 8
    den = lambda ib: fr.denoise(cfg, ib, feats, **p)      # noqa: E731
    ib, a = _step(W, H, 2 * (m - 1)), _step(W, H, m - 1)      # 7 + 7
    out, t, depth, st = lv.denoise_blend_levels(cfg, ib, a, feats, 3, 0.0, m, **p)
    assert np.all(t == 1) and np.all(depth == 2) and st == (0, 0, 0.0) and np.array_equal(ck.bits(out), ck.bits(den(ib)))
    ib, a = _step(W, H, 2 * m), _step(W, H, m)                # 8 + 8
    out, t, depth, st = lv.denoise_blend_levels(cfg, ib, a, feats, 3, 0.0, m, **p)
    assert st[0] == W * H and 0 < st[1] < W * H and (t == 0).any() and (depth == 0).any() and (depth == 1).any()
    # one half short on some pixels: they are neither usable nor anybody's tap
    a[:, 2] = _step(W, H, m - 1)[:, 2]
    a[W // 2, 6] = 0.0
    out, t, depth, st = lv.denoise_blend_levels(cfg, ib, a, feats, 3, 0.0, m, **p)
    assert np.all(t[:, 2] == 1) and np.all(depth[:, 2] == 2) and t[W // 2, 6] == 1 and st[0] == W * H - W - 1
    assert np.array_equal(ck.bits(out[:, 2]), ck.bits(den(ib)[:, 2]))


def test_pixels_without_samples_and_no_levels():
    W, H = 40, 9
    cfg = Config.cornell_v3(W, H, seed=0, max_raytrace=3)
    feats = _flat_features(W, H)
    ib, a = _step(W, H, 16), _step(W, H, 8)
    ib[5:8, 2:5] = 0.0
    a[5:8, 2:5] = 0.0
    for K in (0, 2):
        p = dict(iterations=K, demodulate=1)
        out, t, depth, st = lv.denoise_blend_levels(cfg, ib, a, feats, 2, 0.0, 8, **p)
        assert np.all(t[5:8, 2:5] == 1) and np.all(depth[5:8, 2:5] == K) and st[0] == W * H - 9
        assert np.array_equal(ck.bits(out[5:8, 2:5]), ck.bits(fr.denoise(cfg, ib, feats, **p)[5:8, 2:5]))      # what post_process shows
        if K == 0:
            assert np.all(t == 1) and np.all(depth == 0) and st[1:] == (0, 0.0)
            assert np.array_equal(ck.bits(out), ck.bits(fr.denoise(cfg, ib, feats, **p)))


@pytest.mark.parametrize("family", hz.FAMILIES)
def test_nan_and_infinity_give_weights_in_0_1_and_depths_in_0_K(family):
    w, h = hz.W, hz.H
    scene, cfg = hz.scene_cfg("v3", w, h)
    feats = fr.features(scene, cfg)
    a = hz.buffer_for(family, feats["object"])               # the hostile buffer is half A
    batch, _ = hz.base_buffer(w, h, seed=1)
    ib = a + batch                                           # ... and an ordinary batch of 4 lies in B
    K = 4
    f = lv.Filtered(cfg, ib, a, feats, iterations=K)
    for z in (0.0, 2.0):
        out, t, depth, st = f.blend(3, z, 1)
        assert not np.isnan(t).any() and np.all((t >= 0) & (t <= 1))
        assert not np.isnan(depth).any() and np.all((depth >= 0) & (depth <= K))
        assert st[0] > 0.8 * w * h and 0.0 <= st[2] <= 1.0 and (t < 1).any()
        hz.guard(f"denoise_blend_levels {family}", out)


# ------------------------------------------------------------------ defaults
def test_the_levels_call_shares_the_blends_defaults_with_the_header():
    hdr = open(os.path.join(lv.ROOT, "include", "rtpbr.h")).read()
    found = {m.group(1).lower(): float(m.group(2)) for m in re.finditer(r"#define RTPBR_BLEND_DEFAULT_([A-Z_]+)\s+([0-9.]+)f?\s", hdr)}
    assert found == {k: float(v) for k, v in BlendParams.DEFAULTS.items()} and len(found) == 3
    assert re.search(r"RTPBR_BUF_BLEND_DEPTH\s*=\s*18\b", hdr)
    from raytracingpbr_amd import renderer
    assert renderer.BUF_BLEND_DEPTH == 18
    # the restatement's defaults are the header's: None everywhere is (3, 2, 16)
    W, H = 16, 9
    cfg = Config.cornell_v3(W, H, seed=0, max_raytrace=3)
    feats = _flat_features(W, H)
    ib, a = _step(W, H, 32), _step(W, H, 16)
    f = lv.Filtered(cfg, ib, a, feats, iterations=2, demodulate=0)
    for x, y in zip(f.blend(), f.blend(3, 2.0, 16)):
        assert np.array_equal(x, y)
    assert f.blend()[3][0] == W * H and f.blend(3, 2.0, 17)[3][0] == 0


# ------------------------------------------------------------------ the measurement behind the rule
def test_levels_keep_the_noise_reduction_the_blend_gives_up_on_cornell():
    """Cornell v3 at 64x64, seed 0, max_raytrace 4, rtpbr_denoise's defaults (4 levels) and the header's blend defaults (radius 3,
    z 2, min_half_samples 16); 6 groups of samples with sample_base = g * 4096, halves 8+8 / 16+16 / 32+32 / 64+64 / 256+256 dealt
    by the rule itself from two equal batches; truth: 2048 spp at sample_base 2^20 shown with iterations = 0; score: RMSE of the
    display luminance over pixels and groups.  Asserted: levels / denoised exactly 1 at 8+8 (gated off) and <= 1.03 at 16+16,
    levels <= blend at 32+32, levels / blend <= 0.94 at 64+64 and 256+256.  The float64 prototype had levels / denoised 1.000,
    1.001, 0.918, 0.843, 0.743 and levels / blend 0.878 and 0.907 in the last two rows; the rows this restatement gives are in
    DESIGN.md section 6m.  This measures the restatement, not the kernels."""
    W = H = 64
    cfg, sc = Config.cornell_v3(W, H, seed=0, max_raytrace=4), cornell_box("v3")
    feats = fr.features(sc, cfg)
    shown = lambda ib: _lum(fr.denoise(cfg, ib, feats, iterations=0, demodulate=0)).astype(np.float64)      # noqa: E731
    o = OracleRenderer(sc, cfg)
    o.refresh()
    o.set_sample_base(1 << 20)
    o.sample(2048)
    truth = shown(o.image_buffer)
    halves = (8, 16, 32, 64, 256)
    se = {h: {"raw": [], "denoised": [], "blend": [], "levels": []} for h in halves}
    depth = {h: [] for h in halves}
    for g in range(6):
        o.refresh()
        o.set_sample_base(g * 4096)
        done, snap = 0, {}
        for upto in (8, 16, 32, 64, 128, 256, 512):
            o.sample(upto - done)
            done = upto
            snap[upto] = o.image_buffer
        for h in halves:
            hv = hl.Halves(W, H)
            hv.update(snap[h])
            hv.update(snap[2 * h])
            assert np.all(hv.a[..., 3] == h) and np.all(snap[2 * h][..., 3] == 2 * h)
            out_b, _, st_b = bl.denoise_blend(cfg, snap[2 * h], hv.a, feats)
            out_l, _, d, st_l = lv.denoise_blend_levels(cfg, snap[2 * h], hv.a, feats)
            assert st_l[0] == st_b[0] == (W * H if h >= 16 else 0)
            err = lambda px: (_lum(px).astype(np.float64) - truth) ** 2      # noqa: E731
            se[h]["raw"].append((shown(snap[2 * h]) - truth) ** 2)
            se[h]["denoised"].append(err(fr.denoise(cfg, snap[2 * h], feats)))
            se[h]["blend"].append(err(out_b))
            se[h]["levels"].append(err(out_l))
            depth[h].append(float(d.mean()))
    o.close()
    r = {h: {k: float(np.sqrt(np.mean(v))) for k, v in se[h].items()} for h in halves}
    for h in halves:
        x = r[h]
        print(f"halves {h} + {h}: denoised {x['denoised']:.4f}; / denoised: raw {x['raw'] / x['denoised']:.3f} "
              f"blend {x['blend'] / x['denoised']:.3f} levels {x['levels'] / x['denoised']:.3f}; "
              f"levels / blend {x['levels'] / x['blend']:.3f}; mean depth {np.mean(depth[h]):.2f}")
    assert r[8]["levels"] / r[8]["denoised"] == 1.0, r[8]
    assert r[16]["levels"] / r[16]["denoised"] <= 1.03, r[16]
    assert r[32]["levels"] <= r[32]["blend"], r[32]
    assert r[64]["levels"] / r[64]["blend"] <= 0.94, r[64]
    assert r[256]["levels"] / r[256]["blend"] <= 0.94, r[256]


def test_levels_stay_under_the_blend_on_tokyo():
    """The src/ Tokyo scene at 96x54, Config.src(96, 54, 7, steps_per_launch=4), synthetic_env(192, 96, seed=0) at exposure 1.4 and
    gamma 2.2, rtpbr_denoise's defaults and the header's blend defaults; 4 groups with sample_base = g * 4096, halves of 16 / 32 /
    64 / 128 launches dealt by the rule itself from two equal batches; truth: 64 x sample(64) at sample_base 2^20 shown with
    iterations = 0; score as on Cornell.  Asserted: levels <= blend at 32 + 32 and at 64 + 64.  The rows this restatement gives
    are in DESIGN.md section 6m.  About 45 s of oracle time; this measures the restatement, not the kernels."""
    W, H = 96, 54
    sc, cfg = src_scene(aspect=W / H, tokyo=True), Config.src(W, H, 7, steps_per_launch=4)
    feats = fr.features(sc, cfg)
    shown = lambda ib: _lum(fr.denoise(cfg, ib, feats, iterations=0, demodulate=0)).astype(np.float64)      # noqa: E731
    o = OracleRenderer(sc, cfg)
    o.set_env(synthetic_env(192, 96, seed=0), 1.4, 2.2)
    o.refresh()
    o.set_sample_base(1 << 20)
    for _ in range(64):
        o.sample(64)
    truth = shown(o.image_buffer)
    halves = (16, 32, 64, 128)
    se = {h: {"raw": [], "denoised": [], "blend": [], "levels": []} for h in halves}
    for g in range(4):
        o.refresh()
        o.set_sample_base(g * 4096)
        done, snap = 0, {}
        for upto in (16, 32, 64, 128, 256):
            o.sample(upto - done)
            done = upto
            snap[upto] = o.image_buffer
        for h in halves:
            hv = hl.Halves(W, H)
            hv.update(snap[h])
            hv.update(snap[2 * h])
            out_b = bl.denoise_blend(cfg, snap[2 * h], hv.a, feats)[0]
            out_l = lv.denoise_blend_levels(cfg, snap[2 * h], hv.a, feats)[0]
            err = lambda px: (_lum(px).astype(np.float64) - truth) ** 2      # noqa: E731
            se[h]["raw"].append((shown(snap[2 * h]) - truth) ** 2)
            se[h]["denoised"].append(err(fr.denoise(cfg, snap[2 * h], feats)))
            se[h]["blend"].append(err(out_b))
            se[h]["levels"].append(err(out_l))
    o.close()
    r = {h: {k: float(np.sqrt(np.mean(v))) for k, v in se[h].items()} for h in halves}
    for h in halves:
        x = r[h]
        print(f"halves {h} + {h} launches: denoised {x['denoised']:.4f}; / denoised: raw {x['raw'] / x['denoised']:.3f} "
              f"blend {x['blend'] / x['denoised']:.3f} levels {x['levels'] / x['denoised']:.3f}; levels {x['levels']:.4f} raw {x['raw']:.4f}")
    assert r[32]["levels"] <= r[32]["blend"], r[32]
    assert r[64]["levels"] <= r[64]["blend"], r[64]
