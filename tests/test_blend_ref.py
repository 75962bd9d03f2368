"""CPU tier: the restatement of rtpbr_denoise_blend (tests/post_ref/blend.h) that the GPU tests hold the kernels to — its
filter against feature_ref's, known answers of the rule, and the measurement behind the rule's defaults on the oracle (DESIGN.md
section 6l)."""
import os
import re

import numpy as np
import pytest

import blend_ref_lib as bl
import checks as ck
import feature_ref_lib as fr
import half_ref_lib as hl
import hostile as hz
from oracle_backend import OracleRenderer
from raytracingpbr_amd import Config, cornell_box
from raytracingpbr_amd.dataclass import BlendParams


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
    """luminance 0.5 left of the middle, 1 right of it.  Powers of two: the filter's weighted mean of equal values is then exact
    (w * c rounds as w does), and between 0.5 and 1 the blend FD + 1 * (Pb - FD) gives Pb exactly (Sterbenz)."""
    ib = _image(W, H, (0.5, 0.5, 0.5), count)
    ib[W // 2:] = _image(W, H, (1.0, 1.0, 1.0), count)[W // 2:]
    return ib


# ------------------------------------------------------------------ the filter
def test_the_restated_filter_is_feature_refs_and_its_linear_form_is_what_the_tone_map_takes():
    W, H = 41, 33
    cfg, sc = Config.cornell_v3(W, H, seed=0, max_raytrace=3), cornell_box("v3")
    feats = fr.features(sc, cfg)
    ib, _ = hz.base_buffer(W, H)
    ib[3:6, 4:9] = 0.0                              # pixels without samples
    for iterations in (0, 1, 4):
        for demodulate in (0, 1):
            p = dict(iterations=iterations, demodulate=demodulate)
            shown = bl.filter(cfg, ib, feats, linear=False, **p)
            assert np.array_equal(ck.bits(shown), ck.bits(fr.denoise(cfg, ib, feats, **p)))
            lin = bl.filter(cfg, ib, feats, linear=True, **p)
            assert not lin[3:6, 4:9].any()
            # tone_map(cfg, (c, 1)): the iterations = 0, demodulate = 0 pass of a buffer that holds (c, 1)
            again = fr.denoise(cfg, np.concatenate([lin, np.ones((W, H, 1), np.float32)], axis=2), feats, iterations=0, demodulate=0)
            has = ib[..., 3] > 0
            assert np.array_equal(ck.bits(again)[has], ck.bits(shown)[has])


# ------------------------------------------------------------------ known answers
def test_identical_constant_halves_give_weight_one_and_the_denoised_frame():
    """(Channel values that are powers of two, no demodulation: every filter result is then exactly the constant.  A constant
    the weighted mean rounds leaves the same ulp of residue in both halves, which the rule rightly reads as a bias common to
    both — and blends two colours an ulp apart.)"""
    W, H = 41, 33
    cfg, sc = Config.cornell_v3(W, H, seed=0, max_raytrace=3), cornell_box("v3")
    feats = fr.features(sc, cfg)
    col = (0.5, 0.25, 1.0)
    ib, a = _image(W, H, col, 16), _image(W, H, col, 8)
    for radius in (1, 2, 3):
        for z in (0.0, 2.0):
            out, t, st = bl.denoise_blend(cfg, ib, a, feats, radius, z, 8)
            assert np.all(t == 1) and st == (W * H, 0, 0.0)
            assert np.array_equal(ck.bits(out), ck.bits(fr.denoise(cfg, ib, feats)))


@pytest.mark.parametrize("radius", [1, 2, 3])
def test_noise_free_step_takes_the_raw_colour_where_the_window_sees_the_blur(radius):
    """Both halves equal and noise free: dp = 0, so SC = 0 and every significant window gives t = 0; z = 0 makes every window
    with a blurred pixel in it significant.  Two levels reach 6 pixels: beyond 6 + radius from the step SQ = 0 and t = 1."""
    W, H = 40, 9
    cfg = Config.cornell_v3(W, H, seed=0, max_raytrace=3)
    feats = _flat_features(W, H)
    ib, a = _step(W, H, 16), _step(W, H, 8)
    p = dict(iterations=2, demodulate=0)
    out, t, st = bl.denoise_blend(cfg, ib, a, feats, radius, 0.0, 8, **p)
    fd = bl.filter(cfg, ib, feats, True, **p)
    blurred = _lum(fd) != _lum(ib[..., :3] / ib[..., 3:])
    assert blurred[W // 2 - 6: W // 2 + 6].all() and not blurred[: W // 2 - 6].any() and not blurred[W // 2 + 6:].any()
    near = np.zeros((W, H), bool)
    near[W // 2 - 6 - radius: W // 2 + 6 + radius] = True
    assert np.all(t[near] == 0) and np.all(t[~near] == 1) and (~near).any()
    raw, den = fr.denoise(cfg, ib, feats, iterations=0, demodulate=0), fr.denoise(cfg, ib, feats, **p)
    assert np.array_equal(ck.bits(out)[near], ck.bits(raw)[near]) and np.array_equal(ck.bits(out)[~near], ck.bits(den)[~near])
    assert st == (W * H, int(near.sum()), 1.0)


def test_min_half_samples_gates_at_the_count_itself():
    W, H = 40, 9
    cfg = Config.cornell_v3(W, H, seed=0, max_raytrace=3)
    feats = _flat_features(W, H)
    p = dict(iterations=2, demodulate=0)
    m = 8
    den = lambda ib: fr.denoise(cfg, ib, feats, **p)      # noqa: E731
    ib, a = _step(W, H, 2 * (m - 1)), _step(W, H, m - 1)      # 7 + 7
    out, t, st = bl.denoise_blend(cfg, ib, a, feats, 3, 0.0, m, **p)
    assert np.all(t == 1) and st == (0, 0, 0.0) and np.array_equal(ck.bits(out), ck.bits(den(ib)))
    ib, a = _step(W, H, 2 * m), _step(W, H, m)                # 8 + 8
    out, t, st = bl.denoise_blend(cfg, ib, a, feats, 3, 0.0, m, **p)
    assert st[0] == W * H and 0 < st[1] < W * H and (t == 0).any()
    # one half short on some pixels: they are neither usable nor anybody's tap
    a[:, 2] = _step(W, H, m - 1)[:, 2]
    a[W // 2, 6] = 0.0
    out, t, st = bl.denoise_blend(cfg, ib, a, feats, 3, 0.0, m, **p)
    assert np.all(t[:, 2] == 1) and t[W // 2, 6] == 1 and st[0] == W * H - W - 1
    assert np.array_equal(ck.bits(out[:, 2]), ck.bits(den(ib)[:, 2]))


@pytest.mark.parametrize("family", hz.FAMILIES)
def test_nan_and_infinity_give_weights_in_0_1(family):
    w, h = hz.W, hz.H
    scene, cfg = hz.scene_cfg("v3", w, h)
    feats = fr.features(scene, cfg)
    a = hz.buffer_for(family, feats["object"])               # the hostile buffer is half A
    batch, _ = hz.base_buffer(w, h, seed=1)
    ib = a + batch                                           # ... and an ordinary batch of 4 lies in B
    for z in (0.0, 2.0):
        out, t, st = bl.denoise_blend(cfg, ib, a, feats, 3, z, 1)
        assert not np.isnan(t).any() and np.all((t >= 0) & (t <= 1))
        assert st[0] > 0.8 * w * h and 0.0 <= st[2] <= 1.0 and (t < 1).any()
        hz.guard(f"denoise_blend {family}", out)


# ------------------------------------------------------------------ defaults
def test_python_blend_defaults_match_the_header():
    hdr = open(os.path.join(bl.ROOT, "include", "rtpbr.h")).read()
    found = {m.group(1).lower(): float(m.group(2)) for m in re.finditer(r"#define RTPBR_BLEND_DEFAULT_([A-Z_]+)\s+([0-9.]+)f?\s", hdr)}
    assert found == {k: float(v) for k, v in BlendParams.DEFAULTS.items()} and len(found) == 3
    assert [f for f, _ in BlendParams._fields_] == list(BlendParams.DEFAULTS)


# ------------------------------------------------------------------ the measurement behind the rule
def test_blend_goes_under_the_filters_floor_and_costs_nothing_where_the_halves_see_no_bias():
    """Cornell v3 at 64x64, seed 0, max_raytrace 4, rtpbr_denoise's defaults; 6 groups of samples with sample_base = g * 4096,
    halves 4+4 / 8+8 / 16+16 / 64+64 / 256+256 dealt by the rule itself from two equal batches; truth: 2048 spp at sample_base
    2^20 shown with iterations = 0; score: RMSE of the display luminance over pixels and groups; radius 3, z = 2,
    min_half_samples 8.  Asserted on blended / denoised: <= 0.90 at 256+256, <= 1.00 at 64+64, <= 1.08 at 8+8 and 16+16, exactly 1
    at 4+4 (gated off).  Measured with this restatement: 1.000, 1.030, 1.000, 0.960, 0.819 (DESIGN.md section 6l has the table).
    This measures the restatement, not the kernels."""
    W = H = 64
    cfg, sc = Config.cornell_v3(W, H, seed=0, max_raytrace=4), cornell_box("v3")
    feats = fr.features(sc, cfg)
    shown = lambda ib: _lum(fr.denoise(cfg, ib, feats, iterations=0, demodulate=0)).astype(np.float64)      # noqa: E731
    o = OracleRenderer(sc, cfg)
    o.refresh()
    o.set_sample_base(1 << 20)
    o.sample(2048)
    truth = shown(o.image_buffer)
    halves = (4, 8, 16, 64, 256)
    se = {h: {"raw": [], "denoised": [], "blended": []} for h in halves}
    weight = {h: [] for h in halves}
    for g in range(6):
        o.refresh()
        o.set_sample_base(g * 4096)
        done, snap = 0, {}
        for upto in (4, 8, 16, 32, 64, 128, 256, 512):
            o.sample(upto - done)
            done = upto
            snap[upto] = o.image_buffer
        for h in halves:
            hv = hl.Halves(W, H)
            hv.update(snap[h])
            hv.update(snap[2 * h])
            assert np.all(hv.a[..., 3] == h) and np.all(snap[2 * h][..., 3] == 2 * h)
            out, t, st = bl.denoise_blend(cfg, snap[2 * h], hv.a, feats, 3, 2.0, 8)
            assert st[0] == (W * H if h >= 8 else 0)
            se[h]["raw"].append((shown(snap[2 * h]) - truth) ** 2)
            se[h]["denoised"].append((_lum(fr.denoise(cfg, snap[2 * h], feats)).astype(np.float64) - truth) ** 2)
            se[h]["blended"].append((_lum(out).astype(np.float64) - truth) ** 2)
            weight[h].append(float(t.mean()))
    o.close()
    ratio = {}
    for h in halves:
        r = {k: float(np.sqrt(np.mean(v))) for k, v in se[h].items()}
        ratio[h] = r["blended"] / r["denoised"]
        print(f"halves {h} + {h}: raw {r['raw']:.4f} denoised {r['denoised']:.4f} blended {r['blended']:.4f} "
              f"blended / denoised {ratio[h]:.3f} mean weight {np.mean(weight[h]):.3f}")
    assert ratio[256] <= 0.90 and ratio[64] <= 1.00 and ratio[16] <= 1.08 and ratio[8] <= 1.08 and ratio[4] == 1.0, ratio
