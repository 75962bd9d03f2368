"""CPU tier: the restatement of rtpbr_blend_error (tests/post_ref/blend.h) that the GPU tests hold the kernels to
— the header's mirrors, the identity with rtpbr_denoise_error's restatement, known answers of the rule, and the calibration of
the estimate against the empirical error on the oracle."""
import os
import re

import numpy as np
import pytest

import blend_error_ref_lib as be
import checks as ck
import feature_ref_lib as fr
import half_ref_lib as hl
import hostile as hz
import levels_ref_lib as lv
from oracle_backend import OracleRenderer
from raytracingpbr_amd import Config, _capi, cornell_box, renderer
from raytracingpbr_amd.dataclass import BlendParams, ErrorParams

NEVER = 16777216      # min_half_samples above every count


def _lum(c):
    c = np.asarray(c, np.float32)
    return (np.float32(0.299) * c[..., 0] + np.float32(0.587) * c[..., 1]) + np.float32(0.114) * c[..., 2]


def _lum64(c):
    c = np.asarray(c, np.float64)
    return 0.299 * c[..., 0] + 0.587 * c[..., 1] + 0.114 * c[..., 2]


def _window_mean(v, ok, obj, R):
    """mean of v over the (2R+1)^2 window on the pixel's object over the pixels with ok, float64; NaN where there is none"""
    W, H = obj.shape
    out = np.full((W, H), np.nan)
    for x in range(W):
        for y in range(H):
            xs, ys = slice(max(x - R, 0), x + R + 1), slice(max(y - R, 0), y + R + 1)
            sel = ok[xs, ys] & (obj[xs, ys] == obj[x, y])
            if sel.any():
                out[x, y] = np.asarray(v, np.float64)[xs, ys][sel].mean()
    return out


def _cornell_state(W=41, H=33):
    """Cornell's features, two independent gamma-distributed halves of 4 + 4, a block without samples, a stripe with an empty A
    and a stripe with an empty B"""
    cfg, sc = Config.cornell_v3(W, H, seed=0, max_raytrace=3), cornell_box("v3")
    feats = fr.features(sc, cfg)
    a, _ = hz.base_buffer(W, H, seed=0)
    b2, _ = hz.base_buffer(W, H, seed=1)
    a[:, 5] = 0.0           # A empty
    b2[:, 20] = 0.0         # B empty
    a[3:6, 8:12] = 0.0      # no samples at all
    b2[3:6, 8:12] = 0.0
    return cfg, feats, a + b2, a


# ------------------------------------------------------------------ the header's mirrors
def test_header_enum_entry_points_and_defaults_are_mirrored():
    hdr = open(os.path.join(be.ROOT, "include", "rtpbr.h")).read()
    assert re.search(r"RTPBR_BUF_BLEND_ERROR\s*=\s*19\b", hdr) and renderer.BUF_BLEND_ERROR == 19
    assert re.search(r"RTPBR_BUF_BLEND_DEPTH\s*=\s*18\b", hdr) and renderer.BUF_BLEND_DEPTH == 18
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"int rtpbr_blend_error\(rtpbr_ctx\* ctx, const rtpbr_denoise_params\* p, const rtpbr_blend_params\* e, "
                     r"const rtpbr_error_params\* w,\s*float threshold, rtpbr_noise_stats\* out\);", code)
    assert re.search(r"int rtpbr_select_blend_error\(rtpbr_ctx\* ctx, float threshold, int dilate, uint32_t\* n_selected\);", code)
    assert "blend_error" in _capi.ENTRY_POINTS and "select_blend_error" in _capi.ENTRY_POINTS
    # no parameter struct of its own: the blend's and the error's, with their defaults
    assert BlendParams.DEFAULTS == {"radius": 3, "z": 2.0, "min_half_samples": 16} and ErrorParams.DEFAULTS == {"radius": 2}
    W, H = 16, 9
    cfg = Config.cornell_v3(W, H, seed=0, max_raytrace=3)
    feats = {"albedo": np.full((W, H, 3), 0.5, np.float32), "normal": np.zeros((W, H, 3), np.float32),
             "depth": np.full((W, H), 3.0, np.float32), "object": np.zeros((W, H), np.int32)}
    a, _ = hz.base_buffer(W, H, seed=0)
    b2, _ = hz.base_buffer(W, H, seed=1)
    f = lv.Filtered(cfg, (a + b2) * 8, a * 8, feats, iterations=2)      # 32 + 32
    for x, y in zip(be.from_ladders(f), be.from_ladders(f, 0.0, 3, 2.0, 16, 2)):
        assert np.array_equal(ck.bits(np.asarray(x, np.float32)), ck.bits(np.asarray(y, np.float32)))
    assert not np.array_equal(be.from_ladders(f).error, be.from_ladders(f, window=3).error)


# ------------------------------------------------------------------ the frame is rtpbr_denoise_blend_levels'
@pytest.mark.parametrize("K", [0, 1, 4])
def test_frame_weight_and_depth_are_the_levels_restatements(K):
    cfg, feats, ib, a = _cornell_state()
    for demodulate in (0, 1):
        f = lv.Filtered(cfg, ib, a, feats, iterations=K, demodulate=demodulate)
        for radius, z, m in ((1, 0.0, 1), (3, 2.0, 4), (2, 0.0, 4)):
            out, t, depth, _ = f.blend(radius, z, m)
            got = be.from_ladders(f, 0.0, radius, z, m, 2)
            assert np.array_equal(ck.bits(got.denoised), ck.bits(out)) and np.array_equal(ck.bits(got.weight), ck.bits(t))
            assert np.array_equal(ck.bits(got.depth), ck.bits(depth))


# ------------------------------------------------------------------ the identity with rtpbr_denoise_error
@pytest.mark.parametrize("K", [0, 1, 4])
def test_with_nothing_usable_the_plane_is_rtpbr_denoise_errors_bit_for_bit(K):
    cfg, feats, ib, a = _cornell_state()
    valid = (a[..., 3] > 0) & (ib[..., 3] - a[..., 3] > 0)
    for demodulate in (0, 1):
        p = dict(iterations=K, demodulate=demodulate)
        f = lv.Filtered(cfg, ib, a, feats, **p)
        for window in (1, 2, 3):
            thr = float(np.median(hl.denoise_error(cfg, ib, a, feats, window, 0.0, **p)[0][valid]))      # some above, some below
            want, st, _ = hl.denoise_error(cfg, ib, a, feats, window, thr, **p)
            got = be.from_ladders(f, thr, 3, 0.0, NEVER, window)
            assert np.array_equal(ck.bits(got.error), ck.bits(want)), (K, demodulate, window)
            assert got.stats[:2] == st[:2] and np.float32(got.stats[2]).view(np.uint32) == np.float32(st[2]).view(np.uint32)
            assert got.stats[0] == int(valid.sum()) and 0 < got.stats[1] < got.stats[0]
            assert np.all(got.weight == 1) and not got.bias2.any() and np.all(got.error[~valid] == 0) and np.all(got.error[valid] > 0)


def test_no_levels_give_the_raw_halves_variance_and_no_bias():
    """K = 0: XA is half A's raw average (remodulated), so the variance is that of the raw halves and the bias term vanishes —
    exactly without demodulation; with it XA differs from PA by the rounding of c / albedo * albedo (2 ulp of values below 4:
    5e-7), and bias2 is a mean of products of two such differences (below 1e-12)."""
    cfg, feats, ib, a = _cornell_state()
    for demodulate in (0, 1):
        f = lv.Filtered(cfg, ib, a, feats, iterations=0, demodulate=demodulate)
        got = be.from_ladders(f, 0.0, 2, 0.0, 1, 2)
        assert got.stats[0] > 0 and np.all(got.weight == 1) and np.all(got.depth == 0)
        if demodulate == 0:
            assert not got.bias2.any()
            want = hl.denoise_error(cfg, ib, a, feats, 2, 0.0, iterations=0, demodulate=0)[0]
            assert np.array_equal(ck.bits(got.error), ck.bits(want))
        else:
            assert got.bias2.max() < 1e-12


# ------------------------------------------------------------------ a known answer: no variance, a bias the halves see
def test_identical_halves_blurred_across_a_ramp_give_slope_times_bias():
    """Two objects side by side, a curved luminance ramp across both, halves that are the same 8 samples each: XA = XB, so the
    variance is exactly 0 and the error is s * sqrt(mean over the window on the object of bias^2), bias = lum(XA) - lum(PA).
    z = 1e6 keeps the one level although it blurs (hardly a window is significant), so there is a bias left to report.  The
    expectation is made in float64 from the ladders, the tone map of tests/feature_ref and the levels restatement's weight; the
    restatement makes each bias in f32 as a difference of two luminances below 1 (three products and two sums each, eps 6e-8):
    an absolute error of at most delta = 2.5e-7 per bias, so 2 |bias| delta in bias^2 and s delta in the error, beside 1e-5
    relative for the mean, the root, the slope and the product."""
    W, H = 24, 12
    cfg = Config.cornell_v3(W, H, seed=0, max_raytrace=3)
    n = np.zeros((W, H, 3), np.float32)
    n[..., 2] = 1.0
    obj = np.zeros((W, H), np.int32)
    obj[W // 2:] = 1
    feats = {"albedo": np.full((W, H, 3), 0.5, np.float32), "normal": n, "depth": np.full((W, H), 3.0, np.float32), "object": obj}
    x = (np.arange(W, dtype=np.float32) + 1) / np.float32(W)
    ramp = np.repeat((np.float32(0.1) + np.float32(0.8) * x * x)[:, None], H, axis=1)
    ib = np.empty((W, H, 4), np.float32)
    ib[..., :3] = (ramp * np.float32(16))[..., None] * np.asarray((1.0, 0.5, 0.25), np.float32)
    ib[..., 3] = 16
    a = ib * np.float32(0.5)
    window = 2
    f = lv.Filtered(cfg, ib, a, feats, iterations=1, demodulate=0)
    assert np.array_equal(ck.bits(f.fa), ck.bits(f.fb))
    got = be.from_ladders(f, 0.0, 1, 1e6, 8, window)
    assert got.stats[0] == W * H and not got.variance.any()
    T = lv.denoise_blend_levels(cfg, ib, a, feats, 1, 1e6, 8, iterations=1, demodulate=0)[1].astype(np.float64)
    assert (T == 1).mean() > 0.5      # (a window whose x_q are all equal has v = 0 and is significant at any z)
    xa = f.fa[0] + T[..., None] * (f.fa[1].astype(np.float64) - f.fa[0])
    c = (f.fd[0] + T[..., None] * (f.fd[1].astype(np.float64) - f.fd[0])).astype(np.float32)
    bias = _lum64(xa) - _lum64(a[..., :3].astype(np.float64) / a[..., 3:4])
    assert np.abs(bias).max() > 1e-3
    mean_b2 = _window_mean(bias * bias, np.ones((W, H), bool), obj, window)

    def shown(col):
        b = np.concatenate([col, np.ones((W, H, 1), np.float32)], axis=2)
        return _lum64(fr.denoise(cfg, b, feats, iterations=0, demodulate=0))

    s = (shown(np.float32(1.0625) * c) - shown(c)) / (0.0625 * _lum64(c))
    want = s * np.sqrt(mean_b2)
    assert want.max() > 1e-3
    delta = 2.5e-7
    assert np.all(np.abs(got.error - want) <= s * delta + 1e-5 * want), np.abs(got.error - want).max()
    assert np.allclose(got.slope, s, rtol=1e-5, atol=0)
    assert np.all(np.abs(got.bias2 - mean_b2) <= 2 * np.sqrt(mean_b2) * delta + 1e-5 * mean_b2)
    # the same frame with the gate open (z = 0): the blend refuses the level wherever the halves see it blur, and there the error
    # is 0: nothing is left that the halves could see
    open_gate = be.from_ladders(f, 0.0, 1, 0.0, 8, window)
    refused = _window_mean(open_gate.weight == 0, np.ones((W, H), bool), obj, window) == 1
    assert refused.any() and not open_gate.error[refused].any()


def test_a_valid_pixel_that_is_not_usable_adds_variance_but_no_bias():
    cfg, feats, ib, a = _cornell_state()
    ib, a = ib * np.float32(2), a * np.float32(2)      # 8 + 8 ...
    a[10:20, 10:20] *= np.float32(0.25)                # ... and a block of 2 + 14: valid, not usable at m = 4
    f = lv.Filtered(cfg, ib, a, feats, iterations=2)
    cA, cB = f.a[..., 3], f.hb[..., 3]
    valid, usable = (cA > 0) & (cB > 0), (cA >= 4) & (cB >= 4)
    got = be.from_ladders(f, 0.0, 2, 0.0, 4, 1)
    inner = np.zeros_like(valid)
    inner[12:18, 12:18] = True                         # the whole window is unusable
    assert (valid & ~usable)[inner].all() and got.stats[0] == int(valid.sum())
    assert not got.bias2[inner].any() and np.all(got.variance[inner] > 0)
    assert np.array_equal(ck.bits(got.error[inner]), ck.bits(np.sqrt(got.variance[inner] + np.float32(0))))
    assert (got.bias2[usable] > 0).any()


# ------------------------------------------------------------------ the calibration
# per row: (the measured ratio estimate / empirical of the mean squares, the spread max - min of the four groups' own ratios)
BAND = {16: (6.59, 5.97), 64: (7.42, 2.47)}


def test_the_estimate_is_calibrated_against_the_empirical_error_on_cornell():
    """Cornell v3 at 64x64, seed 0, max_raytrace 4, rtpbr_denoise's defaults, the header's blend defaults and window radius 2;
    4 groups of samples with sample_base = g * 4096, halves of 16 + 16 and 64 + 64 dealt by the rule itself from two equal
    batches.  Truth: two independent renders of 1024 spp (sample_base 2^20 and 2^21) shown with iterations = 0; their mean is
    the reference, and a quarter of the mean square of their difference — the variance the reference itself still has — is
    taken off the empirical mean-square error (9.2e-4 of the 2.9e-3 measured at 64 + 64).  Compared: the mean of error^2 over the
    estimated pixels and the groups against that empirical mean-square error of the blended display luminance.

    Measured (this restatement): estimate / empirical = 6.59 at 16 + 16 (the four groups alone: 3.83 ..
    9.80) and 7.42 at 64 + 64 (5.85 .. 8.32).  THE ESTIMATE IS FAR OUTSIDE 0.5 .. 2: it overstates the mean-square error about
    seven times, nearly all of it in the bias term (the variance term alone is 2 to 4 % of the estimate and about half the
    empirical variance).  The band asserted is each measured ratio give or take the spread of its groups (5.97 and 2.47): a
    pin of what the rule as written gives, not a statement that the estimate is good.  This measures the restatement against
    the empirical error, not the kernels and not the estimate against itself."""
    W = H = 64
    cfg, sc = Config.cornell_v3(W, H, seed=0, max_raytrace=4), cornell_box("v3")
    feats = fr.features(sc, cfg)
    shown = lambda ib: _lum(fr.denoise(cfg, ib, feats, iterations=0, demodulate=0)).astype(np.float64)      # noqa: E731
    o = OracleRenderer(sc, cfg)
    truths = []
    for base in (1 << 20, 1 << 21):
        o.refresh()
        o.set_sample_base(base)
        o.sample(1024)
        truths.append(shown(o.image_buffer))
    truth = 0.5 * (truths[0] + truths[1])
    truth_var = float(np.mean((truths[0] - truths[1]) ** 2)) / 4
    halves = (16, 64)
    est = {h: [] for h in halves}
    emp = {h: [] for h in halves}
    parts = {h: [] for h in halves}
    for g in range(4):
        o.refresh()
        o.set_sample_base(g * 4096)
        done, snap = 0, {}
        for upto in (16, 32, 64, 128):
            o.sample(upto - done)
            done = upto
            snap[upto] = o.image_buffer
        for h in halves:
            hv = hl.Halves(W, H)
            hv.update(snap[h])
            hv.update(snap[2 * h])
            assert np.all(hv.a[..., 3] == h)
            got = be.blend_error(cfg, snap[2 * h], hv.a, feats)
            assert got.stats[0] == W * H
            est[h].append(float(np.mean(got.error.astype(np.float64) ** 2)))
            emp[h].append(float(np.mean((_lum(got.denoised).astype(np.float64) - truth) ** 2)) - truth_var)
            parts[h].append((float(np.mean(got.variance)), float(np.mean(got.slope.astype(np.float64) ** 2 * got.bias2))))
    o.close()
    ratio = {}
    for h in halves:
        per_group = [e / m for e, m in zip(est[h], emp[h])]
        ratio[h] = float(np.sum(est[h]) / np.sum(emp[h]))
        v, b = np.mean(parts[h], axis=0)
        print(f"halves {h} + {h}: estimated rmse {np.sqrt(np.mean(est[h])):.4f} empirical {np.sqrt(np.mean(emp[h])):.4f} "
              f"(reference's own variance {truth_var:.2e} taken off); ratio of the mean squares {ratio[h]:.3f}, per group "
              f"{min(per_group):.3f} .. {max(per_group):.3f}; variance share {v / (v + b):.2f}")
    for h in halves:
        measured, spread = BAND[h]
        assert measured - spread <= ratio[h] <= measured + spread, (h, ratio[h])
