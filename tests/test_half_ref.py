"""CPU tier: the restatement of rtpbr_half_update / rtpbr_denoise_error / rtpbr_select_error (tests/half_ref/half_ref.c) that
the GPU tests hold the kernels to — known answers of the dealing rule and of constant halves, and the calibration of the
estimate against the empirical variance of the denoised luminance on the oracle."""
import os
import re

import numpy as np

import feature_ref_lib as fr
import half_ref_lib as hl
from oracle_backend import OracleRenderer
from raytracingpbr_amd import Config, cornell_box
from raytracingpbr_amd.dataclass import ErrorParams


def _lum(c):
    c = np.asarray(c, np.float32)
    return (np.float32(0.299) * c[..., 0] + np.float32(0.587) * c[..., 1]) + np.float32(0.114) * c[..., 2]


def _image(W, H, colour, count):
    ib = np.empty((W, H, 4), np.float32)
    ib[..., :3] = np.asarray(colour, np.float32) * np.float32(count)
    ib[..., 3] = count
    return ib


# ------------------------------------------------------------------ the dealing rule
def test_equal_batches_alternate_a_b_a():
    h = hl.Halves(3, 2)
    batch = _image(3, 2, (0.5, 0.25, 1.0), 4)
    ib = np.zeros_like(batch)
    want_a = [4, 4, 8, 8, 12]
    for k in range(5):
        ib = ib + batch
        h.update(ib)
        assert np.all(h.a[..., 3] == want_a[k]) and np.array_equal(h.snapshot, ib)
        assert np.array_equal(h.a[..., :3], np.broadcast_to(np.float32([0.5, 0.25, 1.0]) * want_a[k], (3, 2, 3)))


def test_after_4_then_12_the_next_batch_goes_to_a():
    h = hl.Halves(2, 2)
    ib = _image(2, 2, (1, 1, 1), 4)
    h.update(ib)                                  # A: 4
    ib = ib + _image(2, 2, (2, 2, 2), 12)
    h.update(ib)                                  # B: 12 (A.w = 4 > cB = 0)
    assert np.all(h.a[..., 3] == 4)
    ib = ib + _image(2, 2, (3, 3, 3), 2)
    h.update(ib)                                  # A: 4 <= 12
    assert np.all(h.a[..., 3] == 6) and np.all(h.a[..., 0] == 4 * 1 + 2 * 3)
    assert np.all(hl.subtract(ib, h.a)[..., 3] == 12)


def test_a_pixel_without_new_samples_keeps_its_bits_and_a_never_exceeds_the_image():
    rng = np.random.default_rng(0)
    W, H = 9, 7
    h = hl.Halves(W, H)
    ib = np.zeros((W, H, 4), np.float32)
    for _ in range(12):
        got = rng.random((W, H)) < 0.6            # the pixels a selected launch reached
        n = np.float32(rng.integers(1, 6))
        add = np.zeros_like(ib)
        add[..., :3] = rng.random((W, H, 3)).astype(np.float32) * n
        add[..., 3] = n
        before = h.a.copy()
        ib = np.where(got[..., None], ib + add, ib)
        h.update(ib)
        assert np.array_equal(h.a.view(np.uint32)[~got], before.view(np.uint32)[~got])      # d.w = 0
        assert np.all(h.a[..., 3] <= ib[..., 3]) and np.all(h.a[..., 3] >= 0)
        assert np.array_equal(h.snapshot, ib)
    cb = ib[..., 3] - h.a[..., 3]
    assert (h.a[..., 3] > 0).any() and (cb > 0).any()


# ------------------------------------------------------------------ constant halves
def test_constant_halves_give_the_known_error_and_empty_halves_are_selected():
    W, H = 41, 33
    cfg, sc = Config.cornell_v3(W, H, seed=0, max_raytrace=3), cornell_box("v3")
    feats = fr.features(sc, cfg)
    a_col, b_col, cA, cB = (0.2, 0.3, 0.1), (0.6, 0.5, 0.4), 4.0, 12.0
    shown = lambda col: fr.denoise(cfg, _image(W, H, col, 1), feats, iterations=0, demodulate=0)[0, 0]      # noqa: E731  (the tone map)
    want = abs(float(_lum(shown(a_col))) - float(_lum(shown(b_col)))) * np.sqrt(cA * cB) / (cA + cB)
    a, b = _image(W, H, a_col, cA), _image(W, H, b_col, cB)
    a[5:9, 3:8] = 0.0                             # half A empty there
    ib = a + b
    ib[20:23, 10] = a[20:23, 10]                  # half B empty there
    for radius in (1, 2, 3):
        err, st, e = hl.denoise_error(cfg, ib, a, feats, radius=radius, threshold=0.5 * want)
        valid = np.ones((W, H), bool)
        valid[5:9, 3:8] = False
        valid[20:23, 10] = False
        assert np.array_equal(e >= 0, valid)
        np.testing.assert_allclose(err[valid], want, rtol=1e-5)
        assert np.all(err[~valid] == 0)
        assert st[0] == st[1] == int(valid.sum()) and abs(st[2] - want) <= 1e-5 * want
    mask = hl.select(ib, a, err, 2.0 * want, dilate=0)
    assert np.array_equal(mask != 0, ~valid)      # nothing is above: the empty halves alone
    assert hl.select(ib, a, err, 0.5 * want, dilate=0).all()
    # a = b': no difference between the halves, error 0
    same = (0.25, 0.5, 0.125)                     # (dyadic: image_buffer - A is exactly half B)
    err0, st0, _ = hl.denoise_error(cfg, _image(W, H, same, cA + cB), _image(W, H, same, cA), feats)
    assert np.all(err0 == 0) and st0 == (W * H, 0, 0.0)


# ------------------------------------------------------------------ calibration against the oracle
def test_estimate_is_calibrated_against_the_empirical_variance_of_the_denoised_luminance():
    """Cornell v3 at 96x96, seed 0, max_raytrace 4, 10 groups of samples with sample_base = g * 1024, rtpbr_denoise's defaults,
    radius 2.  Halves (4,4), (4,12), (16,16), dealt by the rule itself from batches of those sizes.  Per case the ratio
    sum over pixels of the groups' mean error^2 / sum over pixels of the variance (ddof 1) across the groups of
    lum(denoise(full frame)) must lie within 0.5 .. 2.0: a factor of two around the 1 the derivation gives (include/rtpbr.h).
    This measures the restatement, not the kernels."""
    W = H = 96
    cfg, sc = Config.cornell_v3(W, H, seed=0, max_raytrace=4), cornell_box("v3")
    feats = fr.features(sc, cfg)
    cases = {(4, 4): (4, 8), (4, 12): (4, 16), (16, 16): (16, 32)}      # halves -> (spp when A is dealt, spp of the full frame)
    est = {k: [] for k in cases}
    shown = {k: [] for k in cases}
    o = OracleRenderer(sc, cfg)
    for g in range(10):
        o.refresh()
        o.set_sample_base(g * 1024)
        snap, done = {}, 0
        for upto in (4, 8, 16, 32):
            o.sample(upto - done)
            done = upto
            snap[upto] = o.image_buffer
        for k, (first, full) in cases.items():
            h = hl.Halves(W, H)
            h.update(snap[first])
            h.update(snap[full])
            assert np.all(h.a[..., 3] == k[0]) and np.all(snap[full][..., 3] - h.a[..., 3] == k[1])
            err, st, _ = hl.denoise_error(cfg, snap[full], h.a, feats)
            assert st[0] == W * H
            est[k].append(err.astype(np.float64) ** 2)
            shown[k].append(_lum(fr.denoise(cfg, snap[full], feats)).astype(np.float64))
    for k in cases:
        ratio = np.mean(est[k], axis=0).sum() / np.var(shown[k], axis=0, ddof=1).sum()
        print(f"halves {k}: sum estimate / sum empirical variance = {ratio:.3f}")
        assert 0.5 <= ratio <= 2.0, (k, ratio)


# ------------------------------------------------------------------ defaults
def test_python_error_defaults_match_the_header():
    hdr = open(os.path.join(hl.ROOT, "include", "rtpbr.h")).read()
    found = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define RTPBR_ERROR_DEFAULT_([A-Z_]+)\s+([0-9]+)", hdr)}
    assert found == ErrorParams.DEFAULTS
    assert [f for f, _ in ErrorParams._fields_] == list(ErrorParams.DEFAULTS)
