#!/usr/bin/env python3
"""Calibration of rtpbr_blend_error's estimate against the empirical error, on the CPU restatement and the oracle (no GPU): the
sweep behind DESIGN.md section 6n, longer than tests/test_blend_error_ref.py can afford and split into the estimate's two terms.

    python tools/blend_error_calibration.py                  # Cornell v3 64x64, halves 16 / 64 / 256, 6 groups
    python tools/blend_error_calibration.py --halves 16 64 --groups 4
    python tools/blend_error_calibration.py --bias display   # rtpbr_blend_error_display's rule

Per row: the estimated and the empirical mean-square error of the blended display luminance (the reference's own variance,
a quarter of the mean square of the difference of its two independent halves, taken off), the variance term against the
empirical variance across the groups, the bias term against the empirical squared bias (the groups' mean frame against the
reference, less the variance of that mean and of the reference), and how much of the estimate the largest 1 % of the pixels carry.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import blend_error_ref_lib as be      # noqa: E402
import feature_ref_lib as fr          # noqa: E402
import half_ref_lib as hl             # noqa: E402
from oracle_backend import OracleRenderer      # noqa: E402
from raytracingpbr_amd import Config, cornell_box      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, nargs=2, default=[64, 64])
ap.add_argument("--halves", type=int, nargs="+", default=[16, 64, 256])
ap.add_argument("--groups", type=int, default=6)
ap.add_argument("--ref-spp", type=int, default=2048, help="samples per pixel of each of the reference's two halves")
ap.add_argument("--window", type=int, default=None)
ap.add_argument("--bias", choices=("linear", "display"), default="linear", help="rtpbr_blend_error's rule, or rtpbr_blend_error_display's")
a = ap.parse_args()


def lum(c):
    c = np.asarray(c, np.float64)
    return 0.299 * c[..., 0] + 0.587 * c[..., 1] + 0.114 * c[..., 2]


W, H = a.size
cfg, sc = Config.cornell_v3(W, H, seed=0, max_raytrace=4), cornell_box("v3", aspect=W / H)
feats = fr.features(sc, cfg)
shown = lambda ib: lum(fr.denoise(cfg, ib, feats, iterations=0, demodulate=0))      # noqa: E731
o = OracleRenderer(sc, cfg)
tr = []
for base in (1 << 20, 1 << 21):
    o.refresh()
    o.set_sample_base(base)
    o.sample(a.ref_spp)
    tr.append(shown(o.image_buffer))
truth, tv = 0.5 * (tr[0] + tr[1]), float(np.mean((tr[0] - tr[1]) ** 2)) / 4
print(f"Cornell v3 {W}x{H}, {a.groups} groups, reference 2 x {a.ref_spp} spp (its own variance {tv:.3e}), window {a.window or 2}, {a.bias} bias")
print("  halves    estimated mse   empirical mse   ratio | variance term / empirical variance | bias term / empirical bias^2 | "
      "top 1 % of the pixels carry | ratio without them")
G = a.groups
for h in a.halves:
    outs, ests = [], []
    for g in range(G):
        o.refresh()
        o.set_sample_base(g * 4096)
        hv = hl.Halves(W, H)
        for _ in range(2):
            o.sample(h)
            hv.update(o.image_buffer)
        got = be.blend_error(cfg, o.image_buffer, hv.a, feats, window=a.window, display=a.bias == "display")
        outs.append(lum(got.denoised))
        ests.append(got)
    outs = np.array(outs)
    var_emp = float(outs.var(0, ddof=1).mean())
    bias_emp = float(np.mean((outs.mean(0) - truth) ** 2)) - var_emp / G - tv
    mse_emp = float(np.mean((outs - truth) ** 2)) - tv
    e2 = np.array([e.error.astype(np.float64) ** 2 for e in ests])
    v = float(np.mean([e.variance.mean() for e in ests]))
    # (the display rule's bias2 is in display space already)
    b = float(np.mean([(e.bias2 if a.bias == "display" else e.slope.astype(np.float64) ** 2 * e.bias2).mean() for e in ests]))
    per_pixel = e2.mean(0)
    top = per_pixel >= np.quantile(per_pixel, 0.99)
    rest = float(per_pixel[~top].mean()) / (float(np.mean(((outs - truth) ** 2).mean(0)[~top])) - tv)
    print(f"  {h:4d} + {h:<4d} {e2.mean():.3e}       {mse_emp:.3e}      {e2.mean() / mse_emp:5.2f} | {v:.3e} / {var_emp:.3e} = {v / var_emp:4.2f} | "
          f"{b:.3e} / {bias_emp:.3e} = {b / bias_emp:5.2f} | {per_pixel[top].sum() / per_pixel.sum():.2f} | {rest:5.2f}")
o.close()
