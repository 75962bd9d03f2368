#!/usr/bin/env python3
"""rtpbr_denoise against rtpbr_denoise_coverage on silhouettes.

    python examples/denoise_edges.py [--size 256] [--spp 4] [--truth 2048] [--power P] [--grid 4] [--coverage-fill] [--bench]

Cornell v3: a noisy frame against a converged one of independent samples.  The score is the display RMSE on three pixel sets —
interior (the 5x5 neighbourhood holds one object), coverage below 1 (some sub-ray of the pixel leaves its object) and the whole
frame — for rtpbr_denoise, for rtpbr_denoise_coverage without the resolve, and with it.  --bench adds the wall time of the calls
(the coverage is rendered once per view: it lives as long as the features).  --coverage-fill adds a sparse frame of the same view: samples
on one pixel in four (select_lattice + sample_selected), shown by denoise_fill and by denoise_coverage_fill (option coverage_fill:
the holes filled inside the coverage-weighted levels and resolved).  Runs on the HIP library only.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raytracingpbr_amd import Config, Renderer, cornell_box      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--spp", type=int, default=4)
ap.add_argument("--truth", type=int, default=2048)
ap.add_argument("--power", type=int, default=None)
ap.add_argument("--grid", type=int, default=4)
ap.add_argument("--coverage-fill", action="store_true")
ap.add_argument("--bench", action="store_true")
a = ap.parse_args()

scene, cfg = cornell_box("v3"), Config.cornell_v3(a.size, a.size, 0, 3)
t = Renderer(scene, cfg)
t.set_option("sample_base", 1 << 20)          # samples independent of the noisy frame's
t.sample(a.truth)
t.post_process()
truth = t.image_pixels.astype(np.float64)
t.close()

r = Renderer(scene, cfg)
r.sample(a.spp)
r.render_coverage(a.grid)
obj, cov = r.feature_object, r.coverage
W, H = obj.shape
pad = np.pad(obj, 2, mode="edge")
interior = np.ones((W, H), bool)
for dx in range(5):
    for dy in range(5):
        interior &= pad[dx:dx + W, dy:dy + H] == obj
sets = {"interior": interior, "coverage < 1": cov[..., 0] < cov[..., 3], "frame": np.ones((W, H), bool)}
print(f"Cornell v3 {W}x{H}, {a.spp} spp against {a.truth}: " + ", ".join(f"{k} {int(m.sum())} px" for k, m in sets.items()))


def score(name):
    se = (r.denoised_pixels.astype(np.float64) - truth) ** 2
    print(f"  {name:34s}" + "  ".join(f"{k} {np.sqrt(se[m].mean()):.4f}" for k, m in sets.items()))


r.denoise()
score("denoise")
st = r.denoise_coverage(power=a.power, resolve=0)
score("denoise_coverage, no resolve")
st = r.denoise_coverage(power=a.power, resolve=1)
score("denoise_coverage")
print(f"  candidates {st.pixels_above}, resolved {st.pixels_estimated}, largest 1 - coverage {st.max_noise:.4f}")

if a.coverage_fill:
    r.select_lattice((2, 2), (0, 0))
    r.refresh()
    r.sample_selected(a.spp)
    print(f"the same view, {a.spp} new spp on the (2,2) lattice only (one pixel in four):")
    r.denoise_coverage(power=a.power)
    score("denoise_coverage, with its holes")
    counts = r.denoise_fill()
    score("denoise_fill")
    st, counts_c = r.denoise_coverage_fill(power=a.power, grid=a.grid)
    score("denoise_coverage_fill")
    print(f"  filled / still empty / deepest level: denoise_fill {counts}, denoise_coverage_fill {counts_c}; resolved {st.pixels_estimated}")

if a.bench:
    def ms(fn, n=20):
        fn()
        r.sync()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        r.sync()
        return (time.perf_counter() - t0) / n * 1e3

    def fresh_coverage():
        r.render_features()                   # (the coverage goes with the features: this makes it stale)
        r.render_coverage(a.grid)

    f = ms(r.render_features)
    print(f"  wall ms per call: render_features {f:.3f}, render_coverage (candidates + sub-rays) {ms(fresh_coverage) - f:.3f}, "
          f"denoise {ms(r.denoise):.3f}, denoise_coverage {ms(lambda: r.denoise_coverage(power=a.power)):.3f}")
    if a.coverage_fill:                       # (on the lattice frame)
        print(f"  denoise_fill {ms(r.denoise_fill):.3f}, denoise_coverage_fill {ms(lambda: r.denoise_coverage_fill(power=a.power)):.3f}")
