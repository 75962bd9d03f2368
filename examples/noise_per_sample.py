#!/usr/bin/env python3
"""Per-sample noise tracking (Renderer.set_noise_tracking): every sample is a batch of the noise estimate, folded into the
moments by sample() itself, so ONE call of 8 spp gives an estimate with 7 degrees of freedom per pixel — enough for the
variance-guided denoise and for adaptive sampling without a second full-frame batch.

    python examples/noise_per_sample.py --size 256 256 --spp 8 --out out/per_sample      # guided denoise from one call, then adaptive
    python examples/noise_per_sample.py --bench               # the device times of DESIGN.md section 6i

Headless.  Runs on the HIP library only.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raytracingpbr_amd import Config, Renderer, cornell_box      # noqa: E402
from raytracingpbr_amd.imageio import imwrite                    # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, nargs=2, default=[256, 256])
ap.add_argument("--spp", type=int, default=8)
ap.add_argument("--noise", type=float, default=0.1)
ap.add_argument("--max-spp", type=int, default=1024)
ap.add_argument("--dilate", type=int, default=1)
ap.add_argument("--bounces", type=int, default=3)
ap.add_argument("--out", default="out/per_sample")
ap.add_argument("--bench", action="store_true")
a = ap.parse_args()


def accumulate_ms(r, K, reps=4):
    """best (total - trace) device time of sample(K): what follows the trace kernels, i.e. the accumulate pass(es)"""
    best = None
    for rep in range(reps + 1):
        r.sample(K)
        trace, total, _ = r.last_sample_ms()
        ms = total - trace
        best = ms if rep and (best is None or ms < best) else best
    return best


def update_ms(r, K, reps=4):
    """best wall time of noise_update() between two syncs, new samples deposited before each"""
    best = None
    for rep in range(reps + 1):
        r.sample(K)
        r.sync()
        t0 = time.perf_counter()
        r.noise_update()
        r.sync()
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if rep and (best is None or dt < best) else best
    return best


def bench():
    W, H = 1920, 1080
    scene, cfg = cornell_box("v3", aspect=W / H), Config.cornell_v3(W, H, 0, 3)
    print(f"# {W}x{H} Cornell v3: device ms of sample(K) after its trace kernels (rtpbr_last_sample_ms total - trace), best of 4")
    for K in (4, 16, 256):
        plain, tracked = Renderer(scene, cfg), Renderer(scene, cfg)
        tracked.set_noise_tracking(True)
        p = accumulate_ms(plain, K)
        u = update_ms(plain, K)
        t = accumulate_ms(tracked, K)
        print(f"K = {K}: untracked accumulate {p:.3f} ms + noise_update {u:.3f} ms (wall, synchronised) = {p + u:.3f} ms; "
              f"tracked accumulate {t:.3f} ms ({t - p:+.3f} ms on the pass; traffic per pixel {12 * K + 32} + 80 -> {12 * K + 80} bytes)")
        del plain, tracked


if a.bench:
    bench()
    sys.exit(0)

W, H = a.size
scene, cfg = cornell_box("v3", aspect=W / H), Config.cornell_v3(W, H, 0, a.bounces)
r = Renderer(scene, cfg)
r.set_noise_tracking(True)
r.refresh()
r.sample(a.spp)                      # one call: spp batches of the estimate
st = r.noise_estimate(a.noise)
r.post_process()
r.denoise_guided()
if os.path.dirname(a.out):
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
imwrite(r.image_pixels, a.out + "_noisy.png")
imwrite(r.denoised_pixels, a.out + "_guided.png")
print(f"{W}x{H}, one call of {a.spp} spp: {int(r.moments[..., 3].min())} batches per pixel, {st.pixels_above} of {st.pixels_estimated} "
      f"pixels above noise {a.noise}, max {st.max_noise:.4f}")
# ... and on from the same samples: no second full-frame batch before the first selection
traced = W * H * a.spp
used = a.spp
while used + a.spp <= a.max_spp:
    n_sel = r.select_noisy(a.noise, a.dilate)
    if n_sel == 0:
        break
    r.sample_selected(a.spp)
    traced, used = traced + n_sel * a.spp, used + a.spp
st = r.noise_estimate(a.noise)
r.post_process()
count = r.image_buffer[..., 3]
imwrite(r.image_pixels, a.out + "_adaptive.png")
print(f"adaptive from there (dilate {a.dilate}): {traced} pixel-samples = {traced / (W * H):.1f} spp mean, {count.min():.0f}..{count.max():.0f} "
      f"per pixel, {st.pixels_above} pixels above")
print("wrote", a.out + "_noisy.png,", a.out + "_guided.png and", a.out + "_adaptive.png")
