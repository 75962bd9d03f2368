#!/usr/bin/env python3
"""Adaptive sampling for a host that shows the DENOISED frame: sample until the estimated noise of the denoised picture is under
a threshold (Renderer.render_adaptive_denoised: half_update -> denoise_error -> select_error -> sample_selected), against
Renderer.render_adaptive, whose stop rule describes the raw average, at the same threshold and budget.  Cornell v3.

    python examples/adaptive_denoised.py --size 256 256 --error 0.03 --max-spp 256
    python examples/adaptive_denoised.py --size 64 64 --max-spp 32 --ref-spp 256       # a run of seconds
    python examples/adaptive_denoised.py --bench             # the calls DESIGN.md section 6j times, at 1920x1080
    python examples/adaptive_denoised.py --size 64 64 --max-spp 32 --ref-spp 256 --coverage   # ... ending with the coverage-aware level blend

Prints the pixel-samples both loops spent and both results' display RMSE against a converged frame.  The estimate is variance
only: the denoised frame stops moving early, and what remains of its error is the filter's bias, which more samples of the same
loop do not remove.  --coverage: the denoised loop ends with the level blend on the coverage-weighted
filter (render_adaptive_denoised(blend="levels", coverage=True)) instead of denoise().  Headless; runs on the
HIP library only.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raytracingpbr_amd import Config, Renderer, cornell_box      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, nargs=2, default=[256, 256])
ap.add_argument("--error", type=float, default=0.03)
ap.add_argument("--max-spp", type=int, default=256)
ap.add_argument("--batch", type=int, default=4, help="batch of the denoised loop (render_adaptive takes 4 x this, its default ratio)")
ap.add_argument("--dilate", type=int, default=1)
ap.add_argument("--bounces", type=int, default=4)
ap.add_argument("--ref-spp", type=int, default=2048, help="samples per pixel of the converged frame (other sample indices)")
ap.add_argument("--coverage", action="store_true", help='end the denoised loop with blend="levels", coverage=True')
ap.add_argument("--bench", action="store_true")
a = ap.parse_args()

if a.bench:      # device times: rocprofv3 --kernel-trace --stats -- python examples/adaptive_denoised.py --bench
    import time
    W, H = 1920, 1080
    r = Renderer(cornell_box("v3", aspect=W / H), Config.cornell_v3(W, H, 0, a.bounces))
    for _ in range(2):
        r.sample(2)
        r.half_update()
    r.denoise_error(a.error)
    r.denoise()
    wall = {}

    def timed(what, call):
        r.sync()
        t0 = time.perf_counter()
        call()
        r.sync()
        wall.setdefault(what, []).append((time.perf_counter() - t0) * 1e3)

    for _ in range(12):
        r.sample(1)
        timed("half_update", r.half_update)
        for radius in (1, 2, 3):
            timed(f"denoise_error, radius {radius}", lambda: r.denoise_error(a.error, radius))
        timed("two denoise calls", lambda: (r.denoise(), r.denoise()))
    print("1920x1080, Cornell v3, 12 rounds of sample(1), half_update, denoise_error at radius 1 / 2 / 3, denoise, denoise")
    for what, ms in wall.items():
        print(f"    {what}: wall {np.mean(ms):.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}), blocking, with the launches' host time")
    sys.exit(0)

W, H = a.size
scene = cornell_box("v3", aspect=W / H)
cfg = Config.cornell_v3(W, H, 0, a.bounces)


def rmse(x, ref):
    return float(np.sqrt(np.mean((np.clip(x, 0, 1).astype(np.float64) - ref) ** 2)))


ref_r = Renderer(scene, cfg.copy(seed=12345))
ref_r.render(refreshing=True, spp=a.ref_spp)
ref = np.clip(ref_r.image_pixels, 0, 1).astype(np.float64)
n_pix = W * H

r = Renderer(scene, cfg)
if a.coverage:
    traced, stats = r.render_adaptive_denoised(a.error, a.max_spp, a.batch, a.dilate, blend="levels", coverage=True)
    print(f"the loop ended with denoise_blend_levels_coverage: {r.counter('blend_resolved')} pixels resolved, "
          f"mean depth {float(r.blend_depth.mean()):.2f}")
else:
    traced, stats = r.render_adaptive_denoised(a.error, a.max_spp, a.batch, a.dilate)
r.post_process()
print(f"render_adaptive_denoised({a.error}): {traced} pixel-samples ({traced / n_pix:.1f} spp mean), "
      f"{stats.pixels_above} of {stats.pixels_estimated} pixels above, largest estimate {stats.max_noise:.4f}")
print(f"    display RMSE against {a.ref_spp} spp: denoised {rmse(r.denoised_pixels, ref):.4f}   raw {rmse(r.image_pixels, ref):.4f}")

s = Renderer(scene, cfg)
traced2, stats2 = s.render_adaptive(a.error, a.max_spp, min(4 * a.batch, max(1, a.max_spp // 2)), a.dilate)
s.post_process()
s.denoise()
print(f"render_adaptive({a.error}):          {traced2} pixel-samples ({traced2 / n_pix:.1f} spp mean), "
      f"{stats2.pixels_above} of {stats2.pixels_estimated} pixels above, largest estimate {stats2.max_noise:.4f}")
print(f"    display RMSE against {a.ref_spp} spp: denoised {rmse(s.denoised_pixels, ref):.4f}   raw {rmse(s.image_pixels, ref):.4f}")
print(f"samples spent, denoised loop / raw loop: {traced / max(traced2, 1):.3f}")
