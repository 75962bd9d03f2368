#!/usr/bin/env python3
"""The bias-aware blend of the denoised and the raw frame (Renderer.denoise_blend, rtpbr_denoise_blend): the a-trous filter's error
stops falling once the noise is gone — what is left is blur —, the raw average keeps converging, and the two halves of
half_update() show where the one should give way to the other.  Cornell v3.

    python examples/denoise_blend.py --size 256 256                       # raw / denoised / blended RMSE at growing sample counts
    python examples/denoise_blend.py --size 64 64 --spp 8 32 --ref-spp 256 # a run of seconds
    python examples/denoise_blend.py --size 64 64 --sweep                  # radius {2, 3} x z {1, 2, 3} x min_half_samples {4, 8, 16}
    python examples/denoise_blend.py --bench                               # the calls DESIGN.md section 6l times, at 1920x1080

Prints, per sample count, the RMSE of the display luminance of the raw, the denoised and the blended frame against a converged
frame (another seed), and the mean weight; saves the last weight map (white = the denoised colour, black = the raw one).
Headless; runs on the HIP library only.
"""
import argparse
import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raytracingpbr_amd import Config, Renderer, cornell_box, display_image      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, nargs=2, default=[256, 256])
ap.add_argument("--spp", type=int, nargs="+", default=[8, 16, 32, 128, 512], help="total samples per pixel of each row (two equal halves)")
ap.add_argument("--bounces", type=int, default=4)
ap.add_argument("--ref-spp", type=int, default=2048, help="samples per pixel of the converged frame (another seed)")
ap.add_argument("--radius", type=int, default=None)
ap.add_argument("--z", type=float, default=None)
ap.add_argument("--min-half-samples", type=int, default=None)
ap.add_argument("--sweep", action="store_true")
ap.add_argument("--weight-map", default="out/blend_weight.png")
ap.add_argument("--bench", action="store_true")
a = ap.parse_args()

if a.bench:      # device times: rocprofv3 --kernel-trace --stats -- python examples/denoise_blend.py --bench
    import time
    W, H = 1920, 1080
    r = Renderer(cornell_box("v3", aspect=W / H), Config.cornell_v3(W, H, 0, a.bounces))
    for _ in range(2):
        r.sample(2)
        r.half_update()
    r.denoise()
    r.denoise_error(0.03)
    r.denoise_blend(3, 2.0, 1)
    wall = {}

    def timed(what, call):
        r.sync()
        t0 = time.perf_counter()
        call()
        r.sync()
        wall.setdefault(what, []).append((time.perf_counter() - t0) * 1e3)

    for _ in range(12):
        r.sample(1)
        r.half_update()
        timed("denoise", r.denoise)
        timed("denoise_error, radius 3", lambda: r.denoise_error(0.03, 3))
        for radius in (1, 2, 3):
            timed(f"denoise_blend, radius {radius}", lambda: r.denoise_blend(radius, 2.0, 1))
    print("1920x1080, Cornell v3, 12 rounds of sample(1), half_update, denoise, denoise_error at radius 3, denoise_blend at radius 1 / 2 / 3")
    for what, ms in wall.items():
        print(f"    {what}: wall {np.mean(ms):.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}), blocking, with the launches' host time")
    sys.exit(0)

W, H = a.size
scene = cornell_box("v3", aspect=W / H)
cfg = Config.cornell_v3(W, H, 0, a.bounces)


def lum(c):
    c = np.clip(c, 0, 1).astype(np.float64)
    return 0.299 * c[..., 0] + 0.587 * c[..., 1] + 0.114 * c[..., 2]


def rmse(x, ref):
    return float(np.sqrt(np.mean((lum(x) - ref) ** 2)))


ref_r = Renderer(scene, cfg.copy(seed=12345))
ref_r.render(refreshing=True, spp=a.ref_spp)
ref = lum(ref_r.image_pixels)

settings = [(a.radius, a.z, a.min_half_samples)]
if a.sweep:
    settings = list(itertools.product((2, 3), (1.0, 2.0, 3.0), (4, 8, 16)))
rows = {s: [] for s in settings}
r = Renderer(scene, cfg)
done = 0
print(f"Cornell v3 {W}x{H}, RMSE of the display luminance against {a.ref_spp} spp")
print("  halves      raw   denoised" + ("" if a.sweep else "    blended   blended / denoised   mean weight   pixels blended"))
for spp in sorted(a.spp):
    half = spp // 2
    if half * 2 <= done or half < 1:
        continue
    r.refresh()                     # two equal batches: A, then B
    for _ in range(2):
        r.sample(half)
        r.half_update()
    done = 2 * half
    r.post_process()
    r.denoise()
    raw, den = rmse(r.image_pixels, ref), rmse(r.denoised_pixels, ref)
    line = f"  {half:4d} + {half:<4d} {raw:.4f}   {den:.4f}"
    for s in settings:
        st = r.denoise_blend(*s)
        b = rmse(r.denoised_pixels, ref)
        rows[s].append(b / den)
        if not a.sweep:
            line += f"     {b:.4f}   {b / den:18.3f}   {float(r.blend_weight.mean()):11.3f}   {st.pixels_above:8d} of {st.pixels_estimated}"
    print(line)

if a.sweep:
    print("  blended / denoised per row, and the worst row")
    print("  radius   z   min_half_samples   " + "   ".join(f"{s // 2}+{s // 2}" for s in sorted(a.spp)) + "   worst")
    for s, q in rows.items():
        print(f"  {s[0]:6d} {s[1]:3g} {s[2]:18d}   " + "   ".join(f"{x:.3f}" for x in q) + f"   {max(q):.3f}")
else:
    from PIL import Image
    os.makedirs(os.path.dirname(os.path.abspath(a.weight_map)), exist_ok=True)
    t = np.repeat(r.blend_weight[..., None], 3, axis=2)
    Image.fromarray((np.clip(display_image(t), 0, 1) * 255.0 + 0.5).astype(np.uint8)).save(a.weight_map)
    print(f"weight map of the last row: {a.weight_map}")
