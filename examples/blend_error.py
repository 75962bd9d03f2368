#!/usr/bin/env python3
"""The error estimate of the level-blended frame (Renderer.blend_error, rtpbr_blend_error): how wrong is the frame that
denoise_blend_levels shows?  The levels' weights are applied to each half's own ladder; the difference of the two blended halves
gives the variance, the product of their (blended - raw) the squared bias the halves can see.  Cornell v3.

    python examples/blend_error.py --size 256 256                         # the estimate next to the true error, per sample count
    python examples/blend_error.py --size 64 64 --spp 32 128 --ref-spp 512  # a run of seconds
    python examples/blend_error.py --size 256 256 --bias display          # the bias in display space per tap (rtpbr_blend_error_display)
    python examples/blend_error.py --bench                                # both estimates beside denoise_blend_levels, wall times

Prints, per sample count, the estimated root-mean-square error of the display luminance (the root of the mean of the plane's
squares) and the true error of the blended frame against a longer render (another seed); saves the blended frame and the error
map of the last row (white = --map-white or more).  On this scene the estimate overstates the error
several times — the bias term, beside the light: DESIGN.md section 6n — and with --bias display it does not (section 6o).
Headless; runs on the HIP library only.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raytracingpbr_amd import Config, Renderer, cornell_box, display_image      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, nargs=2, default=[256, 256])
ap.add_argument("--spp", type=int, nargs="+", default=[32, 64, 128, 512], help="total samples per pixel of each row (two equal halves)")
ap.add_argument("--bounces", type=int, default=4)
ap.add_argument("--ref-spp", type=int, default=4096, help="samples per pixel of the longer render (another seed)")
ap.add_argument("--radius", type=int, default=None)
ap.add_argument("--z", type=float, default=None)
ap.add_argument("--min-half-samples", type=int, default=None)
ap.add_argument("--window", type=int, default=None)
ap.add_argument("--iterations", type=int, default=None)
ap.add_argument("--out", default="out/blend_error_frame.png")
ap.add_argument("--error-map", default="out/blend_error_map.png")
ap.add_argument("--map-white", type=float, default=0.25, help="the error shown as white in the map")
ap.add_argument("--bias", choices=("linear", "display"), default="linear", help="blend_error's bias rule")
ap.add_argument("--bench", action="store_true")
a = ap.parse_args()

if a.bench:
    import time
    for W, H in ((1920, 1080), (768, 432)):
        r = Renderer(cornell_box("v3", aspect=W / H), Config.cornell_v3(W, H, 0, a.bounces))
        for _ in range(2):
            r.sample(2)
            r.half_update()
        r.denoise_blend_levels(3, 2.0, 1)
        r.blend_error(0.0, 3, 2.0, 1)
        r.blend_error(0.0, 3, 2.0, 1, bias="display")
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
            timed("denoise_blend_levels, radius 3", lambda: r.denoise_blend_levels(3, 2.0, 1))
            for window in (1, 2, 3):
                timed(f"blend_error, radius 3, window {window}", lambda: r.blend_error(0.0, 3, 2.0, 1, window))
                timed(f"blend_error, radius 3, window {window}, bias display", lambda: r.blend_error(0.0, 3, 2.0, 1, window, bias="display"))
        print(f"{W}x{H}, Cornell v3, 12 rounds of sample(1), half_update, denoise_blend_levels and blend_error with either bias")
        for what, ms in wall.items():
            print(f"    {what}: wall {np.mean(ms):.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}), blocking, with the launches' host time")
        del r
    sys.exit(0)

W, H = a.size
scene = cornell_box("v3", aspect=W / H)
cfg = Config.cornell_v3(W, H, 0, a.bounces)
denoise = {} if a.iterations is None else {"iterations": a.iterations}


def lum(c):
    c = np.asarray(c, np.float64)
    return 0.299 * c[..., 0] + 0.587 * c[..., 1] + 0.114 * c[..., 2]


ref_r = Renderer(scene, cfg.copy(seed=12345))
ref_r.render(refreshing=True, spp=a.ref_spp)
ref = lum(ref_r.image_pixels)

r = Renderer(scene, cfg)
done = 0
print(f"Cornell v3 {W}x{H}, root-mean-square error of the blended frame's display luminance: estimated ({a.bias} bias), and true against {a.ref_spp} spp")
print("  halves      estimated   true    estimated / true   median estimate   largest estimate")
for spp in sorted(a.spp):
    half = spp // 2
    if half * 2 <= done or half < 1:
        continue
    r.refresh()                     # two equal batches: A, then B
    for _ in range(2):
        r.sample(half)
        r.half_update()
    done = 2 * half
    st = r.blend_error(0.0, a.radius, a.z, a.min_half_samples, a.window, bias=a.bias, **denoise)
    err = r.blend_error_map.astype(np.float64)
    est = float(np.sqrt(np.mean(err ** 2)))
    true = float(np.sqrt(np.mean((lum(r.denoised_pixels) - ref) ** 2)))
    print(f"  {half:4d} + {half:<4d}   {est:.4f}    {true:.4f}   {est / true:12.2f}   {float(np.median(err)):15.4f}   {st.max_noise:14.4f}")

from PIL import Image      # noqa: E402
for path, img in ((a.out, r.denoised_pixels), (a.error_map, np.repeat((r.blend_error_map / a.map_white)[..., None], 3, axis=2))):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    Image.fromarray((np.clip(display_image(img), 0, 1) * 255.0 + 0.5).astype(np.uint8)).save(path)
print(f"blended frame of the last row: {a.out}; its error map (white = {a.map_white}): {a.error_map}")
