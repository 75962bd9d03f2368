#!/usr/bin/env python3
"""The bias-aware blend across the a-trous levels (Renderer.denoise_blend_levels, rtpbr_denoise_blend_levels): denoise_blend repairs
the filter's blur by giving way to the raw average and hands the noise back with it; the levels call judges every a-trous level
against the next finer one with the same two halves and narrows the filter instead.  Cornell v3.

    python examples/denoise_levels.py --size 256 256                       # raw / blend / levels against the denoised frame
    python examples/denoise_levels.py --size 64 64 --spp 16 64 --ref-spp 256 # a run of seconds
    python examples/denoise_levels.py --bench                              # the calls DESIGN.md section 6m times, 1920x1080 and 768x432
    python examples/denoise_levels.py --bench --bench-size 768 432         # ... one frame size (one size per profiled process)
    python examples/denoise_levels.py --coverage --size 64 64 --spp 32 128 512 # ... and the level blend on the coverage-weighted filter
    python examples/denoise_levels.py --coverage --bench --bench-size 1920 1080 # the calls DESIGN.md section 6s times, option off beside on

Prints, per sample count, the RMSE of the display luminance of the denoised frame against a converged frame (another seed), the
raw, the blended and the level-blended frame's as ratios to it, and the mean depth (levels kept); saves the last depth map
(white = the whole filter, black = the raw average).  --coverage adds, per sample count, the frame of
denoise_blend_levels_coverage (option blend_coverage: coverage-weighted ladders, two-object pixels resolved) beside
denoise_blend_levels' and denoise_coverage's, scored on the whole frame, on the pixels with coverage below 1 and on the interior
(one object in the 5x5 neighbourhood).  Headless; runs on the HIP library only.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raytracingpbr_amd import Config, Renderer, cornell_box, display_image      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, nargs=2, default=[256, 256])
ap.add_argument("--spp", type=int, nargs="+", default=[16, 32, 64, 128, 512], help="total samples per pixel of each row (two equal halves)")
ap.add_argument("--bounces", type=int, default=4)
ap.add_argument("--ref-spp", type=int, default=2048, help="samples per pixel of the converged frame (another seed)")
ap.add_argument("--radius", type=int, default=None)
ap.add_argument("--z", type=float, default=None)
ap.add_argument("--min-half-samples", type=int, default=None)
ap.add_argument("--iterations", type=int, default=None)
ap.add_argument("--depth-map", default="out/blend_depth.png")
ap.add_argument("--coverage", action="store_true", help="also the level blend on the coverage-weighted filter (option blend_coverage)")
ap.add_argument("--bench", action="store_true")
ap.add_argument("--bench-size", type=int, nargs=2, default=None, help="--bench at this frame alone (one size per profiled process)")
a = ap.parse_args()

if a.bench:      # device times: rocprofv3 --kernel-trace --stats -- python examples/denoise_levels.py --bench
    import time
    for W, H in ([tuple(a.bench_size)] if a.bench_size else [(1920, 1080), (768, 432)]):
        r = Renderer(cornell_box("v3", aspect=W / H), Config.cornell_v3(W, H, 0, a.bounces))
        for _ in range(2):
            r.sample(2)
            r.half_update()
        r.denoise()
        r.denoise_blend(3, 2.0, 1)
        r.denoise_blend_levels(3, 2.0, 1)
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
            for radius in (1, 2, 3):
                timed(f"denoise_blend, radius {radius}", lambda: r.denoise_blend(radius, 2.0, 1))
                timed(f"denoise_blend_levels, radius {radius}", lambda: r.denoise_blend_levels(radius, 2.0, 1))
            if a.coverage:      # option off beside option on, on the same frame (the coverage plane is rendered once: it lives as long as the features)
                timed("denoise_blend_levels, radius 3, blend_coverage 0", lambda: r.denoise_blend_levels(3, 2.0, 1))
                timed("denoise_blend_levels, radius 3, blend_coverage 1", lambda: r.denoise_blend_levels_coverage(radius=3, z=2.0, min_half_samples=1))
                timed("blend_error display, radius 3, blend_coverage 0", lambda: r.blend_error(0.0, 3, 2.0, 1, bias="display"))
                timed("blend_error display, radius 3, blend_coverage 1",
                      lambda: r.blend_error_coverage(0.0, radius=3, z=2.0, min_half_samples=1, bias="display"))
        print(f"{W}x{H}, Cornell v3, 12 rounds of sample(1), half_update, denoise, denoise_blend and denoise_blend_levels at radius 1 / 2 / 3")
        for what, ms in wall.items():
            print(f"    {what}: wall {np.mean(ms):.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}), blocking, with the launches' host time")
        del r
    sys.exit(0)

W, H = a.size
scene = cornell_box("v3", aspect=W / H)
cfg = Config.cornell_v3(W, H, 0, a.bounces)
denoise = {} if a.iterations is None else {"iterations": a.iterations}


def lum(c):
    c = np.clip(c, 0, 1).astype(np.float64)
    return 0.299 * c[..., 0] + 0.587 * c[..., 1] + 0.114 * c[..., 2]


def rmse(x, ref):
    return float(np.sqrt(np.mean((lum(x) - ref) ** 2)))


ref_r = Renderer(scene, cfg.copy(seed=12345))
ref_r.render(refreshing=True, spp=a.ref_spp)
ref = lum(ref_r.image_pixels)

rule = (a.radius, a.z, a.min_half_samples)
r = Renderer(scene, cfg)
done = 0
print(f"Cornell v3 {W}x{H}, RMSE of the display luminance against {a.ref_spp} spp; raw, blend and levels as ratios to the denoised frame's")
print("  halves      denoised     raw   blend   levels   levels / blend   mean depth   pixels narrowed")
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
    r.denoise(**denoise)
    raw, den = rmse(r.image_pixels, ref), rmse(r.denoised_pixels, ref)
    r.denoise_blend(*rule, **denoise)
    b = rmse(r.denoised_pixels, ref)
    st = r.denoise_blend_levels(*rule, **denoise)
    lv = rmse(r.denoised_pixels, ref)
    print(f"  {half:4d} + {half:<4d}   {den:.4f}   {raw / den:.3f}   {b / den:.3f}    {lv / den:.3f}   {lv / b:14.3f}   {float(r.blend_depth.mean()):10.2f}"
          f"   {st.pixels_above:8d} of {st.pixels_estimated}")
    if a.coverage:
        frames = {"denoise": None, "levels": r.denoised_pixels}
        r.denoise(**denoise)
        frames["denoise"] = r.denoised_pixels
        r.denoise_coverage(**denoise)
        frames["coverage"] = r.denoised_pixels
        _, resolved = r.denoise_blend_levels_coverage(None, None, None, *rule, **denoise)
        frames["new"] = r.denoised_pixels
        obj, cov = r.feature_object, r.coverage
        pad = np.pad(obj, 2, mode="edge")
        interior = np.ones(obj.shape, bool)
        for dx in range(5):
            for dy in range(5):
                interior &= pad[dx:dx + W, dy:dy + H] == obj
        for name, px in (("frame", np.ones(obj.shape, bool)), ("coverage below 1", cov[..., 0] < cov[..., 3]), ("interior", interior)):
            e = {k: float(np.sqrt(np.mean(((lum(v) - ref) ** 2)[px]))) for k, v in frames.items()}
            print(f"      {name} ({int(px.sum())} px): denoise {e['denoise']:.4f}  levels {e['levels']:.4f}  coverage {e['coverage']:.4f}  new {e['new']:.4f}"
                  f"   new / levels {e['new'] / e['levels']:.3f}   new / coverage {e['new'] / e['coverage']:.3f}")
        print(f"      pixels resolved: {resolved}")
        r.denoise_blend_levels(*rule, **denoise)      # (the depth map below is the plain call's)

from PIL import Image      # noqa: E402
os.makedirs(os.path.dirname(os.path.abspath(a.depth_map)), exist_ok=True)
K = max(float(r.blend_depth.max()), 1.0)
t = np.repeat((r.blend_depth / K)[..., None], 3, axis=2)
Image.fromarray((np.clip(display_image(t), 0, 1) * 255.0 + 0.5).astype(np.uint8)).save(a.depth_map)
print(f"depth map of the last row: {a.depth_map}")
