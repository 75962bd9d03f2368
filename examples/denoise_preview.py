#!/usr/bin/env python3
"""Noisy and denoised frames side by side: N samples per pixel, then rtpbr_denoise (the reference's post_process() TODO).

    python examples/denoise_preview.py --size 512 512 --spp 4 --out out/denoise

writes <out>_noisy.png (image_pixels, what post_process shows) and <out>_denoised.png (denoised_pixels).  Runs on the HIP
library only.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raytracingpbr_amd import Config, Renderer, cornell_box            # noqa: E402
from raytracingpbr_amd.imageio import imwrite                          # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, nargs=2, default=[512, 512])
ap.add_argument("--spp", type=int, default=4)
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--iterations", type=int, default=None, help="a-trous levels (library default if omitted)")
ap.add_argument("--out", default="denoise")
a = ap.parse_args()
W, H = a.size
r = Renderer(cornell_box("v3", aspect=W / H), Config.cornell_v3(W, H, a.seed))
r.render(refreshing=True, spp=a.spp)
t0 = time.time()
r.denoise(iterations=a.iterations)
r.sync()
dt = time.time() - t0
if os.path.dirname(a.out):
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
imwrite(r.image_pixels, a.out + "_noisy.png")
imwrite(r.denoised_pixels, a.out + "_denoised.png")
print(f"{a.out}_noisy.png, {a.out}_denoised.png: {W}x{H}, {a.spp} spp, denoise {dt * 1e3:.2f} ms wall (features included)")
