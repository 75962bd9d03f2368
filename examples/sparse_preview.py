#!/usr/bin/env python3
"""Whole frames from a fraction of the pixels: sparse sampling on a lattice, completed by the filling denoise.

    python examples/sparse_preview.py [--size 256 256] [--spp 4] [--period 2 2] [--out out/sparse] [--coverage-fill] [--blend] [--bench]
                                      [--device-lattice]

Cornell v3.  First view: select_lattice -> sample_selected -> denoise_fill (rtpbr_denoise with option denoise_fill = 1: a pixel
without samples takes the feature-weighted mean of the sampled pixels of its object) -> present("denoised").  Then the camera
moves: reproject warps what the new view can reuse, and denoise_fill shows a whole frame before any new sample — the holes of the
move filled.  Then px * py frames of the rotating lattice (Renderer.lattice_phase), each tracing one pixel of every cell, after
which every pixel has samples.  Every step's frame is written as an image, next to the same step shown with its holes (denoise).
--bench prints blocking wall times of each step, and of select_lattice by itself on both of its paths: the default, whose mask is
built on the host and crosses to the device on every call, and select_lattice(device=True), where the library builds the same
selection on the device with one kernel and nothing crosses (option select_lattice).  --device-lattice selects that way in every
step: the same frames, bit for bit.  --coverage-fill fills with denoise_coverage_fill instead (rtpbr_denoise_coverage with option coverage_fill =
1: the holes filled inside the coverage-weighted levels, the two-object pixels resolved, filled ones included) and shows the holes
with denoise_coverage.  --blend fills with the level blend instead (denoise_blend_levels(fill=True): rtpbr_denoise_blend_levels with
option blend_fill = 1; with --coverage-fill its coverage-weighted form): the samples are dealt to the two halves as they are traced
and the halves are carried through the move (set_half_mode(per_sample=True, warp=True)), so the best filter of the library shows
every one of these frames without holes; the holes are shown with denoise_blend_levels.  Runs on the HIP library only.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raytracingpbr_amd import Camera, Config, Renderer, cornell_box      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, nargs=2, default=(256, 256))
ap.add_argument("--spp", type=int, default=4)
ap.add_argument("--period", type=int, nargs=2, default=(2, 2))
ap.add_argument("--out", default="out/sparse")
ap.add_argument("--coverage-fill", action="store_true")
ap.add_argument("--blend", action="store_true")
ap.add_argument("--bench", action="store_true")
ap.add_argument("--device-lattice", action="store_true")
a = ap.parse_args()

W, H = a.size
period = tuple(a.period)
scene, cfg = cornell_box("v3", aspect=W / H), Config.cornell_v3(W, H, 0, 3)
r = Renderer(scene, cfg)
if a.blend:
    r.set_half_mode(per_sample=True, warp=True)
os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)


def fill():
    if a.blend:
        return (r.denoise_blend_levels_coverage(fill=True) if a.coverage_fill else r.denoise_blend_levels(fill=True))[1]
    return r.denoise_coverage_fill()[1] if a.coverage_fill else r.denoise_fill()


def holes():
    if a.blend:
        return r.denoise_blend_levels_coverage() if a.coverage_fill else r.denoise_blend_levels()
    return r.denoise_coverage() if a.coverage_fill else r.denoise()


def show(step):
    filled, empty, deepest = fill()
    r.save_image(f"{a.out}_{step}_filled.png", "denoised")
    depth = f", mean blend depth {float(r.blend_depth.mean()):.2f}" if a.blend else ""
    holes()
    r.save_image(f"{a.out}_{step}_holes.png", "denoised")
    print(f"{step}: {filled} pixels filled, {empty} still empty, deepest level {deepest}{depth}")


# the first view: one pixel of every cell
n = r.select_lattice(period, (0, 0), device=a.device_lattice)
r.refresh()
r.sample_selected(a.spp)
print(f"Cornell v3 {W}x{H}: {n} of {W * H} pixels traced at {a.spp} spp")
show("first")

# a camera move: the warped history has holes where the new view sees what the old one did not
c = scene.camera
moved = Camera(lookfrom=(c.lookfrom[0] + 4.0, c.lookfrom[1] + 1.0, c.lookfrom[2]), lookat=tuple(c.lookat), vup=tuple(c.vup), vfov=c.vfov,
               aspect=W / H, aperture=c.aperture, focus=c.focus)
r.reproject(moved)
show("moved")

# the rotating lattice: every pixel of a cell once per px * py frames
for k in range(period[0] * period[1]):
    r.select_lattice(period, Renderer.lattice_phase(k, period), device=a.device_lattice)
    r.sample_selected(a.spp)
    show(f"frame{k}")

if a.bench:
    def ms(fn, reps=20):
        fn()
        r.sync()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        r.sync()
        return (time.perf_counter() - t0) / reps * 1e3

    def lattice_frame(device):
        r.select_lattice(period, (0, 0), device=device)
        r.sample_selected(1)

    r.select_lattice(period, (0, 0), device=a.device_lattice)
    r.refresh()
    r.sample_selected(a.spp)               # a sparse frame again: what denoise_fill is for
    print(f"wall ms per call at {W}x{H}, lattice {period}: select_lattice {ms(lambda: r.select_lattice(period, (0, 0))):.3f}, "
          f"select_lattice + sample_selected(1) {ms(lambda: lattice_frame(False)):.3f}, sample(1) {ms(lambda: r.sample(1)):.3f}")
    print(f"  built on the device: select_lattice {ms(lambda: r.select_lattice(period, (0, 0), device=True)):.3f}, "
          f"select_lattice + sample_selected(1) {ms(lambda: lattice_frame(True)):.3f}")
    r.select_lattice(period, (0, 0), device=a.device_lattice)
    r.refresh()
    r.sample_selected(a.spp)
    if a.blend:
        print(f"  denoise_blend_levels(fill=True) {ms(lambda: r.denoise_blend_levels(fill=True)):.3f}, "
              f"denoise_blend_levels {ms(r.denoise_blend_levels):.3f}")
    if a.coverage_fill:
        print(f"  denoise_coverage_fill {ms(r.denoise_coverage_fill):.3f}, denoise_coverage {ms(r.denoise_coverage):.3f}")
    print(f"  denoise_fill {ms(r.denoise_fill):.3f}, denoise {ms(r.denoise):.3f}, present {ms(lambda: r.present('denoised')):.3f}, "
          f"reproject {ms(lambda: r.reproject(moved)):.3f}")
