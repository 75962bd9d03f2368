#!/usr/bin/env python3
"""A camera fly-through with adaptive sampling of the DENOISED frame, with and without the two switches of rtpbr_set_half_mode.

    python examples/adaptive_flythrough.py                       # Cornell v3 at 256x256, the 11 moves of reproject_flythrough.py
    python examples/adaptive_flythrough.py --size 64 64 --ref-spp 256 --frames 4      # a run of seconds
    python examples/adaptive_flythrough.py --bench               # the calls DESIGN.md section 6k times, at 1920x1080
    python examples/adaptive_flythrough.py --show-moves          # what a viewer sees right after each move, before any new sample

Every frame after the first is reproject(camera) + render_adaptive_denoised(error, max_spp, batch): two full-frame batches, then
denoise_error -> select_error -> sample_selected until the estimated noise of the denoised picture is under ``error``.  Four
settings:
    warp off / on        reproject zeroes half A (the whole history lies in B) / carries it with the image;
    per_sample off / on  a batch goes whole to one half (half_update after each call) / every sample is dealt by the sample call.
Per frame it prints the pixel-samples each setting spent and the display RMSE of its denoised frame against a converged frame at
that camera (independent samples).  --show-moves runs one more pass with warp on and samples dealt per sample, and shows each
moved frame BEFORE any new sample: denoise_blend_levels(fill=True) (option blend_fill: the disoccluded pixels filled by the level
blend's own ladders) against denoise_blend_levels (the same frame with its holes) and denoise_fill; then the frame's loop runs as
in the other settings, ending with the level blend.  Headless; runs on the HIP library only.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raytracingpbr_amd import Camera, Config, Renderer, cornell_box      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, nargs=2, default=[256, 256])
ap.add_argument("--frames", type=int, default=12, help="cameras of the path (the first is not a move)")
ap.add_argument("--error", type=float, default=0.03)
ap.add_argument("--max-spp", type=int, default=32, help="budget of one frame's loop")
ap.add_argument("--batch", type=int, default=4)
ap.add_argument("--dilate", type=int, default=1)
ap.add_argument("--bounces", type=int, default=3)
ap.add_argument("--ref-spp", type=int, default=1024, help="samples per pixel of the converged frames (other sample indices)")
ap.add_argument("--bench", action="store_true")
ap.add_argument("--show-moves", action="store_true")
a = ap.parse_args()


def path(cam, n):
    """each camera 1 % of the eye-target distance sideways and 1.5 % towards the target from the one before"""
    lf, la = np.array(cam.lookfrom, np.float64), np.array(cam.lookat, np.float64)
    up = np.array(cam.vup, np.float64)
    dist = np.linalg.norm(la - lf)
    fwd = (la - lf) / dist
    x = np.cross(fwd, up)
    x /= np.linalg.norm(x)
    out = []
    for k in range(n):
        off = x * (0.01 * k * dist) + fwd * (0.015 * k * dist)
        out.append(Camera(tuple(lf + off), tuple(la + off), tuple(cam.vup), cam.vfov, cam.aspect, cam.aperture, cam.focus))
    return out


if a.bench:      # device times: rocprofv3 --kernel-trace --stats -- python examples/adaptive_flythrough.py --bench
    W, H = 1920, 1080
    scene, cfg = cornell_box("v3", aspect=W / H), Config.cornell_v3(W, H, 0, a.bounces)
    cams = path(scene.camera, 2)
    new_api = Renderer(scene, cfg).api.has("set_half_mode")      # (an older library has neither switch: its kernels alone are timed)
    rounds = 12
    # the accumulate pass of sample(4): plain, noise-tracked, dealt, both
    for tracked, dealt in ((False, False), (True, False), (False, True), (True, True)):
        if dealt and not new_api:
            continue
        r = Renderer(scene, cfg)
        if tracked:
            r.set_noise_tracking(True)
        if dealt:
            r.set_half_mode(per_sample=True)
        for _ in range(rounds):
            r.sample(4)
        r.sync()
        r.close()
    # the gather of reproject and reproject_scene: without halves, with A zeroed, with A carried; moments absent and present
    for moments in (False, True):
        for halves, warp in ((False, False), (True, False), (True, True)):
            if warp and not new_api:
                continue
            r = Renderer(scene, cfg, cams[0])
            r.refresh()
            if warp:
                r.set_half_mode(warp=True)
            for _ in range(2):
                r.sample(2)
                if halves:
                    r.half_update()
                if moments:
                    r.noise_update()
            for k in range(rounds):
                r.reproject(cams[(k + 1) % 2])
                r.reproject_scene(scene, cams[k % 2])
            r.sync()
            r.close()
    print(f"1920x1080, Cornell v3: {rounds} x sample(4) per accumulate instance; {rounds} x reproject + reproject_scene per gather instance"
          + ("" if new_api else " (library without rtpbr_set_half_mode)"))
    sys.exit(0)

W, H = a.size
scene = cornell_box("v3", aspect=W / H)
cfg = Config.cornell_v3(W, H, 0, a.bounces)
cams = path(scene.camera, a.frames)
n_pix = W * H


def rmse(x, ref):
    return float(np.sqrt(np.mean((np.clip(np.nan_to_num(x, nan=0.0), 0, 1).astype(np.float64) - ref) ** 2)))


truth = Renderer(scene, cfg.copy(seed=12345))
truth.set_option("sample_base", 1 << 20)
refs = []
for cam in cams:
    truth.set_camera(cam)
    truth.refresh()
    truth.sample(a.ref_spp)
    truth.post_process()
    refs.append(np.clip(np.nan_to_num(truth.image_pixels, nan=0.0), 0, 1).astype(np.float64))

SETTINGS = [(False, False), (True, False), (False, True), (True, True)]      # (warp, per_sample)
rows = {}
for warp, per_sample in SETTINGS:
    r = Renderer(scene, cfg, cams[0])
    r.set_half_mode(warp=warp)
    r.refresh()
    out = []
    for k, cam in enumerate(cams):
        if k:
            r.reproject(cam)
        traced, stats = r.render_adaptive_denoised(a.error, a.max_spp, a.batch, a.dilate, per_sample=per_sample)
        out.append((traced, rmse(r.denoised_pixels, refs[k]), stats.pixels_above))
    rows[warp, per_sample] = out

name = lambda s: f"warp {'on ' if s[0] else 'off'} per_sample {'on ' if s[1] else 'off'}"      # noqa: E731
print(f"Cornell v3 {W}x{H}, error {a.error}, budget {a.max_spp} spp per frame in batches of {a.batch}: pixel-samples per pixel spent / display "
      f"RMSE of the denoised frame against {a.ref_spp} spp")
print("frame  " + "  ".join(f"{name(s):>28s}" for s in SETTINGS))
for k in range(len(cams)):
    print(f"{k:5d}  " + "  ".join(f"{rows[s][k][0] / n_pix:14.2f} / {rows[s][k][1]:.4f}     " for s in SETTINGS))
moved = slice(1, None) if len(cams) > 1 else slice(0, None)
print(" mean  " + "  ".join(f"{np.mean([t for t, _, _ in rows[s][moved]]) / n_pix:14.2f} / {np.mean([e for _, e, _ in rows[s][moved]]):.4f}     "
                             for s in SETTINGS) + "  (moved frames)")
print("final  " + "  ".join(f"{'RMSE':>14s} / {rows[s][-1][1]:.4f}     " for s in SETTINGS))

if a.show_moves:      # each moved frame as a viewer meets it: warped history, no new sample yet
    r = Renderer(scene, cfg, cams[0])
    r.set_half_mode(per_sample=True, warp=True)
    r.refresh()
    print("right after each move, before any new sample (warp on, per_sample on): pixels without samples / filled / still empty; display RMSE "
          "of denoise_blend_levels with its holes, denoise_fill, denoise_blend_levels(fill=True)")
    for k, cam in enumerate(cams):
        if k:
            r.reproject(cam)
            without = int((r.image_buffer[..., 3] == 0).sum())
            r.denoise_blend_levels()
            e_holes = rmse(r.denoised_pixels, refs[k])
            r.denoise_fill()
            e_fill = rmse(r.denoised_pixels, refs[k])
            _, (filled, empty, _) = r.denoise_blend_levels(fill=True)
            print(f"move {k:3d}: {without:6d} / {filled:6d} / {empty:6d}   {e_holes:.4f}  {e_fill:.4f}  {rmse(r.denoised_pixels, refs[k]):.4f}")
        r.render_adaptive_denoised(a.error, a.max_spp, a.batch, a.dilate, per_sample=True, blend="levels")
