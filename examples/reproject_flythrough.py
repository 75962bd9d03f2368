#!/usr/bin/env python3
"""A camera fly-through (pan plus dolly) rendered three ways, and the sweep the rtpbr_reproject defaults
(include/rtpbr.h RTPBR_REPROJECT_DEFAULT_*) were chosen from.

    python examples/reproject_flythrough.py                      # the table, with the library's defaults
    python examples/reproject_flythrough.py --sweep --out reproject_sweep.json

Two scenes: Cornell v3 at 256x256 (4 spp per frame) and the src/ Tokyo scene at 256x144 (one launch of 4 bounce-steps per
frame).  Each frame of the path moves the camera by 1 % of its eye-target distance sideways and 1.5 % towards the target.  For
every frame after the first it prints the display RMSE against a converged frame at that camera (1024 spp / 16384
bounce-steps, independent samples) of
    refresh    set_camera + refresh + n spp (what the reference does while the camera moves, src/renderer.py:25-32);
    reproject  reproject + n spp;
    +denoise   reproject + n spp + denoise (default parameters).
Pixels without samples count as black.  The sweep scores every setting of max_history x depth_tolerance x normal_cos by the mean
over both scenes and all moved frames of RMSE(reproject) / RMSE(refresh); the defaults are the best setting.
Runs on the HIP library only.
"""
import argparse
import itertools
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raytracingpbr_amd import Camera, Config, Renderer, cornell_box, src_scene      # noqa: E402
from raytracingpbr_amd.dataclass import ReprojectParams                            # noqa: E402
from raytracingpbr_amd.ibl import synthetic_env                                    # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=12)
ap.add_argument("--sweep", action="store_true")
ap.add_argument("--out", default="reproject_sweep.json")
a = ap.parse_args()


def renderer(scene, cfg):
    r = Renderer(scene, cfg)
    if cfg.sky_kind == 1:      # RTPBR_SKY_ENVMAP
        r.set_env(synthetic_env(192, 96, seed=0), 1.4, 2.2)
    return r


def path(cam, n):
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


def display(x):
    return np.nan_to_num(x, nan=0.0)


def rmse(x, y):
    return float(np.sqrt(np.mean((x - y) ** 2)))


scenes = {
    "cornell_v3_256": (cornell_box("v3"), Config.cornell_v3(256, 256, 0, 3), lambda r: r.sample(4), lambda r: r.sample(1024), None),
    "src_tokyo_256x144": (src_scene(aspect=256 / 144), Config.src(256, 144, 7, steps_per_launch=4), lambda r: r.sample(1),
                          lambda r: [r.sample(64) for _ in range(64)], None),
}
truths = {}
for name, (scene, cfg, _, converge, _) in scenes.items():
    t = renderer(scene, cfg)
    t.set_option("sample_base", 1 << 20)          # samples independent of the frames'
    for k, cam in enumerate(path(scene.camera, a.frames)):
        t.set_camera(cam)
        t.refresh()
        converge(t)
        t.post_process()
        truths[name, k] = display(t.image_pixels)


def run(name, params, denoise=False):
    """per moved frame: (RMSE refresh, RMSE reproject, RMSE reproject + denoise or None)"""
    scene, cfg, per_frame, _, _ = scenes[name]
    cams = path(scene.camera, a.frames)
    ref, rep = renderer(scene, cfg), renderer(scene, cfg)
    for r in (ref, rep):
        r.set_camera(cams[0])
        r.refresh()
        per_frame(r)
    rows = []
    for k in range(1, len(cams)):
        ref.set_camera(cams[k])
        ref.refresh()
        per_frame(ref)
        ref.post_process()
        rep.reproject(cams[k], **params)
        per_frame(rep)
        rep.post_process()
        den = None
        if denoise:
            rep.denoise()
            den = rmse(display(rep.denoised_pixels), truths[name, k])
        rows.append((rmse(display(ref.image_pixels), truths[name, k]), rmse(display(rep.image_pixels), truths[name, k]), den))
    return rows


if a.sweep:
    grid = list(itertools.product([8.0, 16.0, 32.0, 64.0, 128.0], [0.01, 0.05, 0.2], [-1.0, 0.5, 0.9]))
    scores = []
    for g in grid:
        p = dict(zip(("max_history", "depth_tolerance", "normal_cos"), g))
        per = {n: float(np.mean([r[1] / r[0] for r in run(n, p)])) for n in scenes}
        scores.append({"setting": list(g), "ratio": per, "mean": float(np.mean(list(per.values())))})
    scores.sort(key=lambda s: s["mean"])
    for s in scores[:5]:
        print("max_history %g depth_tolerance %g normal_cos %g: " % tuple(s["setting"]) +
              ", ".join(f"{k} {v:.3f}" for k, v in s["ratio"].items()) + f", mean {s['mean']:.3f}")
    json.dump(scores, open(a.out, "w"), indent=1)
else:
    print("defaults:", ReprojectParams.DEFAULTS)
    for name in scenes:
        print(f"{name}: display RMSE against a converged frame")
        print("frame  refresh  reproject  +denoise")
        rows = run(name, {}, denoise=True)
        for k, (e0, e1, e2) in enumerate(rows, 1):
            print(f"{k:5d}  {e0:7.4f}  {e1:9.4f}  {e2:8.4f}")
        m = np.mean(np.array(rows), axis=0)
        print(f" mean  {m[0]:7.4f}  {m[1]:9.4f}  {m[2]:8.4f}")
