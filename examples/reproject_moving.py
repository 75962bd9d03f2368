#!/usr/bin/env python3
"""A moving object rendered two ways: refresh on every frame, or keep history with rtpbr_reproject_scene.

    python examples/reproject_moving.py                 # per-frame table with the library's default parameters
    python examples/reproject_moving.py --pan           # ... while the camera pans and dollies as well
    python examples/reproject_moving.py --sweep         # max_history 4..64 x depth_tolerance: the overall ratio of each setting
    python examples/reproject_moving.py --bench         # time of the call beside rtpbr_reproject at 768x432 and 1920x1080

Cornell v3 at 256x256, 4 spp per frame, 11 frames: the small box slides by (0.01, 0, 0.03) scene units and turns by 3 degrees
about y per frame.  For every frame after the first it prints the display RMSE against a converged frame of that pose (4096 spp,
independent samples) of
    refresh    set_scene (+ set_camera) + refresh + 4 spp: every frame starts from nothing;
    reproject  reproject_scene + 4 spp;
their ratio, and the ratio over all frames (root of the mean squared errors).  The history was lit by the old poses, so the
error is also split by region: the box's own pixels, the pixels the box's shadow and bounce light left (converged display value
up by more than 0.04 from the previous pose, 5x5 mean), those they reached (down by more than 0.04), and the rest.
Pixels without samples count as black.  Runs on the HIP library only.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raytracingpbr_amd import Camera, Config, Renderer, Scene, cornell_box      # noqa: E402
from raytracingpbr_amd.dataclass import ReprojectParams, SDFObject              # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=11)
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--spp", type=int, default=4)
ap.add_argument("--truth-spp", type=int, default=4096)
ap.add_argument("--pan", action="store_true")
ap.add_argument("--sweep", action="store_true")
ap.add_argument("--bench", action="store_true")
ap.add_argument("--out", default=None, help="write the numbers as JSON")
a = ap.parse_args()

BOX = 6          # Cornell's small box


def pose(scene, k):
    """frame k: the small box slid and turned k steps; every other word of the table is copied"""
    objs = [SDFObject.from_buffer_copy(bytes(o)) for o in scene.objects]
    t = objs[BOX].transform
    t.position[0] += 0.01 * k
    t.position[2] += 0.03 * k
    t.rotation[1] += 3.0 * k
    return Scene(objs, scene.scale10, scene.camera, scene.name)


def camera(cam, k):
    """--pan: 1 % of the eye-target distance sideways and 1.5 % towards the target per frame"""
    if not a.pan:
        return cam
    lf, la, up = (np.array(v, np.float64) for v in (cam.lookfrom, cam.lookat, cam.vup))
    dist = np.linalg.norm(la - lf)
    fwd = (la - lf) / dist
    x = np.cross(fwd, up)
    x /= np.linalg.norm(x)
    off = x * (0.01 * k * dist) + fwd * (0.015 * k * dist)
    return Camera(tuple(lf + off), tuple(la + off), tuple(cam.vup), cam.vfov, cam.aspect, cam.aperture, cam.focus)


def renderer(scene, cfg, cam):
    r = Renderer(scene, cfg, cam)
    r.set_option("jit", 0)      # a new pose per frame: the ahead-of-time kernels, no compiler in the loop
    return r


def display(r):
    r.post_process()
    return np.nan_to_num(r.image_pixels, nan=0.0)


def mse(x, y, m=None):
    d = ((x - y) ** 2).mean(axis=-1)
    return float(d.mean() if m is None else d[m].mean()) if (m is None or m.any()) else float("nan")


def blur5(x):
    p = np.pad(x, 2, mode="edge")
    return sum(p[i:i + x.shape[0], j:j + x.shape[1]] for i in range(5) for j in range(5)) / 25.0


def bench():
    rows = []
    for w, h in ((768, 432), (1920, 1080)):
        scene, cfg = cornell_box("v3", aspect=w / h), Config.cornell_v3(w, h, 0, 3)
        a.pan = True
        poses, cams = [pose(scene, k) for k in (0, 1)], [camera(scene.camera, k) for k in (0, 1)]
        r = renderer(poses[0], cfg, cams[0])
        r.refresh()
        r.sample(2)
        row = {"size": [w, h]}
        for moments in (False, True):
            if moments:
                r.noise_update()
            calls = {"reproject": lambda k: r.reproject(cams[k & 1]),
                     "reproject_scene": lambda k: r.reproject_scene(poses[k & 1], cams[k & 1]),
                     "reproject_scene_unmoved": lambda k: r.reproject_scene(poses[0], cams[k & 1])}
            for rep in range(3):                    # alternating, so that a drift of the machine shows in all alike
                for name, call in calls.items():
                    for k in range(1, 4):
                        call(k)                     # warm-up (and the old features are valid from here on)
                    r.sync()
                    n = 40
                    t0 = time.perf_counter()
                    for k in range(n):
                        call(k)
                    r.sync()
                    row.setdefault(name + ("+moments" if moments else ""), []).append((time.perf_counter() - t0) / n * 1e3)
                r.set_scene(poses[0])
                r.refresh()
                r.sample(1)
        rows.append(row)
        print(f"{w}x{h}: ms per call, host clock around 40 calls ending in a sync (best of 3; each call renders one feature frame)")
        for k, v in row.items():
            if k != "size":
                print(f"  {k:36s} {min(v):7.3f}   (runs: {', '.join(f'{x:.3f}' for x in v)})")
        for m in ("", "+moments"):
            print(f"  ratio reproject_scene / reproject{m}: {min(row['reproject_scene' + m]) / min(row['reproject' + m]):.3f}")
        r.close()
    return rows


def run(scene, cfg, truths, feats, params):
    """per moved frame: dict of mean squared display errors (refresh, reproject) overall and per region"""
    ref, rep = renderer(pose(scene, 0), cfg, camera(scene.camera, 0)), renderer(pose(scene, 0), cfg, camera(scene.camera, 0))
    for r in (ref, rep):
        r.refresh()
        r.sample(a.spp)
    rows = []
    for k in range(1, a.frames):
        sc, cam = pose(scene, k), camera(scene.camera, k)
        ref.set_scene(sc)
        if a.pan:
            ref.set_camera(cam)
        ref.refresh()
        ref.sample(a.spp)
        rep.reproject_scene(sc, cam if a.pan else None, **params)
        rep.sample(a.spp)
        x0, x1, t = display(ref), display(rep), truths[k]
        row = {"all": (mse(x0, t), mse(x1, t))}
        if not a.pan:               # (the regions compare converged frames pixel by pixel: a still camera only)
            lum = blur5(truths[k].mean(axis=-1)) - blur5(truths[k - 1].mean(axis=-1))
            box = (feats[k] == BOX) | (feats[k - 1] == BOX)
            regions = {"box": feats[k] == BOX, "shadow_left": ~box & (lum > 0.04), "shadow_reached": ~box & (lum < -0.04)}
            regions["rest"] = ~(regions["box"] | regions["shadow_left"] | regions["shadow_reached"])
            for name, m in regions.items():
                row[name] = (mse(x0, t, m), mse(x1, t, m), int(m.sum()))
        rows.append(row)
    ref.close()
    rep.close()
    return rows


def overall(rows, key="all"):
    e0 = np.sqrt(np.nanmean([r[key][0] for r in rows]))
    e1 = np.sqrt(np.nanmean([r[key][1] for r in rows]))
    return float(e0), float(e1), float(e1 / e0)


def main():
    if a.bench:
        out = {"bench": bench()}
    else:
        scene, cfg = cornell_box("v3"), Config.cornell_v3(a.size, a.size, 0, 3)
        truths, feats = [], []
        for k in range(a.frames):
            t = renderer(pose(scene, k), cfg, camera(scene.camera, k))
            t.set_option("sample_base", 1 << 20)          # samples independent of the frames'
            t.refresh()
            t.sample(a.truth_spp)
            truths.append(display(t))
            t.render_features()
            feats.append(t.feature_object)
            t.close()
        if a.sweep:
            out = {"sweep": []}
            print("max_history  depth_tolerance  overall RMSE refresh  reproject  ratio")
            for mh in (4.0, 8.0, 16.0, 32.0, 64.0):
                for tol in (0.02, 0.2):
                    e0, e1, ratio = overall(run(scene, cfg, truths, feats, {"max_history": mh, "depth_tolerance": tol}))
                    out["sweep"].append({"max_history": mh, "depth_tolerance": tol, "refresh": e0, "reproject": e1, "ratio": ratio})
                    print(f"{mh:11g}  {tol:15g}  {e0:20.4f}  {e1:9.4f}  {ratio:.3f}")
            best = min(out["sweep"], key=lambda s: s["ratio"])
            print(f"best: max_history {best['max_history']:g}, depth_tolerance {best['depth_tolerance']:g}: ratio {best['ratio']:.3f}")
        else:
            print("parameters:", ReprojectParams.DEFAULTS, "(the library's defaults)", "with --pan" if a.pan else "camera still")
            rows = run(scene, cfg, truths, feats, {})
            print("frame  refresh  reproject  ratio")
            for k, r in enumerate(rows, 1):
                e0, e1 = np.sqrt(r["all"])
                print(f"{k:5d}  {e0:7.4f}  {e1:9.4f}  {e1 / e0:.3f}")
            out = {"pan": a.pan, "overall": overall(rows)}
            print("  all  %7.4f  %9.4f  %.3f" % out["overall"])
            if not a.pan:
                print("by region (all frames): pixels per frame, display RMSE refresh, reproject, ratio")
                out["regions"] = {}
                for name in ("box", "shadow_left", "shadow_reached", "rest"):
                    e0, e1, ratio = overall(rows, name)
                    n = float(np.mean([r[name][2] for r in rows]))
                    out["regions"][name] = {"pixels": n, "refresh": e0, "reproject": e1, "ratio": ratio}
                    print(f"  {name:15s} {n:8.0f}  {e0:7.4f}  {e1:9.4f}  {ratio:.3f}")
    if a.out:
        json.dump(out, open(a.out, "w"), indent=1)


main()
