#!/usr/bin/env python3
"""The noise estimate at work: the variance-guided a-trous against the plain one, and a render that stops by itself.

    python examples/noise_guided.py                          # the tables, with the library's defaults
    python examples/noise_guided.py --sweep --out noise_guided_sweep.json
    python examples/noise_guided.py --bench                  # the cost of tracking on the headline configuration

Still frames: the two scenes of examples/denoise_sweep.py (Cornell v3 256x256, 4 spp against 1024; the src/ Tokyo scene 256x144,
16 bounce-steps against 16384), rendered as two batches so that every pixel has a temporal estimate.  The score is that sweep's:
display RMSE over the pixels whose 5x5 neighbourhood holds one object, relative to the noisy frame's.
Fly-through: the path, scenes and score of examples/reproject_flythrough.py (display RMSE of the whole frame against a converged
frame per camera, pixels without samples black), every frame one batch, the moments reprojected with the image.
--sweep scores sigma_color x variance_floor x iterations of rtpbr_denoise_guided on the two still frames and ranks by the worst
case over both, the way DESIGN.md section 6b chose rtpbr_denoise's defaults.
Last, Renderer.render_until on Cornell v3: sample until no pixel's estimated noise exceeds the threshold.
Runs on the HIP library only.
"""
import argparse
import itertools
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raytracingpbr_amd import Camera, Config, Renderer, cornell_box, src_scene      # noqa: E402
from raytracingpbr_amd.dataclass import DenoiseGuidedParams                        # noqa: E402
from raytracingpbr_amd.ibl import synthetic_env                                    # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=12)
ap.add_argument("--sweep", action="store_true")
ap.add_argument("--bench", action="store_true")
ap.add_argument("--out", default="noise_guided_sweep.json")
ap.add_argument("--pool-batches", type=int, default=8, help="the pooled estimator of the 'pooled' columns (set_noise_estimator)")
ap.add_argument("--pool-radius", type=int, default=3)
a = ap.parse_args()


def renderer(scene, cfg):
    r = Renderer(scene, cfg)
    if cfg.sky_kind == 1:      # RTPBR_SKY_ENVMAP
        r.set_env(synthetic_env(192, 96, seed=0), 1.4, 2.2)
    return r


def single_object_mask(obj):
    w, h = obj.shape
    p = np.pad(obj, 2, constant_values=-2)
    m = np.ones_like(obj, bool)
    for dx in range(5):
        for dy in range(5):
            m &= p[dx:dx + w, dy:dy + h] == obj
    return m[..., None].repeat(3, axis=2)


def rmse(x, y, m=None):
    d = (x - y) ** 2
    return float(np.sqrt(np.mean(d[m] if m is not None else d)))


def display(x):
    return np.nan_to_num(x, nan=0.0)


if a.bench:
    # bench.py's Cornell configuration: one 256-spp call, then 16 calls of 16 spp with track_noise
    cfg, scene = Config.cornell_v3(1920, 1080, 0, 3), cornell_box("v3", aspect=1920 / 1080)
    for label, calls, per, track in (("one call of 256 spp", 1, 256, False), ("16 calls of 16 spp, track_noise", 16, 16, True)):
        r = renderer(scene, cfg)
        r.set_option("jit", 1)
        r.set_option("jit_bake", 1)
        r.track_noise = track
        best = None
        for rep in range(4):      # the first repetition compiles and warms up
            r.refresh()
            r.sync()
            t0 = time.perf_counter()
            for _ in range(calls):
                r.sample(per)
            r.sync()
            dt = time.perf_counter() - t0
            best = dt if rep and (best is None or dt < best) else best
        print(f"{label}: {1920 * 1080 * 256 / best / 1e6:.0f} Msamples/s ({best * 1e3:.1f} ms)")
    sys.exit(0)

stills = {
    "cornell_v3_256": (cornell_box("v3"), Config.cornell_v3(256, 256, 0, 3), 2, lambda r: r.sample(1024)),
    "src_tokyo_256x144": (src_scene(aspect=256 / 144), Config.src(256, 144, 7, steps_per_launch=4), 2,
                          lambda r: [r.sample(64) for _ in range(64)]),
}
grid = list(itertools.product([4, 5], [1.0, 2.0, 4.0, 8.0, 16.0], [1e-6, 1e-5, 1e-4, 1e-3]))      # iterations, sigma colour, floor
print("guided defaults:", DenoiseGuidedParams.DEFAULTS)
scores = {}
for name, (scene, cfg, per_batch, truth_run) in stills.items():
    t = renderer(scene, cfg)
    t.set_option("sample_base", 1 << 20)          # samples independent of the noisy frame's
    truth_run(t)
    t.post_process()
    truth = t.image_pixels
    r = renderer(scene, cfg)
    r.track_noise = True
    r.sample(per_batch)
    r.sample(per_batch)
    r.post_process()
    r.render_features()
    m = single_object_mask(r.feature_object)
    base = rmse(r.image_pixels, truth, m)
    r.denoise()
    plain = rmse(r.denoised_pixels, truth, m) / base
    r.denoise_guided()
    guided = rmse(r.denoised_pixels, truth, m) / base
    r.set_noise_estimator(a.pool_batches, a.pool_radius)
    r.denoise_guided()
    pooled = rmse(r.denoised_pixels, truth, m) / base
    r.set_noise_estimator()
    print(f"{name}: noisy {base:.4f}; relative to it: denoise() {plain:.3f}, denoise_guided() {guided:.3f}, "
          f"denoise_guided() with the estimate pooled ({a.pool_batches} batches, radius {a.pool_radius}) {pooled:.3f}")
    if a.sweep:
        for g in grid:
            r.denoise_guided(iterations=g[0], sigma_color=g[1], variance_floor=g[2])
            scores.setdefault(g, {})[name] = rmse(r.denoised_pixels, truth, m) / base
if a.sweep:
    ranked = sorted(scores.items(), key=lambda kv: max(kv[1].values()))
    for g, s in ranked[:5]:
        print("iterations %d sigma colour %.1f floor %g: " % g + ", ".join(f"{k} {v:.3f}" for k, v in s.items()))
    json.dump([{"setting": list(g), "ratio": s} for g, s in ranked], open(a.out, "w"), indent=1)
    sys.exit(0)


def path(cam, n):
    lf, la = np.array(cam.lookfrom, np.float64), np.array(cam.lookat, np.float64)
    up = np.array(cam.vup, np.float64)
    dist = np.linalg.norm(la - lf)
    fwd = (la - lf) / dist
    x = np.cross(fwd, up)
    x /= np.linalg.norm(x)
    return [Camera(tuple(lf + x * (0.01 * k * dist) + fwd * (0.015 * k * dist)), tuple(la + x * (0.01 * k * dist) + fwd * (0.015 * k * dist)),
                   tuple(cam.vup), cam.vfov, cam.aspect, cam.aperture, cam.focus) for k in range(n)]


fly = {
    "cornell_v3_256": (cornell_box("v3"), Config.cornell_v3(256, 256, 0, 3), lambda r: r.sample(4), lambda r: r.sample(1024)),
    "src_tokyo_256x144": (src_scene(aspect=256 / 144), Config.src(256, 144, 7, steps_per_launch=4), lambda r: r.sample(1),
                          lambda r: [r.sample(64) for _ in range(64)]),
}
for name, (scene, cfg, per_frame, converge) in fly.items():
    cams = path(scene.camera, a.frames)
    t = renderer(scene, cfg)
    t.set_option("sample_base", 1 << 20)
    r = renderer(scene, cfg)
    r.track_noise = True
    r.set_camera(cams[0])
    r.refresh()
    per_frame(r)
    print(f"{name}: fly-through, display RMSE against a converged frame")
    print("frame  reproject  +denoise  +guided  +guided, pooled")
    rows = []
    for k in range(1, len(cams)):
        t.set_camera(cams[k])
        t.refresh()
        converge(t)
        t.post_process()
        truth = display(t.image_pixels)
        r.reproject(cams[k])
        per_frame(r)
        r.post_process()
        e0 = rmse(display(r.image_pixels), truth)
        r.denoise()
        e1 = rmse(display(r.denoised_pixels), truth)
        r.denoise_guided()
        e2 = rmse(display(r.denoised_pixels), truth)
        r.set_noise_estimator(a.pool_batches, a.pool_radius)
        r.denoise_guided()
        e3 = rmse(display(r.denoised_pixels), truth)
        r.set_noise_estimator()
        rows.append((e0, e1, e2, e3))
        print(f"{k:5d}  {e0:9.4f}  {e1:8.4f}  {e2:7.4f}  {e3:15.4f}")
    mrow = np.mean(np.array(rows), axis=0)
    print(f" mean  {mrow[0]:9.4f}  {mrow[1]:8.4f}  {mrow[2]:7.4f}  {mrow[3]:15.4f}")

scene, cfg = cornell_box("v3"), Config.cornell_v3(256, 256, 0, 3)
for thr in (0.1, 0.05, 0.03):
    r = renderer(scene, cfg)
    r.refresh()
    spp, st = r.render_until(thr, max_spp=2048, batch_spp=16)
    print(f"render_until(noise={thr}): {spp} spp, {st.pixels_above} of {st.pixels_estimated} pixels above, max noise {st.max_noise:.4f}")
