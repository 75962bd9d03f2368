#!/usr/bin/env python3
"""The sweep the rtpbr_denoise defaults (include/rtpbr.h RTPBR_DENOISE_DEFAULT_*) were chosen from.

    python examples/denoise_sweep.py --out denoise_sweep.json

Two scenes, each a noisy frame against a converged one of independent samples: Cornell v3 256x256 (4 spp against 1024) and
the src/ Tokyo scene 256x144 (16 bounce-steps against 16384).  The score is the display RMSE over pixels whose 5x5
neighbourhood holds one object, divided by the noisy frame's.  Every setting of the grid below is scored on both scenes;
the defaults are the setting with the best worst case.  sigma_albedo is not swept: it has no effect (include/rtpbr.h).
Runs on the HIP library only.
"""
import argparse
import itertools
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raytracingpbr_amd import Config, Renderer, cornell_box, src_scene      # noqa: E402
from raytracingpbr_amd.ibl import synthetic_env                             # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="denoise_sweep.json")
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


def rmse(x, y, m):
    return float(np.sqrt(np.mean(((x - y) ** 2)[m])))


scenes = {
    "cornell_v3_256": (cornell_box("v3"), Config.cornell_v3(256, 256, 0, 3), lambda r: r.sample(4), lambda r: r.sample(1024)),
    "src_tokyo_256x144": (src_scene(aspect=256 / 144), Config.src(256, 144, 7, steps_per_launch=4), lambda r: r.sample(4),
                          lambda r: [r.sample(64) for _ in range(64)]),
}
# iterations, demodulate, sigma colour, normal, depth (albedo fixed at 0.1)
grid = list(itertools.product([4, 5, 6], [0, 1], [0.5, 1.0, 2.0, 4.0, 8.0], [0.3, 1.0], [0.05, 0.2]))
scores = {}
for name, (scene, cfg, noisy_run, truth_run) in scenes.items():
    t = renderer(scene, cfg)
    t.set_option("sample_base", 1 << 20)          # samples independent of the noisy frame's
    truth_run(t)
    t.post_process()
    truth = t.image_pixels
    r = renderer(scene, cfg)
    noisy_run(r)
    r.post_process()
    r.render_features()
    m = single_object_mask(r.feature_object)
    base = rmse(r.image_pixels, truth, m)
    for g in grid:
        it, dm, sc, sn, sz = g
        r.denoise(it, dm, sc, sn, sz, 0.1)
        scores.setdefault(g, {})[name] = rmse(r.denoised_pixels, truth, m) / base
ranked = sorted(scores.items(), key=lambda kv: max(kv[1].values()))
for g, s in ranked[:5]:
    print("iterations %d demodulate %d sigma colour %.2f normal %.2f depth %.2f: " % g + ", ".join(f"{k} {v:.3f}" for k, v in s.items()))
json.dump([{"setting": list(g), "ratio": s} for g, s in ranked], open(a.out, "w"), indent=1)
