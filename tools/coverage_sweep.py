#!/usr/bin/env python3
"""The sweep the rtpbr_denoise_coverage default power (include/rtpbr.h RTPBR_COVERAGE_DEFAULT_POWER) was chosen from.

    python tools/coverage_sweep.py [--out coverage_sweep.json]

Runs on the CPU only: the oracle renders, the restatements of tests/ (post_ref, coverage_ref) filter.  Three cases, the two scene
kinds of examples/denoise_sweep.py: Cornell v3 96x96 (max_raytrace 3) at 4 and at 64 spp against 2048 spp of independent samples,
and the src/ Tokyo scene 96x54 at 16 bounce-steps against 4096.  Four groups of samples each.  power 0, 1, 2, 4, 8 x resolve 0, 1
at grid 4, rtpbr_denoise's defaults otherwise.  Score: display RMSE (over the three channels) on three pixel sets — interior (5x5
neighbourhood of one object), coverage below 1, the whole frame — as the mean over the groups, divided by rtpbr_denoise's.  The
default is the power with the best worst-case whole-frame ratio at resolve 1.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import coverage_ref_lib as cl                                        # noqa: E402
import feature_ref_lib as fl                                         # noqa: E402
from oracle_backend import OracleRenderer                            # noqa: E402
from raytracingpbr_amd import Config, cornell_box, src_scene         # noqa: E402
from raytracingpbr_amd.ibl import synthetic_env                      # noqa: E402

POWERS, GROUPS = (0, 1, 2, 4, 8), 4

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
a = ap.parse_args()


def oracle(scene, cfg):
    o = OracleRenderer(scene, cfg)
    if cfg.sky_kind == 1:      # RTPBR_SKY_ENVMAP
        o.set_env(synthetic_env(192, 96, seed=0), 1.4, 2.2)
    return o


def case(name, scene, cfg, noisy, truth_run):
    """noisy: {label: sample() calls to the frame}, cumulative in this order"""
    feats = fl.features(scene, cfg)
    cov = cl.coverage(scene, cfg, 4, feats=feats)
    sets = cl.error_sets(feats["object"], cov)
    shown = lambda ib: fl.denoise(cfg, ib, feats, iterations=0, demodulate=0).astype(np.float64)      # noqa: E731
    o = oracle(scene, cfg)
    o.refresh()
    o.set_sample_base(1 << 20)
    truth_run(o)
    truth = shown(o.image_buffer)
    rows = {}
    for g in range(GROUPS):
        o.refresh()
        o.set_sample_base(g * 4096)
        done = 0
        for label, upto in noisy.items():
            o.sample(upto - done)
            done = upto
            ib = o.image_buffer
            frames = {"denoise": fl.denoise(cfg, ib, feats)}
            for power in POWERS:
                for resolve in (0, 1):
                    frames[f"p{power}r{resolve}"] = cl.denoise_coverage(cfg, ib, feats, cov, power, resolve)[0]
            for k, px in frames.items():
                se = (px.astype(np.float64) - truth) ** 2
                for s, m in sets.items():
                    rows.setdefault((label, k, s), []).append(float(np.sqrt(se[m].mean())))
    o.close()
    out = {}
    for label in noisy:
        print(f"{name} {label}: pixels interior {int(sets['interior'].sum())} edge {int(sets['edge'].sum())} frame {sets['frame'].size}")
        base = {s: float(np.mean(rows[(label, "denoise", s)])) for s in sets}
        print("  denoise          " + "  ".join(f"{s} {base[s]:.4f}" for s in sets))
        for power in POWERS:
            for resolve in (0, 1):
                k = f"p{power}r{resolve}"
                r = {s: float(np.mean(rows[(label, k, s)])) for s in sets}
                out[f"{name} {label} {k}"] = {s: (r[s], r[s] / base[s]) for s in sets}
                print(f"  power {power} resolve {resolve}: " + "  ".join(f"{s} {r[s]:.4f} ({r[s] / base[s]:.3f})" for s in sets))
    return out


res = {}
W = H = 96
res.update(case("cornell_v3_96", cornell_box("v3"), Config.cornell_v3(W, H, seed=0, max_raytrace=3), {"4spp": 4, "64spp": 64},
                lambda o: o.sample(2048)))
W, H = 96, 54
res.update(case("src_tokyo_96x54", src_scene(aspect=W / H), Config.src(W, H, 7, steps_per_launch=4), {"16steps": 4},
                lambda o: [o.sample(64) for _ in range(16)]))
worst = {p: max(v["frame"][1] for k, v in res.items() if k.endswith(f"p{p}r1")) for p in POWERS}
print("worst whole-frame ratio to denoise at resolve 1, per power:", {p: round(w, 4) for p, w in worst.items()})
print("default power:", min(worst, key=worst.get))
if a.out:
    json.dump(res, open(a.out, "w"), indent=1)
