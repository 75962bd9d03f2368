#!/usr/bin/env python3
"""Adaptive sampling with a share of the batch per pixel (Renderer.set_select_tiers, render_adaptive(tiers=)): the
binary loop in batches of 16, the binary loop in one large batch, and the tiered loop in the same large batch, side by side.

    python examples/adaptive_tiers.py --size 256 256 --noise 0.1 --batch 128 --tiers 6
    python examples/adaptive_tiers.py --bench                  # the device timings of DESIGN.md section 6u (1080p)
    python examples/adaptive_tiers.py --profile select 4 1     # 13 select_noisy calls with 4 tiers, dilate 1 (for a kernel trace)
    python examples/adaptive_tiers.py --profile sample 4       # 13 sample_selected(256) calls on a 4-tier selection

Headless.  Prints rounds (selected launches), pixel-samples, wall time and the display RMSE against a frame of other samples for
each loop, and the mean error of the half of the pixels that stopped first (the bias metric of DESIGN.md 6e).  Runs on the HIP
library only.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raytracingpbr_amd import Config, Renderer, cornell_box      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, nargs=2, default=[256, 256])
ap.add_argument("--noise", type=float, default=0.1)
ap.add_argument("--max-spp", type=int, default=4096)
ap.add_argument("--batch", type=int, default=128)
ap.add_argument("--tiers", type=int, default=6)
ap.add_argument("--dilate", type=int, default=1)
ap.add_argument("--truth-spp", type=int, default=16384)
ap.add_argument("--bench", action="store_true")
ap.add_argument("--profile", nargs="+", default=None, metavar=("KIND", "ARG"))
a = ap.parse_args()


def wall_ms(r, call, reps=5):
    best = None
    for rep in range(reps + 1):
        r.sync()
        t0 = time.perf_counter()
        call()
        r.sync()
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if rep and (best is None or dt < best) else best
    return best


def device_ms(r, call, reps=5):
    """best device time of `call` (rtpbr_last_sample_ms: first event of the call to its last) and its launches, after one warm-up"""
    best = None
    for rep in range(reps + 1):
        call()
        ms = r.last_sample_ms()[1]
        best = ms if rep and (best is None or ms < best) else best
    return best, r.last_sample_ms()[2]


def loops(W, H, noise, budget, batch, tiers, dilate, truth_spp, reps=2):
    scene, cfg = cornell_box("v3", aspect=W / H), Config.cornell_v3(W, H, 0, 3)
    t = Renderer(scene, cfg)
    t.set_option("sample_base", 1 << 20)      # samples independent of the renders'
    t.sample(truth_spp)
    t.post_process()
    truth = t.image_pixels
    print(f"# Cornell v3 {W}x{H}, noise {noise}, dilate {dilate}, max {budget} spp; RMSE of image_pixels against {truth_spp} spp of other samples")
    for label, b, T in (("binary, batch 16", 16, 1), (f"binary, batch {batch}", batch, 1), (f"{tiers} tiers, batch {batch}", batch, tiers)):
        r = Renderer(scene, cfg)
        rounds = [0]
        plain = r.sample_selected

        def counted(n, plain=plain, rounds=rounds):
            rounds[0] += 1
            plain(n)
        r.sample_selected = counted
        best = None
        for rep in range(reps):
            rounds[0] = 0
            r.refresh()
            r.set_option("sample_base", 0)
            r.sync()
            t0 = time.perf_counter()
            traced, st = r.render_adaptive(noise, budget, b, dilate, tiers=T)
            r.sync()
            dt = time.perf_counter() - t0
            best = dt if best is None or dt < best else best
        r.post_process()
        e = r.image_pixels - truth
        cnt = r.image_buffer[..., 3]
        low = cnt <= np.quantile(cnt, 0.5)
        print(f"{label}: {rounds[0]} rounds, {traced} pixel-samples ({traced / (W * H):.1f} spp mean, {cnt.min():.0f}..{cnt.max():.0f}), "
              f"{best * 1e3:.1f} ms wall, {st.pixels_above} pixels above, RMSE {np.sqrt(np.mean(e ** 2)):.5f}, "
              f"mean error of the half that stopped first {float(np.mean(e[low])):+.6f}")


def frame_1080p():
    W, H = 1920, 1080
    scene, cfg = cornell_box("v3", aspect=W / H), Config.cornell_v3(W, H, 0, 3)
    r = Renderer(scene, cfg)
    for _ in range(2):
        r.sample(16)
        r.noise_update()
    r.noise_estimate(0.0)
    return r, float(np.quantile(r.noise, 0.75)), W * H


def bench():
    r, thr, n_pix = frame_1080p()
    print("# 1920x1080 Cornell v3 after 2 x 16 spp, threshold = the 0.75 quantile of the noise; blocking wall ms of select_noisy")
    for T in (1, 4, 8):
        r.set_select_tiers(T, 256)
        for d in range(4):
            ms = wall_ms(r, lambda: r.select_noisy(thr, d))
            print(f"select_noisy tiers {T} dilate {d}: {ms:.3f} ms wall, {r.select_noisy(thr, d)} pixels {r.selection_tiers}")
    print("# sample_selected(256) on the selection of dilate 1: device ms (first event to last), launches, pixel-samples")
    for T in (1, 4, 8):
        r.set_select_tiers(T, 256)
        n_sel = r.select_noisy(thr, 1)
        traced = r._selected_samples(n_sel, 256)
        ms, launches = device_ms(r, lambda: r.sample_selected(256), reps=3)
        print(f"sample_selected(256) tiers {T}: {n_sel} pixels {r.selection_tiers}, {traced} pixel-samples, {ms:.3f} ms in {launches} launches, "
              f"{ms * 1e6 / traced:.4f} ns per pixel-sample")
    r.set_select_tiers()
    loops(1920, 1080, 0.1, 1024, 128, 6, 1, 4096, reps=1)


def profile(kind, args):
    """13 calls of one kind after a warm-up, for `rocprofv3 --kernel-trace --stats -- python examples/adaptive_tiers.py --profile ...`"""
    r, thr, _ = frame_1080p()
    T = int(args[0])
    if T != 1:      # (one tier makes no option call: the same calls drive a library from before the options)
        r.set_select_tiers(T, 256)
    if kind == "select":
        d = int(args[1])
        for _ in range(13):
            n = r.select_noisy(thr, d)
        print(f"select_noisy tiers {T} dilate {d}: {n} pixels")
    else:
        n = r.select_noisy(thr, 1)
        for _ in range(13):
            r.sample_selected(256)
        r.sync()
        print(f"sample_selected(256) tiers {T}: {n} pixels, {r._selected_samples(n, 256)} pixel-samples per call")


if a.profile:
    profile(a.profile[0], a.profile[1:])
elif a.bench:
    bench()
else:
    loops(a.size[0], a.size[1], a.noise, a.max_spp, a.batch, a.tiers, a.dilate, a.truth_spp)
