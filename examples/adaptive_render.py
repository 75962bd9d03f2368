#!/usr/bin/env python3
"""Adaptive sampling of the complete-path form: render until every pixel's estimated noise is under a threshold, and stop
sampling each pixel when it is done (Renderer.render_adaptive: select_noisy -> sample_selected -> noise_update).

    python examples/adaptive_render.py --size 256 256 --noise 0.1 --out adaptive.png --counts adaptive_counts.png
    python examples/adaptive_render.py --pool-batches 16 --min-samples 64      # the pooled estimator
    python examples/adaptive_render.py --bench               # the measurements of DESIGN.md sections 6e and 6f

Headless.  Writes the image and a map of how many samples each pixel took (white = the most).  Runs on the HIP library only.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raytracingpbr_amd import Config, Renderer, cornell_box      # noqa: E402
from raytracingpbr_amd.imageio import imwrite                    # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, nargs=2, default=[256, 256])
ap.add_argument("--noise", type=float, default=0.1)
ap.add_argument("--max-spp", type=int, default=2048)
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--dilate", type=int, default=1)
ap.add_argument("--bounces", type=int, default=3)
ap.add_argument("--pool-batches", type=int, default=0, help="0 = off; 3..64: pixels younger than this pool their variance over the neighbours")
ap.add_argument("--pool-radius", type=int, default=3)
ap.add_argument("--min-samples", type=int, default=0, help="select_noisy keeps every pixel selected up to this count")
ap.add_argument("--out", default="out/adaptive.png")
ap.add_argument("--counts", default="out/adaptive_counts.png")
ap.add_argument("--bench", action="store_true")
a = ap.parse_args()


def device_ms(r, call, reps=5):
    """best device time of `call` (rtpbr_last_sample_ms: first event of the call to its last), after one warm-up"""
    best = None
    for rep in range(reps + 1):
        call()
        ms = r.last_sample_ms()[1]
        best = ms if rep and (best is None or ms < best) else best
    return best


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


POOLED = (16, 3, 64)      # pool_batches, pool_radius, min_samples (4 batches of 16): the best point of the grid of DESIGN.md 6f


def bench():
    W, H, K = 1920, 1080, 16
    scene, cfg = cornell_box("v3", aspect=W / H), Config.cornell_v3(W, H, 0, 3)
    r = Renderer(scene, cfg)
    r.set_option("jit", 1)
    r.set_option("jit_bake", 1)
    for _ in range(2):
        r.sample(K)
        r.noise_update()
    print(f"# {W}x{H} Cornell v3, device ms per call of {K} samples per selected pixel")
    print(f"sample({K}) full frame, run-time instance: {device_ms(r, lambda: r.sample(K)):.3f} ms")
    rng = np.random.default_rng(0)
    for share in (1, 4, 16, 256):
        n = W * H // share
        scattered = np.zeros(W * H, np.uint8)
        scattered[rng.choice(W * H, n, replace=False)] = 1
        block = np.zeros((W, H), np.uint8)
        bw = max(1, int(round(W / share ** 0.5)))
        block[:bw, :max(1, n // bw)] = 1
        for label, m in (("scattered", scattered.reshape(W, H)), ("block", block)):
            got = r.select_mask(m)
            ms = device_ms(r, lambda: r.sample_selected(K))
            print(f"sample_selected({K}) 1/{share} of the frame, {label} ({got} pixels): {ms:.3f} ms, {got * K / ms / 1e3:.0f} Msamples/s")
    mask = (rng.random((W, H)) < 0.25).astype(np.uint8)
    print(f"select_mask (25 %): {wall_ms(r, lambda: r.select_mask(mask)):.3f} ms wall (upload + three passes + count read-back)")
    st = r.noise_estimate(0.0)
    thr = float(np.quantile(r.noise, 0.9))
    print(f"noise_estimate: {wall_ms(r, lambda: r.noise_estimate(thr)):.3f} ms wall")
    for radius in (1, 3):
        r.set_noise_estimator(64, radius, 0)      # two batches so far: every pixel is young
        print(f"noise_estimate, pooled over radius {radius}: {wall_ms(r, lambda: r.noise_estimate(thr)):.3f} ms wall")
    r.set_noise_estimator()
    for d in range(4):
        print(f"select_noisy dilate {d}: {wall_ms(r, lambda: r.select_noisy(thr, d)):.3f} ms wall ({r.select_noisy(thr, d)} pixels)")
    del st

    # render_adaptive against render_until on Cornell v3 256x256: pixel-samples, wall time, display RMSE against a converged frame
    scene, cfg = cornell_box("v3"), Config.cornell_v3(256, 256, 0, 3)
    t = Renderer(scene, cfg)
    t.set_option("sample_base", 1 << 20)      # samples independent of the renders'
    t.sample(65536)
    t.post_process()
    truth = t.image_pixels
    print("# Cornell v3 256x256, batches of 16, max 4096 spp; RMSE of image_pixels against 65536 spp")
    for noise in (0.1, 0.05):
        rows = [("render_until", None, None)] + [(f"render_adaptive dilate {d}", d, None) for d in (0, 1, 2)]
        rows += [(f"render_adaptive dilate {d}, pooled {POOLED}", d, POOLED) for d in (0, 1)]
        for label, d, est in rows:
            r = Renderer(scene, cfg)
            if est:
                r.set_noise_estimator(*est)
            best, res = None, None
            for rep in range(2):
                r.refresh()
                r.sync()
                t0 = time.perf_counter()
                if d is None:
                    spp, st = r.render_until(noise, 4096, 16)
                    traced = spp * 256 * 256
                else:
                    traced, st = r.render_adaptive(noise, 4096, 16, d)
                r.sync()
                dt = time.perf_counter() - t0
                best = dt if best is None or dt < best else best
            r.post_process()
            e = r.image_pixels - truth
            cnt = r.image_buffer[..., 3]
            low = cnt <= np.quantile(cnt, 0.5)
            print(f"noise {noise} {label}: {traced} pixel-samples ({traced / 65536:.1f} spp mean, {cnt.min():.0f}..{cnt.max():.0f}), "
                  f"{best * 1e3:.1f} ms wall, {st.pixels_above} pixels above, RMSE {np.sqrt(np.mean(e ** 2)):.5f}, "
                  f"RMSE of the half that stopped first {np.sqrt(np.mean(e[low] ** 2)):.5f}, mean error there {float(np.mean(e[low])):+.6f}")


if a.bench:
    bench()
    sys.exit(0)

W, H = a.size
scene, cfg = cornell_box("v3", aspect=W / H), Config.cornell_v3(W, H, 0, a.bounces)
r = Renderer(scene, cfg)
r.set_noise_estimator(a.pool_batches, a.pool_radius, a.min_samples)
r.refresh()
t0 = time.perf_counter()
traced, st = r.render_adaptive(a.noise, a.max_spp, a.batch, a.dilate)
r.post_process()
r.sync()
dt = time.perf_counter() - t0
count = r.image_buffer[..., 3]
for p in (a.out, a.counts):
    if os.path.dirname(p):
        os.makedirs(os.path.dirname(p), exist_ok=True)
imwrite(r.image_pixels, a.out)
imwrite(np.repeat((count / max(float(count.max()), 1.0))[..., None], 3, axis=2).astype(np.float32), a.counts)
print(f"{W}x{H} to noise {a.noise} (dilate {a.dilate}, pool_batches {a.pool_batches}, min_samples {a.min_samples}): {traced} pixel-samples = {traced / (W * H):.1f} spp mean, {count.min():.0f}..{count.max():.0f} "
      f"per pixel, {st.pixels_above} pixels above, max noise {st.max_noise:.4f}, {dt * 1e3:.0f} ms; a full frame of {count.max():.0f} spp "
      f"is {count.max() * W * H:.0f} pixel-samples")
print("wrote", a.out, "and", a.counts)
