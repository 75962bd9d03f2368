#!/usr/bin/env python3
"""The display frame finished on the device: Renderer.present() / save_image() against the host path of imageio.imwrite.

    python examples/present_frame.py --size 512 512 --spp 16 --out out/present
    python examples/present_frame.py --bench

Renders a Cornell frame, writes <out>_device.png through save_image() (rtpbr_present: clamp, 8-bit quantisation and the
transpose to a top-down row-major picture in one kernel, 3 bytes per pixel read back) and <out>_host.png through
imwrite(image_pixels) (12 bytes per pixel read back, the same three steps in numpy), and checks that the two files hold the
same pixels.

--bench prints, best of five after a warm-up, at 768x432 and 1920x1080: the device time (HIP events on the renderer's stream,
around 20 back-to-back calls) of post_process and of present from image_pixels and from image_buffer, and the wall time of one
displayed frame of the src/ pipeline on the old route (sample(1) + post_process + pipelined read of image_pixels + the host
conversion of imwrite, without the file write) and the new one (sample(1) + present("accum", "rgba8") + pipelined read of the
frame).  Runs on the HIP library only.
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raytracingpbr_amd import Config, Renderer, cornell_box, workloads  # noqa: E402
from raytracingpbr_amd.imageio import _to_image, imwrite                # noqa: E402
from raytracingpbr_amd.renderer import BUF_IMAGE_PIXELS, BUF_PRESENT    # noqa: E402

REPEAT, CALLS = 5, 20


class Events:
    """two HIP events on the renderer's stream"""

    def __init__(self, stream):
        self.hip, self.stream = C.CDLL("libamdhip64.so"), C.c_void_p(stream)
        self.hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        self.hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        self.hip.hipEventSynchronize.argtypes = [C.c_void_p]
        self.ev = [C.c_void_p(), C.c_void_p()]
        for e in self.ev:
            assert self.hip.hipEventCreate(C.byref(e)) == 0

    def ms(self, fn, calls=CALLS):
        """device time of one call of fn: best of REPEAT batches of `calls` calls enqueued back to back"""
        best = float("inf")
        for _ in range(REPEAT + 1):                      # the first batch is the warm-up
            assert self.hip.hipEventRecord(self.ev[0], self.stream) == 0
            for _ in range(calls):
                fn()
            assert self.hip.hipEventRecord(self.ev[1], self.stream) == 0
            assert self.hip.hipEventSynchronize(self.ev[1]) == 0
            t = C.c_float()
            assert self.hip.hipEventElapsedTime(C.byref(t), self.ev[0], self.ev[1]) == 0
            best = min(best, t.value / calls)
        return best


def host_conversion(px):
    """what imwrite does to image_pixels before the encoder sees it"""
    return _to_image((np.clip(np.nan_to_num(px, nan=0.0), 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8))


def best_of(fn):
    fn()
    return min(fn() for _ in range(REPEAT))


def bench(W, H, FRAMES):
    wl = workloads.get("src", W, H, 1)
    r = Renderer(wl.scene, wl.cfg)
    wl.setup(r)
    r.set_option("timing", 0)
    for _ in range(96):                                  # the cost plan of the src/ form exists before anything is timed
        r.render()
    r.sync()
    ev = Events(r.stream())
    dev = {"post_process": ev.ms(r.post_process)}
    for source in ("pixels", "accum"):
        for fmt in ("rgb8", "rgba8"):
            dev[f"present({source}, {fmt})"] = ev.ms(lambda: r.present(source, fmt))
    dev["present(accum, rgba8, dither)"] = ev.ms(lambda: r.present("accum", "rgba8", True))
    r.denoise(iterations=1)
    dev["present(denoised, rgba8)"] = ev.ms(lambda: r.present("denoised", "rgba8"))
    print(f"{W}x{H} device time per call, ms: " + ", ".join(f"{k} {v:.4f}" for k, v in dev.items()))

    px = r.image_pixels
    conv = best_of(lambda: _timed(lambda: host_conversion(px)))
    print(f"{W}x{H} host conversion of imwrite (clip, quantise, transpose; numpy, no file): {conv * 1e3:.3f} ms")

    old_bufs = [r.host_array(BUF_IMAGE_PIXELS) for _ in range(2)]
    r.present("accum", "rgba8")
    new_bufs = [r.host_array(BUF_PRESENT) for _ in range(2)]

    def old_route(convert):
        prev = None
        t0 = time.perf_counter()
        for k in range(FRAMES):
            r.sample(1)
            if prev is not None:
                r.read_wait(prev)
                if convert:
                    host_conversion(old_bufs[(k - 1) & 1])
            r.post_process()
            prev = r.read_async(BUF_IMAGE_PIXELS, old_bufs[k & 1])
        r.read_wait(prev)
        if convert:
            host_conversion(old_bufs[(FRAMES - 1) & 1])
        return (time.perf_counter() - t0) / FRAMES

    def new_route():
        prev = None
        t0 = time.perf_counter()
        for k in range(FRAMES):
            r.sample(1)
            if prev is not None:
                r.read_wait(prev)                        # frame k - 1 is a finished (H, W, 4) uint8 picture in host memory
            r.present("accum", "rgba8")
            prev = r.read_async(BUF_PRESENT, new_bufs[k & 1])
        r.read_wait(prev)
        return (time.perf_counter() - t0) / FRAMES

    t_read = best_of(lambda: old_route(False))
    t_old = best_of(lambda: old_route(True))
    t_new = best_of(new_route)
    print(f"{W}x{H} one displayed frame ({FRAMES} frames), wall ms: pipelined float read-back alone {t_read * 1e3:.3f}; old route (+ host conversion) "
          f"{t_old * 1e3:.3f}; new route (present + {new_bufs[0].nbytes} B read-back) {t_new * 1e3:.3f}; "
          f"read-back bytes {old_bufs[0].nbytes} -> {new_bufs[0].nbytes}")
    # the two routes show the same picture
    r.post_process()
    r.present("accum", "rgb8")
    assert np.array_equal(r.presented, host_conversion(r.image_pixels))
    r.close()


def _timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, nargs=2, default=[512, 512])
ap.add_argument("--spp", type=int, default=16)
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--dither", action="store_true", help="ordered dither in the device file (the two files then differ by at most one level)")
ap.add_argument("--out", default="present")
ap.add_argument("--bench", action="store_true")
a = ap.parse_args()
if a.bench:
    for size in ((768, 432, 200), (1920, 1080, 25)):      # (the old route converts every frame on the host: 1080p takes fewer frames)
        bench(*size)
    sys.exit(0)
W, H = a.size
r = Renderer(cornell_box("v3", aspect=W / H), Config.cornell_v3(W, H, a.seed))
r.render(refreshing=True, spp=a.spp)
if os.path.dirname(a.out):
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
r.save_image(a.out + "_device.png", dither=a.dither)
imwrite(r.image_pixels, a.out + "_host.png")
from PIL import Image                                                    # noqa: E402
dev, host = np.asarray(Image.open(a.out + "_device.png")), np.asarray(Image.open(a.out + "_host.png"))
assert dev.shape == host.shape == (H, W, 3)
diff = int(np.abs(dev.astype(np.int32) - host.astype(np.int32)).max())
assert diff <= (1 if a.dither else 0), diff
print(f"{a.out}_device.png, {a.out}_host.png: {W}x{H}, {a.spp} spp, "
      + ("identical pixels" if diff == 0 else f"largest difference {diff} level (dither)")
      + f"; read back {r.presented.nbytes} bytes instead of {r.image_pixels.nbytes}")
