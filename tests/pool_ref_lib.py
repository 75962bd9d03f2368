"""Test helper: the CPU restatement of rtpbr_noise_estimate under rtpbr_set_noise_estimator (tests/pool_ref/pool_ref.c), built on
demand the way tests/noise_ref_lib.py builds its reference (the oracle's flags, hidden visibility, -Bsymbolic: only pr_*
exported), and the extended selection rule of rtpbr_select_noisy in numpy.

    estimate(image_buffer, moments, obj, threshold, pool_batches, pool_radius) -> (noise, var0, (estimated, above, max_noise))
    select(noise, count, threshold, dilate, min_samples) -> (W,H) uint8
"""
import ctypes as C
import os
import subprocess

import numpy as np

import feature_ref_lib as fr
import select_ref_lib as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "pool_ref")
SRC = os.path.join(DIR, "pool_ref.c")
LIB = os.path.join(DIR, "libpool_ref.so")
FLAGS = fr.FLAGS

_lib = None


def build():
    if os.path.exists(LIB) and os.path.getmtime(LIB) >= os.path.getmtime(SRC):
        return LIB
    tmp = f"{LIB}.{os.getpid()}.tmp"
    subprocess.run([os.environ.get("CC", "gcc")] + FLAGS + [SRC, "-o", tmp, "-lm"], check=True)
    os.replace(tmp, LIB)
    return LIB


def lib():
    global _lib
    if _lib is None:
        l = C.CDLL(build())
        p, i, f = C.c_void_p, C.c_int, C.c_float
        l.pr_estimate.restype = i
        l.pr_estimate.argtypes = [i, i, p, p, p, f, i, i, p, p, p]
        _lib = l
    return _lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def estimate(image_buffer, moments, obj, threshold=0.0, pool_batches=0, pool_radius=3):
    """(noise (W,H), var0 (W,H), (pixels_estimated, pixels_above, max_noise)) — what rtpbr_noise_estimate computes on a context
    whose estimator is (pool_batches, pool_radius)."""
    ib, M = _f32(image_buffer), _f32(moments)
    W, H = ib.shape[:2]
    o = np.ascontiguousarray(obj)
    assert o.dtype == np.int32 and o.shape == (W, H) and M.shape == (W, H, 4)
    noise, var0 = np.empty((W, H), np.float32), np.empty((W, H), np.float32)
    st = np.zeros(3, np.uint32)
    rc = lib().pr_estimate(W, H, _ptr(ib), _ptr(M), _ptr(o), float(threshold), int(pool_batches), int(pool_radius), _ptr(noise),
                           _ptr(var0), _ptr(st))
    assert rc == 0, rc
    return noise, var0, (int(st[0]), int(st[1]), float(st[2:3].view(np.float32)[0]))


def select(noise, count, threshold, dilate=0, min_samples=0):
    """The rule of rtpbr_select_noisy with rtpbr_set_noise_estimator's min_samples: select_ref_lib.select, or
    ``count < (float)min_samples``.  Comparisons only, so exact."""
    if not 0 <= int(min_samples) <= 16777216:
        raise ValueError("min_samples must be 0..16777216")
    base = sr.select(noise, count, threshold, dilate)
    few = np.asarray(count, np.float32) < np.float32(int(min_samples))
    return (base.astype(bool) | few).astype(np.uint8)
