"""Test helper: the CPU restatement of rtpbr_noise_estimate under rtpbr_set_noise_estimator (tests/pool_ref/pool_ref.c), built on
demand the way tests/noise_ref_lib.py builds its reference (the oracle's flags, hidden visibility, -Bsymbolic: only pr_*
exported), and the extended selection rule of rtpbr_select_noisy in numpy.

    estimate(image_buffer, moments, obj, threshold, pool_batches, pool_radius) -> (noise, var0, (estimated, above, max_noise))
    select(noise, count, threshold, dilate, min_samples) -> (W,H) uint8
"""
import numpy as np

import select_ref_lib as sr
from ref_build import F, I, Library, P, ROOT, f32, ptr, stats_of      # noqa: F401 (ROOT: for the tests)

_ref = Library("pool_ref", {
    "pr_estimate": [I, I, P, P, P, F, I, I, P, P, P],
}, deps=[])
build, lib = _ref.build, _ref.lib


def estimate(image_buffer, moments, obj, threshold=0.0, pool_batches=0, pool_radius=3):
    """(noise (W,H), var0 (W,H), (pixels_estimated, pixels_above, max_noise)) — what rtpbr_noise_estimate computes on a context
    whose estimator is (pool_batches, pool_radius)."""
    ib, M = f32(image_buffer), f32(moments)
    W, H = ib.shape[:2]
    o = np.ascontiguousarray(obj)
    assert o.dtype == np.int32 and o.shape == (W, H) and M.shape == (W, H, 4)
    noise, var0 = np.empty((W, H), np.float32), np.empty((W, H), np.float32)
    st = np.zeros(3, np.uint32)
    rc = lib().pr_estimate(W, H, ptr(ib), ptr(M), ptr(o), float(threshold), int(pool_batches), int(pool_radius), ptr(noise),
                           ptr(var0), ptr(st))
    assert rc == 0, rc
    return noise, var0, stats_of(st)


def select(noise, count, threshold, dilate=0, min_samples=0):
    """The rule of rtpbr_select_noisy with rtpbr_set_noise_estimator's min_samples: select_ref_lib.select, or
    ``count < (float)min_samples``.  Comparisons only, so exact."""
    if not 0 <= int(min_samples) <= 16777216:
        raise ValueError("min_samples must be 0..16777216")
    base = sr.select(noise, count, threshold, dilate)
    few = np.asarray(count, np.float32) < np.float32(int(min_samples))
    return (base.astype(bool) | few).astype(np.uint8)
