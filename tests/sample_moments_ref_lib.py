"""Test helper: the CPU restatement of the per-sample fold of rtpbr_set_noise_tracking (tests/sample_moments_ref/
sample_moments_ref.c), built on demand the way tests/noise_ref_lib.py builds the noise reference (the oracle's flags, hidden
visibility: only smr_* exported), and the per-sample colours it is fed with, taken from the unchanged CPU oracle."""
import ctypes as C
import os
import subprocess

import numpy as np

import feature_ref_lib as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "sample_moments_ref")
SRC = os.path.join(DIR, "sample_moments_ref.c")
LIB = os.path.join(DIR, "libsample_moments_ref.so")
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
        p, i = C.c_void_p, C.c_int
        l.smr_fold.restype = i
        l.smr_fold.argtypes = [i, i, i, p, p, p, p, p]
        _lib = l
    return _lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def fold(colours, moments, snapshot, image_buffer, mask=None):
    """(M, s, b) after a tracked sample(n) — sample_selected(n) with ``mask`` (W,H), nonzero = selected — that deposits
    ``colours`` (n,W,H,3) on top of ``moments``, ``snapshot`` and ``image_buffer`` (W,H,4).  The inputs are not modified."""
    c = np.ascontiguousarray(colours, dtype=np.float32)
    n, W, H = c.shape[:3]
    assert c.shape == (n, W, H, 3)
    M, s, b = (np.array(a, dtype=np.float32, order="C", copy=True) for a in (moments, snapshot, image_buffer))
    assert M.shape == s.shape == b.shape == (W, H, 4)
    m = None
    if mask is not None:
        m = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
        assert m.shape == (W, H)
    rc = lib().smr_fold(n, W, H, _ptr(c), None if m is None else _ptr(m), _ptr(M), _ptr(s), _ptr(b))
    assert rc == 0, rc
    return M, s, b


class Tracker:
    """The moments, the snapshot and image_buffer of one context with per-sample tracking on, on the CPU."""

    def __init__(self, W, H):
        self.moments = np.zeros((W, H, 4), np.float32)
        self.snapshot = np.zeros((W, H, 4), np.float32)
        self.image_buffer = np.zeros((W, H, 4), np.float32)

    def sample(self, colours, mask=None):
        self.moments, self.snapshot, self.image_buffer = fold(colours, self.moments, self.snapshot, self.image_buffer, mask)
        return self


def oracle_colours(oracle, first, n):
    """(n,W,H,3): the colours of samples first .. first + n - 1 of every pixel from an OracleRenderer (set up for the scene:
    shape data, environment): refresh(); set_sample_base(k); sample(1) leaves exactly sample k in image_buffer (0 + c = c).
    The oracle's image_buffer is left zeroed at sample base first + n."""
    out = []
    for k in range(first, first + n):
        oracle.refresh()
        oracle.set_sample_base(k)
        oracle.sample(1)
        ib = oracle.image_buffer
        assert (ib[..., 3] == 1).all()
        out.append(ib[..., :3].copy())
    oracle.refresh()
    oracle.set_sample_base(first + n)
    W, H = oracle.config.width, oracle.config.height
    return np.stack(out) if out else np.zeros((0, W, H, 3), np.float32)
