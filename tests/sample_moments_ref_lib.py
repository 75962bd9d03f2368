"""Test helper: the CPU restatement of the per-sample fold of rtpbr_set_noise_tracking (tests/sample_moments_ref/
sample_moments_ref.c), built on demand the way tests/noise_ref_lib.py builds the noise reference (the oracle's flags, hidden
visibility: only smr_* exported), and the per-sample colours it is fed with, taken from the unchanged CPU oracle."""
import numpy as np

from ref_build import I, Library, P, ROOT, ptr      # noqa: F401 (ROOT: for the tests)

_ref = Library("sample_moments_ref", {
    "smr_fold": [I, I, I, P, P, P, P, P],
}, deps=[])
build, lib = _ref.build, _ref.lib


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
    rc = lib().smr_fold(n, W, H, ptr(c), None if m is None else ptr(m), ptr(M), ptr(s), ptr(b))
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
