"""Test helper: the CPU restatement of rtpbr_set_half_mode's two rules (hm_* of tests/post_ref: half_mode.h, gather.h), built on
demand by ref_build.

fold() is the per-sample dealing of a sample call with per_sample on, fed with per-sample colours
(sample_moments_ref_lib.oracle_colours, or the differences of image_buffer where those are exact); gather() is what
rtpbr_reproject / rtpbr_reproject_scene leave with warp on."""
import numpy as np

from ref_build import POST_REF, ROOT, ptr      # noqa: F401 (ROOT: for the tests)
from reproject_scene_ref_lib import scene_gather

build, lib = POST_REF.build, POST_REF.lib


def fold(colours, half_a, half_sh, image_buffer, mask=None):
    """(A, sh, b) after a dealing sample(n) — sample_selected(n) with ``mask`` (W,H), nonzero = selected — that deposits
    ``colours`` (n,W,H,3) on top of ``half_a``, ``half_sh`` and ``image_buffer`` (W,H,4).  The inputs are not modified."""
    c = np.ascontiguousarray(colours, dtype=np.float32)
    n, W, H = c.shape[:3]
    assert c.shape == (n, W, H, 3)
    A, s, b = (np.array(a, dtype=np.float32, order="C", copy=True) for a in (half_a, half_sh, image_buffer))
    assert A.shape == s.shape == b.shape == (W, H, 4)
    m = None
    if mask is not None:
        m = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
        assert m.shape == (W, H)
    rc = lib().hm_fold(n, W, H, ptr(c), ptr(m), ptr(A), ptr(s), ptr(b))
    assert rc == 0, rc
    return A, s, b


class Dealer:
    """Half A, its snapshot and image_buffer of one context with per_sample on, on the CPU."""

    def __init__(self, W, H):
        self.a = np.zeros((W, H, 4), np.float32)
        self.snapshot = np.zeros((W, H, 4), np.float32)
        self.image_buffer = np.zeros((W, H, 4), np.float32)

    def sample(self, colours, mask=None):
        self.a, self.snapshot, self.image_buffer = fold(colours, self.a, self.snapshot, self.image_buffer, mask)
        return self


def gather(cfg, old_scene, new_scene, old_camera, new_camera, image_buffer, half_a, old_feats, new_feats, max_history=None,
           depth_tolerance=None, normal_cos=None):
    """(image_buffer (W,H,4), motion (W,H,2), half A (W,H,4)) — what rtpbr_reproject_scene (rtpbr_reproject when ``new_scene`` is
    ``old_scene``) writes with warp on, from the old image_buffer, the old half A and the features of the old and the new view
    (dicts as feature_ref_lib.features() returns them; None = the library default for a parameter; new_camera None = it stays)."""
    assert half_a is not None
    return scene_gather(lib().hm_gather, cfg, old_scene, new_scene, old_camera, new_camera, image_buffer, half_a, old_feats, new_feats,
                        max_history, depth_tolerance, normal_cos)
