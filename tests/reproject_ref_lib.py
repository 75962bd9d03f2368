"""Test helper: the CPU restatement of rtpbr_reproject's gather (rr_reproject of tests/post_ref/gather.h), built on demand by
ref_build.

The old and new features come from feature_ref_lib.features()."""
import numpy as np

from raytracingpbr_amd.dataclass import ReprojectParams
from ref_build import GEOMETRY, POST_REF, ROOT, camera_of, cfg_ptr, f32, feats_of, fields, ptr      # noqa: F401 (ROOT: for the tests)

build, lib = POST_REF.build, POST_REF.lib


def reproject(cfg, old_camera, new_camera, image_buffer, old_feats, new_feats, max_history=None, depth_tolerance=None, normal_cos=None):
    """(image_buffer (W,H,4), motion (W,H,2)) — what rtpbr_reproject writes, from the old image_buffer and the old and new
    features (dicts as feature_ref_lib.features() returns them; None = the library default for a parameter)."""
    p = ReprojectParams.pack(False, max_history, depth_tolerance, normal_cos)
    W, H = cfg.width, cfg.height
    ib = f32(image_buffer)
    assert ib.shape == (W, H, 4)
    o, n = feats_of(old_feats, GEOMETRY), feats_of(new_feats, GEOMETRY)
    out = np.empty((W, H, 4), np.float32)
    motion = np.empty((W, H, 2), np.float32)
    c0, c1 = camera_of(old_camera), camera_of(new_camera)
    rc = lib().rr_reproject(cfg_ptr(cfg), cfg_ptr(c0), cfg_ptr(c1), ptr(ib), *map(ptr, o), *map(ptr, n), *fields(p), ptr(out), ptr(motion))
    assert rc == 0, rc
    return out, motion
