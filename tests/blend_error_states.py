"""Test helper: the scene, the dealt state and the comparison that tests/test_gpu_blend_error.py and
tests/test_gpu_blend_display.py share (the two calls write the same buffers from the same state)."""
import numpy as np

from checks import same, stats_same
from raytracingpbr_amd import Config, Renderer, cornell_box


def cornell(w, h):
    return cornell_box("v3", aspect=w / h), Config.cornell_v3(w, h, 0, 3)      # several objects in a window, no misses


def stripe(w, h):
    m = np.zeros((w, h), np.uint8)
    m[w // 3: w // 3 + max(w // 4, 3)] = 1
    return m


def dealt_4_4_stripe_6_6(w, h, per_sample=False):
    """4 + 4 everywhere and 6 + 6 on a stripe: dealt by half_update from batches, or sample by sample by the sample calls"""
    scene, cfg = cornell(w, h)
    r = Renderer(scene, cfg)
    if per_sample:
        r.set_half_mode(per_sample=True)
        r.sample(8)
        r.select_mask(stripe(w, h))
        r.sample_selected(4)
    else:
        for _ in range(2):
            r.sample(4)
            r.half_update()
        r.select_mask(stripe(w, h))
        for _ in range(2):
            r.sample_selected(2)
            r.half_update()
    a, b = r.half_buffer[..., 3], r.image_buffer[..., 3]
    on = stripe(w, h) != 0
    assert np.all(a[on] == 6) and np.all(b[on] == 12) and np.all(a[~on] == 4) and np.all(b[~on] == 8)
    r.render_features()
    return cfg, r


def compare(r, stats, want, what):
    """the plane, the returned statistics and the three buffers of the blend against a restatement's BlendError"""
    same(r.blend_error_map, want.error, "blend_error_map " + what)
    stats_same(stats, want.stats, what)
    same(r.denoised_pixels, want.denoised, "denoised_pixels " + what)
    same(r.blend_weight, want.weight, "blend_weight " + what)
    same(r.blend_depth, want.depth, "blend_depth " + what)
