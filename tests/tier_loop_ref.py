"""Test helper: Renderer.render_adaptive on the CPU, composed from the unchanged oracle and the restatements — full-frame oracle
samples at the stage's sample base kept where the selection says (as tests/test_gpu_adaptive.py composes a selected launch), the
noise estimate of tests/noise_ref_lib.py, the selection of tests/tier_ref_lib.py (one tier: rtpbr_select_noisy's binary rule).

    adaptive(scene, cfg, noise, budget, batch, dilate, tiers) -> (image_buffer, pixel-samples traced, selected rounds)
    display(scene, cfg, image_buffer) -> image_pixels as post_process shows them;  truth(scene, cfg, spp) -> display of `spp` other samples
"""
import numpy as np

import feature_ref_lib as fr
import noise_ref_lib as nr
import tier_ref_lib as tr
from oracle_backend import OracleRenderer

TRUTH_BASE = 1 << 20      # sample indices no loop reaches


def adaptive(scene, cfg, noise, budget, batch, dilate, tiers=1):
    W, H = cfg.width, cfg.height
    o = OracleRenderer(scene, cfg)
    o.refresh()
    t = nr.Tracker(W, H)
    obj = fr.features(scene, cfg)["object"]
    traced = used = rounds = 0
    for _ in range(2):
        n = min(batch, budget - used)
        if n <= 0:
            break
        o.set_sample_base(used)
        o.sample(n)
        t.update(o.image_buffer)
        traced, used = traced + W * H * n, used + n
    while used + batch <= budget:
        ib = o.image_buffer
        plane = nr.estimate(ib, t.moments, obj, noise)[0]
        sel = tr.select(plane, ib[..., 3], noise, dilate, tiers, batch)
        cnt = tr.counts(sel, tiers)
        if not sum(cnt):
            break
        for s, lo, hi, L in tr.stage_plan(batch, cnt):
            before = o.image_buffer
            o.set_sample_base(used + lo)
            o.sample(hi - lo)
            o.image_buffer = np.where(((sel != 0) & (sel <= s + 1))[..., None], o.image_buffer, before)
        t.update(o.image_buffer)
        traced, used, rounds = traced + tr.traced(batch, cnt), used + batch, rounds + 1
    return o.image_buffer, traced, rounds


def display(scene, cfg, image_buffer):
    """image_pixels as the oracle's post_process shows this image buffer"""
    o = OracleRenderer(scene, cfg)
    o.image_buffer = np.asarray(image_buffer, np.float32)
    o.post_process()
    return o.image_pixels


def truth(scene, cfg, spp):
    o = OracleRenderer(scene, cfg)
    o.refresh()
    o.set_sample_base(TRUTH_BASE)
    o.sample(spp)
    o.post_process()
    return o.image_pixels
