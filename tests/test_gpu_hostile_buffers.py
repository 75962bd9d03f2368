"""The post stages on hostile image buffers on the GPU (tests/hostile.py has the inputs, the comparison and the guard; the CPU tier
is tests/test_hostile_buffers_ref.py).  Every case writes a hostile buffer with rtpbr_write_buffer(RTPBR_BUF_IMAGE_BUFFER), runs one
stage and compares it with that stage's restatement — the oracle for post_process, tests/*_ref/ for the others — fed the same
buffer and the context's own features, moments and half buffer.  The comparison is hostile.compare(): word for word, NaN against
NaN; no tolerance anywhere.  The coverage guard is asserted on the restatement's output in every case."""
import numpy as np
import pytest

import feature_ref_lib as fr
import half_ref_lib as hl
import hostile as hz
import noise_ref_lib as nr
import pool_ref_lib as pl
import reproject_ref_lib as rr
import reproject_scene_ref_lib as rs
import test_gpu_features_denoise as fd
from raytracingpbr_amd import Renderer

pytestmark = pytest.mark.gpu

THR = 0.05


def _context(preset="v3", frame="97x61", cfg=None):
    """a fresh context with its features rendered, so that the hostile buffer can be planted by object index"""
    w, h = hz.FRAMES[frame]
    scene, c = hz.scene_cfg(preset, w, h)
    cfg = c if cfg is None else cfg(c)
    r = Renderer(scene, cfg)
    r.refresh()                       # (rtpbr_reproject wants one since rtpbr_set_config)
    r.render_features()
    return scene, cfg, r


def _written(r, family):
    ib = hz.buffer_for(family, r.feature_object)
    r.image_buffer = ib
    return ib


def _two_batches(r, family, update):
    """the hostile buffer is written before the first update — by the header everything accumulated until then is the first batch —
    then rtpbr_sample(2) and a second update; returns (hostile buffer, image_buffer now)"""
    ib = _written(r, family)
    update()
    r.sample(2)
    update()
    return ib, r.image_buffer


# ------------------------------------------------------------------ (a) post_process against the oracle
@pytest.mark.parametrize("family,order,trunc", hz.TONEMAP_CASES)
def test_post_process(family, order, trunc):
    scene, cfg, r = _context(cfg=lambda c: hz.tonemap_cfg(c, order, trunc))
    ib = _written(r, family)
    r.post_process()
    want = hz.oracle_post_process(scene, cfg, ib)
    stage = f"post_process {family} order {order} truncated {trunc}"
    hz.guard(stage, want)
    hz.compare(stage, r.image_pixels, want, ib)


# ------------------------------------------------------------------ (b) rtpbr_denoise
@pytest.mark.parametrize("preset,family,iterations,demodulate", hz.DENOISE_CASES)
def test_denoise(preset, family, iterations, demodulate):
    """(an even number of levels ends on the other half of the levels' ping-pong buffer than an odd one)"""
    scene, cfg, r = _context(preset)
    ib = _written(r, family)
    r.denoise(iterations=iterations, demodulate=demodulate, **hz.SIGMAS)
    want = fr.denoise(cfg, ib, fd._gpu_features(r), iterations, demodulate, **hz.SIGMAS)
    stage = f"denoise {preset} {family} {iterations} levels demodulate {demodulate}"
    hz.guard(stage, want)
    hz.compare(stage, r.denoised_pixels, want, ib)


# ------------------------------------------------------------------ (c) rtpbr_noise_estimate, pooling, selection
@pytest.mark.parametrize("family", hz.FAMILIES)
@pytest.mark.parametrize("preset", hz.PRESETS)
def test_noise_estimate_spatial(preset, family):
    scene, cfg, r = _context(preset)
    ib = _written(r, family)
    obj = r.feature_object
    for thr in hz.THRESHOLDS:
        st = r.noise_estimate(thr)
        noise, _, want = nr.estimate(ib, np.zeros_like(ib), obj, thr)
        stage = f"noise_estimate {preset} {family} spatial threshold {thr}"
        hz.guard(stage, noise)
        hz.compare(stage, r.noise, noise, ib)
        hz.compare_stats(stage, st, want)
    assert not r.moments.any()


@pytest.mark.parametrize("family", hz.FAMILIES)
@pytest.mark.parametrize("preset", hz.PRESETS)
def test_noise_estimate_temporal_pooled_and_selection(preset, family):
    scene, cfg, r = _context(preset)
    ib, ib2 = _two_batches(r, family, r.noise_update)
    M, obj = r.moments, r.feature_object
    # the inputs themselves: the device's accumulation onto the hostile buffer and its moments against the oracle and nr_update
    hz.compare(f"sample_after_write {preset} {family}", ib2, hz.second_batch(scene, cfg, ib), ib)
    t = nr.Tracker(hz.W, hz.H)
    t.update(ib)
    t.update(ib2)
    hz.compare(f"noise_update {preset} {family}", M, t.moments, ib)
    assert (M[..., 3] >= 2).mean() > 0.9
    st = r.noise_estimate(THR)
    noise, _, want = nr.estimate(ib2, M, obj, THR)
    stage = f"noise_estimate {preset} {family} temporal"
    hz.guard(stage, noise)
    hz.compare(stage, r.noise, noise, ib2)
    hz.compare_stats(stage, st, want)
    r.set_noise_estimator(4, 3, 0)
    st = r.noise_estimate(THR)
    pooled, _, want = pl.estimate(ib2, M, obj, THR, 4, 3)
    stage = f"noise_estimate_pooled {preset} {family}"
    hz.guard(stage, pooled)
    hz.compare(stage, r.noise, pooled, ib2)
    hz.compare_stats(stage, st, want)
    assert (pooled.view(np.uint32) != noise.view(np.uint32)).any(), "pooling changed nothing: the plain kernel would pass"
    r.set_noise_estimator(4, 3, 3)
    for dilate in (0, 2):
        n = r.select_noisy(THR, dilate)
        stage = f"select_noisy {preset} {family} dilate {dilate}"
        hz.compare(stage.replace("select_noisy", "noise_estimate_pooled as select_noisy writes it,"), r.noise, pooled, ib2)
        mask = pl.select(pooled, ib2[..., 3], THR, dilate, 3)
        hz.compare(stage, r.selection, mask, ib2)
        assert n == int(mask.sum()) and 0 < n


# ------------------------------------------------------------------ (d) rtpbr_denoise_guided
@pytest.mark.parametrize("family,iterations,demodulate,floor", hz.GUIDED_CASES)
def test_denoise_guided(family, iterations, demodulate, floor):
    scene, cfg, r = _context()
    ib = _written(r, family)
    feats = fd._gpu_features(r)
    params = dict(iterations=iterations, demodulate=demodulate, variance_floor=floor, **hz.GUIDED)
    r.denoise_guided(**params)
    noise, var0, _ = nr.estimate(ib, np.zeros_like(ib), feats["object"])
    want = nr.guided(cfg, ib, feats, var0, **params)
    stage = f"denoise_guided {family} {iterations} levels demodulate {demodulate} floor {floor:g}"
    hz.guard(stage, want)
    hz.compare(stage, r.denoised_pixels, want, ib)
    hz.compare(stage.replace("denoise_guided", "noise_estimate as denoise_guided writes it,"), r.noise, noise, ib)


# ------------------------------------------------------------------ (e) rtpbr_reproject, rtpbr_reproject_scene
@pytest.mark.parametrize("family,move,max_history,normal_cos", hz.REPROJECT_CASES)
def test_reproject(family, move, max_history, normal_cos):
    """the hostile buffer is the history; then the same move on a context with moments, whose history is the hostile buffer plus
    two samples"""
    params = dict(max_history=max_history, normal_cos=normal_cos)
    stage = f"reproject {family} {move} max_history {max_history:g} normal_cos {normal_cos:g}"
    old, new = None, None
    for moments in (False, True):
        scene, cfg, r = _context()
        if old is None:
            old, new = hz.moves()[move](scene.camera)
        if moments:
            _, ib = _two_batches(r, family, r.noise_update)
            M = r.moments
        else:
            ib = _written(r, family)
        f0 = fd._gpu_features(r)
        r.reproject(new, **params)
        f1 = fd._gpu_features(r)
        want_ib, want_mv = rr.reproject(cfg, old, new, ib, f0, f1, **params)
        hz.guard(stage, want_ib)
        hz.compare(stage + (" with moments" if moments else ""), r.image_buffer, want_ib, ib)
        hz.compare(stage.replace("reproject", "reproject_motion"), r.motion, want_mv, ib)
        assert (want_mv[..., 0] >= 0).any() and (want_mv[..., 0] < 0).any()
        if moments:
            want_ib2, want_M = nr.reproject(cfg, old, new, ib, M, f0, f1, **params)
            hz.guard(stage + " moments", want_M)
            hz.compare(stage.replace("reproject", "reproject_moments"), r.moments, want_M, ib)
            hz.compare(stage + " (noise_ref)", r.image_buffer, want_ib2, ib)


@pytest.mark.parametrize("family", hz.FAMILIES)
def test_reproject_scene(family):
    scene, cfg, r = _context()
    ib = _written(r, family)
    f0 = fd._gpu_features(r)
    new_scene = rs.moved_scene(scene, hz.BOX_MOVE)
    r.reproject_scene(new_scene)
    f1 = fd._gpu_features(r)
    want_ib, want_mv, _ = rs.reproject_scene(cfg, scene, new_scene, scene.camera, None, ib, f0, f1)
    stage = f"reproject_scene {family}"
    hz.guard(stage, want_ib)
    hz.compare(stage, r.image_buffer, want_ib, ib)
    hz.compare(stage.replace("reproject_scene", "reproject_scene_motion"), r.motion, want_mv, ib)
    on_box = f1["object"] == 6
    assert on_box.any() and (want_mv[on_box][:, 0] >= 0).any()


# ------------------------------------------------------------------ (f) the halves
@pytest.mark.parametrize("family", hz.FAMILIES)
def test_halves(family):
    """the hostile buffer lands in A (the first batch of a fresh context), rtpbr_sample(2) in B"""
    scene, cfg, r = _context()
    ib, ib2 = _two_batches(r, family, r.half_update)
    a, feats = r.half_buffer, fd._gpu_features(r)
    m = hl.Halves(hz.W, hz.H)
    m.update(ib)
    m.update(ib2)
    hz.compare(f"half_update {family}", a, m.a, ib)
    had = ib[..., 3] > 0
    assert (a[..., 3][had] == ib[..., 3][had]).all()      # all of it in A
    none = ib[..., 3] == 0                                 # a count of +0 or -0 is no batch: there the two samples are A's first
    assert (a[..., 3][none] == 2).all() and (none.any() or family == "N")
    r.set_noise_estimator(0, 3, 3)
    for radius in (1, 3):
        for denoise in ({}, dict(iterations=2, demodulate=1, **hz.SIGMAS)):
            st = r.denoise_error(THR, radius, **denoise)
            want, wst, _ = hl.denoise_error(cfg, ib2, a, feats, radius=radius, threshold=THR, **denoise)
            stage = f"denoise_error {family} radius {radius} {'defaults' if not denoise else '2 levels demodulated'}"
            hz.guard(stage, want)
            hz.compare(stage, r.denoised_error, want, ib2)
            hz.compare_stats(stage, st, wst)
            assert wst[0] > 0.8 * hz.W * hz.H
        for dilate in (0, 2):
            n = r.select_error(THR, dilate)
            mask = hl.select(ib2, a, want, THR, dilate, 3)
            hz.compare(f"select_error {family} radius {radius} dilate {dilate}", r.selection, mask, ib2)
            assert n == int(mask.sum()) and 0 < n


# ------------------------------------------------------------------ (g) the 7 x 5 frame
def test_small_frame():
    """family F on a frame smaller than the 5 x 5 tap window at step 2, the radius-3 window and the pool tile"""
    scene, cfg, r = _context(frame="7x5")
    ib = _written(r, "F")
    feats = fd._gpu_features(r)
    r.denoise(iterations=2, demodulate=0, **hz.SIGMAS)
    want = fr.denoise(cfg, ib, feats, 2, 0, **hz.SIGMAS)
    hz.guard("denoise 7x5", want)
    hz.compare("denoise 7x5", r.denoised_pixels, want, ib)
    st = r.noise_estimate(THR)
    noise, var0, wst = nr.estimate(ib, np.zeros_like(ib), feats["object"], THR)
    hz.guard("noise_estimate 7x5", noise)
    hz.compare("noise_estimate 7x5", r.noise, noise, ib)
    hz.compare_stats("noise_estimate 7x5", st, wst)
    params = dict(iterations=1, demodulate=0, variance_floor=1e-5, **hz.GUIDED)
    r.denoise_guided(**params)
    want = nr.guided(cfg, ib, feats, var0, **params)
    hz.guard("denoise_guided 7x5", want)
    hz.compare("denoise_guided 7x5", r.denoised_pixels, want, ib)
    old, new = hz.moves()["translate"](scene.camera)
    r.reproject(new)
    want_ib, want_mv = rr.reproject(cfg, old, new, ib, feats, fd._gpu_features(r))
    hz.guard("reproject 7x5", want_ib)
    hz.compare("reproject 7x5", r.image_buffer, want_ib, ib)
    hz.compare("reproject_motion 7x5", r.motion, want_mv, ib)


def test_totals():
    """the record of the run: per stage the words compared and the words that were NaN on both sides (runs last in this file)"""
    assert hz.TOTALS
    for stage, (words, nan) in sorted(hz.TOTALS.items()):
        print(f"[hostile] total {stage}: {words} words compared, {nan} NaN on both sides")
