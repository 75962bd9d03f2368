"""Per-sample noise tracking on the GPU (rtpbr_set_noise_tracking): what a tracked rtpbr_sample / rtpbr_sample_selected leaves
in RTPBR_BUF_MOMENTS, the snapshot and image_buffer, held bit for bit to the CPU restatement (tests/sample_moments_ref/
sample_moments_ref.c) fed with the per-sample colours of the unchanged CPU oracle, and to an untracked twin renderer.  The
snapshot is internal: it is checked through what the next rtpbr_noise_update does with it (tests/noise_ref_lib.py)."""
import ctypes as C

import numpy as np
import pytest

import checks as ck
import noise_ref_lib as nr
import sample_moments_ref_lib as sm
import test_gpu_features_denoise as fd
import test_gpu_reproject as rp
from checks import EINVAL, ESTATE
from oracle_backend import OracleRenderer
from raytracingpbr_amd import Config, Renderer, cornell_box, src_scene
from raytracingpbr_amd._capi import RtpbrError
from raytracingpbr_amd.renderer import BUF_IMAGE_BUFFER, BUF_MOMENTS, BUF_NOISE

pytestmark = pytest.mark.gpu

FRAMES = {"7x5": (7, 5), "20x13": (20, 13)}      # 35 pixels: less than a wave; 260: the second block holds 4 lanes
KS = (1, 3, 8, 12, 20)                           # scalar loop; scalar; vector loop only; vector + remainder; vector + remainder
N_REF = 20


def _scene(name, w, h):
    if name == "cornell_v3":
        return cornell_box("v3", aspect=w / h), Config.cornell_v3(w, h, 0, 3)
    return src_scene(aspect=w / h, tokyo=True), Config.scene_demo(w, h, 5, 16)      # spheres, boxes and a cylinder


_colours = {}


def _ref_colours(scene_name, frame, n=N_REF):
    """per-sample colours 0 .. n - 1 from the oracle, computed once per scene and frame and never modified"""
    key = (scene_name, frame)
    if key not in _colours:
        scene, cfg = _scene(scene_name, *FRAMES[frame])
        c = sm.oracle_colours(OracleRenderer(scene, cfg), 0, N_REF)
        c.setflags(write=False)
        _colours[key] = c
    return _colours[key][:n]


def _check(r, t, what=""):
    """moments and image_buffer against the CPU tracker; the snapshot through a noise_update, which must find nothing new"""
    ck.same(r.image_buffer, t.image_buffer, what + "image_buffer")
    ck.same(r.moments, t.moments, what + "moments")
    ck.same(t.snapshot, t.image_buffer, what + "restated snapshot")
    r.noise_update()
    ck.same(r.moments, t.moments, what + "moments after a noise_update (the snapshot is image_buffer)")


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("frame", list(FRAMES))
@pytest.mark.parametrize("scene_name", ["cornell_v3", "scene_demo"])
def test_tracked_sample_matches_the_restatement_and_the_untracked_twin(scene_name, frame, K):
    w, h = FRAMES[frame]
    scene, cfg = _scene(scene_name, w, h)
    r, twin = Renderer(scene, cfg), Renderer(scene, cfg)
    r.set_noise_tracking(True)
    assert r.noise_per_sample is True
    r.sample(K)
    twin.sample(K)
    ck.same(r.image_buffer, twin.image_buffer, "image_buffer against the untracked twin")
    assert ck.counters(r) == ck.counters(twin) and r.counters().deposits == w * h * K
    t = sm.Tracker(w, h).sample(_ref_colours(scene_name, frame, K))
    _check(r, t)
    assert (r.moments[..., 3] == K).all() and (r.moments[..., 2] == K).all()
    if K + 3 <= N_REF:      # a second tracked call continues both sums
        r.sample(3)
        twin.sample(3)
        ck.same(r.image_buffer, twin.image_buffer, "image_buffer against the untracked twin, second call")
        _check(r, t.sample(_ref_colours(scene_name, frame)[K:K + 3]), "second call: ")


OPTION_SETS = [{"scheduler": 0}, {"scheduler": 1}, {"primary_split": 2}, {"jit": 1, "stage_dense": 1}]


@pytest.mark.parametrize("options", OPTION_SETS, ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_options_do_not_change_the_bits(options, tmp_path, monkeypatch):
    monkeypatch.setenv("RTPBR_JIT_CACHE", str(tmp_path))
    w, h = FRAMES["20x13"]
    scene, cfg = _scene("cornell_v3", w, h)
    r = Renderer(scene, cfg)
    for k, v in options.items():
        r.set_option(k, v)
    r.set_noise_tracking(True)
    r.sample(8)
    if "stage_dense" in options:
        assert r.counter("jit_active") == 1 and r.counter("dense_launches") == 0      # a run-time instance, item-linear records
    _check(r, sm.Tracker(w, h).sample(_ref_colours("cornell_v3", "20x13", 8)), f"{options}: ")


def test_sub_launches_of_3_3_and_2_samples():
    """the smallest staging budget (1 MiB) holds 3 records of 12 bytes for each of 170 x 130 pixels and not 4 (no primary records):
    8 samples run as sub-launches of 3, 3 and 2 — each sample is its own batch, so the split does not show"""
    w, h = 170, 130
    assert (1 << 20) // (w * h * 12) == 3
    scene, cfg = _scene("cornell_v3", w, h)
    got = []
    for budget in (1 << 20, 1 << 30):
        r = Renderer(scene, cfg)
        r.set_option("primary_split", 0)
        r.set_option("staging_bytes", budget)
        r.set_noise_tracking(True)
        r.sample(8)
        assert r.last_sample_ms()[2] == (3 if budget == 1 << 20 else 1)
        got.append((r.moments, r.image_buffer))
    ck.same(got[0][0], got[1][0], "moments, three sub-launches against one")
    ck.same(got[0][1], got[1][1], "image_buffer, three sub-launches against one")
    t = sm.Tracker(w, h).sample(sm.oracle_colours(OracleRenderer(scene, cfg), 0, 8))
    _check(r, t)


def _third(w, h):
    m = np.zeros((w, h), np.uint8)
    m.reshape(-1)[np.random.default_rng(7).permutation(w * h)[:w * h // 3]] = 1
    return m


@pytest.mark.parametrize("K", [3, 8])
def test_selected_launch_leaves_unselected_pixels_alone(K):
    w, h = FRAMES["20x13"]
    scene, cfg = _scene("cornell_v3", w, h)
    c = _ref_colours("cornell_v3", "20x13")
    mask = _third(w, h)
    r, twin = Renderer(scene, cfg), Renderer(scene, cfg)
    r.set_noise_tracking(True)
    for x in (r, twin):
        x.sample(4)
        assert x.select_mask(mask) == int(mask.sum())
    t = sm.Tracker(w, h).sample(c[:4])
    before = (r.moments, r.image_buffer)
    r.sample_selected(K)
    twin.sample_selected(K)
    ck.same(r.image_buffer, twin.image_buffer, "image_buffer against the untracked twin")
    assert ck.counters(r) == ck.counters(twin) and r.counters().deposits == int(mask.sum()) * K
    keep = mask == 0
    assert np.array_equal(ck.bits(r.moments)[keep], ck.bits(before[0])[keep]) and np.array_equal(ck.bits(r.image_buffer)[keep], ck.bits(before[1])[keep])
    _check(r, t.sample(c[4:4 + K], mask))
    assert np.array_equal(r.moments[..., 3], np.where(mask != 0, 4 + K, 4).astype(np.float32))
    # the sample index advanced for everybody: the next full-frame call deposits samples 4 + K ..
    r.sample(2)
    _check(r, t.sample(c[4 + K:6 + K]), "full frame after the selected launch: ")


@pytest.mark.parametrize("K", [3, 8, 12])      # scalar loop; vector loop; vector loop plus remainder
@pytest.mark.parametrize("selected", [False, True], ids=["full_frame", "selected"])
def test_the_snapshot_holds_all_four_words(selected, K):
    """the snapshot is internal, and rtpbr_noise_update decides "nothing new" from its count alone: its r, g, b show only in the
    batch mean of the NEXT untracked batch.  Tracked call (no noise_update after it), tracking off, sample(2), noise_update: the
    moments must be what noise_ref_lib makes of the restated snapshot and the new image_buffer — a wrong s.rgb is a wrong mean."""
    w, h = FRAMES["20x13"]
    scene, cfg = _scene("cornell_v3", w, h)
    c = _ref_colours("cornell_v3", "20x13")
    r = Renderer(scene, cfg)
    r.set_noise_tracking(True)
    t = sm.Tracker(w, h)
    if selected:
        mask = _third(w, h)
        r.sample(4)
        r.select_mask(mask)
        r.sample_selected(K)
        t.sample(c[:4]).sample(c[4:4 + K], mask)
    else:
        r.sample(K)
        t.sample(c[:K])
    ck.same(r.moments, t.moments, "moments after the tracked call")
    r.set_noise_tracking(False)
    r.sample(2)                                   # one untracked batch of two samples on top of the tracked snapshot
    ib = r.image_buffer
    r.noise_update()
    ref = nr.Tracker(w, h)
    ref.moments, ref.snapshot = t.moments.copy(), t.snapshot.copy()
    ref.update(ib)
    ck.same(r.moments, ref.moments, "moments after an untracked batch on the tracked snapshot")
    # the check has teeth: the same batch on a snapshot with the right count and no colour gives other moments
    wrong = nr.Tracker(w, h)
    wrong.moments, wrong.snapshot = t.moments.copy(), t.snapshot.copy()
    wrong.snapshot[..., :3] = 0
    wrong.update(ib)
    assert (ck.bits(wrong.moments) != ck.bits(ref.moments)).any()
    assert (r.moments[..., 3] == t.moments[..., 3] + 1).all()


def test_a_full_mask_equals_the_unselected_call():
    w, h = FRAMES["20x13"]
    scene, cfg = _scene("cornell_v3", w, h)
    a, b = Renderer(scene, cfg), Renderer(scene, cfg)
    for x in (a, b):
        x.set_noise_tracking(True)
    a.select_mask(np.ones((w, h), np.uint8))
    a.sample_selected(8)
    b.sample(8)
    ck.same(a.moments, b.moments, "moments")
    ck.same(a.image_buffer, b.image_buffer, "image_buffer")
    assert ck.counters(a) == ck.counters(b)
    _check(a, sm.Tracker(w, h).sample(_ref_colours("cornell_v3", "20x13", 8)))


def test_mixed_with_noise_update_and_reproject():
    """tracked sample(4) -> noise_update (nothing new) -> reproject (the moments are warped as today) -> tracked sample(4) ->
    noise_estimate, against noise_ref_lib on the restated moments"""
    w, h = FRAMES["20x13"]
    scene, cfg = _scene("cornell_v3", w, h)
    old, new = rp.MOVES["translate"](scene.camera)
    r = Renderer(scene, cfg, old)
    r.refresh()
    r.set_noise_tracking(True)
    r.sample(4)
    c_old = sm.oracle_colours(OracleRenderer(scene, cfg, old), 0, 4)
    t = sm.Tracker(w, h).sample(c_old)
    M = r.moments
    ck.same(M, t.moments, "moments")
    r.noise_update()
    ck.same(r.moments, M, "moments after noise_update")
    r.render_features()
    old_feats = fd._gpu_features(r)
    ib = r.image_buffer
    r.reproject(new)
    assert r.noise_per_sample and r.camera is new
    new_feats = fd._gpu_features(r)
    ib_w, M_w = nr.reproject(cfg, old, new, ib, M, old_feats, new_feats)
    ck.same(r.image_buffer, ib_w, "warped image_buffer")
    ck.same(r.moments, M_w, "warped moments")
    t.moments, t.image_buffer, t.snapshot = M_w.copy(), ib_w.copy(), ib_w.copy()
    r.sample(4)
    # the sample index goes on across rtpbr_reproject: the new view's samples 4 .. 7
    c_new = sm.oracle_colours(OracleRenderer(scene, cfg, new), 4, 4)
    t.sample(c_new)
    ck.same(r.image_buffer, t.image_buffer, "image_buffer after the second tracked call")
    ck.same(r.moments, t.moments, "moments after the second tracked call")
    st = r.noise_estimate(0.02)
    noise, _, want = nr.estimate(t.image_buffer, t.moments, fd._gpu_features(r)["object"], 0.02)
    ck.same(r.noise, noise, "noise")
    assert (st.pixels_estimated, st.pixels_above) == want[:2]


def test_state_rules():
    w, h = FRAMES["20x13"]
    scene, cfg = _scene("cornell_v3", w, h)
    c = _ref_colours("cornell_v3", "20x13")
    r = Renderer(scene, cfg)
    r.sample(2)                                   # untracked: the set call folds these as one batch, as noise_update would
    with pytest.raises(RtpbrError) as e:
        r._read(BUF_MOMENTS)
    assert e.value.code == ESTATE
    r.set_noise_tracking(True)
    t2 = nr.Tracker(w, h)
    t2.update(r.image_buffer)
    ck.same(r.moments, t2.moments, "moments after the set call")
    t = sm.Tracker(w, h)
    t.moments, t.snapshot, t.image_buffer = t2.moments.copy(), t2.snapshot.copy(), r.image_buffer
    r.sample(3)
    _check(r, t.sample(c[2:5]), "after a batch and three samples: ")
    # refresh zeroes M and s, tracking stays on
    r.refresh()
    assert (r.moments == 0).all()
    r.sample(3)                                   # (the sample index goes on across a refresh: samples 5 .. 7)
    _check(r, sm.Tracker(w, h).sample(c[5:8]), "after refresh: ")
    # write_buffer(IMAGE_BUFFER) re-takes s: written data is no batch, and the next samples continue from it
    ib = r.image_buffer
    ib[3:6, 2:9] = 0.0
    r.image_buffer = ib
    M = r.moments
    r.noise_update()
    ck.same(r.moments, M, "moments after a write and a noise_update")
    t = sm.Tracker(w, h)
    t.moments, t.snapshot, t.image_buffer = M.copy(), ib.copy(), ib.copy()
    r.sample(2)
    _check(r, t.sample(c[8:10]), "after a write: ")
    # OFF sets the mode and nothing else: the next call is a plain one, its samples are one batch of the next noise_update
    M = r.moments
    r.set_noise_tracking(False)
    ck.same(r.moments, M, "moments after OFF")
    r.sample(2)
    ck.same(r.moments, M, "moments after an untracked call")
    # a new resolution frees the buffers; the mode survives and the next tracked call makes them again, zeroed
    r.set_noise_tracking(True)
    w2, h2 = FRAMES["7x5"]
    scene2, cfg2 = _scene("cornell_v3", w2, h2)
    r.set_config(cfg2)
    r.set_camera(scene2.camera)
    with pytest.raises(RtpbrError) as e:
        r._read(BUF_MOMENTS)
    assert e.value.code == ESTATE
    r.refresh()
    r.set_option("sample_base", 0)
    r.sample(3)
    _check(r, sm.Tracker(w2, h2).sample(_ref_colours("cornell_v3", "7x5", 3)), "after a new resolution: ")
    # set_scene keeps the mode
    r.set_scene(scene2)
    r.refresh()
    r.sample(1)
    assert (r.moments[..., 3] == 1).all()


def _code(call, *a):
    with pytest.raises(RtpbrError) as e:
        call(*a)
    return e.value.code


def test_refusals_change_nothing():
    from raytracingpbr_amd import _capi
    api = _capi.hip_api()
    ctx = C.c_void_p()
    api.call("create", 0, C.byref(ctx))
    try:
        assert api.fn["set_noise_tracking"](ctx, 1) == ESTATE           # before set_config
        assert api.fn["set_noise_tracking"](None, 1) == EINVAL
    finally:
        api.call("destroy", ctx)
    w, h = FRAMES["20x13"]
    scene, cfg = _scene("cornell_v3", w, h)
    r = Renderer(scene, cfg)
    r.set_noise_tracking(True)
    r.sample(3)
    r.select_mask(_third(w, h))
    keep = {b: r._read(b) for b in (BUF_IMAGE_BUFFER, BUF_MOMENTS)}
    counters = ck.counters(r)
    for mode in (2, -1, 7):
        assert r.api.fn["set_noise_tracking"](r._ctx, mode) == EINVAL
    r.set_tiles(16, 16, 0, 2)
    assert _code(r.set_noise_tracking, True) == ESTATE
    assert _code(r.sample, 1) == ESTATE
    assert _code(r.sample_selected, 1) == ESTATE
    r.set_tiles(0, 0, 0, 1)
    r.set_option("precision", 1)
    assert _code(r.sample, 1) == ESTATE
    r.set_option("precision", 0)
    assert r.noise_per_sample is True
    assert ck.counters(r) == counters
    for b, a in keep.items():
        ck.same(r._read(b), a, f"buffer {b} after refused calls")
    # ... and neither the mode nor the sample index moved: the next tracked call deposits samples 3 and 4
    r.sample(2)
    _check(r, sm.Tracker(w, h).sample(_ref_colours("cornell_v3", "20x13", 5)))
    # the persistent-ray form has no per-sample records
    scene, cfg = src_scene(aspect=20 / 13), Config.src(20, 13, 7, steps_per_launch=1)
    p = fd._renderer(scene, cfg)
    p.sample(2)
    p.set_noise_tracking(True)                   # the set call itself is noise_update: any form
    before, M = p.image_buffer, p.moments
    assert _code(p.sample, 1) == ESTATE
    ck.same(p.image_buffer, before, "image_buffer")
    ck.same(p.moments, M, "moments")
    p.set_noise_tracking(False)
    p.sample(1)


def test_render_until_and_render_adaptive_per_sample():
    scene, cfg = cornell_box("v3"), Config.cornell_v3(48, 32, 0, 3)
    noise, batch, max_spp = 0.08, 8, 40
    # render_until: tracked batches, an estimate after each (the first included), until nothing is above
    r, host = Renderer(scene, cfg), Renderer(scene, cfg)
    r.track_noise = True
    used, st = r.render_until(noise, max_spp, batch_spp=batch, per_sample=True)
    assert r.noise_per_sample is False and r.track_noise is True
    host.set_noise_tracking(True)
    h_used, h_st, estimates = 0, None, 0
    while h_used < max_spp:
        host.sample(batch)
        h_used += batch
        h_st = host.noise_estimate(noise)
        estimates += 1
        if h_st.pixels_above == 0:
            break
    assert used == h_used and (st.pixels_estimated, st.pixels_above) == (h_st.pixels_estimated, h_st.pixels_above)
    ck.same(r.image_buffer, host.image_buffer, "render_until: image_buffer")
    ck.same(r.moments, host.moments, "render_until: moments")
    ck.same(r.noise, host.noise, "render_until: noise")
    assert (r.moments[..., 3] == used).all()
    # a one-batch budget is estimated from that batch alone
    one = Renderer(scene, cfg)
    used1, st1 = one.render_until(0.0, batch, batch_spp=batch, per_sample=True)
    assert used1 == batch and st1.pixels_estimated == 48 * 32 and (one.moments[..., 3] == batch).all()
    # render_adaptive: ONE full-frame batch, then select_noisy -> sample_selected
    a, host = Renderer(scene, cfg), Renderer(scene, cfg)
    a.set_noise_tracking(True)                   # on before: stays on after
    traced, st = a.render_adaptive(noise, max_spp, batch_spp=batch, dilate=1, per_sample=True)
    assert a.noise_per_sample is True
    host.set_noise_tracking(True)
    host.sample(batch)
    h_traced, h_used = 48 * 32 * batch, batch
    while h_used + batch <= max_spp:
        n_sel = host.select_noisy(noise, 1)
        if n_sel == 0:
            break
        host.sample_selected(batch)
        h_traced, h_used = h_traced + n_sel * batch, h_used + batch
    h_st = host.noise_estimate(noise)
    assert traced == h_traced == int(a.image_buffer[..., 3].sum())
    assert (st.pixels_estimated, st.pixels_above) == (h_st.pixels_estimated, h_st.pixels_above)
    ck.same(a.image_buffer, host.image_buffer, "render_adaptive: image_buffer")
    ck.same(a.moments, host.moments, "render_adaptive: moments")
    assert np.array_equal(a.moments[..., 3], a.image_buffer[..., 3]) and a.image_buffer[..., 3].min() >= batch
    with pytest.raises(ValueError):
        a.render_adaptive(noise, 0, per_sample=True)
