"""Temporal reuse across rigid object motion on the GPU (rtpbr_reproject_scene): the gather held bit for bit to the CPU restatement
tests/post_ref/gather.h, an unmoved table held to rtpbr_reproject itself, the oracle continuing from the
warped image_buffer, the state and error rules of include/rtpbr.h, one call sequence over the stateful stages, and the quality
gain over refreshing while a box slides and turns.

Every renderer here runs the ahead-of-time kernels (option jit = 0): a moved Cornell table is a scene no baked instance serves,
and no test may start a compiler."""
import numpy as np
import pytest

import checks as ck
import feature_ref_lib as fr
import noise_ref_lib as nr
import pool_ref_lib as pl
import present_ref_lib as pr
import reproject_ref_lib as rr
import reproject_scene_ref_lib as rs
import test_gpu_features_denoise as fd
import test_gpu_reproject as tg
from oracle_backend import OracleRenderer
from raytracingpbr_amd import SHAPE, Config, Scene, cornell_box, src_scene
from raytracingpbr_amd._capi import RtpbrError
from raytracingpbr_amd.dataclass import SDFObject
from raytracingpbr_amd.ibl import synthetic_env

pytestmark = pytest.mark.gpu

ESTATE, EINVAL = -4, -1
W, H = 97, 61          # no multiple of the 256-lane blocks, H no multiple of 64
_same = tg._assert_same_bits


def _renderer(scene, cfg, cam=None):
    r = fd._renderer(scene, cfg)
    r.set_option("jit", 0)
    r.set_camera(cam if cam is not None else scene.camera)
    r.refresh()
    return r


def _oracle(scene, cfg, cam=None):
    o = OracleRenderer(scene, cfg, cam)
    if cfg.sky_kind == 1:
        o.set_env(synthetic_env(192, 96, seed=0), 1.4, 2.2)
    o.refresh()
    return o


def _spp(cfg):
    return 4 if cfg.kernel_form == 0 else 8      # (past the cap of 3 the second parameter set uses)


# ---------------------------------------------------------------- 1. bit identity with the restatement
def _cornell():
    return cornell_box("v3", aspect=W / H), Config.cornell_v3(W, H, 0, 3)


def _src():
    return src_scene(aspect=W / H), Config.src(W, H, 7, steps_per_launch=1)


# scene -> (translated object, its offset; rotated object): Cornell's small box; the src/ scene's blue sphere and its back box
# (objects sorted by type: four spheres — the first the ground, a sphere of radius 100 —, two boxes, the cylinder)
_WHO = {"cornell_v3": (6, (0.08, 0.0, 0.05), 6), "src": (2, (0.25, 0.0, 0.1), 5)}
_SCENES = {"cornell_v3": _cornell, "src": _src}


def _moves(name, scene):
    t, off, rot = _WHO[name]
    n = len(scene.objects)
    unit = 0.1 if scene.scale10 else 1.0
    both = {t: (off, (0, 0, 0)), rot: ((0, 0, 0), (0, 7, 0))} if t != rot else {t: (off, (0, 7, 0))}
    return {
        "translate": ({t: (off, (0, 0, 0))}, None),
        "rotate": ({rot: ((0, 0, 0), (0, 7, 0))}, None),
        "both_and_camera": (both, tg.MOVES["translate"](scene.camera)[1]),
        "every_object": ({k: ((0.03 * unit * ((k % 3) - 1), 0.02 * unit, -0.025 * unit), (0, 1.5, 0)) for k in range(n)}, None),
    }


def _restated(scene, cfg, new_scene, new_cam, ib, moments=None, **params):
    w = tg._bunny_weights(scene)
    f0 = fr.features(scene, cfg, scene.camera, w)
    f1 = fr.features(new_scene, cfg, new_cam if new_cam is not None else scene.camera, w)
    return f1, rs.reproject_scene(cfg, scene, new_scene, scene.camera, new_cam, ib, f0, f1, moments=moments, **params)


def _check_against_restatement(scene, cfg, new_scene, new_cam, with_moments=False, **params):
    r = _renderer(scene, cfg)
    M = None
    if with_moments:
        for _ in range(2):
            r.sample(_spp(cfg))
            r.noise_update()
        M = r.moments
    else:
        r.sample(_spp(cfg))
    ib = r.image_buffer
    r.reproject_scene(new_scene, new_cam, **params)
    f1, (want_ib, want_mv, want_M) = _restated(scene, cfg, new_scene, new_cam, ib, M, **params)
    fd._assert_features_equal(fd._gpu_features(r), f1)
    _same(r.image_buffer, want_ib, "image_buffer")
    _same(r.motion, want_mv, "motion")
    if with_moments:
        _same(r.moments, want_M, "moments")
        assert (want_M[..., 3] > 0).any()
    r.close()
    return ib, want_ib, want_mv, f1


@pytest.mark.parametrize("move", ["translate", "rotate", "both_and_camera", "every_object"])
@pytest.mark.parametrize("name", list(_SCENES))
def test_gather_bit_identical_to_restatement(name, move):
    scene, cfg = _SCENES[name]()
    moves, new_cam = _moves(name, scene)[move]
    new_scene = rs.moved_scene(scene, moves)
    assert rs.moved(scene, new_scene).tolist() == [k in moves for k in range(len(scene.objects))]
    for kw in ({}, {"max_history": 3.0, "depth_tolerance": 0.05, "normal_cos": 0.9}, {"with_moments": True}):
        ib, out, mv, f1 = _check_against_restatement(scene, cfg, new_scene, new_cam, **kw)
        kept = ~((mv[..., 0] == -1) & (mv[..., 1] == -1))
        assert kept.any() and (~kept).any(), kw
        assert (out[kept][:, 3] > 0).all() and (out[~kept] == 0).all()
        on_moved = np.isin(f1["object"], list(moves))
        assert (kept & on_moved).any(), kw          # the moved objects' own history is reused, not only dropped


# ---------------------------------------------------------------- 2. fewer pixels than table words
def test_a_frame_smaller_than_the_object_table():
    """7 x 5: 35 pixels, one block, and 8 x 25 = 200 table words to stage — the staging loop must not be driven by the lanes that
    own a pixel"""
    scene, cfg = cornell_box("v3", aspect=7 / 5), Config.cornell_v3(7, 5, 0, 3)
    moves = {5: ((0.06, 0, 0), (0, 5, 0)), 6: ((0.1, 0, 0.05), (0, 7, 0))}
    new_scene = rs.moved_scene(scene, moves)
    for kw in ({}, {"with_moments": True}):
        ib, out, mv, f1 = _check_against_restatement(scene, cfg, new_scene, None, **kw)
        assert np.isin(f1["object"], [5, 6]).any() and (out[..., 3] > 0).any()


# ---------------------------------------------------------------- 3. an unmoved table is rtpbr_reproject
@pytest.mark.parametrize("camera_moves", [False, True])
@pytest.mark.parametrize("name", list(_SCENES))
def test_unmoved_table_is_rtpbr_reproject(name, camera_moves):
    scene, cfg = _SCENES[name]()
    cam = tg.MOVES["translate"](scene.camera)[1] if camera_moves else None
    a, b = _renderer(scene, cfg), _renderer(scene, cfg)
    for r in (a, b):
        for _ in range(2):
            r.sample(_spp(cfg))
            r.noise_update()
    a.reproject_scene(rs.moved_scene(scene, {}), cam)
    b.reproject(cam if camera_moves else scene.camera)
    _same(a.image_buffer, b.image_buffer, "image_buffer")
    _same(a.motion, b.motion, "motion")
    _same(a.moments, b.moments, "moments")
    assert (a.image_buffer[..., 3] > 0).any()
    for r in (a, b):
        r.sample(3)
        r.noise_update()               # (the snapshot both calls left is what this batch is taken against)
    _same(a.image_buffer, b.image_buffer, "3 more samples")
    _same(a.moments, b.moments, "moments after the next batch")
    a.close()
    b.close()


# ---------------------------------------------------------------- 4. what does not move keeps its bits
def test_a_still_camera_keeps_the_bits_of_everything_the_box_never_covers():
    scene, cfg = _cornell()
    new_scene = rs.moved_scene(scene, {6: ((0.08, 0.0, 0.05), (0, 0, 0))})
    r = _renderer(scene, cfg)
    r.sample(2)
    ib = r.image_buffer
    r.reproject_scene(new_scene, None, max_history=1e6)
    out, mv = r.image_buffer, r.motion
    f0, f1 = fr.features(scene, cfg), fr.features(new_scene, cfg)
    still = (f0["object"] == f1["object"]) & (f0["object"] >= 0) & (f0["object"] != 6)
    assert still.sum() > W * H // 2
    assert np.array_equal(ck.bits(out[still]), ck.bits(ib[still]))
    xs, ys = np.meshgrid(np.arange(W), np.arange(H), indexing="ij")
    own = (mv[..., 0] == xs) & (mv[..., 1] == ys)
    assert own[still].all()
    box = f1["object"] == 6
    assert box.sum() >= 20 and not own[box].any()
    assert (mv[box][:, 0] >= 0).any()              # ... and some of the box's pixels found their history where the box was
    r.close()


# ---------------------------------------------------------------- 5. the oracle continues the render
def _oracle_continues(name):
    scene, cfg = _SCENES[name]()
    t, off, rot = _WHO[name]
    new_scene = rs.moved_scene(scene, {t: (off, (0, 0, 0)), rot: ((0, 0, 0), (0, 7, 0))} if t != rot else {t: (off, (0, 7, 0))})
    new_cam = tg.MOVES["translate"](scene.camera)[1]
    r = _renderer(scene, cfg)
    r.sample(3)
    r.sample(2)
    r.reproject_scene(new_scene, new_cam)
    ib = r.image_buffer
    r.sample(5)
    got = r.image_buffer
    o = _oracle(scene, cfg)
    o.sample(3)
    o.sample(2)                 # the same sample_base as the GPU's
    o.set_scene(new_scene)
    o.set_camera(new_cam)
    o.refresh()
    o.image_buffer = ib
    o.sample(5)
    _same(got, o.image_buffer, "image_buffer after reproject_scene + 5 sample calls")
    assert (ib[..., 3] > 0).any() and not np.array_equal(ib, got)
    r.close()
    o.close()


def test_oracle_holds_the_samples_after_the_call_complete_path():
    _oracle_continues("cornell_v3")


def test_oracle_holds_the_samples_after_the_call_persistent():
    _oracle_continues("src")


# ---------------------------------------------------------------- 6. errors and state
def _variant(scene, change):
    objs = [SDFObject.from_buffer_copy(bytes(o)) for o in scene.objects]
    change(objs)
    return Scene(objs, scene.scale10, scene.camera, scene.name)


def _set(path, value):
    def change(objs):
        o = objs[6]
        if path == "type":
            o.type = int(value)
        elif path == "scale":
            o.transform.scale[2] = value
        elif path == "ior":
            o.material.ior = value
        elif path == "albedo":
            o.material.albedo[1] = value
    return change


def test_errors_and_state():
    w, h = 32, 24
    scene, cfg = cornell_box("v3", aspect=w / h), Config.cornell_v3(w, h, 0, 3)
    moved = rs.moved_scene(scene, {6: ((0.05, 0, 0.03), (0, 7, 0))})
    cams = [tg._translated(scene.camera, 0.01 * k) for k in range(1, 8)]
    r, twin = _renderer(scene, cfg), _renderer(scene, cfg)       # the twin makes every call but the refused ones
    for x in (r, twin):
        x.sample(1)
        x.reproject(scene.camera)                                  # the motion buffer exists from here on

    def table(x):
        return b"".join(bytes(o) for o in x.get_scene())

    def refused(code, call, what):
        before = table(r), r.image_buffer, r.motion, r.scene, r.camera
        with pytest.raises(RtpbrError) as e:
            call()
        assert e.value.code == code, what
        assert table(r) == before[0], what
        _same(r.image_buffer, before[1], f"image_buffer after a refused call ({what})")
        _same(r.motion, before[2], f"motion after a refused call ({what})")
        assert r.scene is before[3] and r.camera is before[4], what

    def reproject_as_the_twin(cam, code=None):
        got = []
        for x in (r, twin):
            try:
                x.reproject(cam)
                got.append(None)
            except RtpbrError as e:
                got.append(e.code)
        assert got == [code, code]
        _same(r.image_buffer, twin.image_buffer, "image_buffer after the following rtpbr_reproject")
        _same(r.motion, twin.motion, "motion after the following rtpbr_reproject")

    # the rigidity check: each violation alone is RTPBR_EINVAL, and so are NULL objects
    violations = {
        "n": Scene(list(moved.objects)[:7], True, scene.camera),
        "type": _variant(moved, _set("type", SHAPE.SPHERE)),
        "scale": _variant(moved, _set("scale", 0.26)),
        "material ior": _variant(moved, _set("ior", 1.25)),
        "material albedo": _variant(moved, _set("albedo", 0.41)),
        "scale10": Scene(list(moved.objects), False, scene.camera),
    }
    for k, (what, bad) in enumerate(violations.items()):
        assert rs.moved(scene, bad) is None, what
        refused(EINVAL, lambda: r.reproject_scene(bad), what)
        assert "not a rigid motion" in str(pytest.raises(RtpbrError, r.reproject_scene, bad).value)
        reproject_as_the_twin(cams[k])
    refused(EINVAL, lambda: r.api.call("reproject_scene", r._ctx, None, None, 8, 1, None), "NULL objects")
    for bad in ({"max_history": 0.0}, {"depth_tolerance": -0.1}, {"normal_cos": 1.5}, {"max_history": float("nan")}):
        refused(EINVAL, lambda: r.reproject_scene(moved, **bad), str(bad))
    # history that set_scene broke is not repaired
    for x in (r, twin):
        x.set_scene(scene)
    refused(ESTATE, lambda: r.reproject_scene(moved), "after set_scene")
    reproject_as_the_twin(cams[6], ESTATE)
    for x in (r, twin):
        x.refresh()
        x.sample(1)
    # tiles of world > 1
    for x in (r, twin):
        x.set_tiles(16, 16, 0, 2)
    refused(ESTATE, lambda: r.reproject_scene(moved), "tiles of world > 1")
    reproject_as_the_twin(cams[6], ESTATE)
    for x in (r, twin):
        x.set_tiles(0, 0, 0, 1)
    reproject_as_the_twin(cams[6])
    # a changed animation frame
    for x in (r, twin):
        x.set_config(cfg.copy(frame=17))
    refused(ESTATE, lambda: r.reproject_scene(moved), "after a config change of frame")
    reproject_as_the_twin(cams[5], ESTATE)
    for x in (r, twin):
        x.refresh()
        x.sample(1)
    # a success: the new table is the context's, history and features are valid
    r.reproject_scene(moved, cams[0])
    assert r.scene is moved and r.camera is cams[0]
    fresh = _renderer(moved, cfg)
    assert table(r) == table(fresh)
    assert (r.image_buffer[..., 3] > 0).any()
    r.reproject(cams[1])
    r.reproject_scene(rs.moved_scene(moved, {5: ((0, 0, 0.02), (0, 0, 0))}))        # and again, from the history it left
    for x in (r, twin, fresh):
        x.close()


# ---------------------------------------------------------------- 7. one call sequence, every stage held to its restatement
def test_call_sequence_over_the_stateful_stages():
    w, h = 67, 45
    scene, cfg = cornell_box("v3", aspect=w / h), Config.cornell_v3(w, h, 3, 3)
    new_scene = rs.moved_scene(scene, {6: ((0.06, 0, 0.04), (0, 7, 0))})
    cam0, cam2 = scene.camera, tg._translated(scene.camera, 0.015)
    threshold, dilate = 0.05, 1
    r, o, tracker = _renderer(scene, cfg), _oracle(scene, cfg), nr.Tracker(w, h)
    r.set_noise_estimator(0, 3, 0)

    def sample_and_update(n):
        r.sample(n)
        o.sample(n)
        _same(r.image_buffer, o.image_buffer, f"image_buffer after sample({n})")
        r.noise_update()
        _same(r.moments, tracker.update(o.image_buffer), "moments after noise_update")

    sample_and_update(3)
    sample_and_update(2)
    # reproject_scene
    f0, f1 = fr.features(scene, cfg, cam0), fr.features(new_scene, cfg, cam0)
    want_ib, want_mv, want_M = rs.reproject_scene(cfg, scene, new_scene, cam0, None, o.image_buffer, f0, f1, moments=tracker.moments)
    r.reproject_scene(new_scene)
    _same(r.image_buffer, want_ib, "image_buffer after reproject_scene")
    _same(r.motion, want_mv, "motion after reproject_scene")
    _same(r.moments, want_M, "moments after reproject_scene")
    tracker.moments[:], tracker.snapshot[:] = want_M, want_ib
    o.set_scene(new_scene)
    o.refresh()
    o.image_buffer = want_ib
    sample_and_update(2)          # (against the snapshot the call left)
    # select_noisy
    ib = o.image_buffer
    noise, _, _ = pl.estimate(ib, tracker.moments, f1["object"], threshold, 0, 3)
    mask = pl.select(noise, ib[..., 3], threshold, dilate, 0)
    n_sel = r.select_noisy(threshold, dilate)
    _same(r.noise, noise, "noise")
    assert np.array_equal(r.selection, mask) and n_sel == int(mask.sum())
    assert 0 < n_sel < w * h
    # sample_selected
    o.sample(2)
    ib = np.where((mask != 0)[..., None], o.image_buffer, ib)
    o.image_buffer = ib
    r.sample_selected(2)
    _same(r.image_buffer, ib, "image_buffer after sample_selected")
    # reproject
    f2 = fr.features(new_scene, cfg, cam2)
    want_ib, want_mv = rr.reproject(cfg, cam0, cam2, ib, f1, f2)
    ib_m, want_M = nr.reproject(cfg, cam0, cam2, ib, tracker.moments, f1, f2)
    assert np.array_equal(ck.bits(ib_m), ck.bits(want_ib))
    r.reproject(cam2)
    _same(r.image_buffer, want_ib, "image_buffer after reproject")
    _same(r.motion, want_mv, "motion after reproject")
    _same(r.moments, want_M, "moments after reproject")
    # present("accum")
    o.set_camera(cam2)
    o.refresh()
    o.image_buffer = want_ib
    o.post_process()
    r.present("accum", "rgba8", False)
    assert np.array_equal(r.presented, pr.present(o.image_pixels, pr.FORMAT_RGBA8, False))
    r.close()
    o.close()


# ---------------------------------------------------------------- 8. quality while a box slides and turns
def _pose(scene, k):
    """frame k of the animation of examples/reproject_moving.py: Cornell's small box slides (0.01, 0, 0.03) and turns 3 degrees a frame"""
    return rs.moved_scene(scene, {6: ((0.01 * k, 0, 0.03 * k), (0, 3.0 * k, 0))})


def test_reproject_scene_beats_refresh_while_a_box_moves():
    """64 x 64, 4 spp a frame, 6 frames, max_history = 16: overall display RMSE against converged frames of the same poses, with
    reproject_scene over that of refreshing on every frame.  The only claim is a ratio below 1 (the same measurement on the CPU
    oracle with the restatement, 512-spp truths: 0.909; the history carries the old frames' shadows of the box)."""
    w = h = 64
    spp, frames, max_history = 4, 6, 16.0
    scene, cfg = cornell_box("v3"), Config.cornell_v3(w, h, 0, 3)
    a, b = _renderer(_pose(scene, 0), cfg), _renderer(_pose(scene, 0), cfg)
    a.sample(spp)
    b.sample(spp)
    se_a, se_b = [], []
    for k in range(1, frames):
        new = _pose(scene, k)
        a.set_scene(new)
        a.refresh()
        a.sample(spp)
        a.post_process()
        b.reproject_scene(new, max_history=max_history)
        b.sample(spp)
        b.post_process()
        t = _renderer(new, cfg)
        t.set_option("sample_base", 1 << 20)       # samples independent of the frames'
        t.sample(1024)
        t.post_process()
        truth = tg._display(t)
        t.close()
        e_a, e_b = tg._rmse(tg._display(a), truth), tg._rmse(tg._display(b), truth)
        print(f"frame {k}: display RMSE refresh {e_a:.4f}, reproject_scene {e_b:.4f}")
        se_a.append(e_a ** 2)
        se_b.append(e_b ** 2)
    ratio = float(np.sqrt(np.mean(se_b)) / np.sqrt(np.mean(se_a)))
    print(f"overall display RMSE ratio reproject_scene / refresh: {ratio:.4f}")
    assert ratio < 1.0, ratio
    a.close()
    b.close()
