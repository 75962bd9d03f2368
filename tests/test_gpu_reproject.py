"""Temporal reuse on the GPU (rtpbr_reproject): the gather held bit for bit to the CPU restatement tests/post_ref/gather.h,
the oracle continuing from a reprojected image_buffer, the state and error rules of include/rtpbr.h, and the quality gain over
refreshing on a moving camera."""
import math

import numpy as np
import pytest

import checks as ck
import feature_ref_lib as fr
import reproject_ref_lib as rr
import test_gpu_features_denoise as fd
from checks import EINVAL, ESTATE
from oracle_backend import OracleRenderer
from raytracingpbr_amd import SHAPE, Camera, Config, Renderer, cornell_box, src_scene
from raytracingpbr_amd._capi import RtpbrError
from raytracingpbr_amd.ibl import load_bunny_weights, synthetic_env
from raytracingpbr_amd.renderer import (BUF_FEAT_ALBEDO, BUF_FEAT_DEPTH, BUF_FEAT_NORMAL, BUF_FEAT_OBJECT, BUF_IMAGE_BUFFER,
                                        BUF_MOTION)

pytestmark = pytest.mark.gpu

W, H = 97, 61


def _assert_same_bits(got, want, what):
    bad = ck.bits(got) != ck.bits(want)
    assert not bad.any(), f"{what}: {int(bad.sum())} words differ, first at {np.argwhere(bad)[:4].tolist()}"


def _cam(c, lookfrom=None, lookat=None, vfov=None, aperture=None):
    return Camera(tuple(lookfrom if lookfrom is not None else c.lookfrom), tuple(lookat if lookat is not None else c.lookat), tuple(c.vup),
                  c.vfov if vfov is None else vfov, c.aspect, c.aperture if aperture is None else aperture, c.focus)


def _axes(c):
    lf, la, up = (np.array(v, np.float64) for v in (c.lookfrom, c.lookat, c.vup))
    z = (lf - la) / np.linalg.norm(lf - la)
    x = np.cross(up, z)
    return lf, la, up / np.linalg.norm(up), x / np.linalg.norm(x), float(np.linalg.norm(lf - la))


def _translated(c, fx, fz=0.0):
    """moved by fx of the eye-target distance along the camera's x axis and fz along its viewing direction"""
    lf, la, _, x, dist = _axes(c)
    fwd = (la - lf) / dist
    off = x * fx * dist + fwd * fz * dist
    return _cam(c, lf + off, la + off)


def _yawed(c, deg):
    lf, la, up, _, _ = _axes(c)
    v = la - lf
    a = math.radians(deg)
    v = v * math.cos(a) + np.cross(up, v) * math.sin(a) + up * np.dot(up, v) * (1 - math.cos(a))    # Rodrigues about vup
    return _cam(c, lf, lf + v)


MOVES = {
    "translate": lambda c: (c, _translated(c, 0.02)),
    "yaw": lambda c: (c, _yawed(c, 2.0)),
    "vfov": lambda c: (c, _cam(c, vfov=c.vfov * 1.1)),
    "thin_lens": lambda c: (_cam(c, aperture=0.3 * _axes(c)[4] / 35.0), _yawed(_translated(_cam(c, aperture=0.3 * _axes(c)[4] / 35.0), -0.015), -1.0)),
}


def _bunny_weights(scene):
    return load_bunny_weights() if any(o.type == SHAPE.BUNNY for o in scene.objects) else None


def _with_history(scene, cfg, cam, n=2):
    r = fd._renderer(scene, cfg)
    r.set_camera(cam)
    r.refresh()
    if n:
        r.sample(n)
    return r


def _check_against_restatement(scene, cfg, old, new, **params):
    r = _with_history(scene, cfg, old, 2 if cfg.kernel_form == 0 else 8)
    ib = r.image_buffer
    r.reproject(new, **params)
    w = _bunny_weights(scene)
    f0, f1 = fr.features(scene, cfg, old, w), fr.features(scene, cfg, new, w)
    want_ib, want_mv = rr.reproject(cfg, old, new, ib, f0, f1, **params)
    fd._assert_features_equal(fd._gpu_features(r), f1)
    _assert_same_bits(r.image_buffer, want_ib, "image_buffer")
    _assert_same_bits(r.motion, want_mv, "motion")
    return ib, want_ib, want_mv


@pytest.mark.parametrize("move", list(MOVES))
@pytest.mark.parametrize("name", list(fd._scenes(W, H)))
def test_gather_bit_identical_to_restatement(name, move):
    scene, cfg = fd._scenes(W, H)[name]
    old, new = MOVES[move](scene.camera)
    ib, out, mv = _check_against_restatement(scene, cfg, old, new)
    kept = ~((mv[..., 0] == -1) & (mv[..., 1] == -1))      # (a kept pixel may draw from x0 = -1 or y0 = -1 with a fraction)
    assert kept.any() and (~kept).any()       # (every move shows something the old frame did not)
    assert (out[kept][:, 3] > 0).all() and (out[~kept] == 0).all()


def test_gather_bit_identical_at_1080p():
    scene, cfg = cornell_box("v3", aspect=1920 / 1080), Config.cornell_v3(1920, 1080, 0, 3)
    old, new = MOVES["translate"](scene.camera)
    _check_against_restatement(scene, cfg, old, new, max_history=3.0, depth_tolerance=0.02, normal_cos=0.95)


def test_identical_camera_keeps_the_buffer_and_the_sample_sequence():
    scene, cfg = cornell_box("v3", aspect=W / H), Config.cornell_v3(W, H, 0, 3)
    a = _with_history(scene, cfg, scene.camera, 4)
    b = _with_history(scene, cfg, scene.camera, 4)
    ib = a.image_buffer
    a.reproject(scene.camera, max_history=1e6)
    _assert_same_bits(a.image_buffer, ib, "image_buffer after an identical reprojection")
    assert (a.motion[ib[..., 3] > 0] >= 0).all()
    a.sample(3)
    b.sample(3)
    _assert_same_bits(a.image_buffer, b.image_buffer, "3 more samples")


def _oracle_continues(scene, cfg, options=()):
    old, new = MOVES["translate"](scene.camera)
    r = _with_history(scene, cfg, old, 3)
    for k, v in options:
        r.set_option(k, v)
    r.sample(2)
    r.reproject(new)
    ib = r.image_buffer
    r.sample(5)
    got = r.image_buffer
    o = OracleRenderer(scene, cfg, old)
    if cfg.sky_kind == 1:
        o.set_env(synthetic_env(192, 96, seed=0), 1.4, 2.2)
    o.refresh()
    o.sample(3)
    o.sample(2)                 # the same sample_base as the GPU's
    o.set_camera(new)
    o.refresh()
    o.image_buffer = ib
    o.sample(5)
    _assert_same_bits(got, o.image_buffer, "image_buffer after reproject + 5 sample calls")
    assert (ib[..., 3] > 0).any() and not np.array_equal(ib, got)


def test_oracle_holds_the_samples_after_a_reprojection_complete_path():
    _oracle_continues(cornell_box("v3", aspect=W / H), Config.cornell_v3(W, H, 0, 3))


@pytest.mark.parametrize("lazy", [1, 0])
def test_oracle_holds_the_samples_after_a_reprojection_persistent(lazy):
    _oracle_continues(src_scene(aspect=W / H), Config.src(W, H, 7, steps_per_launch=1), (("src_lazy", lazy),))


def test_state_after_the_call():
    scene, cfg = src_scene(aspect=W / H), Config.src(W, H, 7, steps_per_launch=1).copy(adaptive_sampling=1)
    old, new = MOVES["yaw"](scene.camera)
    r = _with_history(scene, cfg, old, 5)
    r.post_process()
    r.render_features()
    ptrs = {b: r.device_ptr(b) for b in (BUF_IMAGE_BUFFER, BUF_FEAT_ALBEDO, BUF_FEAT_NORMAL, BUF_FEAT_DEPTH, BUF_FEAT_OBJECT)}
    assert (r.ray_depth() != 0).any()
    c0 = r.counters()
    r.reproject(new)
    assert {b: r.device_ptr(b) for b in ptrs} == ptrs
    c1 = r.counters()
    assert [getattr(c0, f) for f, _ in c0._fields_] == [getattr(c1, f) for f, _ in c1._fields_]
    feats = fd._gpu_features(r)
    r.render_features()
    fd._assert_features_equal(fd._gpu_features(r), feats)
    assert (r.ray_depth() == 0).all()
    ref = _with_history(scene, cfg, old, 5)
    ref.post_process()
    ref.set_camera(new)
    ref.refresh()
    _assert_same_bits(r.diff_buffer, ref.diff_buffer, "diff_buffer")
    _assert_same_bits(r.diff_pixels, ref.diff_pixels, "diff_pixels")


def test_async_read_of_image_buffer_lands_the_pre_call_contents():
    scene, cfg = cornell_box("v3", aspect=3840 / 2160), Config.cornell_v3(3840, 2160, 0, 3)
    r = _with_history(scene, cfg, scene.camera, 1)
    first = r.image_buffer
    out = r.host_array(BUF_IMAGE_BUFFER)
    t = r.read_async(BUF_IMAGE_BUFFER, out)
    r.reproject(_translated(scene.camera, 0.01))
    r.read_wait(t)
    _assert_same_bits(out, first, "the read-back")
    r.sync()
    assert not np.array_equal(r.image_buffer, first)


def test_errors():
    scene, cfg = cornell_box("v3"), Config.cornell_v3(32, 24, 0, 3)
    r = Renderer(scene, cfg)
    moved = _translated(scene.camera, 0.01)
    with pytest.raises(RtpbrError) as e:
        r._read(BUF_MOTION)
    assert e.value.code == ESTATE
    with pytest.raises(RtpbrError) as e:       # set_config ran and no refresh since
        r.reproject(moved)
    assert e.value.code == ESTATE
    r.refresh()
    r.sample(1)
    for bad in ({"max_history": 0.0}, {"max_history": -1.0}, {"max_history": float("inf")}, {"max_history": float("nan")},
                {"depth_tolerance": -0.1}, {"depth_tolerance": float("inf")}, {"normal_cos": 1.5}, {"normal_cos": -1.01},
                {"normal_cos": float("nan")}):
        with pytest.raises(RtpbrError) as e:
            r.reproject(moved, **bad)
        assert e.value.code == EINVAL, bad
    r.reproject(moved, depth_tolerance=0.0, normal_cos=-1.0)
    r.reproject(scene.camera)
    assert r.motion.shape == (32, 24, 2)
    with pytest.raises(RtpbrError) as e:
        r._write(BUF_MOTION, np.zeros((32, 24, 2), np.float32))
    assert e.value.code == EINVAL
    setters = {
        "set_config": lambda: r.set_config(cfg.copy(seed=5)),
        "set_scene": lambda: r.set_scene(scene),
        "set_env": lambda: r.set_env(synthetic_env(64, 32, seed=1), 1.0, 1.0),
        "set_shape_data": lambda: r.set_shape_data(SHAPE.BUNNY, load_bunny_weights()),
    }
    for name, setter in setters.items():
        setter()
        ib = r.image_buffer
        with pytest.raises(RtpbrError) as e:
            r.reproject(moved)
        assert e.value.code == ESTATE, name
        assert r.camera is not moved
        _assert_same_bits(r.image_buffer, ib, f"image_buffer after a refused call ({name})")
        r.refresh()
        r.sample(1)
        r.reproject(moved)
        r.reproject(scene.camera)
    r.set_tiles(16, 16, 0, 2)
    with pytest.raises(RtpbrError) as e:
        r.reproject(moved)
    assert e.value.code == ESTATE
    r.set_tiles(0, 0, 0, 1)
    r.reproject(moved)


# ---------------------------------------------------------------- quality over a camera path
def _path(c, n=6):
    """pan plus dolly: each frame moves 1.5 % of the eye-target distance sideways and 2 % towards the target"""
    return [_translated(c, 0.015 * k, 0.02 * k) for k in range(n)]


def _display(r):
    return np.nan_to_num(r.image_pixels, nan=0.0)      # pixels without samples show black


def _rmse(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)))


def _truth(scene, cfg, cam, converge):
    t = fd._renderer(scene, cfg)
    t.set_camera(cam)
    t.set_option("sample_base", 1 << 20)       # samples independent of the frames'
    t.refresh()
    converge(t)
    t.post_process()
    return _display(t)


@pytest.mark.parametrize("name", ["cornell_v3", "src_tokyo"])
def test_reprojection_beats_refresh_on_a_moving_camera(name):
    if name == "cornell_v3":
        scene, cfg = cornell_box("v3"), Config.cornell_v3(128, 128, 0, 3)
        per_frame, converge, truth_cfg = (lambda r: r.sample(4)), (lambda r: r.sample(1024)), cfg
    else:
        scene, cfg = src_scene(aspect=128 / 72), Config.src(128, 72, 7, steps_per_launch=1)
        per_frame, converge = (lambda r: r.sample(1)), (lambda r: [r.sample(64) for _ in range(64)])
        truth_cfg = cfg.copy(steps_per_launch=4)
    path = _path(scene.camera)
    a = _with_history(scene, cfg, path[0], 0)
    b = _with_history(scene, cfg, path[0], 0)
    per_frame(a)
    per_frame(b)
    for k, cam in enumerate(path[1:], 1):
        a.set_camera(cam)
        a.refresh()
        per_frame(a)
        a.post_process()
        b.reproject(cam)
        per_frame(b)
        b.post_process()
        truth = _truth(scene, truth_cfg, cam, converge)
        e_ref, e_rep = _rmse(_display(a), truth), _rmse(_display(b), truth)
        print(f"{name} frame {k}: display RMSE refresh {e_ref:.4f}, reproject {e_rep:.4f}")
        assert e_rep < e_ref, (k, e_ref, e_rep)
