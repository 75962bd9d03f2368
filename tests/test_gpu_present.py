"""The present stage on the GPU (rtpbr_present, rt_present.hip) held byte for byte to the numpy restatement
tests/present_ref_lib.py.  The kernel's tile is 64 x 64 pixels: the frame sizes cover every residue of W mod 4 (an RGB8 row of
3 W bytes starts dword-aligned in every row only when W % 4 == 0), one pixel and one row, and both axes below, at and above 64
and 128."""
import ctypes as C

import numpy as np
import pytest

import checks as ck
import present_ref_lib as pr
import test_gpu_features_denoise as fd
import test_present_ref as tp
from checks import EINVAL, ESTATE
from raytracingpbr_amd import Config, PresentParams, Renderer, cornell_box, imageio, src_scene
from raytracingpbr_amd._capi import RtpbrError
from raytracingpbr_amd.renderer import BUF_IMAGE_PIXELS, BUF_PRESENT

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 7), (7, 1), (2, 3), (5, 4), (63, 65), (64, 64), (65, 63), (127, 130), (130, 127), (257, 66)]
FORMATS = {"rgb8": pr.FORMAT_RGB8, "rgba8": pr.FORMAT_RGBA8}
F = np.float32


def _renderer(w, h):
    return Renderer(cornell_box("v3", aspect=w / h), Config.cornell_v3(w, h, 0, 3))


def _field(w, h, seed=0):
    """uniform values in [-0.25, 1.25] with the special values (NaN, the infinities, the zeros, 1, the float32 neighbours of every
    (k + 0.5) / 255) scattered over it: all of them where the frame has room (from 63 x 65 on), a random draw of them in half of
    the elements otherwise"""
    rng = np.random.default_rng(1000 * w + h + seed)
    a = rng.uniform(-0.25, 1.25, (w, h, 3)).astype(F)
    s = tp.specials()
    m = min(len(s), a.size // 2 + 1)
    a.reshape(-1)[rng.permutation(a.size)[:m]] = s if m == len(s) else rng.choice(s, m)
    return a


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.shape} {got.dtype} against {want.shape} {want.dtype}"
    bad = got != want
    assert not bad.any(), f"{what}: {int(bad.sum())} bytes differ, first at {np.argwhere(bad)[:4].tolist()}"


def _counters(r):
    c = r.counters()
    return tuple(getattr(c, f) for f, _ in c._fields_)


@pytest.mark.parametrize("dither", [False, True], ids=["plain", "dither"])
@pytest.mark.parametrize("fmt", ["rgb8", "rgba8"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pixels_byte_exact(shape, fmt, dither):
    w, h = shape
    r = _renderer(w, h)
    a = _field(w, h)
    r._write(BUF_IMAGE_PIXELS, a)
    r.present("pixels", fmt, dither)
    got = r.presented
    _same(got, pr.present(a, FORMATS[fmt], dither), f"{w}x{h} {fmt} dither={dither}")
    if fmt == "rgba8":
        assert (got[..., 3] == 255).all()
    if not dither and fmt == "rgb8":      # the drop-in claim: the bytes imageio.imwrite hands to the encoder
        _same(got, tp._host_path(a), "against the host path")


def _accum_setups():
    w, h = 65, 63
    yield "cornell_v3", cornell_box("v3", aspect=w / h), Config.cornell_v3(w, h, 0, 3), 2
    yield "src_adaptive", src_scene(aspect=w / h), Config.src(w, h, 7, steps_per_launch=1).copy(adaptive_sampling=1), 12


@pytest.mark.parametrize("setup", list(_accum_setups()), ids=lambda s: s[0])
def test_accum_is_post_process_without_its_writes(setup):
    _, scene, cfg, n = setup
    r = fd._renderer(scene, cfg)
    r.refresh()
    r.sample(n)
    r.post_process()            # image_pixels and the diff buffers hold an OLDER frame than image_buffer from here on
    r.sample(n)
    ib = r.image_buffer
    ib[3, 5] = 0                # a pixel without samples: 0 / 0
    r.image_buffer = ib
    assert (ib[..., 3] > 0).sum() > ib.shape[0] * ib.shape[1] // 4 and not (ib[3, 5] != 0).any()
    before = [r.image_buffer, r.image_pixels, r.diff_buffer, r.diff_pixels]
    counters = _counters(r)
    shown = {}
    for fmt in FORMATS:
        for dither in (False, True):
            r.present("accum", fmt, dither)
            shown[fmt, dither] = r.presented
    for a, b, name in zip(before, [r.image_buffer, r.image_pixels, r.diff_buffer, r.diff_pixels],
                          ["image_buffer", "image_pixels", "diff_buffer", "diff_pixels"]):
        assert np.array_equal(ck.bits(a), ck.bits(b)), f"present(accum) changed {name}"
    assert _counters(r) == counters
    r.post_process()
    px = r.image_pixels
    assert not np.array_equal(ck.bits(px), ck.bits(before[1])), "the second batch changed nothing: the test would pass on stale pixels"
    for (fmt, dither), got in shown.items():
        r.present("pixels", fmt, dither)
        _same(got, r.presented, f"accum against post_process + pixels, {fmt} dither={dither}")
        _same(got, pr.present(px, FORMATS[fmt], dither), f"accum against the restatement of image_pixels, {fmt} dither={dither}")
    assert (shown["rgb8", False][cfg.height - 1 - 5, 3] == pr.present(px, pr.FORMAT_RGB8, False)[cfg.height - 1 - 5, 3]).all()


@pytest.mark.parametrize("shape", [(65, 63), (130, 127)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_denoised(shape):
    w, h = shape
    r = _renderer(w, h)
    r.render(refreshing=True, spp=2)
    with pytest.raises(RtpbrError) as e:
        r.present("denoised")
    assert e.value.code == ESTATE
    with pytest.raises(RtpbrError) as e:      # ... and the refused call made no buffer
        r.presented
    assert e.value.code == ESTATE
    r.denoise(iterations=2)
    d = r.denoised_pixels
    assert not np.array_equal(ck.bits(d), ck.bits(r.image_pixels))
    for fmt in FORMATS:
        for dither in (False, True):
            r.present("denoised", fmt, dither)
            _same(r.presented, pr.present(d, FORMATS[fmt], dither), f"denoised {fmt} dither={dither}")


def test_nothing_else_moves():
    w, h = 65, 63
    r = _renderer(w, h)
    r.render(refreshing=True, spp=2)
    r.denoise(iterations=1)
    before = [r.image_buffer, r.image_pixels, r.denoised_pixels, r.diff_buffer, r.diff_pixels, r.ray_buffer]
    counters = _counters(r)
    assert counters[0] == w * h * 2
    for source in PresentParams.SOURCES:
        r.present(source, "rgb8", True)
        r.present(source)
    after = [r.image_buffer, r.image_pixels, r.denoised_pixels, r.diff_buffer, r.diff_pixels, r.ray_buffer]
    for a, b in zip(before, after):
        assert np.array_equal(ck.bits(a), ck.bits(b))
    assert _counters(r) == counters


def test_tiles_of_a_larger_world_present_whole_buffers():
    w, h = 65, 63
    r = _renderer(w, h)
    r.set_tiles(16, 16, 1, 2)
    a = _field(w, h, 3)
    r._write(BUF_IMAGE_PIXELS, a)
    r.present("pixels", "rgb8", True)
    _same(r.presented, pr.present(a, pr.FORMAT_RGB8, True), "world = 2")


def test_buffer_life():
    w, h = 65, 63
    r = _renderer(w, h)
    a = _field(w, h, 1)
    r._write(BUF_IMAGE_PIXELS, a)
    for call in (lambda: r.presented, lambda: r.device_ptr(BUF_PRESENT), lambda: r.host_array(BUF_PRESENT)):
        with pytest.raises(RtpbrError) as e:
            call()
        assert e.value.code == ESTATE
    # the reported size follows the last format
    r.present("pixels", "rgba8")
    addr, n = r.device_ptr(BUF_PRESENT)
    assert n == w * h * 4 and r.presented.shape == (h, w, 4)
    r.present("pixels", "rgb8")
    assert r.device_ptr(BUF_PRESENT) == (addr, w * h * 3) and r.presented.shape == (h, w, 3)
    wrong = np.empty((h, w, 4), np.uint8)
    assert r.api.fn["read_buffer"](r._ctx, BUF_PRESENT, wrong.ctypes.data_as(C.c_void_p), wrong.nbytes) == EINVAL
    # NULL parameters: image_pixels as RGBA8 without dither
    r.api.call("present", r._ctx, None)
    _same(r.presented, pr.present(a, pr.FORMAT_RGBA8, False), "defaults")
    # an output only
    frame = r.presented
    assert r.api.fn["write_buffer"](r._ctx, BUF_PRESENT, frame.ctypes.data_as(C.c_void_p), frame.nbytes) == EINVAL
    # bad parameters are refused and leave the frame (and its format) as it was
    for bad in ((-1, 1, 0), (3, 1, 0), (0, -1, 0), (0, 2, 0), (0, 1, 2), (0, 1, -1), (2, 0, 7)):
        p = PresentParams(*bad)
        assert r.api.fn["present"](r._ctx, C.byref(p)) == EINVAL, bad
    with pytest.raises(ValueError):
        r.present("bgra")
    _same(r.presented, frame, "after refused calls")
    # another resolution frees the buffer; the next present makes it again
    w2, h2 = 34, 70
    r.set_config(Config.cornell_v3(w2, h2, 0, 3))
    with pytest.raises(RtpbrError) as e:
        r.presented
    assert e.value.code == ESTATE
    b = _field(w2, h2, 2)
    r._write(BUF_IMAGE_PIXELS, b)
    r.present("pixels", "rgb8", True)
    _same(r.presented, pr.present(b, pr.FORMAT_RGB8, True), "after set_config")


def test_present_before_set_config_is_estate():
    from raytracingpbr_amd import _capi
    api = _capi.hip_api()
    ctx = C.c_void_p()
    api.call("create", 0, C.byref(ctx))
    try:
        assert api.fn["present"](ctx, None) == ESTATE
        p = PresentParams(5, 1, 0)
        assert api.fn["present"](ctx, C.byref(p)) == EINVAL
    finally:
        api.call("destroy", ctx)


def test_async_read_is_ordered_before_the_next_present():
    """frame A is still on its way to the host when frame B is presented into the same buffer: the device-side ordering keeps A"""
    w, h = 1920, 1080
    r = _renderer(w, h)
    rng = np.random.default_rng(5)
    a = rng.uniform(-0.25, 1.25, (w, h, 3)).astype(F)
    r._write(BUF_IMAGE_PIXELS, a)
    r.present("pixels", "rgba8")
    out = r.host_array(BUF_PRESENT)
    assert out.shape == (h, w, 4) and out.dtype == np.uint8
    b = np.ascontiguousarray(F(1) - a)
    r._write(BUF_IMAGE_PIXELS, b)
    t = r.read_async(BUF_PRESENT, out)
    r.present("pixels", "rgba8", True)
    r.read_wait(t)
    _same(out, pr.present(a, pr.FORMAT_RGBA8, False), "the asynchronous read holds frame A")
    _same(r.presented, pr.present(b, pr.FORMAT_RGBA8, True), "the blocking read afterwards holds frame B")
    into = np.empty((h, w, 4), np.uint8)
    assert r.read_into(BUF_PRESENT, into) is into and np.array_equal(into, r.presented)


def test_device_array_zero_copy():
    import torch
    w, h = 130, 127
    r = _renderer(w, h)
    r._write(BUF_IMAGE_PIXELS, _field(w, h, 4))
    r.present()
    r.sync()
    t = torch.as_tensor(r.device_array(BUF_PRESENT), device="cuda")
    assert tuple(t.shape) == (h, w, 4) and t.dtype == torch.uint8 and t.data_ptr() == r.device_ptr(BUF_PRESENT)[0]
    assert np.array_equal(t.cpu().numpy(), r.presented)


def test_save_image_equals_imwrite(tmp_path):
    from PIL import Image
    w, h = 65, 63
    r = _renderer(w, h)
    r.render(refreshing=True, spp=4)
    new, old = str(tmp_path / "new.png"), str(tmp_path / "old.png")
    r.save_image(new)
    imageio.imwrite(r.image_pixels, old)
    got, want = np.asarray(Image.open(new)), np.asarray(Image.open(old))
    assert got.shape == (h, w, 3) and got.dtype == np.uint8 and got.std() > 10
    _same(got, want, "save_image against imwrite(image_pixels)")
    r.save_image(new, source="accum", dither=True)
    _same(np.asarray(Image.open(new)), pr.present(r.image_pixels, pr.FORMAT_RGB8, True), "save_image(accum, dither)")


def test_the_example_writes_equal_files(tmp_path):
    import os
    import subprocess
    import sys
    from PIL import Image
    script = os.path.join(pr.ROOT, "examples", "present_frame.py")
    out = subprocess.run([sys.executable, script, "--size", "70", "45", "--spp", "2", "--out", str(tmp_path / "p")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "identical pixels" in out.stdout, out.stdout + out.stderr
    assert np.array_equal(np.asarray(Image.open(tmp_path / "p_device.png")), np.asarray(Image.open(tmp_path / "p_host.png")))
