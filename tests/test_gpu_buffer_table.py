"""One lifecycle over all twenty public buffer ids (include/rtpbr.h RTPBR_BUF_*): what rtpbr_buffer_device_ptr reports, what
rtpbr_read_buffer and rtpbr_write_buffer accept, and what rtpbr_set_config keeps or frees, before and after every stage has made
its buffers.  The stages' own lifecycle assertions live with their tests (test_gpu_levels, test_gpu_half, test_gpu_noise,
test_gpu_present, ...); this one holds the ids to one another."""
import ctypes as C

import numpy as np
import pytest

from blend_error_states import cornell
from raytracingpbr_amd import Renderer

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -4
W, H = 16, 12                       # deliberately not square
RAY_BYTES = 40                      # sizeof(rtpbr_ray)
PRESENT_CHANNELS = 3                # the lifecycle presents "rgb8": the buffer has room for 4, the reported size is the last present's
# bytes per pixel of every id, from the comments of the enum in include/rtpbr.h: (W,H,4) f32, (W,H,3) f32, (W,H) of rtpbr_ray,
# (W,H,2) f32, (W,H) f32 | (W,H,3) f32 x 2, (W,H) f32, (W,H) i32, (W,H,3) f32 | (W,H,2) f32 | (W,H,4) f32, (W,H) f32 | (W,H) u8 |
# (H,W,C) u8 | (W,H,4) f32, (W,H) f32 x 4
PIXEL_BYTES = [16, 12, RAY_BYTES, 8, 4, 12, 12, 4, 4, 12, 8, 16, 4, 1, PRESENT_CHANNELS, 16, 4, 4, 4, 4]
CORE, OUTPUTS = range(0, 5), range(5, 20)


def _renderer(w, h):
    scene, cfg = cornell(w, h)
    r = Renderer(scene, cfg)
    r.set_option("jit", 0)          # nothing is compiled at run time
    return r


def _ptr(r, which):
    """(return code, device address, bytes) of rtpbr_buffer_device_ptr"""
    p, n = C.c_void_p(), C.c_size_t()
    rc = r.api.fn["buffer_device_ptr"](r._ctx, which, C.byref(p), C.byref(n))
    return rc, p.value, n.value


def _read(r, which, nbytes):
    out = np.empty(nbytes, np.uint8)
    return r.api.fn["read_buffer"](r._ctx, which, out.ctypes.data_as(C.c_void_p), nbytes), out


def _outputs_refuse_writes(r):
    src = np.zeros(W * H * 16, np.uint8)
    for which in OUTPUTS:
        for nbytes in (W * H * PIXEL_BYTES[which], 1):
            assert r.api.fn["write_buffer"](r._ctx, which, src.ctypes.data_as(C.c_void_p), nbytes) == EINVAL, which
            assert b"outputs only" in r.api.fn["last_error"](), which


def _every_stage(r):
    """one call of every stage that makes a public buffer"""
    r.render(refreshing=True, spp=4)
    r.render_features()
    r.denoise(iterations=2)
    r.reproject(r.camera)
    r.noise_update()
    r.noise_estimate(0.0)
    r.select_noisy(0.0)
    r.present("pixels", "rgb8")
    r.half_update()
    r.denoise_error()
    r.denoise_blend()
    r.blend_error(bias="display")
    r.sync()


def test_twenty_ids_through_one_lifecycle():
    r = _renderer(W, H)
    # 1. after construction: the five core buffers exist, the fifteen outputs do not, and no output is ever writable
    for which in CORE:
        rc, p, n = _ptr(r, which)
        assert rc == 0 and p and n == W * H * PIXEL_BYTES[which], which
    for which in OUTPUTS:
        assert _ptr(r, which)[0] == ESTATE, which
        assert b"buffer not allocated yet" in r.api.fn["last_error"](), which
    _outputs_refuse_writes(r)
    assert _ptr(r, 20)[0] == EINVAL and _ptr(r, -1)[0] == EINVAL

    # 2. after every stage: each id reports the size of its shape and reads back with exactly that size
    _every_stage(r)
    ptrs = []
    for which in range(20):
        rc, p, n = _ptr(r, which)
        assert rc == 0 and p and n == W * H * PIXEL_BYTES[which], which
        assert _read(r, which, n)[0] == 0, which
        assert _read(r, which, n + 1)[0] == EINVAL, which
        ptrs.append(p)
    assert len(set(ptrs)) == 20
    _outputs_refuse_writes(r)

    # 3. the same resolution again: every buffer stays where it is
    r.set_config(r.config)
    assert [_ptr(r, which)[1] for which in range(20)] == ptrs

    # 4. another resolution: the outputs are gone, the core buffers are new, of the new size, and zero
    W2 = 20
    r.set_config(r.config.copy(width=W2))
    for which in OUTPUTS:
        assert _ptr(r, which)[0] == ESTATE, which
    for which in CORE:
        rc, p, n = _ptr(r, which)
        assert rc == 0 and p and n == W2 * H * PIXEL_BYTES[which], which
        rc, got = _read(r, which, n)
        assert rc == 0 and not got.any(), which

    # 5. destroy; a second context goes through the same calls and is destroyed with everything allocated
    r.close()
    r2 = _renderer(W, H)
    _every_stage(r2)
    assert all(_ptr(r2, which)[0] == 0 for which in range(20))
    r2.close()
