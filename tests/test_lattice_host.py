"""Host side of the lattice selection built on the device: what Renderer.select_lattice(device=True) hands across the C ABI (one
set_option, nothing else), over the recording stand-in of tests/test_fill_host.py, and option select_lattice's values, messages and
refusals on a context without a device, as test_host_logic.test_every_option_keeps_its_bounds_and_messages holds the others."""
import ctypes as C

import numpy as np
import pytest

from raytracingpbr_amd import Renderer
from raytracingpbr_amd import dataclass as dc
from test_fill_host import new_renderer
from test_renderer_marshalling import H, W

# include/rtpbr.h: RTPBR_SELECT_LATTICE_REFUSAL, and what rtpbr_select_mask says in the same states
LATTICE_MESSAGE = ("select_lattice must be 0 (nothing) or px + 16 * py + 256 * phx + 4096 * phy with 1 <= px, py <= 8, 0 <= phx < px "
                   "and 0 <= phy < py")
STATE_MESSAGE = "set_config, set_scene and set_camera first"
EINVAL, ESTATE = -1, -4


def code(period, phase):
    return period[0] + 16 * period[1] + 256 * phase[0] + 4096 * phase[1]


def test_the_device_path_is_one_set_option_and_the_closed_form_count():
    r, api = new_renderer()
    assert (W, H) == (6, 4)
    for period, phase, count in (((2, 2), (0, 0), 6), ((3, 2), (2, 1), 4), ((1, 1), (0, 0), 24), ((8, 8), (7, 7), 0)):
        del api.calls[:]
        assert r.select_lattice(period, phase, device=True) == count
        assert api.calls == [("set_option", "ctx", b"select_lattice", code(period, phase))]
        want = sum(x % period[0] == phase[0] and y % period[1] == phase[1] for x in range(W) for y in range(H))
        assert count == want
    assert code((3, 2), (2, 1)) == 3 + 32 + 512 + 4096 and code((8, 8), (7, 7)) == 0x7788
    del api.calls[:]
    r.select_lattice(device=True)          # the defaults: (2, 2) at (0, 0)
    assert api.calls == [("set_option", "ctx", b"select_lattice", 0x22)]


def test_the_count_is_the_masks_on_every_small_frame():
    for w in range(1, 12):
        for h in range(1, 12):
            for period, phase in (((2, 2), (1, 0)), ((3, 2), (2, 1)), ((8, 8), (7, 4)), ((1, 5), (0, 4)), ((4, 4), (3, 1))):
                mask = np.logical_and.outer(np.arange(w) % period[0] == phase[0], np.arange(h) % period[1] == phase[1])
                assert Renderer.lattice_count(w, h, period, phase) == int(mask.sum())


def test_the_device_path_refuses_bad_periods_and_phases_before_any_call():
    r, api = new_renderer()
    for period, phase in (((0, 2), (0, 0)), ((2, 9), (0, 0)), ((2, 2), (2, 0)), ((2, 2), (0, -1)), ((4, 4), (0, 4)), ((2.0, 2), (0, 0)),
                          ((2, 2), (0.5, 0)), ((2,), (0, 0)), (2, (0, 0)), ((2, 2), 0), ((True, 2), (0, 0))):
        with pytest.raises(ValueError):
            r.select_lattice(period, phase, device=True)
    assert api.calls == []


def test_the_default_is_still_the_select_mask_call():
    r, api = new_renderer(script={"select_mask": [6, 6]})
    want = np.logical_and.outer(np.arange(W) % 2 == 0, np.arange(H) % 2 == 0).astype(np.uint8).tobytes()
    for kw in ({}, {"device": False}):
        del api.calls[:]
        assert r.select_lattice((2, 2), (0, 0), **kw) == 6
        assert api.calls == [("select_mask", "ctx", want, W * H, ("ref", bytes(4)))]


@pytest.fixture
def answer(tmp_path, monkeypatch):
    """rtpbr_jit_prebuild's answer to an option string: (code, message); it applies the string with rtpbr_set_option to a context
    without a device before anything is compiled, and nothing is"""
    from raytracingpbr_amd import prebuild, workloads
    monkeypatch.setenv("HIPCC", "/nonexistent/hipcc")          # (a mistake in this test cannot start a compiler)
    monkeypatch.setenv("RTPBR_JIT_CACHE", str(tmp_path))
    lib = prebuild._lib()
    wl = workloads.get("c2", 0, 0)
    n = len(wl.scene.objects)
    arr = (dc.SDFObject * n)(*wl.scene.objects)
    buf = C.create_string_buffer(1024)

    def answer(options, tiles=(0, 0, 1)):
        rc = lib.rtpbr_jit_prebuild(arr, n, 1 if wl.scene.scale10 else 0, C.byref(wl.cfg), C.byref(wl.scene.camera), *tiles,
                                    options.encode(), buf, 1024)
        return rc, lib.rtpbr_last_error().decode()

    yield answer
    assert not list(tmp_path.iterdir())                        # nothing was compiled


def test_value_0_is_accepted_and_does_nothing(answer):
    assert answer("select_lattice=0 nosuchkey=0") == (EINVAL, "unknown option nosuchkey")


def test_values_that_are_no_lattice_answer_the_options_own_message(answer):
    for name, value in (("px = 0", 0x10), ("py = 0", 0x01), ("px = 9", 0x19), ("py = 9", 0x91), ("phx = px", 0x222), ("phy = py", 0x2022),
                        ("phx beyond 8", 0x988), ("a stray high bit", 0x10022), ("bit 40", (1 << 40) + 0x22), ("negative", -1),
                        ("the most negative", -0x22)):
        assert answer("select_lattice=%d nosuchkey=0" % value) == (EINVAL, LATTICE_MESSAGE), name


def test_a_lattice_is_refused_in_select_masks_words_where_select_mask_is(answer):
    """a context without a device has no frame to select in; with tiles of world > 1 the state comes first, as in rtpbr_select_mask"""
    for value in (0x11, 0x22, 0x1123, 0x7788):
        assert answer("select_lattice=%d nosuchkey=0" % value) == (ESTATE, STATE_MESSAGE), hex(value)
    assert answer("select_lattice=34", tiles=(64, 64, 2)) == (ESTATE, STATE_MESSAGE)
