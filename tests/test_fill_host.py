"""Host side of the fill: option denoise_fill's bounds and message on a context without a device (as
test_host_logic.test_every_option_keeps_its_bounds_and_messages holds the others), and what Renderer.select_lattice /
denoise_fill / lattice_phase hand across the C ABI, over a recording stand-in for the library."""
import ctypes as C
import itertools

import numpy as np
import pytest

from raytracingpbr_amd import Config, Renderer, cornell_box
from raytracingpbr_amd import dataclass as dc
from test_renderer_marshalling import H, W, Recorder, Scripted, packed

FILL_MESSAGE = ("denoise_fill must be 0 (pixels without samples stay as rtpbr_post_process shows them) or 1 (rtpbr_denoise "
                "reconstructs them from their neighbours)")


def test_the_option_keeps_its_bounds_and_message(tmp_path, monkeypatch):
    from raytracingpbr_amd import prebuild, workloads
    monkeypatch.setenv("HIPCC", "/nonexistent/hipcc")          # (a mistake in this test cannot start a compiler)
    monkeypatch.setenv("RTPBR_JIT_CACHE", str(tmp_path))
    lib = prebuild._lib()
    wl = workloads.get("c2", 0, 0)
    n = len(wl.scene.objects)
    arr = (dc.SDFObject * n)(*wl.scene.objects)
    buf = C.create_string_buffer(1024)

    def answer(options):
        rc = lib.rtpbr_jit_prebuild(arr, n, 1 if wl.scene.scale10 else 0, C.byref(wl.cfg), C.byref(wl.scene.camera), 0, 0, 1,
                                    options.encode(), buf, 1024)
        return rc, lib.rtpbr_last_error().decode()

    unknown = (-1, "unknown option nosuchkey")
    for value in (-1, 2):
        assert answer("denoise_fill=%d nosuchkey=0" % value) == (-1, FILL_MESSAGE)
    for value in (0, 1):
        assert answer("denoise_fill=%d nosuchkey=0" % value) == unknown
    assert not list(tmp_path.iterdir())                        # nothing was compiled


class Counting(Recorder):
    """... whose get_counter answers from ``counters`` (name -> value)"""

    def __init__(self, counters, **kw):
        super().__init__(**kw)
        self.counters = counters

    def call(self, name, *args):
        rc = super().call(name, *args)
        if name == "get_counter":
            args[-1]._obj.value = self.counters[args[1].decode()]
        return rc


def new_renderer(**kw):
    api = Counting({"fill_filled": 17, "fill_empty": 1, "fill_deepest": 2}, **kw)
    r = Renderer(cornell_box("v3"), Config.cornell_v3(W, H, 0, 3), api=api)
    del api.calls[:]
    return r, api


def test_denoise_fill_sets_the_option_for_the_call_and_reads_the_three_counters():
    r, api = new_renderer()
    given = {"iterations": 3, "demodulate": 1, "sigma_depth": 0.125}
    assert r.denoise_fill(**given) == (17, 1, 2)
    n0 = ("ref", bytes(8))
    assert api.calls == [("set_option", "ctx", b"denoise_fill", 1), ("denoise", "ctx", packed(dc.DenoiseParams, **given)),
                         ("set_option", "ctx", b"denoise_fill", 0), ("get_counter", "ctx", b"fill_filled", n0),
                         ("get_counter", "ctx", b"fill_empty", n0), ("get_counter", "ctx", b"fill_deepest", n0)]
    del api.calls[:]
    r.denoise_fill()                       # nothing given: denoise hands the library NULL, as it does by itself
    assert api.calls[:3] == [("set_option", "ctx", b"denoise_fill", 1), ("denoise", "ctx", None), ("set_option", "ctx", b"denoise_fill", 0)]
    del api.calls[:]
    r.denoise(iterations=2)                # denoise itself sets nothing
    assert api.calls == [("denoise", "ctx", packed(dc.DenoiseParams, iterations=2))]


def test_denoise_fill_puts_the_option_back_when_denoise_raises():
    r, api = new_renderer(fail=("denoise", 1))
    with pytest.raises(Scripted):
        r.denoise_fill(iterations=2)
    assert [c[0] for c in api.calls] == ["set_option", "denoise", "set_option"]
    assert api.calls[0][2:] == (b"denoise_fill", 1) and api.calls[2][2:] == (b"denoise_fill", 0)


def test_an_unknown_parameter_is_a_type_error_before_any_call():
    r, api = new_renderer()
    with pytest.raises(TypeError, match=r"denoise_fill: unknown denoise parameters \['power', 'variance_floor'\]"):
        r.denoise_fill(variance_floor=1.0, power=2)
    assert api.calls == []


def test_select_lattice_hands_select_mask_the_lattices_bytes():
    r, api = new_renderer(script={"select_mask": [6, 4, 24]})
    n0 = ("ref", bytes(4))
    for period, phase, count in (((2, 2), (0, 0), 6), ((3, 2), (2, 1), 4), ((1, 1), (0, 0), 24)):
        del api.calls[:]
        want = np.zeros((W, H), np.uint8)
        for x in range(W):
            for y in range(H):
                want[x, y] = x % period[0] == phase[0] and y % period[1] == phase[1]
        assert r.select_lattice(period, phase) == count and int(want.sum()) == count
        assert api.calls == [("select_mask", "ctx", want.tobytes(), W * H, n0)]
    del api.calls[:]
    r.select_lattice()                     # the defaults: (2, 2) at (0, 0)
    assert api.calls[0][2] == np.logical_and.outer(np.arange(W) % 2 == 0, np.arange(H) % 2 == 0).astype(np.uint8).tobytes()


def test_select_lattice_refuses_bad_periods_and_phases_before_any_call():
    r, api = new_renderer()
    for period, phase in (((0, 2), (0, 0)), ((2, 9), (0, 0)), ((2, 2), (2, 0)), ((2, 2), (0, -1)), ((4, 4), (0, 4)), ((2.0, 2), (0, 0)),
                          ((2, 2), (0.5, 0)), ((2,), (0, 0)), (2, (0, 0)), ((2, 2), 0), ((True, 2), (0, 0))):
        with pytest.raises(ValueError):
            r.select_lattice(period, phase)
    with pytest.raises(ValueError):
        Renderer.lattice_phase(0, (9, 1))
    assert api.calls == []


def test_lattice_phase_visits_every_phase_once_per_cycle():
    assert [Renderer.lattice_phase(k) for k in range(5)] == [(0, 0), (1, 1), (1, 0), (0, 1), (0, 0)]
    for px, py in itertools.product(range(1, 9), repeat=2):
        cells = set(itertools.product(range(px), range(py)))
        for start in (0, 7 * px * py):
            seen = [Renderer.lattice_phase(start + k, (px, py)) for k in range(px * py)]
            assert set(seen) == cells and len(seen) == len(cells), (px, py)
        assert Renderer.lattice_phase(px * py + 3, (px, py)) == Renderer.lattice_phase(3, (px, py))
        assert all(type(v) is int for v in Renderer.lattice_phase(1, (px, py)))
