"""Host side of the coverage fill: option coverage_fill's bounds and message on a context without a device (as
test_fill_host holds denoise_fill's), and what Renderer.denoise_coverage_fill hands across the C ABI and in which order, over a
recording stand-in for the library."""
import ctypes as C

import pytest

from raytracingpbr_amd import dataclass as dc
from raytracingpbr_amd.renderer import NoiseStats
from test_fill_host import FILL_MESSAGE, new_renderer
from test_renderer_marshalling import STATS0, Scripted, packed

COVERAGE_FILL_MESSAGE = ("coverage_fill must be 0 (pixels without samples stay as rtpbr_post_process shows them) or 1 "
                         "(rtpbr_denoise_coverage reconstructs them from their neighbours)")


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
        assert answer("coverage_fill=%d nosuchkey=0" % value) == (-1, COVERAGE_FILL_MESSAGE)
    for value in (0, 1):
        assert answer("coverage_fill=%d nosuchkey=0" % value) == unknown
    # the two fill options are two keys: either is checked by its own row
    assert answer("coverage_fill=1 denoise_fill=2") == (-1, FILL_MESSAGE)
    assert answer("denoise_fill=1 coverage_fill=2") == (-1, COVERAGE_FILL_MESSAGE)
    assert not list(tmp_path.iterdir())                        # nothing was compiled


def test_denoise_coverage_fill_sets_the_option_for_the_call_and_reads_the_three_counters():
    r, api = new_renderer(script={"denoise_coverage": [(5, 9, 0.25)]})
    d = {"iterations": 3, "demodulate": 1, "sigma_depth": 0.125}
    c = {"grid": 2, "power": 8, "resolve": 0}
    stats, counts = r.denoise_coverage_fill(**c, **d)
    assert isinstance(stats, NoiseStats) and (stats.pixels_estimated, stats.pixels_above, stats.max_noise) == (5, 9, 0.25)
    assert counts == (17, 1, 2)
    n0 = ("ref", bytes(8))
    assert api.calls == [("set_option", "ctx", b"coverage_fill", 1),
                         ("denoise_coverage", "ctx", packed(dc.DenoiseParams, **d), packed(dc.CoverageParams, **c), STATS0),
                         ("set_option", "ctx", b"coverage_fill", 0), ("get_counter", "ctx", b"fill_filled", n0),
                         ("get_counter", "ctx", b"fill_empty", n0), ("get_counter", "ctx", b"fill_deepest", n0)]
    del api.calls[:]
    r.denoise_coverage_fill(4, 1)          # power and resolve by position, as denoise_coverage takes them
    assert api.calls[:3] == [("set_option", "ctx", b"coverage_fill", 1),
                             ("denoise_coverage", "ctx", packed(dc.DenoiseParams), packed(dc.CoverageParams, power=4, resolve=1), STATS0),
                             ("set_option", "ctx", b"coverage_fill", 0)]
    del api.calls[:]
    r.denoise_coverage(iterations=2)       # denoise_coverage itself sets nothing
    assert api.calls == [("denoise_coverage", "ctx", packed(dc.DenoiseParams, iterations=2), packed(dc.CoverageParams), STATS0)]
    del api.calls[:]
    r.denoise_fill()                       # ... and the plain fill sets its own key, not this one
    assert [c[2] for c in api.calls if c[0] == "set_option"] == [b"denoise_fill", b"denoise_fill"]


def test_denoise_coverage_fill_puts_the_option_back_when_the_call_raises():
    r, api = new_renderer(fail=("denoise_coverage", 1))
    with pytest.raises(Scripted):
        r.denoise_coverage_fill(iterations=2)
    assert [c[0] for c in api.calls] == ["set_option", "denoise_coverage", "set_option"]      # (and no counter is read)
    assert api.calls[0][2:] == (b"coverage_fill", 1) and api.calls[2][2:] == (b"coverage_fill", 0)


def test_an_unknown_parameter_is_a_type_error_before_any_call():
    r, api = new_renderer()
    with pytest.raises(TypeError, match=r"denoise_coverage_fill: unknown denoise parameters \['sigma', 'variance_floor'\]"):
        r.denoise_coverage_fill(variance_floor=1.0, sigma=2.0)
    with pytest.raises(TypeError):
        r.denoise_coverage_fill(power=1, nope=2)
    assert api.calls == []
