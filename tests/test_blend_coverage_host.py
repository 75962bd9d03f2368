"""Host side of the coverage-aware level blend: the four blend_coverage options' bounds and messages on a context without a device
(as test_fill_host holds denoise_fill's), what Renderer.denoise_blend_levels_coverage / blend_error_coverage /
render_adaptive_denoised(coverage=...) hand across the C ABI and in which order, over a recording stand-in for the library, and
that include/rtpbr.h documents the options and the counter."""
import ctypes as C
import os
import re

import pytest

from raytracingpbr_amd import Config, Renderer, cornell_box
from raytracingpbr_amd import dataclass as dc
from test_fill_host import Counting
from test_renderer_marshalling import H, STATS0, W, Scripted, packed

MESSAGES = {
    "blend_coverage": ("blend_coverage must be 0 (the plain filter's ladders) or 1 (rtpbr_denoise_blend_levels, rtpbr_blend_error and "
                       "rtpbr_blend_error_display run the coverage-weighted ladders and the edge resolve)"),
    "blend_coverage_grid": "blend_coverage_grid must be 2 or 4",
    "blend_coverage_power": "blend_coverage_power must be 0..8",
    "blend_coverage_resolve": "blend_coverage_resolve must be 0 or 1",
}
# option -> (values accepted, values refused): the lowest and the highest value, and their neighbours
BOUNDS = {"blend_coverage": ((0, 1), (-1, 2)), "blend_coverage_grid": ((2, 4), (1, 3, 5)), "blend_coverage_power": ((0, 8), (-1, 9)),
          "blend_coverage_resolve": ((0, 1), (-1, 2))}


def test_every_option_keeps_its_bounds_and_its_own_message(tmp_path, monkeypatch):
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
    assert len(set(MESSAGES.values())) == 4
    for key, (good, bad) in BOUNDS.items():
        for value in bad:
            assert answer(f"{key}={value} nosuchkey=0") == (-1, MESSAGES[key]), (key, value)
        for value in good:
            assert answer(f"{key}={value} nosuchkey=0") == unknown, (key, value)
    # four keys: each is checked by its own row, whatever the others hold
    assert answer("blend_coverage=1 blend_coverage_grid=2 blend_coverage_power=9") == (-1, MESSAGES["blend_coverage_power"])
    assert answer("blend_coverage_power=8 blend_coverage_resolve=2 blend_coverage=2") == (-1, MESSAGES["blend_coverage_resolve"])
    assert answer("blend_coverage=1 coverage_fill=1 denoise_fill=1 blend_coverage_grid=3") == (-1, MESSAGES["blend_coverage_grid"])
    assert not list(tmp_path.iterdir())                        # nothing was compiled


def new_renderer(**kw):
    api = Counting({"blend_resolved": 23}, **kw)
    r = Renderer(cornell_box("v3"), Config.cornell_v3(W, H, 0, 3), api=api)
    del api.calls[:]
    return r, api


def _options(grid=4, power=4, resolve=1):
    return [("set_option", "ctx", b"blend_coverage", 1), ("set_option", "ctx", b"blend_coverage_grid", grid),
            ("set_option", "ctx", b"blend_coverage_power", power), ("set_option", "ctx", b"blend_coverage_resolve", resolve)]


OFF = ("set_option", "ctx", b"blend_coverage", 0)
COUNTER = ("get_counter", "ctx", b"blend_resolved", ("ref", bytes(8)))


def test_the_two_methods_set_the_four_options_for_the_call_and_read_the_counter():
    r, api = new_renderer(script={"denoise_blend_levels": [(5, 9, 0.25)], "blend_error_display": [(7, 1, 0.5)]})
    d = {"iterations": 3, "demodulate": 1, "sigma_depth": 0.125}
    e = {"radius": 2, "z": 0.0, "min_half_samples": 8}
    stats, resolved = r.denoise_blend_levels_coverage(power=8, resolve=0, grid=2, **e, **d)
    assert isinstance(stats, dc.NoiseStats) and (stats.pixels_estimated, stats.pixels_above, stats.max_noise) == (5, 9, 0.25)
    assert resolved == 23
    assert api.calls == _options(2, 8, 0) + [("denoise_blend_levels", "ctx", packed(dc.DenoiseParams, **d), packed(dc.BlendParams, **e), STATS0),
                                             OFF, COUNTER]
    del api.calls[:]
    r.denoise_blend_levels_coverage()      # nothing given: the library's defaults, and the call itself is handed NULL twice
    assert api.calls == _options() + [("denoise_blend_levels", "ctx", None, None, STATS0), OFF, COUNTER]
    del api.calls[:]
    stats, resolved = r.blend_error_coverage(0.5, 1, 1, 4, window=3, bias="display", **e, **d)      # power, resolve, grid by position
    assert (stats.pixels_estimated, stats.pixels_above, stats.max_noise) == (7, 1, 0.5) and resolved == 23
    assert api.calls == _options(4, 1, 1) + [("blend_error_display", "ctx", packed(dc.DenoiseParams, **d), packed(dc.BlendParams, **e),
                                              packed(dc.ErrorParams, radius=3), 0.5, STATS0), OFF, COUNTER]
    del api.calls[:]
    r.blend_error_coverage()
    assert api.calls == _options() + [("blend_error", "ctx", None, None, None, 0.0, STATS0), OFF, COUNTER]
    del api.calls[:]
    r.denoise_blend_levels(iterations=2)   # the plain methods set nothing
    r.blend_error(0.25)
    assert [c[0] for c in api.calls] == ["denoise_blend_levels", "blend_error"]


@pytest.mark.parametrize("method,entry", [("denoise_blend_levels_coverage", "denoise_blend_levels"), ("blend_error_coverage", "blend_error")])
def test_the_option_is_put_back_when_the_call_raises(method, entry):
    r, api = new_renderer(fail=(entry, 1))
    with pytest.raises(Scripted):
        getattr(r, method)(iterations=2)
    assert api.calls[:4] == _options() and [c[0] for c in api.calls[4:]] == [entry, "set_option"]      # (and no counter is read)
    assert api.calls[-1] == OFF
    # ... and when one of the parameters is refused: the call is never made
    r, api = new_renderer(fail=("set_option", 3))
    with pytest.raises(Scripted):
        getattr(r, method)(power=9)
    assert api.calls == _options(4, 9)[:3] + [OFF]


def test_bad_parameters_raise_before_any_call():
    r, api = new_renderer()
    with pytest.raises(TypeError, match=r"denoise_blend_levels_coverage: unknown denoise parameters \['variance_floor', 'window'\]"):
        r.denoise_blend_levels_coverage(variance_floor=1.0, window=2)
    with pytest.raises(TypeError, match=r"blend_error_coverage: unknown denoise parameters \['sigma'\]"):
        r.blend_error_coverage(sigma=2.0)
    with pytest.raises(ValueError):
        r.blend_error_coverage(bias="srgb")
    assert api.calls == []


def test_render_adaptive_denoised_takes_coverage_with_the_level_blend_only():
    r, api = new_renderer()
    args = (0.02, 8, 4, 1)
    for bad in (dict(coverage=True), dict(coverage=True, blend=True), dict(coverage={}, blend=False), dict(coverage=False, blend="levels"),
                dict(coverage=1, blend="levels"), dict(coverage={"radius": 2}, blend="levels"), dict(coverage="on", blend="levels"),
                dict(coverage=True, stop="blend")):
        with pytest.raises(ValueError):
            r.render_adaptive_denoised(*args, **bad)
    assert api.calls == []
    # stop="filter": denoise_error estimates, the new call ends the loop
    r.render_adaptive_denoised(*args, blend="levels", coverage=True, iterations=2)
    names = [c[0] for c in api.calls]
    assert "blend_error" not in names and names.count("denoise_blend_levels") == 1
    at = names.index("denoise_blend_levels")
    assert api.calls[at - 4:at] == _options() and api.calls[at + 1:at + 3] == [OFF, COUNTER]
    assert api.calls[at][2] == packed(dc.DenoiseParams, iterations=2)
    # stop="blend": every estimate is the new call, with the dict's parameters, and nothing follows the last one
    del api.calls[:]
    r.render_adaptive_denoised(*args, blend="levels", stop="blend", bias="display", coverage={"power": 8, "grid": 2})
    names = [c[0] for c in api.calls]
    assert "denoise_blend_levels" not in names and "blend_error" not in names and names.count("blend_error_display") >= 1
    for at in (i for i, n in enumerate(names) if n == "blend_error_display"):
        assert api.calls[at - 4:at] == _options(2, 8, 1) and api.calls[at + 1:at + 3] == [OFF, COUNTER]
    last = len(names) - 1 - names[::-1].index("blend_error_display")
    assert not [n for n in names[last + 1:] if n.startswith(("denoise", "blend"))]
    # coverage=None: the loop's calls are those of the parent
    del api.calls[:]
    r.render_adaptive_denoised(*args, blend="levels", stop="blend")
    assert not [c for c in api.calls if c[0] == "set_option" and c[2].startswith(b"blend_coverage")]
    assert "get_counter" not in [c[0] for c in api.calls]


def test_the_header_documents_the_options_and_the_counter():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "rtpbr.h")) as f:
        header = f.read()
    for key in list(MESSAGES) + ["blend_resolved"]:
        assert re.search(r"\b%s\b" % key, header), key
    with open(os.path.join(root, "raytracingpbr_amd", "csrc", "rt_capi.hip")) as f:
        capi = f.read()
    assert '!strcmp(name, "blend_resolved")' in capi           # the counter's name resolves (read on a device: tests/test_gpu_blend_coverage.py)
    for key, text in MESSAGES.items():
        assert text in capi.replace('"\n', "") or text in capi, key
