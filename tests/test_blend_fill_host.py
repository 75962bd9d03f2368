"""Host side of the filling level blend: option blend_fill's bounds and message on a context without a device (as test_fill_host
holds denoise_fill's), what the ``fill`` keyword of Renderer.denoise_blend_levels / blend_error / denoise_blend_levels_coverage /
blend_error_coverage / render_adaptive_denoised hands across the C ABI and in which order, over a recording stand-in for the
library — with ``fill=False`` exactly the calls the methods made before they had the keyword —, and that include/rtpbr.h documents
the option."""
import ctypes as C
import os
import re

import pytest

from raytracingpbr_amd import Config, Renderer, cornell_box
from raytracingpbr_amd import dataclass as dc
from test_fill_host import Counting
from test_renderer_marshalling import H, STATS0, W, Scripted, packed

MESSAGE = ("blend_fill must be 0 (pixels without samples stay as rtpbr_post_process shows them) or 1 (rtpbr_denoise_blend_levels, "
           "rtpbr_blend_error and rtpbr_blend_error_display reconstruct them from their neighbours)")
COUNTS = {"fill_filled": 17, "fill_empty": 1, "fill_deepest": 2, "blend_resolved": 23}
ON, OFF = ("set_option", "ctx", b"blend_fill", 1), ("set_option", "ctx", b"blend_fill", 0)
N0 = ("ref", bytes(8))
COUNTERS = [("get_counter", "ctx", b"fill_" + k, N0) for k in (b"filled", b"empty", b"deepest")]
COVER = [("set_option", "ctx", b"blend_coverage", 1), ("set_option", "ctx", b"blend_coverage_grid", 4),
         ("set_option", "ctx", b"blend_coverage_power", 4), ("set_option", "ctx", b"blend_coverage_resolve", 1)]
COVER_OFF = [("set_option", "ctx", b"blend_coverage", 0), ("get_counter", "ctx", b"blend_resolved", N0)]


def test_the_option_accepts_0_and_1_and_refuses_their_neighbours_in_its_own_words(tmp_path, monkeypatch):
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
        assert answer(f"blend_fill={value} nosuchkey=0") == (-1, MESSAGE), value
    for value in (0, 1):
        assert answer(f"blend_fill={value} nosuchkey=0") == unknown, value
    # its own row: the other fill options and blend_coverage beside it do not answer for it, nor it for them
    assert answer("denoise_fill=1 coverage_fill=1 blend_coverage=1 blend_fill=2") == (-1, MESSAGE)
    rc, text = answer("blend_fill=1 denoise_fill=2")
    assert rc == -1 and text.startswith("denoise_fill must be") and text != MESSAGE
    assert not list(tmp_path.iterdir())                        # nothing was compiled


def new_renderer(**kw):
    api = Counting(dict(COUNTS), **kw)
    r = Renderer(cornell_box("v3"), Config.cornell_v3(W, H, 0, 3), api=api)
    del api.calls[:]
    return r, api


D = {"iterations": 3, "demodulate": 1, "sigma_depth": 0.125}
E = {"radius": 2, "z": 0.0, "min_half_samples": 8}


def test_fill_false_makes_the_calls_the_methods_always_made_and_returns_what_they_returned():
    r, api = new_renderer(script={"denoise_blend_levels": [(5, 9, 0.25)] * 4, "blend_error": [(7, 1, 0.5)] * 2})      # (a call each per round; the coverage method makes one more)
    for kw in ({}, {"fill": False}):
        del api.calls[:]
        stats = r.denoise_blend_levels(**E, **D, **kw)
        assert isinstance(stats, dc.NoiseStats) and (stats.pixels_estimated, stats.pixels_above, stats.max_noise) == (5, 9, 0.25)
        assert api.calls == [("denoise_blend_levels", "ctx", packed(dc.DenoiseParams, **D), packed(dc.BlendParams, **E), STATS0)]
        del api.calls[:]
        stats = r.blend_error(0.5, window=3, **E, **D, **kw)
        assert isinstance(stats, dc.NoiseStats) and (stats.pixels_estimated, stats.pixels_above, stats.max_noise) == (7, 1, 0.5)
        assert api.calls == [("blend_error", "ctx", packed(dc.DenoiseParams, **D), packed(dc.BlendParams, **E),
                              packed(dc.ErrorParams, radius=3), 0.5, STATS0)]
        del api.calls[:]
        stats, resolved = r.denoise_blend_levels_coverage(**kw)
        assert isinstance(stats, dc.NoiseStats) and resolved == 23
        assert api.calls == COVER + [("denoise_blend_levels", "ctx", None, None, STATS0)] + COVER_OFF
        del api.calls[:]
        stats, resolved = r.blend_error_coverage(bias="display", **kw)
        assert isinstance(stats, dc.NoiseStats) and resolved == 23
        assert api.calls == COVER + [("blend_error_display", "ctx", None, None, None, 0.0, STATS0)] + COVER_OFF
    # the loop: the same calls with and without the keyword, and neither touches the option or the fill counters
    args = (0.02, 8, 4, 1)
    seen = []
    for kw in ({}, {"fill": False}):
        del api.calls[:]
        out = r.render_adaptive_denoised(*args, blend="levels", stop="blend", iterations=2, **kw)
        assert isinstance(out, tuple) and len(out) == 2 and isinstance(out[0], int) and isinstance(out[1], dc.NoiseStats)
        seen.append(list(api.calls))
        assert not [c for c in api.calls if c[0] == "set_option" and c[2] == b"blend_fill"]
        assert not [c for c in api.calls if c[0] == "get_counter" and c[2].startswith(b"fill_")]
    assert seen[0] == seen[1]


def test_fill_true_brackets_the_call_with_the_option_and_adds_the_three_counters():
    r, api = new_renderer(script={"denoise_blend_levels": [(5, 9, 0.25)], "blend_error_display": [(7, 1, 0.5)]})
    stats, counts = r.denoise_blend_levels(fill=True, **E, **D)
    assert isinstance(stats, dc.NoiseStats) and (stats.pixels_estimated, stats.pixels_above, stats.max_noise) == (5, 9, 0.25)
    assert counts == (17, 1, 2)
    assert api.calls == [ON, ("denoise_blend_levels", "ctx", packed(dc.DenoiseParams, **D), packed(dc.BlendParams, **E), STATS0), OFF] + COUNTERS
    del api.calls[:]
    stats, counts = r.blend_error(0.5, window=3, bias="display", fill=True, **E, **D)
    assert (stats.pixels_estimated, stats.pixels_above, stats.max_noise) == (7, 1, 0.5) and counts == (17, 1, 2)
    assert api.calls == [ON, ("blend_error_display", "ctx", packed(dc.DenoiseParams, **D), packed(dc.BlendParams, **E),
                              packed(dc.ErrorParams, radius=3), 0.5, STATS0), OFF] + COUNTERS
    del api.calls[:]
    (stats, resolved), counts = r.denoise_blend_levels_coverage(fill=True)
    assert isinstance(stats, dc.NoiseStats) and resolved == 23 and counts == (17, 1, 2)
    assert api.calls == [ON] + COVER + [("denoise_blend_levels", "ctx", None, None, STATS0)] + COVER_OFF + [OFF] + COUNTERS
    del api.calls[:]
    (stats, resolved), counts = r.blend_error_coverage(0.25, fill=True)
    assert isinstance(stats, dc.NoiseStats) and resolved == 23 and counts == (17, 1, 2)
    assert api.calls == [ON] + COVER + [("blend_error", "ctx", None, None, None, 0.25, STATS0)] + COVER_OFF + [OFF] + COUNTERS


@pytest.mark.parametrize("method,entry", [("denoise_blend_levels", "denoise_blend_levels"), ("blend_error", "blend_error"),
                                          ("denoise_blend_levels_coverage", "denoise_blend_levels"),
                                          ("blend_error_coverage", "blend_error")])
def test_the_option_is_put_back_when_the_library_refuses(method, entry):
    r, api = new_renderer(fail=(entry, 1))
    with pytest.raises(Scripted):
        getattr(r, method)(iterations=2, fill=True)
    assert api.calls[0] == ON and api.calls[-1] == OFF and entry in [c[0] for c in api.calls]
    assert not [c for c in api.calls if c[0] == "get_counter" and c[2].startswith(b"fill_")]      # no counter is read
    # ... and when the option itself is refused (it then still holds 0), the call is never made
    r, api = new_renderer(fail=("set_option", 1))
    with pytest.raises(Scripted):
        getattr(r, method)(fill=True)
    assert api.calls == [ON]


def test_render_adaptive_denoised_takes_fill_with_the_level_blend_only():
    r, api = new_renderer()
    args = (0.02, 8, 4, 1)
    for bad in (dict(fill=True), dict(fill=True, blend=True), dict(fill=True, blend=False)):
        with pytest.raises(ValueError):
            r.render_adaptive_denoised(*args, **bad)
    assert api.calls == []
    for extra in (dict(), dict(stop="blend", bias="display"), dict(coverage=True)):
        del api.calls[:]
        out = r.render_adaptive_denoised(*args, blend="levels", fill=True, iterations=2, **extra)
        (traced, stats), counts = out
        assert isinstance(traced, int) and isinstance(stats, dc.NoiseStats) and counts == (17, 1, 2)
        assert api.calls[0] == ON and api.calls[-4:] == [OFF] + COUNTERS
        inner = api.calls[1:-4]
        assert not [c for c in inner if c[0] == "set_option" and c[2] == b"blend_fill"]
        assert [c for c in inner if c[0] in ("denoise_blend_levels", "blend_error", "blend_error_display")]
        # between the two the loop makes exactly the calls it makes without the keyword
        del api.calls[:]
        r.render_adaptive_denoised(*args, blend="levels", iterations=2, **extra)
        assert api.calls == inner
    # a refusal inside the loop puts the option back
    r, api = new_renderer(fail=("denoise_blend_levels", 1))
    with pytest.raises(Scripted):
        r.render_adaptive_denoised(*args, blend="levels", fill=True)
    assert api.calls[0] == ON and api.calls[-1] == OFF


def test_the_header_documents_the_option():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "rtpbr.h")) as f:
        header = f.read()
    assert re.search(r"\bblend_fill\b", header)
    with open(os.path.join(root, "raytracingpbr_amd", "csrc", "rt_capi.hip")) as f:
        capi = f.read()
    assert MESSAGE in capi
