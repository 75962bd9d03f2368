"""What Renderer hands across the C ABI, checked without a library: a recording stand-in for CApi takes every call, and the
expected bytes are struct.pack of the fields (DEFAULTS plus the overrides), written here independently of the packer."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from raytracingpbr_amd import Config, Renderer, _capi, cornell_box, renderer
from raytracingpbr_amd import dataclass as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTX = 0xC0DE
W, H = 6, 4
# the calls whose last argument is a uint32 count / a rtpbr_noise_stats the library fills
COUNTS = ("select_mask", "select_noisy", "select_error", "select_blend_error")
STATS = ("noise_estimate", "denoise_error", "denoise_blend", "denoise_blend_levels", "blend_error", "blend_error_display", "denoise_coverage")
# the calls that hand over host memory to read: name -> (index of the pointer, bytes behind it from the arguments)
INPUTS = {"select_mask": (1, lambda a: a[2]), "write_buffer": (2, lambda a: a[3]), "set_shape_data": (2, lambda a: 4 * a[3]),
          "set_env": (1, lambda a: a[2] * a[3] * 3 * (1 if a[4] == 0 else 4))}


class Scripted(RuntimeError):
    """what a scripted failure raises"""


def decode(a):
    """an argument as the library would see it: byref(x) -> the bytes of x, an array -> its bytes, a scalar -> its value"""
    if a is None or isinstance(a, (bool, int, float, bytes)):
        return a
    if hasattr(a, "_obj"):
        return ("ref", bytes(a._obj))
    if isinstance(a, C.Array):
        return bytes(a)
    if isinstance(a, C.c_void_p):
        return "ctx" if a.value == CTX else "null" if not a.value else "ptr"
    return a.value


class Recorder:
    """CApi's call / has / fn, recording.  ``script``: name -> the values its calls return through their out-parameters, one per
    call (then the default: count 0, statistics (W * H, 0, 0.0)); ``fail``: (name, k) raises Scripted from the k-th call of
    name, after recording it; ``missing``: the names has() denies."""

    def __init__(self, script=None, fail=None, missing=()):
        self.calls, self.fn = [], {}
        self.script = {k: list(v) for k, v in (script or {}).items()}
        self.fail, self.missing, self.seen, self.blocks = fail, set(missing), {}, []

    def has(self, name):
        return name not in self.missing

    def next(self, name, default):
        s = self.script.get(name)
        return s.pop(0) if s else default

    def call(self, name, *args):
        rec = [decode(a) for a in args]
        if name in INPUTS:
            i, size = INPUTS[name]
            rec[i] = C.string_at(args[i], size(args))
        self.calls.append((name,) + tuple(rec))
        self.seen[name] = self.seen.get(name, 0) + 1
        if self.fail == (name, self.seen[name]):
            raise Scripted(name)
        out = args[-1]._obj if args and hasattr(args[-1], "_obj") else None
        if name == "create":
            out.value = CTX
        elif name in COUNTS:
            out.value = self.next(name, 0)
        elif name in STATS:
            out.pixels_estimated, out.pixels_above, out.max_noise = self.next(name, (W * H, 0, 0.0))
        elif name == "buffer_device_ptr":
            args[2]._obj.value, out.value = 0x1000, self.next(name, W * H * 4)
        elif name == "host_alloc":
            self.blocks.append(C.create_string_buffer(args[1]))
            out.value = C.addressof(self.blocks[-1])
        elif name == "read_buffer_async":
            out.value = self.seen[name]
        return 0


def new_renderer(**kw):
    """(renderer over a Recorder, the Recorder with the set-up calls dropped)"""
    api = Recorder(**kw)
    r = Renderer(cornell_box("v3"), Config.cornell_v3(W, H, 0, 3), api=api)
    del api.calls[:]
    return r, api


# ------------------------------------------------------------------ the parameter structs: the header's field types, restated
FORMATS = {dc.DenoiseParams: "iiffff", dc.DenoiseGuidedParams: "iiffff", dc.BlendParams: "ifi", dc.ErrorParams: "i",
           dc.ReprojectParams: "fff", dc.CoverageParams: "iii", dc.NoiseEstimator: "iii", dc.HalfMode: "ii", dc.PresentParams: "iii"}
DENOISE = {"iterations": 2, "demodulate": 1, "sigma_color": 0.5, "sigma_normal": 0.25, "sigma_depth": 0.125, "sigma_albedo": 0.75}
GUIDED = {"iterations": 3, "demodulate": 1, "sigma_color": 8.0, "sigma_normal": 0.25, "sigma_depth": 0.125, "variance_floor": 0.5}
BLEND = {"radius": 1, "z": 1.5, "min_half_samples": 4}
REPROJECT = {"max_history": 8.0, "depth_tolerance": 0.5, "normal_cos": 0.25}
COVERAGE = {"grid": 2, "power": 2, "resolve": 0}


def packed(cls, **over):
    """("ref", the bytes of the struct): DEFAULTS plus ``over``, every field converted as the header's type says"""
    assert not set(over) - set(cls.DEFAULTS)
    v = [(int if f == "i" else float)(over.get(k, d)) for f, (k, d) in zip(FORMATS[cls], cls.DEFAULTS.items())]
    return ("ref", struct.pack("=" + FORMATS[cls], *v))


def subsets(params):
    """nothing, each parameter alone, all of them"""
    return [{}] + [{k: v} for k, v in params.items()] + [dict(params)]


def null_or(cls, given):
    return packed(cls, **given) if given else None


STATS0 = ("ref", bytes(12))


def test_defaults_are_in_field_order_and_the_formats_have_the_structs_sizes():
    for cls, fmt in FORMATS.items():
        assert [n for n, _ in cls._fields_] == list(cls.DEFAULTS) and struct.calcsize("=" + fmt) == C.sizeof(cls)
        assert [f for f in fmt] == ["f" if t is C.c_float else "i" for _, t in cls._fields_]


@pytest.mark.parametrize("method,cls,params", [("denoise", dc.DenoiseParams, DENOISE), ("denoise_guided", dc.DenoiseGuidedParams, GUIDED)])
def test_denoise_and_denoise_guided_pass_null_when_nothing_is_given(method, cls, params):
    r, api = new_renderer()
    for given in subsets(params):
        del api.calls[:]
        getattr(r, method)(**given)
        assert api.calls == [(method, "ctx", null_or(cls, given))]


def test_reproject_and_reproject_scene_pass_null_when_nothing_is_given():
    r, api = new_renderer()
    sc, cam = r.scene, r.scene.camera
    objs = bytes((dc.SDFObject * len(sc.objects))(*sc.objects))
    for given in subsets(REPROJECT):
        del api.calls[:]
        r.reproject(cam, **given)
        r.reproject_scene(sc, **given)
        r.reproject_scene(sc, cam, **given)
        p = null_or(dc.ReprojectParams, given)
        assert api.calls == [("reproject", "ctx", ("ref", bytes(cam)), p),
                             ("reproject_scene", "ctx", None, objs, len(sc.objects), 1 if sc.scale10 else 0, p),
                             ("reproject_scene", "ctx", ("ref", bytes(cam)), objs, len(sc.objects), 1 if sc.scale10 else 0, p)]


def test_the_half_calls_pass_null_for_each_struct_independently():
    r, api = new_renderer()
    for d in subsets(DENOISE):
        for b in subsets(BLEND):
            for w in (None, 3):
                del api.calls[:]
                r.denoise_error(0.25, radius=w, **d)
                r.denoise_blend(**b, **d)
                r.denoise_blend_levels(**b, **d)
                r.blend_error(0.5, window=w, **b, **d)
                r.blend_error(0.5, window=w, bias="display", **b, **d)
                p, e = null_or(dc.DenoiseParams, d), null_or(dc.BlendParams, b)
                ew = None if w is None else packed(dc.ErrorParams, radius=w)
                assert api.calls == [("denoise_error", "ctx", p, ew, 0.25, STATS0), ("denoise_blend", "ctx", p, e, STATS0),
                                     ("denoise_blend_levels", "ctx", p, e, STATS0), ("blend_error", "ctx", p, e, ew, 0.5, STATS0),
                                     ("blend_error_display", "ctx", p, e, ew, 0.5, STATS0)]


def test_the_coverage_calls_always_pass_filled_structs():
    r, api = new_renderer()
    r.render_coverage()
    r.render_coverage(grid=2)
    assert api.calls == [("render_coverage", "ctx", packed(dc.CoverageParams)), ("render_coverage", "ctx", packed(dc.CoverageParams, grid=2))]
    for d in subsets(DENOISE):
        for c in subsets(COVERAGE):
            del api.calls[:]
            r.denoise_coverage(**c, **d)
            assert api.calls == [("denoise_coverage", "ctx", packed(dc.DenoiseParams, **d), packed(dc.CoverageParams, **c), STATS0)]
    del api.calls[:]
    r.denoise_coverage(iterations=None, sigma_color=None)      # None = the default, as everywhere
    assert api.calls == [("denoise_coverage", "ctx", packed(dc.DenoiseParams), packed(dc.CoverageParams), STATS0)]


def test_present_the_estimator_and_the_half_mode_always_pass_structs():
    r, api = new_renderer()
    r.present()
    r.present("denoised", "rgb8", True)
    r.present("accum", dither=0)
    r.set_noise_estimator()
    r.set_noise_estimator(8, 2, 16)
    r.set_noise_estimator(min_samples=4.9)
    r.set_half_mode()
    r.set_half_mode(True)
    r.set_half_mode(warp=2)      # truth values: any true value is 1
    P, E, M = dc.PresentParams, dc.NoiseEstimator, dc.HalfMode
    assert api.calls == [("present", "ctx", packed(P)), ("present", "ctx", packed(P, source=1, format=0, dither=1)),
                         ("present", "ctx", packed(P, source=2)),
                         ("set_noise_estimator", "ctx", packed(E)), ("set_noise_estimator", "ctx", packed(E, pool_batches=8, pool_radius=2, min_samples=16)),
                         ("set_noise_estimator", "ctx", packed(E, min_samples=4)),
                         ("set_half_mode", "ctx", packed(M)), ("set_half_mode", "ctx", packed(M, per_sample=1)), ("set_half_mode", "ctx", packed(M, warp=1))]
    assert bytes(r.noise_estimator) == packed(E, min_samples=4)[1] and bytes(r.half_mode) == packed(M, warp=1)[1]
    with pytest.raises(ValueError, match="present: unknown source or format 'srgb'"):
        r.present("srgb")


def test_integers_for_floats_and_floats_for_integers_are_coerced_by_the_field_type():
    r, api = new_renderer()
    r.denoise(iterations=2.7, demodulate=True, sigma_color=1)
    r.denoise_blend(radius=2.9, z=2, min_half_samples=True)
    r.reproject(r.scene.camera, max_history=8)
    r.denoise_error(radius=1.5)
    assert api.calls == [("denoise", "ctx", ("ref", struct.pack("=iiffff", 2, 1, 1.0, 0.3, 0.2, 0.1))),
                         ("denoise_blend", "ctx", None, ("ref", struct.pack("=ifi", 2, 2.0, 1)), STATS0),
                         ("reproject", "ctx", ("ref", bytes(r.scene.camera)), ("ref", struct.pack("=fff", 8.0, 0.2, -1.0))),
                         ("denoise_error", "ctx", None, ("ref", struct.pack("=i", 1)), 0.0, STATS0)]
    assert [type(x) for x in api.calls[3][3:5]] == [tuple, float]


def test_an_unknown_parameter_is_a_type_error_before_any_call():
    r, api = new_renderer()
    with pytest.raises(TypeError, match=r"denoise_coverage: unknown denoise parameters \['sigma', 'variance_floor'\]"):
        r.denoise_coverage(variance_floor=1.0, sigma=2.0)
    for cls in FORMATS:
        with pytest.raises(TypeError):
            cls.pack(False, nope=1)
        with pytest.raises(TypeError):
            cls.pack(True, nope=None)
    assert api.calls == []


def test_blend_error_asks_the_library_for_its_entry_point_first():
    r, api = new_renderer(missing=("blend_error_display",))
    with pytest.raises(NotImplementedError, match="this library has no rtpbr_blend_error_display"):
        r.blend_error(bias="display")
    with pytest.raises(ValueError, match='bias must be "linear" or "display"'):
        r.blend_error(bias="srgb")
    assert api.calls == []
    r.blend_error()
    assert api.calls == [("blend_error", "ctx", None, None, None, 0.0, STATS0)]


# ------------------------------------------------------------------ the entry-point table
def test_the_entry_point_lists_are_the_table_and_hold_what_they_held():
    names = list(_capi.SIGNATURES)
    assert _capi.ENTRY_POINTS == [n for n in names if n != "test_math"] and "test_math" in names and len(names) == len(set(names)) == 64
    assert isinstance(_capi.ENTRY_POINTS, list) and isinstance(_capi.ALWAYS_OPTIONAL, tuple)
    assert _capi.ALWAYS_OPTIONAL == (
        "render_features", "denoise", "reproject", "noise_update", "noise_estimate", "denoise_guided", "select_mask", "select_noisy",
        "sample_selected", "set_noise_estimator", "present", "reproject_scene", "set_noise_tracking", "half_update", "denoise_error",
        "select_error", "set_half_mode", "denoise_blend", "denoise_blend_levels", "blend_error", "select_blend_error",
        "blend_error_display", "render_coverage", "denoise_coverage", "read_coverage")
    assert _capi.ENTRY_POINTS[:38] == [
        "create", "destroy", "last_error", "backend", "set_config", "set_scene", "get_scene", "set_camera", "set_env", "set_tiles",
        "refresh", "sample", "post_process", "sync", "read_buffer", "write_buffer", "host_alloc", "host_free", "buffer_device_ptr",
        "read_buffer_async", "read_wait", "packed_bytes", "pack_tiles", "unpack_tiles", "get_counters", "get_counter", "last_sample_ms",
        "last_primary_ms", "get_stream", "set_option", "set_shape_data", "rccl_unique_id", "rccl_init", "rccl_init_all", "gather_tiles",
        "gather_tiles_all", "rccl_info", "jit_prebuild"]
    assert _capi.ENTRY_POINTS[38:] == list(_capi.ALWAYS_OPTIONAL)
    for res, args in _capi.SIGNATURES.values():
        assert res in (C.c_int, C.c_char_p) and isinstance(args, list)


def test_capi_binds_the_table_and_lets_only_the_optional_rows_be_missing(tmp_path):
    src = tmp_path / "lib.c"
    src.write_text("".join(f"int t_{n}(void) {{ return {i}; }}\n" for i, n in enumerate(_capi.ENTRY_POINTS[:38])))
    subprocess.run([os.environ.get("CC", "gcc"), "-shared", "-fPIC", str(src), "-o", str(tmp_path / "lib.so")], check=True)
    api = _capi.CApi(str(tmp_path / "lib.so"), "t_")
    assert list(api.fn) == _capi.ENTRY_POINTS[:38] and not api.has("test_math") and not api.has("denoise") and api.has("sample")
    assert api.fn["set_option"].argtypes == [C.c_void_p, C.c_char_p, C.c_longlong] and api.fn["backend"].restype is C.c_char_p
    with pytest.raises(AttributeError):
        _capi.CApi(str(tmp_path / "lib.so"), "t_", optional=())      # test_math is missing and no longer optional
    with pytest.raises(FileNotFoundError, match="not found — build it first"):
        _capi.CApi(str(tmp_path / "nope.so"))


# ------------------------------------------------------------------ the buffer table
def test_the_buffer_ids_are_the_headers_without_gaps():
    hdr = open(os.path.join(ROOT, "include", "rtpbr.h")).read()
    ids = {m.group(1): int(m.group(2)) for m in re.finditer(r"\bRTPBR_BUF_(\w+)\s*=\s*(\d+)", hdr)}
    assert sorted(ids.values()) == list(range(20))
    assert {k[4:]: v for k, v in vars(renderer).items() if k.startswith("BUF_")} == ids
    assert [row[0] for row in renderer.BUFFERS] == list(range(20))
    from raytracingpbr_amd.renderer import BUF_BLEND_ERROR, BUF_IMAGE_PIXELS      # noqa: F401 (the names import as before)
    assert (BUF_IMAGE_PIXELS, BUF_BLEND_ERROR) == (1, 19)


SHAPES = {"image_buffer": ((W, H, 4), "f4"), "image_pixels": ((W, H, 3), "f4"), "ray_buffer": ((W, H, 10), "f4"), "diff_buffer": ((W, H, 2), "f4"),
          "diff_pixels": ((W, H), "f4"), "feature_albedo": ((W, H, 3), "f4"), "feature_normal": ((W, H, 3), "f4"), "feature_depth": ((W, H), "f4"),
          "feature_object": ((W, H), "i4"), "denoised_pixels": ((W, H, 3), "f4"), "motion": ((W, H, 2), "f4"), "moments": ((W, H, 4), "f4"),
          "noise": ((W, H), "f4"), "selection": ((W, H), "u1"), "presented": ((H, W, 4), "u1"), "half_buffer": ((W, H, 4), "f4"),
          "denoised_error": ((W, H), "f4"), "blend_weight": ((W, H), "f4"), "blend_depth": ((W, H), "f4"), "blend_error_map": ((W, H), "f4")}


def test_every_buffer_reads_through_its_property_with_its_shape_and_only_two_can_be_set():
    r, api = new_renderer()
    for which, (name, (shape, dt)) in enumerate(SHAPES.items()):
        del api.calls[:]
        a = getattr(r, name)
        assert a.shape == shape and a.dtype == np.dtype(dt)
        probe = [("buffer_device_ptr", "ctx", which, ("ref", bytes(8)), ("ref", bytes(8)))] if name == "presented" else []
        assert api.calls == probe + [("read_buffer", "ctx", which, "ptr", a.nbytes)]
        prop = getattr(Renderer, name)
        assert (prop.fset is not None) == (name in ("image_buffer", "ray_buffer"))
        if name not in ("image_pixels", "diff_pixels", "denoised_pixels") and not name.startswith(("image_buffer", "feature_")):
            assert prop.__doc__ and ("(W,H" in prop.__doc__ or "(H, W, C)" in prop.__doc__ or "src/fileds.py" in prop.__doc__)
    del api.calls[:]
    x = np.arange(W * H * 4, dtype=np.float64).reshape(W, H, 4)
    r.image_buffer = x
    assert api.calls == [("write_buffer", "ctx", 0, x.astype(np.float32).tobytes(), W * H * 16)]
    with pytest.raises(AttributeError):
        r.image_pixels = x
    del api.calls[:]
    r._write(renderer.BUF_NOISE, np.ones((W, H)))      # Python does not refuse a read-only id: the library does
    assert api.calls == [("write_buffer", "ctx", 12, np.ones((W, H), np.float32).tobytes(), W * H * 4)]
    with pytest.raises(ValueError, match=r"expected shape \(6, 4\), got \(4, 6\)"):
        r._write(renderer.BUF_NOISE, np.ones((H, W)))
    assert r.coverage.shape == (W, H, 4) and api.calls[-1] == ("read_coverage", "ctx", "ptr", W * H * 16)


def test_read_into_and_read_async_refuse_a_wrong_destination_before_any_call():
    r, api = new_renderer()
    good = np.empty((W, H, 3), np.float32)
    bad = [np.empty((H, W, 3), np.float32), np.empty((W, H, 3), np.float64), np.empty((W, H, 6), np.float32)[..., ::2]]
    for read in (r.read_into, r.read_async):
        for out in bad:
            with pytest.raises(ValueError, match=r"expected a C-contiguous <class 'numpy.float32'> array of shape \(6, 4, 3\)"):
                read(renderer.BUF_IMAGE_PIXELS, out)
    assert api.calls == []
    assert r.read_into(renderer.BUF_IMAGE_PIXELS, good) is good and r.read_async(renderer.BUF_IMAGE_PIXELS, good) == 1
    assert api.calls == [("read_buffer", "ctx", 1, "ptr", good.nbytes), ("read_buffer_async", "ctx", 1, "ptr", good.nbytes, ("ref", bytes(4)))]
    a = r.host_array(renderer.BUF_SELECTION)
    assert a.shape == (W, H) and a.dtype == np.uint8 and api.calls[-1][:3] == ("host_alloc", "ctx", W * H)


# ------------------------------------------------------------------ the count and the statistics calls
def test_the_select_calls_return_the_count_and_the_estimates_the_statistics():
    r, api = new_renderer(script={"select_noisy": [7], "select_error": [5], "select_blend_error": [3], "select_mask": [2],
                                  "noise_estimate": [(24, 9, 0.5)]})
    mask = np.zeros((W, H), np.int64)
    mask[1, 2] = mask[3, 0] = 5
    assert (r.select_mask(mask), r.select_noisy(0.25, 2.0), r.select_error(0.5), r.select_blend_error(1, True)) == (2, 7, 5, 3)
    s = r.noise_estimate(1)
    assert (s.pixels_estimated, s.pixels_above, s.max_noise) == (24, 9, 0.5)
    n0 = ("ref", bytes(4))
    assert api.calls == [("select_mask", "ctx", (mask != 0).astype(np.uint8).tobytes(), W * H, n0), ("select_noisy", "ctx", 0.25, 2, n0),
                         ("select_error", "ctx", 0.5, 0, n0), ("select_blend_error", "ctx", 1.0, 1, n0), ("noise_estimate", "ctx", 1.0, STATS0)]
    assert [type(x) for x in api.calls[3][2:4]] == [float, int]
    with pytest.raises(ValueError, match=r"expected a mask of shape \(6, 4\), got \(4, 6\)"):
        r.select_mask(mask.T)


# ------------------------------------------------------------------ the render loops: one call order each
def names(api):
    return [(c[0],) + tuple(x for x in c[2:] if isinstance(x, (int, float))) for c in api.calls]


def test_render_until_call_order():
    above, none = (24, 3, 0.5), (24, 0, 0.01)
    r, api = new_renderer(script={"noise_estimate": [above, none]})
    r.track_noise = True
    assert r.render_until(0.25, 10, 4)[0] == 10 and r.track_noise is True      # 4 + 4, estimate, + 2 (the budget), estimate
    assert names(api) == [("sample", 4), ("noise_update",), ("sample", 4), ("noise_update",), ("noise_estimate", 0.25),
                          ("sample", 2), ("noise_update",), ("noise_estimate", 0.25)]
    r, api = new_renderer(script={"noise_estimate": [above, none]})
    used, stats = r.render_until(0.25, 64, 4, per_sample=True)      # an estimate after the first batch; restored after
    assert used == 8 and stats.pixels_above == 0
    assert names(api) == [("set_noise_tracking", 1), ("sample", 4), ("noise_estimate", 0.25), ("sample", 4), ("noise_estimate", 0.25),
                          ("set_noise_tracking", 0)]
    r, api = new_renderer(fail=("sample", 2))
    r.track_noise = True
    with pytest.raises(Scripted):
        r.render_until(0.25, 64, 1, per_sample=True)
    assert names(api) == [("set_noise_tracking", 1), ("sample", 1), ("sample", 1), ("set_noise_tracking", 0)] and r.track_noise is True
    with pytest.raises(ValueError, match="batch_spp and max_spp must be >= 1"):
        r.render_until(0.25, 0)


def test_render_adaptive_call_order():
    r, api = new_renderer(script={"select_noisy": [5, 0]})
    r.track_halves = True      # (not this loop's: the halves keep being dealt)
    assert r.render_adaptive(0.25, 64, 4, dilate=1)[0] == 2 * W * H * 4 + 5 * 4
    assert names(api) == [("sample", 4), ("half_update",), ("noise_update",), ("sample", 4), ("half_update",), ("noise_update",),
                          ("select_noisy", 0.25, 1), ("sample_selected", 4), ("half_update",), ("noise_update",), ("select_noisy", 0.25, 1),
                          ("noise_estimate", 0.25)]
    r, api = new_renderer(script={"select_noisy": [5, 7, 9]})
    r.set_noise_tracking(True)
    del api.calls[:]
    assert r.render_adaptive(0.25, 10, 4, per_sample=True)[0] == W * H * 4 + 5 * 4      # the budget ends it: 4 + 4, and 4 more would pass 10
    assert names(api) == [("set_noise_tracking", 1), ("sample", 4), ("select_noisy", 0.25, 0), ("sample_selected", 4), ("noise_estimate", 0.25),
                          ("set_noise_tracking", 1)]
    r, api = new_renderer()
    assert r.render_adaptive(0.25, 3, 4)[0] == W * H * 3      # a budget below one batch: one short batch, no second
    assert names(api) == [("sample", 3), ("noise_update",), ("noise_estimate", 0.25)]


def test_render_adaptive_denoised_call_order():
    above, none = (24, 3, 0.5), (24, 0, 0.01)
    r, api = new_renderer(script={"denoise_error": [above, none], "select_error": [6]})
    r.track_noise = r.track_halves = True
    traced, stats = r.render_adaptive_denoised(0.25, 64, 2, iterations=2)
    assert traced == 2 * W * H * 2 + 6 * 2 and stats.pixels_above == 0 and r.track_noise is True and r.track_halves is True
    p = packed(dc.DenoiseParams, iterations=2)
    assert [c[0] for c in api.calls] == ["sample", "half_update", "sample", "half_update", "denoise_error", "select_error", "sample_selected",
                                         "half_update", "denoise_error", "denoise"]
    assert api.calls[4] == ("denoise_error", "ctx", p, None, 0.25, STATS0) and api.calls[5][2:4] == (0.25, 1) and api.calls[-1] == ("denoise", "ctx", p)
    # per sample, the level blend's own estimate, ended by a failure: the half mode comes back, with the warp it had
    r, api = new_renderer(script={"blend_error_display": [above]}, fail=("sample_selected", 1))
    r.set_half_mode(False, True)
    del api.calls[:]
    with pytest.raises(Scripted):
        r.render_adaptive_denoised(0.25, 64, 2, 0, True, "levels", stop="blend", bias="display")
    M = dc.HalfMode
    assert [c for c in api.calls if c[0] == "set_half_mode"] == [("set_half_mode", "ctx", packed(M, per_sample=1, warp=1)),
                                                                 ("set_half_mode", "ctx", packed(M, warp=1))]
    assert [c[0] for c in api.calls] == ["set_half_mode", "sample", "sample", "blend_error_display", "select_blend_error", "sample_selected",
                                         "set_half_mode"]
    for blend, last in ((True, "denoise_blend"), ("levels", "denoise_blend_levels")):
        r, api = new_renderer()
        r.render_adaptive_denoised(0.25, 2, 2, blend=blend)
        assert [c[0] for c in api.calls] == ["sample", "half_update", "denoise_error", last]
