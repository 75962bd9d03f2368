"""POD data model shared with the C ABI (include/rtpbr.h).

Mirrors the reference's ``@ti.dataclass`` types field for field
(reference: src/dataclass.py:5-46): Ray, Material, Transform, SDFObject, Camera.
They are ``ctypes.Structure`` so a list of SDFObject can be handed to
``rtpbr_set_scene`` without conversion.
"""
import ctypes as C
from enum import IntEnum

vec3_t = C.c_float * 3


def vec3(x, y=None, z=None):
    """taichi.math.vec3-like constructor: vec3(1) -> (1,1,1); vec3(a,b,c)."""
    if y is None and z is None:
        if isinstance(x, (tuple, list)) or hasattr(x, "__len__"):
            x, y, z = x
        else:
            y = z = x
    return (float(x), float(y), float(z))


class SHAPE(IntEnum):
    """reference: src/sdf.py:12-18; BUNNY = neural SDF of bunny_sdf_glass.py:149-203."""
    NONE = 0
    SPHERE = 1
    BOX = 2
    CYLINDER = 3
    CONE = 4
    PLANE = 5
    BUNNY = 6


class _Pod(C.Structure):
    def __repr__(self):
        parts = []
        for name, typ in self._fields_:
            v = getattr(self, name)
            if hasattr(v, "__len__"):
                v = tuple(v)
            parts.append(f"{name}={v}")
        return f"{type(self).__name__}({', '.join(parts)})"


class Ray(_Pod):
    """reference: src/dataclass.py:5-10 (40 B)."""
    _fields_ = [("origin", vec3_t), ("direction", vec3_t), ("color", vec3_t), ("depth", C.c_int32)]


class Material(_Pod):
    """reference: src/dataclass.py:13-20 (40 B). emission is multiplicative."""
    _fields_ = [("albedo", vec3_t), ("emission", vec3_t), ("roughness", C.c_float),
                ("metallic", C.c_float), ("transmission", C.c_float), ("ior", C.c_float)]

    def __init__(self, albedo=(1, 1, 1), emission=(1, 1, 1), roughness=1.0, metallic=0.0,
                 transmission=0.0, ior=1.0):
        super().__init__(vec3_t(*vec3(albedo)), vec3_t(*vec3(emission)), roughness, metallic,
                         transmission, ior)


class Transform(_Pod):
    """reference: src/dataclass.py:23-28 (72 B). rotation in Euler degrees; matrix is filled
    by the library at scene upload (src/scene.py:99-109)."""
    _fields_ = [("position", vec3_t), ("rotation", vec3_t), ("scale", vec3_t), ("matrix", C.c_float * 9)]

    def __init__(self, position=(0, 0, 0), rotation=(0, 0, 0), scale=(1, 1, 1)):
        super().__init__(vec3_t(*vec3(position)), vec3_t(*vec3(rotation)), vec3_t(*vec3(scale)))


class SDFObject(_Pod):
    """reference: src/dataclass.py:31-35 (116 B)."""
    _fields_ = [("type", C.c_int32), ("transform", Transform), ("material", Material)]

    def __init__(self, type=SHAPE.BOX, transform=None, material=None):
        super().__init__(int(type), transform or Transform(), material or Material())


class Camera(_Pod):
    """reference: src/dataclass.py:38-46 (52 B); vfov in degrees."""
    _fields_ = [("lookfrom", vec3_t), ("lookat", vec3_t), ("vup", vec3_t), ("vfov", C.c_float),
                ("aspect", C.c_float), ("aperture", C.c_float), ("focus", C.c_float)]

    def __init__(self, lookfrom=(0, 0, 0), lookat=(0, 0, 1), vup=(0, 1, 0), vfov=35.0, aspect=1.0,
                 aperture=0.01, focus=4.0):
        super().__init__(vec3_t(*vec3(lookfrom)), vec3_t(*vec3(lookat)), vec3_t(*vec3(vup)), vfov,
                         aspect, aperture, focus)


class Counters(_Pod):
    _fields_ = [("samples", C.c_uint64), ("raycasts", C.c_uint64), ("march_steps", C.c_uint64),
                ("hits", C.c_uint64), ("sky_lookups", C.c_uint64), ("deposits", C.c_uint64)]


assert C.sizeof(Ray) == 40 and C.sizeof(Material) == 40 and C.sizeof(Transform) == 72
assert C.sizeof(SDFObject) == 116 and C.sizeof(Camera) == 52


class _Params(_Pod):
    """A parameter struct of a call: ``DEFAULTS`` holds, field by field, what the library uses when it is handed NULL."""

    @classmethod
    def pack(cls, null_if_default, *values, **given):
        """The struct filled from ``values`` (in field order) and ``given`` (by name): a field not given, or given as ``None``,
        takes its DEFAULTS entry, and each goes through int() or float() as its ctypes type says.  ``null_if_default``: ``None``
        instead of the struct when nothing was given, for the caller that hands the library NULL then."""
        given = {**dict(zip(cls.DEFAULTS, values)), **given}
        unknown = set(given) - set(cls.DEFAULTS)
        if unknown or len(values) > len(cls.DEFAULTS):
            raise TypeError(f"{cls.__name__}: unknown parameters {sorted(unknown) or values[len(cls.DEFAULTS):]}")
        if null_if_default and all(v is None for v in given.values()):
            return None
        return cls(*((float if t is C.c_float else int)(cls.DEFAULTS[k] if given.get(k) is None else given[k]) for k, t in cls._fields_))


class DenoiseParams(_Params):
    """rtpbr_denoise_params (include/rtpbr.h): a-trous levels, albedo demodulation and the four edge-stopping sigmas."""
    _fields_ = [("iterations", C.c_int32), ("demodulate", C.c_int32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float),
                ("sigma_depth", C.c_float), ("sigma_albedo", C.c_float)]

    # include/rtpbr.h RTPBR_DENOISE_DEFAULT_*, what rtpbr_denoise(ctx, NULL) uses; Renderer.denoise() fills the parameters not
    # given from here (tests/test_feature_ref.py::test_python_denoise_defaults_match_the_header keeps the two equal)
    DEFAULTS = {"iterations": 4, "demodulate": 0, "sigma_color": 2.0, "sigma_normal": 0.3, "sigma_depth": 0.2, "sigma_albedo": 0.1}


class CoverageParams(_Params):
    """rtpbr_coverage_params (include/rtpbr.h): the sub-ray grid of rtpbr_render_coverage, and the tap-weight power and the edge
    resolve of rtpbr_denoise_coverage."""
    _fields_ = [("grid", C.c_int32), ("power", C.c_int32), ("resolve", C.c_int32)]

    # include/rtpbr.h RTPBR_COVERAGE_DEFAULT_*, what the two calls use for NULL (tests/test_coverage_ref.py keeps the two equal)
    DEFAULTS = {"grid": 4, "power": 4, "resolve": 1}


class ReprojectParams(_Params):
    """rtpbr_reproject_params (include/rtpbr.h): the history cap and the depth and normal tests of a reprojection tap."""
    _fields_ = [("max_history", C.c_float), ("depth_tolerance", C.c_float), ("normal_cos", C.c_float)]

    # include/rtpbr.h RTPBR_REPROJECT_DEFAULT_*, what rtpbr_reproject(ctx, cam, NULL) uses; Renderer.reproject() fills the
    # parameters not given from here (tests/test_reproject_ref.py keeps the two equal)
    DEFAULTS = {"max_history": 64.0, "depth_tolerance": 0.2, "normal_cos": -1.0}


class NoiseStats(_Pod):
    """rtpbr_noise_stats (include/rtpbr.h): what rtpbr_noise_estimate counts over the frame."""
    _fields_ = [("pixels_estimated", C.c_uint32), ("pixels_above", C.c_uint32), ("max_noise", C.c_float)]


class NoiseEstimator(_Params):
    """rtpbr_noise_estimator (include/rtpbr.h): the optional estimator setting of a context — pooling of the young pixels'
    within-pixel sums of squares over the neighbours on the same object, and a minimum sample count for select_noisy."""
    _fields_ = [("pool_batches", C.c_int32), ("pool_radius", C.c_int32), ("min_samples", C.c_int32)]

    # include/rtpbr.h RTPBR_NOISE_ESTIMATOR_DEFAULT_*, what rtpbr_set_noise_estimator(ctx, NULL) sets: off
    # (tests/test_pool_ref.py keeps the two equal)
    DEFAULTS = {"pool_batches": 0, "pool_radius": 3, "min_samples": 0}


class ErrorParams(_Params):
    """rtpbr_error_params (include/rtpbr.h): the window of rtpbr_denoise_error's two-half estimate."""
    _fields_ = [("radius", C.c_int32)]

    # include/rtpbr.h RTPBR_ERROR_DEFAULT_*, what rtpbr_denoise_error(ctx, p, NULL, ...) uses (tests/test_half_ref.py keeps the two equal)
    DEFAULTS = {"radius": 2}


class BlendParams(_Params):
    """rtpbr_blend_params (include/rtpbr.h): the window, the significance gate and the minimum half size of rtpbr_denoise_blend."""
    _fields_ = [("radius", C.c_int32), ("z", C.c_float), ("min_half_samples", C.c_int32)]

    # include/rtpbr.h RTPBR_BLEND_DEFAULT_*, what rtpbr_denoise_blend(ctx, p, NULL, ...) uses (tests/test_blend_ref.py keeps the two equal)
    DEFAULTS = {"radius": 3, "z": 2.0, "min_half_samples": 16}


class HalfMode(_Params):
    """rtpbr_half_mode (include/rtpbr.h): halves dealt per sample by the sample calls, half A carried through the reprojections."""
    _fields_ = [("per_sample", C.c_int32), ("warp", C.c_int32)]

    # include/rtpbr.h RTPBR_HALF_MODE_DEFAULT_*, what rtpbr_set_half_mode(ctx, NULL) sets: off (tests/test_half_mode_ref.py keeps the two equal)
    DEFAULTS = {"per_sample": 0, "warp": 0}


class DenoiseGuidedParams(_Params):
    """rtpbr_denoise_guided_params (include/rtpbr.h): the a-trous whose colour term is measured in standard deviations of the
    pixel's estimated noise."""
    _fields_ = [("iterations", C.c_int32), ("demodulate", C.c_int32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float),
                ("sigma_depth", C.c_float), ("variance_floor", C.c_float)]

    # include/rtpbr.h RTPBR_DENOISE_GUIDED_DEFAULT_*, what rtpbr_denoise_guided(ctx, NULL) uses; Renderer.denoise_guided() fills
    # the parameters not given from here (tests/test_noise_ref.py keeps the two equal)
    DEFAULTS = {"iterations": 4, "demodulate": 0, "sigma_color": 16.0, "sigma_normal": 0.3, "sigma_depth": 0.2, "variance_floor": 1e-3}


class PresentParams(_Params):
    """rtpbr_present_params (include/rtpbr.h): which display buffer becomes the packed 8-bit frame, its pixel format, and
    whether the quantisation is ordered-dithered."""
    _fields_ = [("source", C.c_int32), ("format", C.c_int32), ("dither", C.c_int32)]

    # include/rtpbr.h RTPBR_PRESENT_DEFAULT_*, what rtpbr_present(ctx, NULL) uses: image_pixels as RGBA8, no dither
    # (tests/test_present_ref.py keeps the two equal)
    DEFAULTS = {"source": 0, "format": 1, "dither": 0}
    SOURCES = {"pixels": 0, "denoised": 1, "accum": 2}      # RTPBR_PRESENT_PIXELS / _DENOISED / _ACCUM
    FORMATS = {"rgb8": 0, "rgba8": 1}                        # RTPBR_PRESENT_RGB8 / _RGBA8
