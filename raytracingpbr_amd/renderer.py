"""Renderer: the host-side mirror of the reference's render loop.

reference: src/renderer.py:12-32 — ``refresh()``, ``render(refreshing)`` =
``[refresh()] ; SAMPLES_PER_FRAME x pathtrace() ; post_process()`` — and the examples'
kernels ``render(camera_position, camera_lookat, camera_up, moving)``
(cornell_box_v3/renderer.py:11-42) / ``sample() refresh() render()``
(bunny_sdf_glass.py:393-432).  Buffers keep the reference's field names and layout:
``image_buffer`` (W,H,4) f32 = (sum r,g,b, count), ``image_pixels`` (W,H,3) f32,
``ray_buffer`` (W,H) of Ray; index [i, j] = column from the left, row from the bottom.
"""
import contextlib
import ctypes as C

import numpy as np

from . import _capi
from .config import FORM, Config
from .dataclass import BlendParams, Camera, Counters, CoverageParams, DenoiseGuidedParams, DenoiseParams, ErrorParams, HalfMode, NoiseEstimator, NoiseStats, PresentParams, Ray, ReprojectParams, SDFObject
from .scene import Scene

f32 = np.float32
# The public buffers (include/rtpbr.h RTPBR_BUF_*), one row each: id, BUF_ name, shape after (W, H), dtype, the Renderer property
# that reads it, whether Python can also assign to that property, the property's docstring.  Buffers 5 and up exist from the first
# call that writes them on (the call their docstring names; the features: render_features, denoised_pixels: denoise).
BUFFERS = [
    (0, "IMAGE_BUFFER", (4,), f32, "image_buffer", True, None),
    (1, "IMAGE_PIXELS", (3,), f32, "image_pixels", False, None),
    (2, "RAY_BUFFER", (10,), f32, "ray_buffer", True, "(W,H,10) float32 view of Ray; the last column holds the int32 depth bit pattern."),
    (3, "DIFF_BUFFER", (2,), f32, "diff_buffer", False, "adaptive-sampling statistics (src/fileds.py:21): (sum of display change, count)"),
    (4, "DIFF_PIXELS", (), f32, "diff_pixels", False, None),
    (5, "FEAT_ALBEDO", (3,), f32, "feature_albedo", False, None),
    (6, "FEAT_NORMAL", (3,), f32, "feature_normal", False, None),
    (7, "FEAT_DEPTH", (), f32, "feature_depth", False, None),
    (8, "FEAT_OBJECT", (), np.int32, "feature_object", False, None),
    (9, "DENOISED_PIXELS", (3,), f32, "denoised_pixels", False, None),
    (10, "MOTION", (2,), f32, "motion", False,
     "(W,H,2): the old-frame pixel coordinates the last reproject() took each pixel's history from, (-1,-1) = none"),
    (11, "MOMENTS", (4,), f32, "moments", False,
     "(W,H,4): (sum c L, sum c L^2, sum c, K) over the K batches noise_update() has folded in (with set_noise_tracking(True): "
     "every sample is a batch, c = 1), c samples each, L the compressed luminance of the batch mean"),
    (12, "NOISE", (), f32, "noise", False,
     "(W,H): the last noise_estimate() / denoise_guided()'s standard deviation of each pixel's displayed luminance"),
    (13, "SELECTION", (), np.uint8, "selection", False, "(W,H) uint8: 1 = selected by the last select_mask() / select_noisy(); after set_select_tiers(T > 1): 1 + the pixel's tier"),
    # not a field: top-down, C = 3 or 4 as the last present() said, which the library knows (_shape asks it)
    (14, "PRESENT", None, np.uint8, "presented", False, "(H, W, C) uint8: the frame of the last present(), top row first (blocking read)"),
    (15, "HALF_BUFFER", (4,), f32, "half_buffer", False,
     "(W,H,4): half A's (sum r, sum g, sum b, count) as half_update() dealt it; half B is image_buffer minus this"),
    (16, "DENOISED_ERROR", (), f32, "denoised_error", False,
     "(W,H): the last denoise_error()'s standard deviation of each pixel's denoised luminance, 0 where a half is empty"),
    (17, "BLEND_WEIGHT", (), f32, "blend_weight", False,
     "(W,H): the last denoise_blend()'s weight of the denoised colour, 1 where the halves are not usable or see no bias"),
    (18, "BLEND_DEPTH", (), f32, "blend_depth", False,
     "(W,H): how many a-trous levels the last denoise_blend_levels() kept, 0 (the raw average) .. iterations (the whole filter)"),
    (19, "BLEND_ERROR", (), f32, "blend_error_map", False,
     "(W,H): the last blend_error()'s root-mean-square error of each pixel's level-blended luminance, 0 where a half is empty"),
]
globals().update({"BUF_" + row[1]: row[0] for row in BUFFERS})      # BUF_IMAGE_BUFFER = 0, ...
_TAIL_AND_DTYPE = {row[0]: row[2:4] for row in BUFFERS}
ENV_RGB8, ENV_RGB32F = 0, 1


def _ref(struct):
    """a struct by address, NULL for None"""
    return None if struct is None else C.byref(struct)


class Renderer:
    def __init__(self, scene: Scene, config: Config, camera: Camera = None, device: int = 0, api=None):
        self.api = api if api is not None else _capi.hip_api()
        self._ctx = C.c_void_p()
        self.api.call("create", int(device), C.byref(self._ctx))
        self.device = device
        self.samples_per_frame = 1           # SAMPLES_PER_FRAME, src/config.py:9
        self._host_arrays = {}               # address -> bytes of the page-locked blocks handed out by host_array()
        self.noise_estimator = NoiseEstimator.pack(False)      # what set_noise_estimator() last set
        self.track_noise = False             # True: every sample() call is one batch of the noise estimate (noise_update() after it)
        self.noise_per_sample = False        # what set_noise_tracking() last set: every SAMPLE is a batch, folded in by sample() itself
        self.track_halves = False            # True: every sample() / sample_selected() call is one batch of the two halves (half_update() after it)
        self.half_mode = HalfMode.pack(False)      # what set_half_mode() last set
        self.select_tiers = (1, 16)          # what set_select_tiers() last set: (tiers, batch)
        self.set_config(config)
        self.set_scene(scene)
        self.set_camera(camera if camera is not None else scene.camera)

    # ------------------------------------------------------------ setup
    def set_config(self, config: Config):
        # (kept only once the library has taken it: a refused configuration leaves the buffers' shapes as they were)
        c = config.copy()
        self.api.call("set_config", self._ctx, C.byref(c))
        self.config = c

    def set_scene(self, scene: Scene):
        n = len(scene.objects)
        arr = (SDFObject * n)(*scene.objects)
        self.api.call("set_scene", self._ctx, arr, n, 1 if scene.scale10 else 0)
        self.scene = scene

    def get_scene(self):
        n = len(self.scene.objects)
        arr = (SDFObject * n)()
        self.api.call("get_scene", self._ctx, arr, n)
        return list(arr)

    def set_camera(self, camera: Camera):
        self.camera = camera
        self.api.call("set_camera", self._ctx, C.byref(camera))

    def set_env(self, texels: np.ndarray, exposure: float = 1.0, gamma: float = 1.0):
        """texels: (W_e,H_e,3) uint8 (as ti.tools.imread returns, src/ibl.py:15) or float32."""
        t = np.ascontiguousarray(texels)
        if t.ndim != 3 or t.shape[2] != 3:
            raise ValueError("env texels must have shape (W, H, 3)")
        if t.dtype == np.uint8:
            fmt = ENV_RGB8
        elif t.dtype == np.float32:
            fmt = ENV_RGB32F
        else:
            raise TypeError("env texels must be uint8 or float32")
        self.api.call("set_env", self._ctx, t.ctypes.data_as(C.c_void_p), t.shape[0], t.shape[1], fmt,
                      float(exposure), float(gamma))

    def set_shape_data(self, shape: int, data: np.ndarray):
        """Per-shape data blob; the bunny MLP's 625 weights (bunny_sdf_glass.py:157-201)."""
        d = np.ascontiguousarray(data, dtype=np.float32)
        self.api.call("set_shape_data", self._ctx, int(shape), d.ctypes.data_as(C.c_void_p), d.size)

    def set_tiles(self, tile_w, tile_h, rank, world):
        self.api.call("set_tiles", self._ctx, tile_w, tile_h, rank, world)
        self.tiles = (tile_w, tile_h, rank, world)

    def set_option(self, key: str, value: int):
        self.api.call("set_option", self._ctx, key.encode(), int(value))

    # ------------------------------------------------------------ the reference's calls
    def refresh(self):
        """src/renderer.py:12-22."""
        self.api.call("refresh", self._ctx)

    def sample(self, n: int = 1):
        """complete-path form: n samples per pixel; persistent-ray form: n pathtrace() launches."""
        self.api.call("sample", self._ctx, int(n))
        if self.track_noise:
            self.noise_update()
        if self.track_halves:
            self.half_update()

    pathtrace = sample

    def post_process(self):
        """src/postprocessor.py:24-43."""
        self.api.call("post_process", self._ctx)

    def render(self, refreshing: bool = False, spp: int = None):
        """src/renderer.py:25-32.  ``spp`` overrides SAMPLES_PER_FRAME for this call."""
        if refreshing:
            self.refresh()
        self.sample(self.samples_per_frame if spp is None else spp)
        self.post_process()

    def sync(self):
        self.api.call("sync", self._ctx)

    def _count(self, name, *args) -> int:
        """a call whose last argument is the uint32 it counts into"""
        n = C.c_uint32()
        self.api.call(name, self._ctx, *args, C.byref(n))
        return int(n.value)

    def _stats(self, name, *args) -> NoiseStats:
        """a call whose last argument is the rtpbr_noise_stats it fills"""
        s = NoiseStats()
        self.api.call(name, self._ctx, *args, C.byref(s))
        return s

    @contextlib.contextmanager
    def _loop_state(self, halves=False, noise_per_sample=False, half_per_sample=False, select_tiers=None):
        """What a render loop that folds its batches itself sets for its duration and puts back after, however it ends:
        ``track_noise`` off (``halves``: and ``track_halves``), per-sample noise tracking or per-sample halves on where asked,
        ``select_tiers`` = (tiers, batch) where given."""
        mode, half_mode, tiers = self.noise_per_sample, self.half_mode, self.select_tiers
        if half_per_sample:
            self.set_half_mode(True, bool(half_mode.warp))
        keep = self.track_noise, self.track_halves
        self.track_noise = False
        if halves:
            self.track_halves = False
        try:
            if noise_per_sample:
                self.set_noise_tracking(True)
            if select_tiers is not None:
                self.set_select_tiers(*select_tiers)
            yield
        finally:
            self.track_noise, self.track_halves = keep
            if select_tiers is not None:
                self.set_select_tiers(*tiers)
            if noise_per_sample:
                self.set_noise_tracking(mode)
            if half_per_sample:
                self.set_half_mode(bool(half_mode.per_sample), bool(half_mode.warp))

    # ------------------------------------------------------------ first-hit features and the denoise (include/rtpbr.h)
    def render_features(self):
        """One primary ray through every pixel centre: albedo, shading normal, depth and object index of the first hit."""
        self.api.call("render_features", self._ctx)

    def denoise(self, iterations=None, demodulate=None, sigma_color=None, sigma_normal=None, sigma_depth=None, sigma_albedo=None):
        """Edge-aware a-trous filter of image_buffer into ``denoised_pixels`` (the features are rendered first when stale).
        ``None`` = the library's default for that parameter."""
        p = DenoiseParams.pack(True, iterations, demodulate, sigma_color, sigma_normal, sigma_depth, sigma_albedo)
        self.api.call("denoise", self._ctx, _ref(p))

    def denoise_fill(self, **denoise):
        """``denoise`` (same keyword parameters) with option ``denoise_fill`` set for the call: a pixel without samples takes the
        feature-weighted mean of the pixels of its object that have a colour, at the first a-trous level that reaches one
        (include/rtpbr.h rtpbr_denoise).  Returns (pixels filled, pixels still empty, the deepest level that filled one).  The
        option is 0 again afterwards, also when the call is refused.  Blocks."""
        unknown = set(denoise) - set(DenoiseParams.DEFAULTS)
        if unknown:
            raise TypeError(f"denoise_fill: unknown denoise parameters {sorted(unknown)}")
        self.set_option("denoise_fill", 1)
        try:
            self.denoise(**denoise)
        finally:
            self.set_option("denoise_fill", 0)
        return tuple(self.counter(k) for k in ("fill_filled", "fill_empty", "fill_deepest"))

    # ------------------------------------------------------------ coverage-aware denoise (include/rtpbr.h rtpbr_denoise_coverage)
    def render_coverage(self, grid=None):
        """Write ``coverage``: for every pixel next to a silhouette, how many of its ``grid`` x ``grid`` sub-rays (2 or 4) hit the
        pixel's own object and which other object takes most of the rest.  ``None`` = the library's default, 4.  The features
        are rendered first when stale; a sliver that passes between pixel centres is missed."""
        self.api.call("render_coverage", self._ctx, C.byref(CoverageParams.pack(False, grid)))

    def denoise_coverage(self, power=None, resolve=None, grid=None, **denoise) -> NoiseStats:
        """``denoise`` (same keyword parameters) with every tap weighted by (its pixel's own-object coverage)^``power``, and with
        the pixels that hold two objects resolved to the mix of the filter's result and the second object's 3x3 mean
        (``resolve``), into ``denoised_pixels``.  ``None`` = the library's default.  Returns the NoiseStats words as (resolved
        pixels, candidate pixels, largest 1 - coverage).  Blocks."""
        unknown = set(denoise) - set(DenoiseParams.DEFAULTS)
        if unknown:
            raise TypeError(f"denoise_coverage: unknown denoise parameters {sorted(unknown)}")
        p, cv = DenoiseParams.pack(False, **denoise), CoverageParams.pack(False, grid, power, resolve)
        return self._stats("denoise_coverage", C.byref(p), C.byref(cv))

    def denoise_coverage_fill(self, power=None, resolve=None, grid=None, **denoise):
        """``denoise_coverage`` (same parameters) with option ``coverage_fill`` set for the call: a pixel without samples takes
        the coverage- and feature-weighted mean of the pixels of its object that have a colour, at the first a-trous level whose
        weighted sum over them is above 0, and the resolve treats a pixel that has a colour after the last level as one with
        samples (include/rtpbr.h rtpbr_denoise_coverage).  Returns (``denoise_coverage``'s NoiseStats, (pixels filled, pixels
        still empty, the deepest level that filled one)).  The option is 0 again afterwards, also when the call is refused.
        Blocks."""
        unknown = set(denoise) - set(DenoiseParams.DEFAULTS)
        if unknown:
            raise TypeError(f"denoise_coverage_fill: unknown denoise parameters {sorted(unknown)}")
        self.set_option("coverage_fill", 1)
        try:
            stats = self.denoise_coverage(power, resolve, grid, **denoise)
        finally:
            self.set_option("coverage_fill", 0)
        return stats, tuple(self.counter(k) for k in ("fill_filled", "fill_empty", "fill_deepest"))

    # ------------------------------------------------------------ temporal reuse (include/rtpbr.h rtpbr_reproject)
    def reproject(self, camera: Camera, max_history=None, depth_tolerance=None, normal_cos=None):
        """set_camera(camera) + refresh() that keeps what the new view can reuse: the accumulated image_buffer is warped into
        the new view (first-hit depth, object and normal tests; count capped at ``max_history``), ``motion`` says where each
        pixel's history came from.  Needs a refresh() (or an earlier reproject()) since the last set_config / set_scene /
        set_shape_data / set_env.  ``None`` = the library's default for that parameter."""
        p = ReprojectParams.pack(True, max_history, depth_tolerance, normal_cos)
        self.api.call("reproject", self._ctx, C.byref(camera), _ref(p))
        self.camera = camera

    def reproject_scene(self, scene: Scene, camera: Camera = None, max_history=None, depth_tolerance=None, normal_cos=None):
        """set_scene(scene) (+ set_camera(camera) if given) + refresh() that keeps history, for a scene whose objects moved
        rigidly: same count, types, scales and materials, only positions and rotations changed (anything else: EINVAL, use
        set_scene + refresh).  A first hit on a moved object is followed back to where that surface point was; every other
        pixel is warped as reproject() warps it.  The history still shows the old shadows and interreflections of the moved
        objects until new samples outweigh it: use a smaller ``max_history`` than for camera moves (include/rtpbr.h
        rtpbr_reproject_scene).  ``None`` = the library's default for that parameter."""
        n = len(scene.objects)
        arr = (SDFObject * n)(*scene.objects)
        p = ReprojectParams.pack(True, max_history, depth_tolerance, normal_cos)
        self.api.call("reproject_scene", self._ctx, _ref(camera), arr, n, 1 if scene.scale10 else 0, _ref(p))
        self.scene = scene
        if camera is not None:
            self.camera = camera

    # ------------------------------------------------------------ noise estimation (include/rtpbr.h rtpbr_noise_*)
    def noise_update(self):
        """Fold the samples deposited since the last call into ``moments`` as one batch (the first call's batch is everything
        accumulated so far).  The estimate needs two batches per pixel; before that ``noise_estimate`` looks at the neighbours."""
        self.api.call("noise_update", self._ctx)

    def set_noise_tracking(self, per_sample: bool):
        """``True``: from now on sample() and sample_selected() of the complete-path form fold every sample into ``moments`` as a
        batch of its own, in the pass that adds it to image_buffer: n spp give the estimate n - 1 degrees of freedom per pixel
        (not calls - 1), it is valid after the first call, and no noise_update() is needed (what was deposited before is folded
        as one batch by this call; ``track_noise``'s extra noise_update() finds nothing new).  "Batches" in
        ``set_noise_estimator(pool_batches=...)`` then means samples.  ``False``: back to batches per noise_update().  Refused by
        sample() in the persistent-ray form, with option precision = 1 and with tiles of world > 1.  Kept across refresh /
        set_config / set_scene / reproject."""
        self.api.call("set_noise_tracking", self._ctx, 1 if per_sample else 0)
        self.noise_per_sample = bool(per_sample)

    def set_noise_estimator(self, pool_batches: int = 0, pool_radius: int = 3, min_samples: int = 0):
        """The estimator behind noise_estimate / select_noisy / denoise_guided (and so render_until / render_adaptive); the
        defaults are off.  ``pool_batches`` 3..64: a pixel with fewer batches than this (but two or more) takes the larger of
        its own variance and the one pooled from the within-pixel sums of squares of the pixels on its object within
        ``pool_radius`` (1..3), so a pixel whose few batches agree by chance is not taken for converged.  ``min_samples`` > 0:
        select_noisy also selects every pixel with fewer samples.  Kept across refresh / set_config / set_scene / reproject."""
        e = NoiseEstimator.pack(False, pool_batches, pool_radius, min_samples)
        self.api.call("set_noise_estimator", self._ctx, C.byref(e))
        self.noise_estimator = e

    def noise_estimate(self, threshold: float = 0.0) -> NoiseStats:
        """Write ``noise`` (the estimated standard deviation of each pixel's displayed luminance, in the c / (1 + c) domain) and
        return how many pixels have samples, how many of them are noisier than ``threshold``, and the largest value.  Blocks.
        With ``set_noise_estimator(pool_batches=...)`` a pixel of two or more but fewer batches than that takes
        max(its own variance, the variance pooled over its neighbours on the same object): include/rtpbr.h has the rule."""
        return self._stats("noise_estimate", float(threshold))

    def denoise_guided(self, iterations=None, demodulate=None, sigma_color=None, sigma_normal=None, sigma_depth=None, variance_floor=None):
        """The a-trous of ``denoise`` with the colour distance measured in standard deviations of each pixel's estimated noise
        (``sigma_color`` of them), the variance filtered along level by level.  Writes ``denoised_pixels`` and ``noise``.
        ``None`` = the library's default for that parameter."""
        p = DenoiseGuidedParams.pack(True, iterations, demodulate, sigma_color, sigma_normal, sigma_depth, variance_floor)
        self.api.call("denoise_guided", self._ctx, _ref(p))

    def render_until(self, noise: float, max_spp: int, batch_spp: int = 16, per_sample: bool = False):
        """Sample in batches of ``batch_spp`` (sample() calls of that size, each one batch of the noise estimate) until no pixel's
        estimated noise exceeds ``noise`` or ``max_spp`` is spent; never fewer than two batches, which the estimate needs.
        Returns (spp used, NoiseStats of the last estimate).  Continues whatever is accumulated: refresh() first for a new frame.
        ``per_sample``: with set_noise_tracking(True) for the duration of the call (restored after), no noise_update(), and the
        first estimate as soon as this call has traced two samples per pixel — after the first batch when ``batch_spp`` >= 2."""
        if not (batch_spp >= 1 and max_spp >= 1):
            raise ValueError("batch_spp and max_spp must be >= 1")
        batch, budget = int(batch_spp), int(max_spp)
        with self._loop_state(noise_per_sample=per_sample):
            used, batches, stats = 0, 0, None
            while used < budget:
                n = min(batch, budget - used)
                self.sample(n)
                if not per_sample:
                    self.noise_update()
                used, batches = used + n, batches + 1
                if (used if per_sample else batches) >= 2 or used >= budget:      # (the estimate needs two batches; per sample, two samples)
                    stats = self.noise_estimate(noise)
                    if stats.pixels_above == 0:
                        break
            return used, stats

    # ------------------------------------------------------------ adaptive sampling (include/rtpbr.h rtpbr_select_* / rtpbr_sample_selected)
    def select_mask(self, mask, raw=False) -> int:
        """Select the pixels where ``mask`` (W,H) is nonzero — a region of interest.  Returns how many.  ``raw``: the mask is
        uint8 and its bytes cross as they are, which with ``set_select_tiers(T > 1)`` makes them tiers: 1 = the full share of
        the batch, 2 = half of it, ... (bytes above T count as T)."""
        W, H = self.config.width, self.config.height
        if raw:
            if np.asarray(mask).dtype != np.uint8:
                raise TypeError("a raw mask must be uint8")
            m = np.ascontiguousarray(mask)
        else:
            m = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
        if m.shape != (W, H):
            raise ValueError(f"expected a mask of shape {(W, H)}, got {m.shape}")
        return self._count("select_mask", m.ctypes.data_as(C.c_void_p), m.nbytes)

    def set_select_tiers(self, tiers: int = 1, batch: int = 16):
        """Options ``select_tiers`` and ``select_batch`` for the select calls that follow: with ``tiers`` > 1 every selected pixel
        gets one of that many shares of the batch — ``sample_selected(n)`` gives a pixel of tier t ``max(1, n >> t)`` samples —
        and the noise-driven rules (select_noisy, select_error, select_blend_error) pick the smallest share of ``batch`` that
        brings the pixel to the threshold (include/rtpbr.h).  1 (the default): every selected pixel takes the whole batch.
        A selection keeps the tiers it was built with."""
        tiers, batch = int(tiers), int(batch)
        self.set_option("select_tiers", tiers)
        self.set_option("select_batch", batch)
        self.select_tiers = (tiers, batch)

    @property
    def selection_tiers(self):
        """How many pixels of the current selection are in tier 0, 1, ...: a tuple of as many counts as ``set_select_tiers`` last
        set tiers (no synchronisation: the select call brought them to the host)."""
        return tuple(self.counter("select_tier%d" % t) for t in range(self.select_tiers[0]))

    @staticmethod
    def tier_shares(n: int, tiers: int):
        """What ``sample_selected(n)`` gives a pixel of tier 0 .. ``tiers`` - 1: max(1, n >> t), nothing when n is 0."""
        return tuple(max(1, n >> t) if n >= 1 else 0 for t in range(tiers))

    def _selected_samples(self, n_sel, n):
        """the pixel-samples sample_selected(n) traces through the current selection of n_sel pixels"""
        tiers = self.select_tiers[0]
        if tiers == 1:
            return n_sel * n
        return sum(c * s for c, s in zip(self.selection_tiers, self.tier_shares(n, tiers)))

    def select_lattice(self, period=(2, 2), phase=(0, 0), device=False) -> int:
        """Select the pixels with ``x % px == phx and y % py == phy``: one pixel of every ``px`` x ``py`` cell, for sparse frames
        that ``denoise_fill`` completes.  Periods 1..8 per axis, 0 <= phase < period.  Returns how many pixels are selected.
        By default the mask is built on the host and crosses to the device with the call (W * H bytes), which blocks.
        ``device=True``: the library builds the same selection on the device (option ``select_lattice``): one call that
        enqueues one kernel and returns, no copy, no wait; the count is the closed form.  Same state and same samples
        afterwards, bit for bit."""
        (px, py), (phx, phy) = self._lattice_args(period, phase)
        W, H = self.config.width, self.config.height
        if device:
            self.set_option("select_lattice", px + 16 * py + 256 * phx + 4096 * phy)
            return self.lattice_count(W, H, (px, py), (phx, phy))
        return self.select_mask(np.logical_and.outer(np.arange(W) % px == phx, np.arange(H) % py == phy))

    @staticmethod
    def lattice_count(width, height, period, phase) -> int:
        """How many pixels of a ``width`` x ``height`` frame are on the lattice: per axis (extent - phase + period - 1) // period,
        0 where the phase is beyond the frame."""
        def axis(extent, p, ph):
            return (extent - ph + p - 1) // p if ph < extent else 0
        return axis(width, period[0], phase[0]) * axis(height, period[1], phase[1])

    @staticmethod
    def _lattice_args(period, phase):
        try:
            (px, py), (phx, phy) = period, phase
        except (TypeError, ValueError):
            raise ValueError("lattice period and phase are pairs (x, y)") from None
        for v in (px, py, phx, phy):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError("lattice period and phase must be integers")
        if not (1 <= px <= 8 and 1 <= py <= 8):
            raise ValueError(f"lattice period must be 1..8 per axis, got {(px, py)}")
        if not (0 <= phx < px and 0 <= phy < py):
            raise ValueError(f"lattice phase must be 0 <= phase < period, got {(phx, phy)} for period {(px, py)}")
        return (int(px), int(py)), (int(phx), int(phy))

    @staticmethod
    def lattice_phase(frame: int, period=(2, 2)):
        """The phase of frame ``frame`` of a rotating lattice: every pixel of a period cell is visited once per ``px * py`` frames.
        (2, 2): (0,0), (1,1), (1,0), (0,1) — the diagonal first, so that two frames already spread over both axes.  Any other
        period: frame k of a cycle takes cell index j = (k * step) % (px * py), step the smallest integer above px * py / 2
        coprime to px * py (1 when px * py <= 2), as (j % px, j // px): consecutive frames land far apart."""
        (px, py), _ = Renderer._lattice_args(period, (0, 0))
        n = px * py
        k = int(frame) % n
        if (px, py) == (2, 2):
            return ((0, 0), (1, 1), (1, 0), (0, 1))[k]
        step = 1 if n <= 2 else next(s for s in range(n // 2 + 1, 2 * n) if np.gcd(s, n) == 1)
        j = (k * step) % n
        return (j % px, j // px)

    def select_noisy(self, threshold: float, dilate: int = 0) -> int:
        """Select the pixels without samples and those with a pixel noisier than ``threshold`` within ``dilate`` (0..3) pixels
        (Chebyshev distance), from a fresh noise estimate (``noise`` is written).  Returns how many.  Blocks."""
        return self._count("select_noisy", float(threshold), int(dilate))

    def sample_selected(self, n: int = 1):
        """``sample(n)`` through the selected pixels only: every other pixel keeps its bits, the sample index advances by ``n``
        for all of them.  Complete-path form."""
        self.api.call("sample_selected", self._ctx, int(n))
        if self.track_noise:
            self.noise_update()
        if self.track_halves:
            self.half_update()

    def render_adaptive(self, noise: float, max_spp: int, batch_spp: int = 16, dilate: int = 0, per_sample: bool = False, tiers: int = 1):
        """``render_until`` that stops sampling a pixel once it is done: two full-frame batches of ``batch_spp`` (the temporal
        estimate needs two), then select_noisy(noise, dilate) -> sample_selected(batch_spp) -> noise_update() until nothing is
        selected or another batch would take a pixel past ``max_spp``.  Returns (pixel-samples traced, NoiseStats of the last
        estimate).  Continues whatever is accumulated: refresh() first for a new frame.  Stopping a pixel on an estimate made
        from its own samples favours pixels whose batches agree by chance: with ``dilate`` = 0 a pixel whose first two batches
        both missed the light stops there and stays too dark (Cornell v3: five times the display RMSE of render_until);
        ``dilate`` >= 1 keeps the neighbours of a noisy pixel sampling and removes most of it.  The estimator of
        ``set_noise_estimator`` applies: with pooling a pixel that stopped can be selected again in a later round (its
        neighbours' spread counts while it is young), and ``min_samples`` keeps every pixel selected up to that count
        (DESIGN.md 6f).  ``per_sample``: with set_noise_tracking(True) for the duration of the call (restored after): ONE
        full-frame batch, whose ``batch_spp`` samples are that many batches of the estimate, then select_noisy ->
        sample_selected as above without any noise_update().  ``tiers`` > 1: with
        set_select_tiers(tiers, batch_spp) for the duration of the call (restored after): every round gives a selected pixel the
        smallest share ``max(1, batch_spp >> t)`` of the batch that its noise asks for, so one large batch does the work of many
        small ones without overshooting the pixels that were nearly done; a pixel then holds samples
        0 .. share - 1 of every round's ``batch_spp`` indices."""
        if not (batch_spp >= 1 and max_spp >= 1):
            raise ValueError("batch_spp and max_spp must be >= 1")
        batch, budget = int(batch_spp), int(max_spp)
        n_pix = self.config.width * self.config.height
        with self._loop_state(noise_per_sample=per_sample, select_tiers=(int(tiers), batch) if int(tiers) != 1 else None):
            traced, used = 0, 0
            for _ in range(1 if per_sample else 2):
                n = min(batch, budget - used)
                if n <= 0:
                    break
                self.sample(n)
                if not per_sample:
                    self.noise_update()
                traced, used = traced + n_pix * n, used + n
            while used + batch <= budget:
                n_sel = self.select_noisy(noise, dilate)
                if n_sel == 0:
                    break
                self.sample_selected(batch)
                if not per_sample:
                    self.noise_update()
                traced, used = traced + self._selected_samples(n_sel, batch), used + batch
            return traced, self.noise_estimate(noise)

    # ------------------------------------------------------------ the error of the denoised frame (include/rtpbr.h rtpbr_half_update / rtpbr_denoise_error)
    def half_update(self):
        """Deal the samples deposited since the last call to one of two halves: per pixel the half with fewer samples takes the
        batch (half A on a tie, so equal batches alternate).  ``half_buffer`` is half A; half B is ``image_buffer`` minus it.
        The first call's batch is everything accumulated so far."""
        self.api.call("half_update", self._ctx)

    def set_half_mode(self, per_sample: bool = False, warp: bool = False):
        """``per_sample``: from now on sample() and sample_selected() of the complete-path form deal every sample to a half
        themselves, in the pass that adds it to image_buffer: one sample(8) gives halves of 4 + 4, and no half_update() is needed
        (what was deposited before is dealt as one batch by this call; a later half_update() finds nothing new).  Refused by
        sample() in the persistent-ray form, with option precision = 1 and with tiles of world > 1.  ``warp``: reproject() and
        reproject_scene() carry half A with the image instead of zeroing it, so pixels with history stay estimated across a
        move.  Both are off by default and kept across refresh / set_config / set_scene / reproject."""
        m = HalfMode.pack(False, bool(per_sample), bool(warp))
        self.api.call("set_half_mode", self._ctx, C.byref(m))
        self.half_mode = m

    def denoise_error(self, threshold: float = 0.0, radius=None, iterations=None, demodulate=None, sigma_color=None, sigma_normal=None,
                      sigma_depth=None, sigma_albedo=None) -> NoiseStats:
        """Write ``denoised_error``: the estimated standard deviation of the luminance of what ``denoise`` (with the same
        parameters) shows, from the difference of the filter's results on the two halves, averaged over the (2 radius + 1)^2
        window on each pixel's object.  Returns how many pixels have samples in both halves, how many of them are above
        ``threshold``, and the largest value.  Blocks.  Variance only: the filter's bias (blur) is the same in both halves and is
        not seen.  ``denoised_pixels`` is not written.  ``None`` = the library's default for that parameter."""
        p = DenoiseParams.pack(True, iterations, demodulate, sigma_color, sigma_normal, sigma_depth, sigma_albedo)
        return self._stats("denoise_error", _ref(p), _ref(ErrorParams.pack(True, radius)), float(threshold))

    def select_error(self, threshold: float, dilate: int = 0) -> int:
        """select_noisy's counterpart on ``denoised_error`` as the last denoise_error() wrote it (not recomputed): the pixels
        without samples, those with an empty half, those below the estimator's ``min_samples`` and those with a pixel above
        ``threshold`` within ``dilate`` (0..3) pixels.  Returns how many.  Blocks."""
        return self._count("select_error", float(threshold), int(dilate))

    def denoise_blend(self, radius=None, z=None, min_half_samples=None, iterations=None, demodulate=None, sigma_color=None,
                      sigma_normal=None, sigma_depth=None, sigma_albedo=None) -> NoiseStats:
        """Write ``denoised_pixels`` as ``denoise`` (with the same parameters) does, blended per pixel with the raw average where
        the two halves show that the filter's bias outweighs the noise it removes, and ``blend_weight`` (1 = the denoised
        colour, 0 = the raw one).  The statistics are sums over the (2 radius + 1)^2 window on each pixel's object, of pixels
        whose halves both hold ``min_half_samples``; the weight leaves 1 only where the squared bias exceeds ``z`` standard
        errors.  Returns how many pixels had usable halves, how many of them got a weight below 1, and the largest 1 - weight.
        Blocks.  ``None`` = the library's default for that parameter."""
        p = DenoiseParams.pack(True, iterations, demodulate, sigma_color, sigma_normal, sigma_depth, sigma_albedo)
        e = BlendParams.pack(True, radius, z, min_half_samples)
        return self._stats("denoise_blend", _ref(p), _ref(e))

    def _with_blend_fill(self, call):
        """``call()`` with option ``blend_fill`` set; the option is 0 again afterwards, also when the call is refused.  Returns
        (what ``call`` returns, (pixels filled, pixels still empty, the deepest level that filled one))."""
        self.set_option("blend_fill", 1)
        try:
            result = call()
        finally:
            self.set_option("blend_fill", 0)
        return result, tuple(self.counter(k) for k in ("fill_filled", "fill_empty", "fill_deepest"))

    def denoise_blend_levels(self, radius=None, z=None, min_half_samples=None, iterations=None, demodulate=None, sigma_color=None,
                             sigma_normal=None, sigma_depth=None, sigma_albedo=None, fill=False) -> NoiseStats:
        """denoise_blend's rule applied to every a-trous level against the next finer one instead of to the whole filter
        against the raw average: where the halves see a level blurring, that level's increment and every coarser one are scaled
        down, so the filter narrows per pixel and keeps the noise reduction of the levels that hold.  Writes
        ``denoised_pixels``, ``blend_weight`` (the product of the levels' weights: 1 = exactly ``denoise``'s colour) and
        ``blend_depth`` (the sum of the running products, 0..iterations: how many levels were kept).  Same parameters,
        defaults and statistics as denoise_blend.  Blocks.
        ``fill``: with option ``blend_fill`` set for the call (include/rtpbr.h): the three ladders fill their pixels without
        samples as ``denoise_fill`` does, and a pixel without samples that the whole buffer's ladder reached is shown with its
        last level's colour (``blend_weight`` 1, ``blend_depth`` = iterations; one it did not reach stays as post_process shows
        it, depth 0).  The return value is then (the NoiseStats, (pixels filled, pixels still empty, the deepest level that
        filled one))."""
        if fill:
            return self._with_blend_fill(lambda: self.denoise_blend_levels(radius, z, min_half_samples, iterations, demodulate, sigma_color,
                                                                           sigma_normal, sigma_depth, sigma_albedo))
        p = DenoiseParams.pack(True, iterations, demodulate, sigma_color, sigma_normal, sigma_depth, sigma_albedo)
        e = BlendParams.pack(True, radius, z, min_half_samples)
        return self._stats("denoise_blend_levels", _ref(p), _ref(e))

    def blend_error(self, threshold: float = 0.0, radius=None, z=None, min_half_samples=None, window=None, iterations=None,
                    demodulate=None, sigma_color=None, sigma_normal=None, sigma_depth=None, sigma_albedo=None,
                    bias="linear", fill=False) -> NoiseStats:
        """denoise_blend_levels (same parameters, same ``denoised_pixels``, ``blend_weight`` and ``blend_depth``) and besides
        ``blend_error_map``: the estimated root-mean-square error of the luminance of the frame it shows.  The levels' weights
        are applied to each half's own ladder; the difference of the two blended halves gives the variance, the product of their
        (blended - raw) the squared bias the halves can see, both averaged over the (2 ``window`` + 1)^2 window on each pixel's
        object (``window`` = denoise_error's radius).  Returns how many pixels have samples in both halves, how many of them are
        above ``threshold``, and the largest value.  Blocks.  ``None`` = the library's default for that parameter.
        ``bias``: "linear" (the default) averages the squared bias in linear radiance and converts the mean with the slope of the
        tone map at the centre pixel; "display" (rtpbr_blend_error_display) converts each tap's product with the tap's own slope
        before summing, so a saturated pixel in the window no longer lends its linear bias to its neighbours.  Both write
        ``blend_error_map``: the last call wins.
        ``fill``: as denoise_blend_levels' — the frame shows the filled pixels, the estimate still sees them as pixels without
        samples (0 in ``blend_error_map``, selected by select_blend_error); the return value becomes (the NoiseStats, (filled,
        empty, deepest))."""
        if bias not in ("linear", "display"):
            raise ValueError('bias must be "linear" or "display"')
        if fill:
            return self._with_blend_fill(lambda: self.blend_error(threshold, radius, z, min_half_samples, window, iterations, demodulate,
                                                                  sigma_color, sigma_normal, sigma_depth, sigma_albedo, bias))
        entry = "blend_error_display" if bias == "display" else "blend_error"
        if not self.api.has(entry):
            raise NotImplementedError(f"this library has no rtpbr_{entry}")
        p = DenoiseParams.pack(True, iterations, demodulate, sigma_color, sigma_normal, sigma_depth, sigma_albedo)
        e = BlendParams.pack(True, radius, z, min_half_samples)
        return self._stats(entry, _ref(p), _ref(e), _ref(ErrorParams.pack(True, window)), float(threshold))

    # ------------------------------------------------------------ the level blend on the coverage-weighted filter (include/rtpbr.h, option blend_coverage)
    def _with_blend_coverage(self, power, resolve, grid, call):
        """``call()`` with option ``blend_coverage`` set and its three parameters (``None`` = the library's default); the option is
        0 again afterwards, also when the call is refused.  Returns (what ``call`` returns, counter ``blend_resolved``)."""
        cv = CoverageParams.pack(False, grid, power, resolve)
        self.set_option("blend_coverage", 1)
        try:
            for key in ("grid", "power", "resolve"):
                self.set_option("blend_coverage_" + key, getattr(cv, key))
            stats = call()
        finally:
            self.set_option("blend_coverage", 0)
        return stats, self.counter("blend_resolved")

    def denoise_blend_levels_coverage(self, power=None, resolve=None, grid=None, radius=None, z=None, min_half_samples=None, fill=False,
                                      **denoise):
        """``denoise_blend_levels`` (same parameters) on the coverage-weighted filter: the three ladders are ``denoise_coverage``'s
        levels (every tap weighted by (its pixel's own-object coverage)^``power``, at ``grid`` x ``grid`` sub-rays), the windows'
        rule is unchanged, and the pixels that hold two objects are resolved from the blended linear frame (``resolve``) before
        the tone map.  ``blend_weight`` and ``blend_depth`` are the ladder's.  Returns (``denoise_blend_levels``' NoiseStats, the
        pixels the resolve changed).  Blocks.
        ``fill``: with option ``blend_fill`` set for the call: the ladders fill as ``denoise_coverage_fill`` does and the resolve
        treats a filled pixel as one with a colour; the return value becomes (that pair, (filled, empty, deepest))."""
        unknown = set(denoise) - set(DenoiseParams.DEFAULTS)
        if unknown:
            raise TypeError(f"denoise_blend_levels_coverage: unknown denoise parameters {sorted(unknown)}")
        if fill:
            return self._with_blend_fill(lambda: self.denoise_blend_levels_coverage(power, resolve, grid, radius, z, min_half_samples,
                                                                                    **denoise))
        return self._with_blend_coverage(power, resolve, grid, lambda: self.denoise_blend_levels(radius, z, min_half_samples, **denoise))

    def blend_error_coverage(self, threshold: float = 0.0, power=None, resolve=None, grid=None, radius=None, z=None,
                             min_half_samples=None, window=None, bias="linear", fill=False, **denoise):
        """``blend_error`` (same parameters) on the coverage-weighted filter, as ``denoise_blend_levels_coverage``: the same
        ``denoised_pixels``, ``blend_weight`` and ``blend_depth``, and ``blend_error_map`` as the estimate of the blended frame
        BEFORE the resolve.  Returns (``blend_error``'s NoiseStats, the pixels the resolve changed).  Blocks.
        ``fill``: as denoise_blend_levels_coverage's; the return value becomes (that pair, (filled, empty, deepest))."""
        unknown = set(denoise) - set(DenoiseParams.DEFAULTS)
        if unknown:
            raise TypeError(f"blend_error_coverage: unknown denoise parameters {sorted(unknown)}")
        if bias not in ("linear", "display"):
            raise ValueError('bias must be "linear" or "display"')
        if fill:
            return self._with_blend_fill(lambda: self.blend_error_coverage(threshold, power, resolve, grid, radius, z, min_half_samples,
                                                                           window, bias, **denoise))
        return self._with_blend_coverage(power, resolve, grid,
                                         lambda: self.blend_error(threshold, radius, z, min_half_samples, window, bias=bias, **denoise))

    def select_blend_error(self, threshold: float, dilate: int = 0) -> int:
        """select_error's rule on ``blend_error_map`` as the last blend_error() wrote it (not recomputed).  Returns how many
        pixels are selected.  Blocks."""
        return self._count("select_blend_error", float(threshold), int(dilate))

    def render_adaptive_denoised(self, error: float, max_spp: int, batch_spp: int = 4, dilate: int = 1, per_sample: bool = False,
                                 blend=False, *, stop="filter", bias="linear", coverage=None, fill=False, tiers=1, **denoise_params):
        """``render_adaptive`` for a host that shows the DENOISED frame: two full-frame batches of ``batch_spp`` with a
        half_update() after each (both halves hold samples), then denoise_error(error) -> select_error(error, dilate) ->
        sample_selected(batch_spp) -> half_update() until no pixel's estimated denoised noise exceeds ``error`` or another batch
        would take a pixel past ``max_spp``; it ends with denoise(), so ``denoised_pixels`` is the filter of the whole buffer.
        ``denoise_params`` go to both denoise_error and denoise.  Returns (pixel-samples traced, NoiseStats of the last
        estimate).  Continues whatever is accumulated: refresh() first for a new frame.  The estimate is variance only: the
        loop stops when the denoised picture has stopped moving, which the filter's bias does not prevent.
        ``per_sample``: with set_half_mode(per_sample=True) for the duration of the call (``warp`` as it is; restored after):
        every batch is split evenly over the halves by the sample calls themselves and the loop makes no half_update().
        ``blend``: True: the loop ends with denoise_blend() (its defaults) instead of denoise(); "levels": with
        denoise_blend_levels(); the stop rule is unchanged.
        ``stop``: "filter" (the default) is the rule above.  "blend" (with ``blend="levels"`` only) loops on blend_error(error)
        -> select_blend_error(error, dilate) instead: the estimate is the error of the level-blended frame, variance and the
        bias the halves can see, and the call ends with the frame the last blend_error() wrote.
        ``bias`` (with ``stop="blend"`` only): blend_error's ``bias``, "linear" (the default) or "display".
        ``coverage`` (with ``blend="levels"`` only): ``None`` (the default) leaves the loop as it is; True or a dict of
        ``power`` / ``resolve`` / ``grid`` makes the ending denoise_blend_levels() and the blend_error() estimates of
        ``stop="blend"`` the coverage-weighted calls (denoise_blend_levels_coverage, blend_error_coverage).
        ``fill`` (with ``blend="levels"`` only): option ``blend_fill`` is set for the duration of the call, so every level-blend
        call of the loop fills the pixels without samples; the return value becomes ((pixel-samples traced, NoiseStats), (filled,
        empty, deepest) of the last filling call).
        ``tiers`` > 1: with set_select_tiers(tiers, batch_spp) for the duration of the call (restored after), as in
        render_adaptive: the select calls give every selected pixel the smallest share of the batch its estimated error asks for."""
        if isinstance(blend, str) and blend != "levels":
            raise ValueError('blend must be True, False or "levels"')
        if fill:
            if blend != "levels":
                raise ValueError('fill selects the filling level blend: blend must be "levels"')
            return self._with_blend_fill(lambda: self.render_adaptive_denoised(error, max_spp, batch_spp, dilate, per_sample, blend, stop=stop,
                                                                               bias=bias, coverage=coverage, tiers=tiers, **denoise_params))
        if stop not in ("filter", "blend"):
            raise ValueError('stop must be "filter" or "blend"')
        if stop == "blend" and blend != "levels":
            raise ValueError('stop="blend" estimates the level-blended frame: blend must be "levels"')
        if bias not in ("linear", "display"):
            raise ValueError('bias must be "linear" or "display"')
        if bias != "linear" and stop != "blend":
            raise ValueError('bias selects the rule of blend_error(): stop must be "blend"')
        if coverage is not None:
            if coverage is True:
                coverage = {}
            if not isinstance(coverage, dict) or set(coverage) - {"power", "resolve", "grid"}:
                raise ValueError("coverage must be None, True or a dict of power / resolve / grid")
            if blend != "levels":
                raise ValueError('coverage selects the coverage-weighted level blend: blend must be "levels"')
        if not (batch_spp >= 1 and max_spp >= 1):
            raise ValueError("batch_spp and max_spp must be >= 1")
        batch, budget = int(batch_spp), int(max_spp)
        n_pix = self.config.width * self.config.height
        with self._loop_state(halves=True, half_per_sample=per_sample, select_tiers=(int(tiers), batch) if int(tiers) != 1 else None):
            traced, used = 0, 0
            for _ in range(2):
                n = min(batch, budget - used)
                if n <= 0:
                    break
                self.sample(n)
                if not per_sample:
                    self.half_update()
                traced, used = traced + n_pix * n, used + n
            while True:
                if stop == "blend" and coverage is not None:
                    stats = self.blend_error_coverage(error, bias=bias, **coverage, **denoise_params)[0]
                elif stop == "blend":
                    stats = self.blend_error(error, bias=bias, **denoise_params)
                else:
                    stats = self.denoise_error(error, **denoise_params)
                if stats.pixels_above == 0 or used + batch > budget:
                    break
                n_sel = self.select_blend_error(error, dilate) if stop == "blend" else self.select_error(error, dilate)
                self.sample_selected(batch)
                if not per_sample:
                    self.half_update()
                traced, used = traced + self._selected_samples(n_sel, batch), used + batch
            if stop == "blend":
                pass      # (the last blend_error() wrote the frame of the whole buffer)
            elif blend == "levels" and coverage is not None:
                self.denoise_blend_levels_coverage(**coverage, **denoise_params)
            elif blend == "levels":
                self.denoise_blend_levels(**denoise_params)
            elif blend:
                self.denoise_blend(**denoise_params)
            else:
                self.denoise(**denoise_params)
            return traced, stats

    # ------------------------------------------------------------ the present stage (include/rtpbr.h rtpbr_present)
    def present(self, source="pixels", format="rgba8", dither=False):
        """Enqueue the display frame: ``source`` ("pixels" = image_pixels, "denoised" = denoised_pixels, "accum" = the tone map of
        image_buffer, i.e. what post_process() would show, without running it) is clamped, quantised to 8 bit (``dither``: ordered,
        Bayer 8 x 8) and transposed into ``presented``: (H, W, 3 | 4) uint8, top row first — what a window, an encoder or an
        image file takes.  Asynchronous; returns nothing."""
        try:
            p = PresentParams.pack(False, PresentParams.SOURCES[source], PresentParams.FORMATS[format], bool(dither))
        except KeyError as e:
            raise ValueError(f"present: unknown source or format {e.args[0]!r}") from None
        self.api.call("present", self._ctx, C.byref(p))

    def save_image(self, path, source="pixels", dither=False):
        """present(source, "rgb8", dither) and write the frame to ``path`` (any format Pillow knows by the extension): the bytes
        imageio.imwrite(image_pixels, path) writes, without the host's clamp / quantise / transpose."""
        from PIL import Image
        self.present(source, "rgb8", dither)
        Image.fromarray(self.presented).save(path)

    # ------------------------------------------------------------ buffers (field.to_numpy())
    def _shape(self, which):
        W, H = self.config.width, self.config.height
        if which == BUF_PRESENT:      # not a field: (H, W, C) with the last present's C, which the library knows (ESTATE before the first)
            _, n = self.device_ptr(which)
            return (H, W, n // (W * H)), np.uint8
        tail, dt = _TAIL_AND_DTYPE[which]
        return (W, H) + tail, dt

    def _destination(self, which, out):
        """refuse an array that is not a buffer's shape and dtype, C-contiguous"""
        shape, dt = self._shape(which)
        if out.shape != tuple(shape) or out.dtype != np.dtype(dt) or not out.flags.c_contiguous:
            raise ValueError(f"expected a C-contiguous {dt} array of shape {shape}")

    def _read(self, which):
        shape, dt = self._shape(which)
        out = np.empty(shape, dt)
        self.api.call("read_buffer", self._ctx, which, out.ctypes.data_as(C.c_void_p), out.nbytes)
        return out

    def host_array(self, which):
        """A page-locked numpy array of a buffer's shape (rtpbr_host_alloc): the destination a host that shows every frame reads
        into again and again — ``r.read_into(BUF_IMAGE_PIXELS, a)`` or ``r.read_async(BUF_IMAGE_PIXELS, a)``.  The memory
        belongs to the renderer (numpy cannot own page-locked memory): it is released by ``host_release(a)`` or, with every
        other block, by ``close()`` — the array must not be touched after either.  Copy (``a.copy()``) what has to outlive them."""
        shape, dt = self._shape(which)
        n = int(np.prod(shape)) * np.dtype(dt).itemsize
        ptr = C.c_void_p()
        self.api.call("host_alloc", self._ctx, n, C.byref(ptr))
        buf = (C.c_char * n).from_address(ptr.value)
        a = np.frombuffer(buf, dtype=dt).reshape(shape)
        self._host_arrays[ptr.value] = n
        return a

    def host_release(self, arr):
        """Give a host_array() block back (rtpbr_host_free); waits for copies into it.  The array is dead afterwards."""
        addr = arr.ctypes.data
        if addr not in self._host_arrays:
            raise ValueError("not an array of this renderer's host_array()")
        self.api.call("host_free", self._ctx, C.c_void_p(addr))
        del self._host_arrays[addr]

    # ------------------------------------------------------------ the frame without a stall (round 6)
    def device_ptr(self, which):
        """(device address, bytes) of a buffer: zero copy for a consumer on the same GPU — what ``canvas.set_image(image_pixels)``
        does in the reference (src/main.py:64).  Order the consumer behind ``stream()`` (or call ``sync()``)."""
        ptr, n = C.c_void_p(), C.c_size_t()
        self.api.call("buffer_device_ptr", self._ctx, which, C.byref(ptr), C.byref(n))
        return ptr.value, n.value

    def device_array(self, which):
        """The buffer as an object with ``__cuda_array_interface__`` (no copy): ``torch.as_tensor(r.device_array(BUF_IMAGE_PIXELS),
        device="cuda")`` is a tensor ON the renderer's memory."""
        addr, _ = self.device_ptr(which)
        shape, dt = self._shape(which)

        class _DeviceView:
            __cuda_array_interface__ = {"shape": tuple(shape), "typestr": np.dtype(dt).str, "data": (addr, False), "version": 2, "strides": None}
        return _DeviceView()

    def read_async(self, which, out) -> int:
        """Enqueue the copy of a buffer into a ``host_array()`` behind everything enqueued so far and return a ticket at once; the
        renderer's next kernels run while the copy is in flight (only a call that overwrites the buffer waits for it, on the
        device).  ``read_wait(ticket)`` blocks until ``out`` holds the frame."""
        self._destination(which, out)
        t = C.c_int()
        self.api.call("read_buffer_async", self._ctx, which, out.ctypes.data_as(C.c_void_p), out.nbytes, C.byref(t))
        return t.value

    def read_wait(self, ticket: int):
        self.api.call("read_wait", self._ctx, int(ticket))

    def read_into(self, which, out):
        """field.to_numpy() into an array the caller keeps (any C-contiguous array of the buffer's shape and dtype)."""
        self._destination(which, out)
        self.api.call("read_buffer", self._ctx, which, out.ctypes.data_as(C.c_void_p), out.nbytes)
        return out

    def _write(self, which, arr):
        shape, dt = self._shape(which)
        a = np.ascontiguousarray(arr, dtype=dt)
        if a.shape != shape:
            raise ValueError(f"expected shape {shape}, got {a.shape}")
        self.api.call("write_buffer", self._ctx, which, a.ctypes.data_as(C.c_void_p), a.nbytes)

    @property
    def coverage(self):
        """(W,H,4) int32 (n_own, second_object, n_second, n_sub) as the last ``render_coverage`` / ``denoise_coverage`` wrote it"""
        out = np.empty((self.config.width, self.config.height, 4), np.int32)
        self.api.call("read_coverage", self._ctx, out.ctypes.data_as(C.c_void_p), out.nbytes)
        return out

    def ray_depth(self):
        return self.ray_buffer[..., 9].view(np.int32)

    # ------------------------------------------------------------ measurement
    def counters(self) -> Counters:
        c = Counters()
        self.api.call("get_counters", self._ctx, C.byref(c))
        return c

    def counter(self, name: str) -> int:
        """one named work counter of the last sample() call; beyond Counters: "mlp_wave_evals", "mlp_lane_evals"."""
        v = C.c_uint64()
        self.api.call("get_counter", self._ctx, name.encode(), C.byref(v))
        return int(v.value)

    def last_sample_ms(self):
        a, b, n = C.c_float(), C.c_float(), C.c_int()
        self.api.call("last_sample_ms", self._ctx, C.byref(a), C.byref(b), C.byref(n))
        return a.value, b.value, n.value

    def last_primary_ms(self):
        """(device ms of the primary_rays launches of the last sample(), number of launches)."""
        a, n = C.c_float(), C.c_int()
        self.api.call("last_primary_ms", self._ctx, C.byref(a), C.byref(n))
        return a.value, n.value

    # ------------------------------------------------------------ multi-GPU helpers
    def packed_bytes(self) -> int:
        n = C.c_size_t()
        self.api.call("packed_bytes", self._ctx, C.byref(n))
        return n.value

    def pack_tiles(self, device_ptr: int):
        self.api.call("pack_tiles", self._ctx, C.c_void_p(device_ptr))

    def unpack_tiles(self, device_ptr: int, src_rank: int):
        self.api.call("unpack_tiles", self._ctx, C.c_void_p(device_ptr), int(src_rank))

    # RCCL directly, without torch.distributed (include/rtpbr.h "the ONE collective")
    def rccl_unique_id(self) -> bytes:
        buf = C.create_string_buffer(128)
        self.api.call("rccl_unique_id", buf, 128)
        return buf.raw

    def rccl_init(self, unique_id: bytes, rank: int, world: int):
        """collective over all ranks (ncclCommInitRank); rank/world as given to set_tiles"""
        self.api.call("rccl_init", self._ctx, C.c_char_p(unique_id), len(unique_id), int(rank), int(world))

    def gather_tiles(self):
        """collective: pack -> one ncclGather to rank 0 -> rank 0 unpacks, on this context's stream"""
        self.api.call("gather_tiles", self._ctx)

    def rccl_info(self):
        """(ranks in this context's communicator, its rank, RCCL version) as RCCL reports them"""
        n, r, v = C.c_int(), C.c_int(), C.c_int()
        self.api.call("rccl_info", self._ctx, C.byref(n), C.byref(r), C.byref(v))
        return n.value, r.value, v.value

    def stream(self) -> int:
        s = C.c_void_p()
        self.api.call("get_stream", self._ctx, C.byref(s))
        return s.value or 0

    def close(self):
        """rtpbr_destroy: frees the device buffers AND every host_array() block — arrays obtained from host_array() must not be
        used afterwards (their memory is gone)."""
        if self._ctx:
            self.api.call("destroy", self._ctx)
            self._ctx = C.c_void_p()
            self._host_arrays.clear()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _buffer_property(which, writable, doc):
    return property(lambda self: self._read(which), (lambda self, arr: self._write(which, arr)) if writable else None, doc=doc)


for _which, _, _, _, _name, _writable, _doc in BUFFERS:      # r.image_buffer, r.image_pixels, ...: field.to_numpy() (blocking reads)
    setattr(Renderer, _name, _buffer_property(_which, _writable, _doc))
    getattr(Renderer, _name).__set_name__(Renderer, _name)      # (as in a class body: an assignment to a read-only one names it)


def display_image(image_pixels: np.ndarray) -> np.ndarray:
    """(W,H,3) field layout -> (H,W,3) top-down image, the transform ti.tools.imwrite /
    canvas.set_image apply (src/main.py:55)."""
    return np.ascontiguousarray(np.swapaxes(image_pixels, 0, 1)[::-1])
