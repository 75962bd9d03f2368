"""Test helper: hostile image buffers for the stages built on image_buffer (tone map, a-trous, noise estimate, pooling, selection,
the reprojections, the two-half error), their placement, the one comparison the hostile tests use and the coverage guard.

include/rtpbr.h accepts any words in RTPBR_BUF_IMAGE_BUFFER (rtpbr_write_buffer is a supported input) and makes promises for the
special ones: "count > 0 is false" is the no-samples test, fmaxf turns NaN into 0, exp(-min(e, 80)) never sees a lost argument,
the statistics' maximum is an unsigned one over bit patterns >= +0.  The rendered buffers of the other GPU tests never reach those
clauses; these do.

Two families, both planted on a seeded pseudo-random base (gamma-distributed radiance times the count, count 4):

  F  finite: the zeros, denormals, FLT_MIN, 1e30, negative radiance, per-sample means of exactly -1 (the pole of r(c) = c / (1 + c))
     and of its two float32 neighbours in colour words; denormal, fractional, 2^24, 1e30, +0, -0 and -3 in count words (the last
     three are "no samples").  A special count carries radiance * count as its colour, so its mean is an ordinary radiance.
     About 4 % of the pixels drawn over the frame, the whole column x = 0, the whole row y = H - 1 (every tap offset and both
     edges meet a special value), and at least one pixel on every object index of the frame.
     The colour word 1e30 stands on the objects of family N only (bright_objects() says why).
  N  non-finite: NaN, +inf, -inf and FLT_MAX in colour and in count words, confined to the two smallest objects that own at
     least 40 pixels (n_objects()): taps never cross object indices, so the damage stays there.

compare() is word for word on uint32 except where both sides are NaN (the sign and payload of a generated NaN are unspecified:
x86 makes the negative quiet NaN, gfx950 the positive one); the NaN masks themselves must be equal.
guard() is a condition on the inputs, asserted on the RESTATEMENT's output: at most 10 % of the pixels may be wiped (all three
display words 0 or NaN; NaN for a scalar output) — otherwise the comparison would compare nothing."""
import numpy as np

from raytracingpbr_amd import Config, cornell_box

F32 = np.float32
W, H = 97, 61            # partial 256-lane blocks, H no multiple of 64: the size of the denoise, noise and reproject tests
SMALL = (7, 5)           # smaller than the 5x5 tap window at step 2, than the radius-3 window and than the pool tile
FRAMES = {"97x61": (W, H), "7x5": SMALL}
PRESETS = ("v3", "v2")   # tone-map order 0 turns NaN into 0 (the final clamp); order 1 lets NaN through to the display
FAMILIES = ("F", "N")
WIPED_MAX = 0.10
SIGMAS = dict(sigma_color=0.5, sigma_normal=0.3, sigma_depth=0.05, sigma_albedo=0.1)      # test_denoise_bit_identical_to_reference
FLT_MIN, FLT_MAX = F32(np.finfo(F32).tiny), F32(np.finfo(F32).max)
_M1 = F32(-1.0)
COUNT = F32(4.0)

# ---- the special words.  ("c", word): a colour word beside count 4 (so word / 4 is the per-sample mean, exactly);
#      ("n", word): a count word, the colour becomes radiance * count.
# The order is the one the edges cycle through; it spreads the kinds that wipe their own pixel under Cornell v3's tone map (a
# negative mean makes pow() NaN, the ACES matrix mixes it into all three channels and the clamp shows 0) so that the first
# eleven — all the 7 x 5 frame's column and row hold — contain two of them, and puts radiance -100, which also drags its
# neighbours' averages below zero, last.
F_KINDS = (
    ("n", F32(0.5)), ("c", F32(1e-45)), ("c", _M1 * COUNT), ("n", F32(2.0 ** 24)), ("c", F32(0.0)), ("n", F32(-0.0)),
    ("c", F32(1e30)), ("n", F32(1e-40)), ("c", FLT_MIN), ("n", F32(-3.0)), ("c", F32(1e-40)), ("n", F32(1e30)),
    ("c", F32(-0.0)), ("n", F32(1e-45)), ("c", np.nextafter(_M1, F32(0)) * COUNT), ("n", F32(0.0)), ("c", F32(-1e-3) * COUNT),
    ("c", np.nextafter(_M1, F32(-2)) * COUNT), ("c", F32(-100.0) * COUNT),
)
# how often the pixels drawn over the frame take each kind: radiance -100 wipes a 5 x 5 neighbourhood under preset v3, so it is rare
F_WEIGHTS = np.array([1.0] * (len(F_KINDS) - 1) + [0.15])
N_VALUES = (F32(np.nan), F32(np.inf), F32(-np.inf), FLT_MAX)


def scene_cfg(preset, w=W, h=H):
    """cornell_box("v3") with Config.cornell_v3 (tone-map order 0), cornell_box("v2") with Config.cornell_v2 (order 1)"""
    if preset == "v3":
        return cornell_box("v3", aspect=w / h), Config.cornell_v3(w, h, 0, 3)
    assert preset == "v2"
    return cornell_box("v2", aspect=w / h), Config.cornell_v2(w, h, 1, 3)


def base_buffer(w, h, seed=0):
    """(image_buffer (w,h,4), radiance (w,h,3)): gamma-distributed radiance times the count, count 4"""
    rng = np.random.default_rng(1000 + seed)
    rad = rng.gamma(2.0, 0.25, (w, h, 3)).astype(F32)
    ib = np.empty((w, h, 4), F32)
    ib[..., :3] = rad * COUNT
    ib[..., 3] = COUNT
    return ib, rad


BRIGHT = 6      # F_KINDS[BRIGHT] = the colour word 1e30 (see bright_objects)
assert F_KINDS[BRIGHT] == ("c", F32(1e30))


def _put(ib, rad, x, y, k, mask, bright_ok=True):
    if k == BRIGHT and not bright_ok:
        k = k + 1
    what, word = F_KINDS[k]
    if what == "c":
        for c in range(3):
            if mask >> c & 1:
                ib[x, y, c] = word
    else:
        ib[x, y, :3] = rad[x, y] * word
        ib[x, y, 3] = word


def family_f(obj, seed=0):
    """the finite-hostile buffer for a frame whose first-hit object indices are `obj` (W,H) int32; returns (image_buffer, planted
    mask)"""
    w, h = obj.shape
    ib, rad = base_buffer(w, h, seed)
    rng = np.random.default_rng(2000 + seed)
    planted = np.zeros((w, h), bool)
    bright = np.isin(obj, bright_objects(obj))
    edge = [(0, y) for y in range(h)] + [(x, h - 1) for x in range(1, w)]
    for k, (x, y) in enumerate(edge):
        _put(ib, rad, x, y, k % len(F_KINDS), 1 + k % 7, bright[x, y])
        planted[x, y] = True
    inner = [(x, y) for x in range(1, w) for y in range(h - 1)]
    pick = rng.permutation(len(inner))[:max(1, round(0.04 * w * h))]
    kinds = rng.choice(len(F_KINDS), len(pick), p=F_WEIGHTS / F_WEIGHTS.sum())
    # one channel mostly, two sometimes, all three rarely: a pixel hostile in every channel shows nothing to compare
    masks = rng.choice([1, 2, 4, 3, 5, 6, 7], len(pick), p=[0.22, 0.22, 0.22, 0.08, 0.08, 0.08, 0.10])
    for j, k, m in zip(pick, kinds, masks):
        x, y = inner[j]
        _put(ib, rad, x, y, int(k), int(m), bright[x, y])
        planted[x, y] = True
    xs, ys = np.nonzero(bright & ~planted)      # the colour word 1e30 itself, wherever the draw put none
    j = int(rng.integers(len(xs)))
    _put(ib, rad, xs[j], ys[j], BRIGHT, 1 << int(rng.integers(3)))
    planted[xs[j], ys[j]] = True
    for o in np.unique(obj):            # every object index of the frame, the miss index -1 included
        on = obj == o
        if not (planted & on).any():
            xs, ys = np.nonzero(on)
            j = int(rng.integers(len(xs)))
            _put(ib, rad, xs[j], ys[j], int(rng.integers(len(F_KINDS) - 1)), 1 << int(rng.integers(3)), bright[xs[j], ys[j]])
            planted[xs[j], ys[j]] = True
    return ib, planted


def n_objects(obj):
    """The two smallest objects that own at least 40 pixels: smallest by the pixels they own (ties: the lower index).  Read as
    "lowest index" the rule picks the miss index and object 0 of the Cornell frames, 13.4 % of 97 x 61 — a filter of three
    levels or more turns a whole object NaN, and the 10 % guard could not hold."""
    ids, cnt = np.unique(obj, return_counts=True)
    big = sorted((int(c), int(i)) for i, c in zip(ids, cnt) if c >= 40)
    return [i for _, i in big[:2]]


def bright_objects(obj):
    """where a colour word of 1e30 may stand: n_objects(obj), or the object with the fewest pixels in a frame that has no object of
    40.  A mean of 2.5e29 is finite but no edge stops it: r(c) saturates at 1, so the colour weight to an ordinary neighbour stays
    near exp(-2) and the average of everything within reach becomes ~1e27 — after five levels the whole object shows (1, 1, 1)
    under tone-map order 0 and NaN under order 1 (x * x overflows in the ACES fit).  Confined like family N it costs one small
    object; everywhere else the kind is replaced by the next one of F_KINDS."""
    n = n_objects(obj)
    if n:
        return n
    ids, cnt = np.unique(obj, return_counts=True)
    return [int(ids[int(np.argmin(cnt))])]


def family_n(obj, seed=0):
    """the non-finite buffer: NaN, +inf, -inf and FLT_MAX in colour words (count 4) and in count words (the base colour), on
    5 % of the pixels (at least 8: every value both ways) of each of n_objects(obj)"""
    w, h = obj.shape
    ib, _ = base_buffer(w, h, seed)
    rng = np.random.default_rng(3000 + seed)
    planted = np.zeros((w, h), bool)
    for o in n_objects(obj):
        xs, ys = np.nonzero(obj == o)
        pick = rng.permutation(len(xs))[:max(8, round(0.05 * len(xs)))]
        for j, p in enumerate(pick):
            x, y, v = xs[p], ys[p], N_VALUES[j % 4]
            if (j // 4) % 2 == 0:
                for c in range(3):
                    if (1 + j % 7) >> c & 1:
                        ib[x, y, c] = v
            else:
                ib[x, y, 3] = v
            planted[x, y] = True
    return ib, planted


def buffer_for(family, obj, seed=0):
    return (family_f if family == "F" else family_n)(np.ascontiguousarray(obj), seed)[0]


# ---------------------------------------------------------------- the comparison
def _words(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a


def _hex(v):
    return "[" + " ".join(f"{int(b):08x}" for b in np.atleast_1d(_words(np.asarray(v))).reshape(-1)) + "]"


TOTALS = {}      # stage -> [words compared, words NaN on both sides]


def compare(stage, got, want, image_buffer=None):
    """Word for word as uint32, except where both sides are NaN; the NaN masks must be equal.  The message names the stage, the
    first differing pixels, their input words and both outputs.  Returns (words compared, words NaN on both sides) and prints
    them as a [hostile] line."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{stage}: {got.shape} {got.dtype} against {want.shape} {want.dtype}"
    if got.dtype.kind == "f":
        gn, wn = np.isnan(got), np.isnan(want)
        both = gn & wn
        bad = (gn != wn) | ((_words(got) != _words(want)) & ~both)
    else:
        both = np.zeros(got.shape, bool)
        bad = got != want
    if bad.any():
        px = bad.reshape(bad.shape[0], bad.shape[1], -1).any(axis=2)
        lines = []
        for x, y in np.argwhere(px)[:4]:
            inp = "" if image_buffer is None else f" input {_hex(image_buffer[x, y])}"
            lines.append(f"  ({x},{y}){inp} got {_hex(got[x, y])} want {_hex(want[x, y])}")
        raise AssertionError(f"{stage}: {int(bad.sum())} words of {bad.size} differ on {int(px.sum())} pixels\n" + "\n".join(lines))
    t = TOTALS.setdefault(stage.split(" ")[0], [0, 0])
    t[0] += got.size
    t[1] += int(both.sum())
    print(f"[hostile] {stage}: {got.size} words compared, {int(both.sum())} NaN on both sides")
    return got.size, int(both.sum())


def compare_stats(stage, stats, want):
    """rtpbr_noise_stats against the restatement's (pixels_estimated, pixels_above, max_noise): the maximum by its bits"""
    got = (int(stats.pixels_estimated), int(stats.pixels_above), int(F32(stats.max_noise).view(np.uint32)))
    exp = (int(want[0]), int(want[1]), int(F32(want[2]).view(np.uint32)))
    assert got == exp, f"{stage}: statistics (estimated, above, bits of max) {got} against {exp}"


# ---------------------------------------------------------------- the coverage guard
def wiped_display(out):
    """share of the pixels whose three display words are all 0 or NaN"""
    out = np.asarray(out)
    return float(((out == 0) | np.isnan(out)).all(axis=2).mean())


def wiped_scalar(out):
    """share of the pixels whose single word is NaN"""
    return float(np.isnan(np.asarray(out)).mean())


def guard(stage, ref_out):
    """Asserted on the restatement's output in every parametrised case: at most 10 % of the pixels are wiped."""
    ref_out = np.asarray(ref_out)
    share = wiped_display(ref_out) if ref_out.ndim == 3 and ref_out.shape[2] == 3 else \
        wiped_scalar(ref_out) if ref_out.ndim == 2 else float(np.isnan(ref_out).any(axis=2).mean())
    assert share <= WIPED_MAX, f"{stage}: {share:.1%} of the pixels are wiped in the restatement's output: the inputs leave nothing to compare"
    return share


# ---------------------------------------------------------------- the cases, shared by the CPU and the GPU file
DENOISE_CASES = [(preset, family, it, demod) for preset in PRESETS for family in FAMILIES for it in (0, 1, 2, 3, 5) for demod in (0, 1)]
TONEMAP_CASES = [(family, order, trunc) for family in FAMILIES for order in (0, 1, 2, 3) for trunc in (0, 1)]
THRESHOLDS = (0.0, 0.05, float("inf"))
GUIDED_CASES = [(family, it, demod, 1e-5) for family in FAMILIES for it in (1, 2, 4) for demod in (0, 1)]
GUIDED = dict(sigma_color=2.0, sigma_normal=0.3, sigma_depth=0.05)      # test_guided_levels_and_demodulation


def smallest_floor(sigma_color):
    """the smallest variance_floor rtpbr_denoise_guided accepts beside this sigma_color: finite, > 0 and 1 / (sigma_color^2 floor)
    does not overflow (include/rtpbr.h, the errors of the noise section), found by bisection over the bit patterns (the
    condition is monotone).  For sigma_color = 2 it is a denormal, 2^-130 + 2^-149."""
    sc2 = F32(sigma_color) * F32(sigma_color)
    ok = lambda bits: bool(np.isfinite(F32(1) / (sc2 * np.uint32(bits).view(F32))))      # noqa: E731
    lo, hi = 0, int(F32(1).view(np.uint32))          # lo fails (floor 0), hi passes
    with np.errstate(all="ignore"):
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if ok(mid) else (mid, hi)
    return float(np.uint32(hi).view(F32))


GUIDED_CASES += [(family, 2, 0, smallest_floor(GUIDED["sigma_color"])) for family in FAMILIES]
REPROJECT_CASES = [(family, move, mh, nc) for family in FAMILIES for move in ("translate", "yaw") for mh in (64.0, 2.0) for nc in (-1.0, 0.9)]
BOX_MOVE = {6: ((0.08, 0.0, 0.05), (0, 0, 0))}      # Cornell's small box, translated (test_gpu_reproject_scene.py)


def moves():
    import test_gpu_reproject as rp      # the move definitions of the reproject tests
    return rp.MOVES


def second_batch(scene, cfg, image_buffer, n=2):
    """image_buffer after rtpbr_sample(n) on a fresh context that was written `image_buffer` first — from the oracle, which the
    sample kernels are held to bit for bit"""
    from oracle_backend import OracleRenderer
    o = OracleRenderer(scene, cfg)
    o.image_buffer = image_buffer
    o.sample(n)
    out = o.image_buffer
    o.close()
    return out


def tonemap_cfg(cfg, order, trunc):
    return cfg.copy(tonemap_order=order, aces_truncated=trunc)


def oracle_post_process(scene, cfg, image_buffer):
    """image_pixels of the oracle's post_process() on this image_buffer"""
    from oracle_backend import OracleRenderer
    o = OracleRenderer(scene, cfg)
    o.image_buffer = image_buffer
    o.post_process()
    out = o.image_pixels
    o.close()
    return out


# ---------------------------------------------------------------- the stages since: fill, coverage, blend error, blend options, tiers
# Frames 97x61 with both families and 7x5 with family F (family N needs an object of 40 pixels); scene and config are
# scene_cfg("v3", w, h); the sigmas are SIGMAS wherever a case does not say "defaults".
FRAME_FAMILIES = (("97x61", "F"), ("97x61", "N"), ("7x5", "F"))
LATTICES = (None, (2, 2), (4, 4))      # None: the only holes are the hostile counts +0, -0, -3 and NaN
BLEND_THR = 0.05                       # threshold of the blend-error cases and of their select_blend_error
TIER_MIN_SAMPLES = 3                   # the estimator's min_samples of the tier cases: "fewer than min_samples" is on


def lattices_of(frame):
    """on 7x5 a lattice wipes 23 - 51 % of the restatement's output (the guard is 10 %): that frame runs without one"""
    return LATTICES if frame == "97x61" else (None,)


def holes(image_buffer, lattice):
    """the hostile buffer with holes cut: everything off the lattice (phase (0, 0)) is zero, as sample_selected leaves it on a
    refreshed context.  Column x = 0 and row y = H - 1 = 60 keep every second (fourth) pixel of the planted edge."""
    import fill_ref_lib as fi
    if lattice is None:
        return np.array(image_buffer, dtype=F32)
    w, h = image_buffer.shape[:2]
    return fi.masked(image_buffer, fi.lattice(w, h, lattice))


def second_batch_on_lattice(scene, cfg, image_buffer, lattice, n=2):
    """second_batch() where only the lattice was selected: what select_lattice + sample_selected(n) leave (the other pixels keep
    their bits)"""
    import fill_ref_lib as fi
    out = second_batch(scene, cfg, image_buffer, n)
    if lattice is None:
        return out
    w, h = image_buffer.shape[:2]
    return np.where(fi.lattice(w, h, lattice)[..., None], out, np.asarray(image_buffer, F32))


# (frame, family, lattice, iterations, demodulate): denoise_fill, and denoise_coverage_fill at the default grid and power with
# resolve 0 and 1
FILL_CASES = [(frame, family, lattice, it, demod) for frame, family in FRAME_FAMILIES for lattice in lattices_of(frame)
              for it in (1, 2, 4) for demod in (0, 1)]
FILL_RESOLVES = (0, 1)
# (frame, family, iterations, demodulate, power, resolve)
COVERAGE_CASES = [(frame, family, it, demod, power, resolve) for frame, family in FRAME_FAMILIES for it in (0, 1, 3) for demod in (0, 1)
                  for power in (0, 4) for resolve in (0, 1)]
# (radius, z, denoise parameters): the rule tuples of test_gpu_levels.py::test_hostile_image_buffer; min_half_samples = 1
BLEND_RULES = ((1, 0.0, {}), (3, 0.0, dict(iterations=2, demodulate=1, **SIGMAS)), (3, 2.0, {}), (2, 0.0, dict(iterations=0)))
BLEND_WINDOWS = (None, 1, 3)
BLEND_DILATES = (0, 2)
# (frame, family, display, radius, z, window, denoise); each is followed by select_blend_error(BLEND_THR, dilate in BLEND_DILATES)
BLEND_ERROR_CASES = [(frame, family, display, radius, z, window, denoise) for frame, family in FRAME_FAMILIES for display in (False, True)
                     for radius, z, denoise in BLEND_RULES for window in BLEND_WINDOWS]
BLEND_MODES = ("levels", "linear", "display")
BLEND_OPTION_DENOISE = ({}, dict(iterations=3, **SIGMAS))      # both run in every case
BLEND_OPTION_RULE = dict(radius=2, z=0.0, min_half_samples=1)
# (frame, family, mode, coverage, fill, lattice)
BLEND_OPTION_CASES = [(frame, family, mode, cover, fill, lattice) for frame, family in FRAME_FAMILIES for mode in BLEND_MODES
                      for cover, fill in ((1, 0), (0, 1), (1, 1)) for lattice in (lattices_of(frame)[:2] if fill else (None,))]
# (family, call, threshold, tiers, batch, dilate) on 97x61.  Threshold 0.125 puts pixels into every tier for all three calls in
# both families (asserted on the restatements, tests/test_hostile_buffers_ref.py); at threshold 0 every selected pixel is tier 0.
TIER_CALLS = ("noisy", "error", "blend_error")
TIER_THR = 0.125
TIER_CASES = [(family, call, thr, tiers, batch, dilate) for family in FAMILIES for call in TIER_CALLS for thr in (0.0, TIER_THR)
              for tiers, batch in ((4, 16), (8, 256), (2, 1)) for dilate in (0, 2)]
# The planes the error calls select on: denoise_error(window 2) and blend_error(radius 2, z 0, min_half_samples 1, window 2) of
# the 2-level demodulated filter.  Measured on the restatements at (8, 256), threshold 0.125, dilate 0: family F (182, 19, 15,
# 474, 3353, 1635, 108, 38) and (182, 19, 16, 384, 3479, 1637, 102, 29), family N (12, 29, 27, 863, 3289, 1391, 33, 4) and (12,
# 29, 27, 677, 3475, 1389, 35, 4).  (With the default filter, 4 levels at sigma_color 2, family N's denoise_error plane leaves tier
# 2 empty at 0.125, and tiers 1 and 3 at its median 0.16203: the filter's parameters were changed, not the threshold.)
TIER_DENOISE = dict(iterations=2, demodulate=1, **SIGMAS)
TIER_BLEND = dict(radius=2, z=0.0, min_half_samples=1)


# Preset v3's tone map (order 0) clamps last and shows a NaN as 0: in the tables above family N reaches the display as wiped pixels,
# compared word for word as zeros.  One family-N case per display stage under preset v2 (order 1: a NaN gets through) puts the
# NaN words themselves on both sides of the comparison; test_totals of the GPU file asks for them.
NAN_PRESET = "v2"
NAN_FILL_CASES = [("97x61", "N", (2, 2), 2, 0)]
NAN_COVERAGE_CASES = [("97x61", "N", 3, 0, 4, 1)]
NAN_BLEND_ERROR_CASES = [("97x61", "N", display, 3, 0.0, None, BLEND_RULES[1][2]) for display in (False, True)]
NAN_BLEND_OPTION_CASES = [("97x61", "N", "levels", 1, 0, None), ("97x61", "N", "display", 1, 1, (2, 2)), ("97x61", "N", "linear", 0, 1, None)]


def case_id(v):
    """pytest ids of the case tuples: a dict of denoise parameters by its levels"""
    if isinstance(v, dict):
        return "defaults" if not v else f"K{v.get('iterations', 4)}" + ("d" if v.get("demodulate") else "")
    if isinstance(v, tuple):
        return "x".join(str(x) for x in v)
    return str(v)
