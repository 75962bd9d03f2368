"""The display stages built since tests/test_gpu_hostile_buffers.py on hostile image buffers on the GPU: rtpbr_denoise with
denoise_fill, rtpbr_denoise_coverage without and with coverage_fill, rtpbr_blend_error / rtpbr_blend_error_display with their
selection, the three blend calls with blend_coverage and blend_fill, and the tiered selections (tests/hostile.py has the inputs,
the case tables, the comparison and the guard; the CPU tier is tests/test_hostile_buffers_ref.py).

Every case makes a fresh context, plants the hostile buffer by the context's own object plane, writes it with
rtpbr_write_buffer(RTPBR_BUF_IMAGE_BUFFER), runs one stage and compares it with that stage's restatement (tests/*_ref/) fed the
device's own planes: its features, half A, moments, image_buffer after the second batch and coverage plane.  The comparison is
hostile.compare(): word for word, NaN against NaN with equal NaN masks; statistics through hostile.compare_stats(), counters as
integers.  No tolerance anywhere.  The coverage guard is asserted on the restatement's output in every case."""
import numpy as np
import pytest

import blend_coverage_ref_lib as bc
import blend_error_ref_lib as be
import blend_fill_ref_lib as bf
import checks as ck
import coverage_fill_ref_lib as cf
import coverage_ref_lib as cl
import feature_ref_lib as fr
import fill_ref_lib as fi
import half_ref_lib as hl
import hostile as hz
import noise_ref_lib as nr
import tier_ref_lib as tr
from raytracingpbr_amd import Renderer

pytestmark = pytest.mark.gpu

DISPLAY_STAGES = ("denoise_fill", "denoise_coverage_fill", "denoise_coverage", "blend_error", "blend_error_display", "blend_coverage",
                  "blend_fill", "blend_fill+coverage")
NAN_SEEN = {}      # (display stage, family) -> words that were NaN on both sides of its frames


def _context(preset, frame):
    """a fresh context with its features rendered, so that the hostile buffer can be planted by object index"""
    w, h = hz.FRAMES[frame]
    scene, cfg = hz.scene_cfg(preset, w, h)
    r = Renderer(scene, cfg)
    r.refresh()
    r.render_features()
    return scene, cfg, r


def _display(stage, family, got, want, image_buffer):
    """a display frame: the guard on the restatement's, the comparison, and the record test_totals reads"""
    hz.guard(stage, want)
    _, nan = hz.compare(stage, got, want, image_buffer)
    key = (stage.split(" ")[0], family)
    assert key[0] in DISPLAY_STAGES
    NAN_SEEN[key] = NAN_SEEN.get(key, 0) + nan


def _plane(stage, got, want, image_buffer):
    hz.guard(stage, want)
    hz.compare(stage, got, want, image_buffer)


def _two_batches(scene, cfg, r, family, lattice, update):
    """The hostile buffer, masked by the lattice where there is one, is written before the first update — everything accumulated
    until then is the first batch — then two samples (through the lattice, built on the device) and a second update.  The inputs
    are proven before the stage is judged: image_buffer against the oracle's second batch.  Returns (batch one, image_buffer now)."""
    w, h = cfg.width, cfg.height
    ib = hz.holes(hz.buffer_for(family, r.feature_object), lattice)
    r.image_buffer = ib
    update()
    if lattice is None:
        r.sample(2)
    else:
        assert r.select_lattice(lattice, device=True) == int(fi.lattice(w, h, lattice).sum())
        r.sample_selected(2)
    update()
    ib2 = r.image_buffer
    hz.compare(f"sample_after_write {family} lattice {lattice}", ib2, hz.second_batch_on_lattice(scene, cfg, ib, lattice), ib)
    return ib, ib2


def _halves(scene, cfg, r, family, lattice):
    """_two_batches with rtpbr_half_update, and half A against half_ref_lib.Halves; returns (image_buffer now, half A)"""
    ib, ib2 = _two_batches(scene, cfg, r, family, lattice, r.half_update)
    a = r.half_buffer
    m = hl.Halves(cfg.width, cfg.height)
    m.update(ib)
    m.update(ib2)
    hz.compare(f"half_update {family} lattice {lattice}", a, m.a, ib)
    if lattice is not None:      # the holes are holes in image_buffer, A and B alike
        off = ~fi.lattice(cfg.width, cfg.height, lattice)
        assert not ib2[off].any() and not a[off].any()
    return ib2, a


def _counters(r):
    return tuple(r.counter(k) for k in ("fill_filled", "fill_empty", "fill_deepest"))


# ------------------------------------------------------------------ (a) the filling denoise, plain and coverage-aware
def _fill(preset, frame, family, lattice, iterations, demodulate):
    scene, cfg, r = _context(preset, frame)
    w, h = cfg.width, cfg.height
    ib = hz.holes(hz.buffer_for(family, r.feature_object), lattice)
    r.image_buffer = ib
    feats = ck.feats(r)
    p = dict(iterations=iterations, demodulate=demodulate, **hz.SIGMAS)
    what = f"{preset} {frame} {family} lattice {lattice} {iterations} levels demodulate {demodulate}"
    reach = fi.reach(ib[..., 3] > 0, feats["object"], iterations)[1]
    counts = r.denoise_fill(**p)
    want, want_counts = fi.denoise_fill(cfg, ib, feats, **p)
    _display("denoise_fill " + what, family, r.denoised_pixels, want, ib)
    assert counts == want_counts == reach == _counters(r), (what, counts, want_counts, reach)
    assert counts[0] > 0 and (lattice is None or iterations < 2 or counts[0] > w * h / 2), (what, counts)
    for resolve in hz.FILL_RESOLVES:
        stats, counts = r.denoise_coverage_fill(resolve=resolve, **p)
        want, want_stats, want_counts = cf.denoise_coverage_fill(cfg, ib, feats, r.coverage, resolve=resolve, **p)
        stage = f"denoise_coverage_fill {what} resolve {resolve}"
        _display(stage, family, r.denoised_pixels, want, ib)
        hz.compare_stats(stage, stats, want_stats)
        assert counts == want_counts == reach == _counters(r), (stage, counts, want_counts, reach)
    # the option off on the same context: nothing of the hostile fill stays behind in the shared ping-pong planes
    r.denoise(**p)
    hz.compare("denoise_after_fill " + what, r.denoised_pixels, fr.denoise(cfg, ib, feats, **p), ib)
    assert _counters(r) == reach                           # ... and the counters still describe the last filling call
    ck.same(r.image_buffer, ib, "image_buffer after the calls")


@pytest.mark.parametrize("frame,family,lattice,iterations,demodulate", hz.FILL_CASES, ids=hz.case_id)
def test_fill(frame, family, lattice, iterations, demodulate):
    _fill("v3", frame, family, lattice, iterations, demodulate)


# ------------------------------------------------------------------ (b) the coverage-aware denoise
def _coverage(preset, frame, family, iterations, demodulate, power, resolve):
    scene, cfg, r = _context(preset, frame)
    ib = hz.buffer_for(family, r.feature_object)
    r.image_buffer = ib
    p = dict(power=power, resolve=resolve, iterations=iterations, demodulate=demodulate, **hz.SIGMAS)
    stats = r.denoise_coverage(**p)
    want, want_stats = cl.denoise_coverage(cfg, ib, ck.feats(r), r.coverage, **p)
    stage = f"denoise_coverage {preset} {frame} {family} {iterations} levels demodulate {demodulate} power {power} resolve {resolve}"
    _display(stage, family, r.denoised_pixels, want, ib)
    hz.compare_stats(stage, stats, want_stats)
    assert want_stats[1] > 0 and (want_stats[0] > 0) == bool(resolve and iterations), (stage, want_stats)


@pytest.mark.parametrize("frame,family,iterations,demodulate,power,resolve", hz.COVERAGE_CASES, ids=hz.case_id)
def test_coverage(frame, family, iterations, demodulate, power, resolve):
    _coverage("v3", frame, family, iterations, demodulate, power, resolve)


# ------------------------------------------------------------------ (c) the blend error, both bias modes, and its selection
def _median(plane):
    return float(np.median(plane[np.isfinite(plane) & (plane > 0)]))


def _blend_error(preset, frame, family, display, radius, z, window, denoise):
    scene, cfg, r = _context(preset, frame)
    w, h = cfg.width, cfg.height
    ib2, a = _halves(scene, cfg, r, family, None)
    feats = ck.feats(r)
    stats = r.blend_error(hz.BLEND_THR, radius, z, 1, window, bias="display" if display else "linear", **denoise)
    want = be.blend_error(cfg, ib2, a, feats, hz.BLEND_THR, radius, z, 1, window, display, **denoise)
    name = "blend_error_display" if display else "blend_error"
    what = f"{preset} {frame} {family} radius {radius} z {z} window {window} {hz.case_id(denoise)}"
    _display(f"{name} {what}", family, r.denoised_pixels, want.denoised, ib2)
    _plane(f"{name}_map {what}", r.blend_error_map, want.error, ib2)
    _plane(f"{name}_weight {what}", r.blend_weight, want.weight, ib2)
    _plane(f"{name}_depth {what}", r.blend_depth, want.depth, ib2)
    hz.compare_stats(f"{name} {what}", stats, want.stats)
    assert want.stats[0] > 0.5 * w * h
    # the selection on the restatement's plane.  At 0.05 nearly everybody is above the threshold (everybody in some cases: the
    # CPU tier has the figures), so `0 < n < W * H` is asked at the median of the restatement's plane
    r.set_noise_estimator(0, 3, hz.TIER_MIN_SAMPLES)
    for thr, dilate in [(hz.BLEND_THR, d) for d in hz.BLEND_DILATES] + [(_median(want.error), 0)]:
        n = r.select_blend_error(thr, dilate)
        mask = hl.select(ib2, a, want.error, thr, dilate, hz.TIER_MIN_SAMPLES)
        hz.compare(f"select_blend_error {what} threshold {thr:g} dilate {dilate}", r.selection, mask, ib2)
        assert n == int(mask.sum()) and 0 < n <= w * h and (n < w * h or thr == hz.BLEND_THR), (what, thr, dilate, n)
    hz.compare(f"{name}_map after the selections, {what}", r.blend_error_map, want.error, ib2)


@pytest.mark.parametrize("frame,family,display,radius,z,window,denoise", hz.BLEND_ERROR_CASES, ids=hz.case_id)
def test_blend_error(frame, family, display, radius, z, window, denoise):
    _blend_error("v3", frame, family, display, radius, z, window, denoise)


# ------------------------------------------------------------------ (d) the three blend calls with blend_coverage / blend_fill
def _blend_call(r, mode, cover, fill, **p):
    """the call of ``mode`` through the Python surface of the options: (NoiseStats, blend_resolved or None, fill counters or None)"""
    if mode == "levels":
        call = r.denoise_blend_levels_coverage if cover else r.denoise_blend_levels
    else:
        call = r.blend_error_coverage if cover else r.blend_error
        p.update(threshold=hz.BLEND_THR, bias=mode)
    got = call(fill=True, **p) if fill else call(**p)
    got, counts = got if fill else (got, None)
    stats, resolved = got if cover else (got, None)
    return stats, resolved, counts


def _blend_options(preset, frame, family, mode, cover, fill, lattice):
    scene, cfg, r = _context(preset, frame)
    w, h = cfg.width, cfg.height
    ib2, a = _halves(scene, cfg, r, family, lattice)
    feats = ck.feats(r)
    cov = None
    if cover:
        r.render_coverage()
        cov = r.coverage
    for denoise in hz.BLEND_OPTION_DENOISE:
        K = denoise.get("iterations", 4)
        if fill:
            want = bf.blend_fill(cfg, ib2, a, feats, cov, mode, threshold=hz.BLEND_THR, **hz.BLEND_OPTION_RULE, **denoise)
            name = "blend_fill+coverage" if cover else "blend_fill"
        else:
            want = bc.blend_coverage(cfg, ib2, a, feats, cov, mode, threshold=hz.BLEND_THR, **hz.BLEND_OPTION_RULE, **denoise)
            name = "blend_coverage"
        stats, resolved, counts = _blend_call(r, mode, cover, fill, **hz.BLEND_OPTION_RULE, **denoise)
        what = f"{preset} {frame} {family} {mode} lattice {lattice} {hz.case_id(denoise)}"
        _display(f"{name} {what}", family, r.denoised_pixels, want.denoised, ib2)
        _plane(f"{name}_weight {what}", r.blend_weight, want.weight, ib2)
        _plane(f"{name}_depth {what}", r.blend_depth, want.depth, ib2)
        if want.error is not None:
            _plane(f"{name}_map {what}", r.blend_error_map, want.error, ib2)
        hz.compare_stats(f"{name} {what}", stats, want.stats)
        assert not np.isnan(want.weight).any() and np.all((want.weight >= 0) & (want.weight <= 1))
        assert not np.isnan(want.depth).any() and np.all((want.depth >= 0) & (want.depth <= K))
        if cover:
            assert resolved == want.resolved == r.counter("blend_resolved") and resolved > 0, (what, resolved, want.resolved)
        if fill:
            reach = fi.reach(ib2[..., 3] > 0, feats["object"], K)[1]
            assert counts == want.counts == reach == _counters(r), (what, counts, want.counts, reach)
            assert counts[0] > 0 and (lattice is None or counts[0] > w * h / 2), (what, counts)
    ck.same(r.image_buffer, ib2, "image_buffer after the calls")
    ck.same(r.half_buffer, a, "half A after the calls")


@pytest.mark.parametrize("frame,family,mode,cover,fill,lattice", hz.BLEND_OPTION_CASES, ids=hz.case_id)
def test_blend_options(frame, family, mode, cover, fill, lattice):
    _blend_options("v3", frame, family, mode, cover, fill, lattice)


# ------------------------------------------------------------------ (e) family N under the tone map that shows a NaN
def test_family_n_reaches_the_display_as_nan_under_preset_v2():
    """hostile.NAN_*: preset v3 (tone-map order 0) shows a NaN as 0, preset v2 lets it through.  One case per display stage."""
    for case in hz.NAN_FILL_CASES:
        _fill(hz.NAN_PRESET, *case)
    for case in hz.NAN_COVERAGE_CASES:
        _coverage(hz.NAN_PRESET, *case)
    for case in hz.NAN_BLEND_ERROR_CASES:
        _blend_error(hz.NAN_PRESET, *case)
    for case in hz.NAN_BLEND_OPTION_CASES:
        _blend_options(hz.NAN_PRESET, *case)


# ------------------------------------------------------------------ (f) the tiered selections
@pytest.mark.parametrize("family,call,thr,tiers,batch,dilate", hz.TIER_CASES, ids=hz.case_id)
def test_tiers(family, call, thr, tiers, batch, dilate):
    scene, cfg, r = _context("v3", "97x61")
    w, h = cfg.width, cfg.height
    what = f"{family} threshold {thr} ({tiers},{batch}) dilate {dilate}"
    if call == "noisy":
        ib, ib2 = _two_batches(scene, cfg, r, family, None, r.noise_update)
    else:
        ib2, a = _halves(scene, cfg, r, family, None)
    feats = ck.feats(r)
    r.set_noise_estimator(0, 3, hz.TIER_MIN_SAMPLES)
    r.set_select_tiers(tiers, batch)
    try:
        # the device's own plane, itself compared with its restatement first
        if call == "noisy":
            M = r.moments
            t = nr.Tracker(w, h)
            t.update(ib)
            t.update(ib2)
            hz.compare(f"noise_update {what}", M, t.moments, ib)
            n = r.select_noisy(thr, dilate)
            plane, half_count = r.noise, None
            want_plane = nr.estimate(ib2, M, feats["object"], thr)[0]
        elif call == "error":
            r.denoise_error(thr, **hz.TIER_DENOISE)
            n = r.select_error(thr, dilate)
            plane, half_count = r.denoised_error, a[..., 3]
            want_plane = hl.denoise_error(cfg, ib2, a, feats, threshold=thr, **hz.TIER_DENOISE)[0]
        else:
            r.blend_error(thr, **hz.TIER_BLEND, **hz.TIER_DENOISE)
            n = r.select_blend_error(thr, dilate)
            plane, half_count = r.blend_error_map, a[..., 3]
            want_plane = be.blend_error(cfg, ib2, a, feats, thr, **hz.TIER_BLEND, **hz.TIER_DENOISE).error
        _plane(f"select_{call}_plane {what}", plane, want_plane, ib2)
        want = tr.select(plane, ib2[..., 3], thr, dilate, tiers, batch, hz.TIER_MIN_SAMPLES, half_count)
        sel = r.selection
        hz.compare(f"select_{call}_tiers {what}", sel, want, ib2)
        counts = tr.counts(want, tiers)
        assert r.selection_tiers == counts and n == sum(counts) and 0 < n <= w * h, (what, r.selection_tiers, counts, n)
        if thr == 0.0:
            assert sum(counts[1:]) == 0                    # r is infinite: every selected pixel is tier 0
        elif dilate == 0 and (tiers, batch) != (2, 1):
            assert min(counts) > 0, (what, counts)         # the comparison was not of empty sets
        if (tiers, batch, thr, dilate) == (4, 16, hz.TIER_THR, 0):
            # one traced launch: every pixel's count word gains exactly its tier's share where the old count is an ordinary number
            # (finite and below 2^20: the sum is exact); unselected pixels keep their bits, NaN and infinite ones included
            r.sample_selected(4)
            after = r.image_buffer
            share = np.array((0,) + tr.shares(4, tiers), np.float32)[want]
            ordinary = np.isfinite(ib2[..., 3]) & (np.abs(ib2[..., 3]) < 2.0 ** 20)
            assert (ordinary & (want != 0)).sum() > 0.9 * n
            assert np.array_equal(after[..., 3][ordinary] - ib2[..., 3][ordinary], share[ordinary])
            assert np.array_equal(ck.bits(after)[want == 0], ck.bits(ib2)[want == 0])
            odd = ~ordinary & (want == 0)
            assert odd.any() or call != "noisy"            # (select_noisy leaves 2^24, 1e30, +inf and FLT_MAX counts out: they kept their bits)
            c = r.counters()
            assert c.samples == c.deposits == tr.traced(4, counts), (what, c.samples, c.deposits)
    finally:
        r.set_select_tiers()


# ------------------------------------------------------------------ (g) the record of the run
def test_totals():
    """per stage the words compared and the words that were NaN on both sides (runs last in this file).  Family N must have put NaN
    words on both sides of every display stage's frames: otherwise the non-finite family never reached the output."""
    assert hz.TOTALS
    for stage, (words, nan) in sorted(hz.TOTALS.items()):
        print(f"[hostile] total {stage}: {words} words compared, {nan} NaN on both sides")
    for stage in DISPLAY_STAGES:
        for family in hz.FAMILIES:
            print(f"[hostile] total {stage} frames, family {family}: {NAN_SEEN.get((stage, family), 0)} NaN on both sides")
    for stage in DISPLAY_STAGES:
        assert NAN_SEEN.get((stage, "N"), 0) > 0, f"{stage}: no NaN word of family N reached its frames"
