"""The tiered selection on the GPU (options select_tiers / select_batch; include/rtpbr.h).  Every comparison is ``==`` on bit
patterns: the selection against the numpy restatement of the tier rule (tests/tier_ref_lib.py) on the GPU's own planes, a tiered
launch against image buffers composed from the unchanged CPU oracle — per stage of the plan, full-frame samples at the stage's
sample base, ``np.where(tier <= t, after, before)`` — and against the same stages made with plain calls on a second Renderer."""
import numpy as np
import pytest

import checks as ck
import select_ref_lib as sr
import test_gpu_reproject as rp
import tier_ref_lib as tr
from cases import all_cases
from checks import ESTATE
from oracle_backend import OracleRenderer
from raytracingpbr_amd import Config, Renderer, cornell_box

pytestmark = pytest.mark.gpu


def _small_cases():
    """every complete-path case of tests/cases.py, 40 pixels wide"""
    out = {}
    for c in all_cases():
        if c.cfg.kernel_form == 0:
            h = max(8, round(c.cfg.height * 40 / c.cfg.width))
            out[c.name] = (c, c.cfg.copy(width=40, height=h))
    return out


CORNELL = "c1_cornell_v3_256_16spp_4b"


def _raw_mask(w, h, seed, tiers=4, share=0.6):
    """random bytes: 0 with probability 1 - share, else 1 .. tiers + 2 (bytes above T count as T)"""
    rng = np.random.default_rng(seed)
    return (rng.integers(1, tiers + 3, (w, h)) * (rng.random((w, h)) < share)).astype(np.uint8)


def _oracle_selected(o, base, n, sel, tiers):
    """a tiered sample_selected(n) at sample base ``base`` on the oracle: one full-frame launch per stage, kept where tier <= t"""
    for t, lo, hi, L in tr.stage_plan(n, tr.counts(sel, tiers)):
        before = o.image_buffer
        o.set_sample_base(base + lo)
        o.sample(hi - lo)
        keep = (sel != 0) & (sel <= t + 1)
        assert int(keep.sum()) == L
        o.image_buffer = np.where(keep[..., None], o.image_buffer, before)


def _oracle_sample(o, base, n):
    o.set_sample_base(base)
    o.sample(n)


def _check_counters(r, n, sel, tiers):
    c = r.counters()
    assert c.samples == c.deposits == tr.traced(n, tr.counts(sel, tiers))


# ------------------------------------------------------------------ 1. the tiered selection against the restatement, without tracing
FW, FH = 300, 230      # 69 000 pixels = 270 blocks of 256: more than one 256-entry scan tile even with one tier, the last block partial


@pytest.fixture(scope="module")
def noisy_frame():
    """Moments from traced batches (three full-frame ones and one through a random mask), then an image buffer crafted on top:
    whole texels scaled by 1, 4 or 16 (the counts spread over 6 .. 160 behind the same noise), 2 % of the pixels without samples.
    (Written data is no batch of the estimate — rtpbr_write_buffer re-takes the snapshot — so the moments have to be traced.)"""
    scene, cfg = cornell_box("v3", aspect=FW / FH), Config.cornell_v3(FW, FH, 0, 3)
    r = Renderer(scene, cfg)
    for _ in range(3):
        r.sample(2)
        r.noise_update()
    r.select_mask(np.random.default_rng(11).random((FW, FH)) < 0.4)
    r.sample_selected(4)
    r.noise_update()
    rng = np.random.default_rng(12)
    ib = r.image_buffer
    ib *= rng.choice(np.array([1, 1, 4, 16], np.float32), (FW, FH))[..., None]
    ib[rng.random((FW, FH)) < 0.02] = 0
    r.image_buffer = ib
    r.noise_estimate(0.0)
    noise = r.noise
    return r, float(np.quantile(noise[noise > 0], 0.5))


@pytest.mark.parametrize("tiers", [2, 4, 8])
def test_select_noisy_gives_the_restatements_tiers(noisy_frame, tiers):
    r, thr = noisy_frame
    seen = set()
    for dilate in (0, 3):
        for batch in (16, 256):
            r.set_select_tiers(tiers, batch)
            n = r.select_noisy(thr, dilate)
            ib = r.image_buffer
            want = tr.select(r.noise, ib[..., 3], thr, dilate, tiers, batch)
            got = r.selection
            assert got.dtype == np.uint8 and np.array_equal(got, want), f"{int((got != want).sum())} pixels differ ({dilate}, {batch})"
            assert n == int((want != 0).sum()) and r.selection_tiers == tr.counts(want, tiers)
            assert np.array_equal(want != 0, sr.select(r.noise, ib[..., 3], thr, dilate) != 0)
            seen |= set(np.unique(want).tolist())
            print(f"T={tiers} dilate={dilate} B={batch}: tiers {r.selection_tiers}")
    assert seen == set(range(tiers + 1))      # every tier occurred: the comparison was not of empty sets
    r.set_select_tiers()


def test_the_list_of_a_large_frame_is_the_tiers_prefixes(noisy_frame):
    """270 blocks x 4 tiers: the scan runs over five tiles.  One traced sample_selected(8): every pixel gained its tier's share."""
    r, thr = noisy_frame
    r.set_select_tiers(4, 64)
    try:
        r.select_noisy(thr, 1)
        sel, before = r.selection, r.image_buffer
        r.sample_selected(8)
        after = r.image_buffer
        share = np.array((0,) + tr.shares(8, 4), np.float32)[sel]
        assert np.array_equal(after[..., 3] - before[..., 3], share)
        assert np.array_equal(ck.bits(after)[sel == 0], ck.bits(before)[sel == 0])
        _check_counters(r, 8, sel, 4)
    finally:
        r.image_buffer = before      # (the frame is shared: the next test finds it as this one did)
        r.set_select_tiers()


def test_one_tier_is_the_parents_rule(noisy_frame):
    r, thr = noisy_frame
    r.set_select_tiers(1, 256)
    for dilate in (0, 3):
        n = r.select_noisy(thr, dilate)
        want = sr.select(r.noise, r.image_buffer[..., 3], thr, dilate)
        assert np.array_equal(r.selection, want) and n == int(want.sum()) and r.selection_tiers == (n,)
        assert [r.counter("select_tier%d" % t) for t in range(1, 8)] == [0] * 7
    r.set_select_tiers()


def test_select_error_gives_the_restatements_tiers():
    w, h = 96, 64
    scene, cfg = cornell_box("v3", aspect=w / h), Config.cornell_v3(w, h, 0, 3)
    r = Renderer(scene, cfg)
    for _ in range(2):
        r.sample(3)
        r.half_update()
    r.select_mask(np.random.default_rng(13).random((w, h)) < 0.5)
    r.sample_selected(6)
    r.half_update()
    r.denoise_error(0.0)
    err = r.denoised_error
    thr = float(np.quantile(err[err > 0], 0.4))
    r.set_select_tiers(4, 32)
    for dilate in (0, 2):
        n = r.select_error(thr, dilate)
        want = tr.select(r.denoised_error, r.image_buffer[..., 3], thr, dilate, 4, 32, half_count=r.half_buffer[..., 3])
        assert np.array_equal(r.selection, want) and n == int((want != 0).sum()) and r.selection_tiers == tr.counts(want, 4)
        assert len(np.unique(want)) >= 4


# ------------------------------------------------------------------ 2. the tiered launch against the composed oracle
NS = (1, 5, 16)


@pytest.mark.parametrize("name", list(_small_cases()))
def test_tiered_launches_bit_identical_to_composed_oracle(name):
    case, cfg = _small_cases()[name]
    w, h = cfg.width, cfg.height
    r, o = case.setup(Renderer(case.scene, cfg)), case.setup(OracleRenderer(case.scene, cfg))
    r.set_select_tiers(4)
    r.sample(2)
    _oracle_sample(o, 0, 2)
    base = 2
    for k, n in enumerate(NS):
        raw = _raw_mask(w, h, 20 + k)
        sel = tr.mask(raw, 4)
        assert r.select_mask(raw, raw=True) == int((sel != 0).sum())
        assert np.array_equal(r.selection, sel) and r.selection_tiers == tr.counts(sel, 4)
        r.sample_selected(n)
        _check_counters(r, n, sel, 4)
        _oracle_selected(o, base, n, sel, 4)
        ck.same(r.image_buffer, o.image_buffer, f"image_buffer after sample_selected({n})")
        r.sample(2)                                    # sample_base advanced by n for everybody
        _oracle_sample(o, base + n, 2)
        base += n + 2
        ck.same(r.image_buffer, o.image_buffer, f"image_buffer after the full-frame launch behind sample_selected({n})")
    assert len(np.unique(r.image_buffer[..., 3])) >= 5


# ------------------------------------------------------------------ 3. equivalence with plain calls
@pytest.mark.parametrize("n", NS)
def test_a_tiered_launch_is_its_stages_as_plain_selected_launches(n):
    case, cfg = _small_cases()[CORNELL]
    raw = _raw_mask(cfg.width, cfg.height, 31)
    sel = tr.mask(raw, 4)
    a, b = Renderer(case.scene, cfg), Renderer(case.scene, cfg)
    for x in (a, b):
        x.set_noise_tracking(True)
        x.set_half_mode(per_sample=True)
        x.sample(3)
    a.set_select_tiers(4)
    a.select_mask(raw, raw=True)
    a.sample_selected(n)
    _check_counters(a, n, sel, 4)
    total = 0
    for t, lo, hi, L in tr.stage_plan(n, tr.counts(sel, 4)):
        assert b.select_mask((sel != 0) & (sel <= t + 1)) == L
        b.set_option("sample_base", 3 + lo)
        b.sample_selected(hi - lo)
        c = b.counters()
        assert c.samples == c.deposits == L * (hi - lo)
        total += c.samples
    assert total == tr.traced(n, tr.counts(sel, 4))
    b.set_option("sample_base", 3 + n)
    for x in (a, b):
        x.sample(1)
    ck.same(a.image_buffer, b.image_buffer, "image_buffer")
    ck.same(a.moments, b.moments, "moments")
    ck.same(a.half_buffer, b.half_buffer, "half A")
    assert np.array_equal(a.image_buffer[..., 3], 4 + np.array((0,) + tr.shares(n, 4), np.float32)[sel])


# ------------------------------------------------------------------ 4. edge cases
def _edge_masks(w, h):
    rng = np.random.default_rng(41)
    some = rng.random((w, h)) < 0.5
    one = np.zeros((w, h), np.uint8)
    one[w // 3, h - 2] = 3
    return {"tier0_empty": (rng.integers(2, 5, (w, h)) * some).astype(np.uint8), "only_the_last_tier": (4 * some).astype(np.uint8),
            "one_pixel": one, "empty": np.zeros((w, h), np.uint8), "all_in_tier0": np.ones((w, h), np.uint8)}


@pytest.mark.parametrize("which", ["tier0_empty", "only_the_last_tier", "one_pixel", "empty", "all_in_tier0"])
def test_edge_selections(which):
    case, cfg = _small_cases()[CORNELL]
    raw = _edge_masks(cfg.width, cfg.height)[which]
    sel = tr.mask(raw, 4)
    r, o = Renderer(case.scene, cfg), OracleRenderer(case.scene, cfg)
    r.set_select_tiers(4)
    r.sample(2)
    _oracle_sample(o, 0, 2)
    assert r.select_mask(raw, raw=True) == int((sel != 0).sum()) and r.selection_tiers == tr.counts(sel, 4)
    r.sample_selected(5)
    _check_counters(r, 5, sel, 4)
    tiered_counters = ck.counters(r)
    assert r.last_sample_ms()[2] == len(tr.stage_plan(5, tr.counts(sel, 4)))
    _oracle_selected(o, 2, 5, sel, 4)
    ck.same(r.image_buffer, o.image_buffer, "image_buffer after the tiered launch")
    r.sample_selected(0)                                  # traces nothing, moves nothing
    assert r.last_sample_ms()[2] == 0 and ck.counters(r) == [0] * 6
    r.sample(2)
    _oracle_sample(o, 7, 2)
    ck.same(r.image_buffer, o.image_buffer, "image_buffer after the next full-frame launch")
    if which == "all_in_tier0":      # the plain selected launch, work counters included (its 5 samples in three stages here)
        plain = Renderer(case.scene, cfg)
        plain.sample(2)
        plain.select_mask(raw)
        plain.sample_selected(5)
        assert tiered_counters == ck.counters(plain)
        plain.sample(2)
        ck.same(r.image_buffer, plain.image_buffer, "image_buffer against the binary selection")


def test_stages_split_into_sub_launches():
    """a staging budget of 1 MiB holds ~74 898 items: stage 0 of n = 64 (32 samples through ~2870 pixels) needs two sub-launches;
    the work counters are zeroed between sub-launches and between stages, or the later ones would trace nothing"""
    scene, cfg = cornell_box("v3"), Config.cornell_v3(64, 64, 0, 3)
    rng = np.random.default_rng(42)
    raw = rng.choice(np.array([1, 1, 1, 1, 1, 1, 1, 2, 3, 4], np.uint8), (64, 64))
    cnt = tr.counts(raw, 4)
    plan = tr.stage_plan(64, cnt)
    assert len(plan) == 4 and cnt[0] * 32 > 74898 > max(L * (hi - lo) for t, lo, hi, L in plan[:3])
    got = []
    for budget in (1 << 20, 1 << 30):
        r = Renderer(scene, cfg)
        r.set_option("staging_bytes", budget)
        r.set_select_tiers(4, 64)
        r.sample(1)
        r.select_mask(raw, raw=True)
        r.sample_selected(64)
        _check_counters(r, 64, raw, 4)
        assert r.last_sample_ms()[2] == (5 if budget == 1 << 20 else 4)
        r.sample(1)
        got.append(r.image_buffer)
    ck.same(got[0], got[1], "image_buffer, five sub-launches against four")
    assert np.array_equal(got[0][..., 3], 2 + np.array((0,) + tr.shares(64, 4), np.float32)[raw])


def test_a_selection_keeps_its_tiers_and_a_new_resolution_drops_it():
    case, cfg = _small_cases()[CORNELL]
    raw = _raw_mask(cfg.width, cfg.height, 43)
    sel = tr.mask(raw, 4)
    r, o = Renderer(case.scene, cfg), OracleRenderer(case.scene, cfg)
    r.set_select_tiers(4, 16)
    r.select_mask(raw, raw=True)
    r.set_option("select_tiers", 1)           # read by the select calls only: the selection keeps the tiers it was built with
    r.set_option("select_batch", 999)
    assert r.selection_tiers == tr.counts(sel, 4)
    r.sample_selected(5)
    _check_counters(r, 5, sel, 4)
    _oracle_selected(o, 0, 5, sel, 4)
    ck.same(r.image_buffer, o.image_buffer, "image_buffer")
    assert r.select_mask(raw, raw=True) == int((raw != 0).sum())      # the next select call reads the option: one tier
    assert np.array_equal(r.selection, (raw != 0).astype(np.uint8))
    assert [r.counter("select_tier%d" % t) for t in range(4)] == [int((raw != 0).sum()), 0, 0, 0]
    r.set_option("select_tiers", 4)
    r.select_mask(raw, raw=True)
    r.set_config(cfg.copy(seed=5))            # the same resolution keeps the selection and its tiers
    assert r.selection_tiers == tr.counts(sel, 4)
    r.set_config(Config.cornell_v3(48, 24, 0, 3))
    assert [r.counter("select_tier%d" % t) for t in range(8)] == [0] * 8
    assert ck.code(lambda: r.sample_selected(1)) == ESTATE
    raw2 = _raw_mask(48, 24, 44)
    assert r.select_mask(raw2, raw=True) == int((raw2 != 0).sum()) and np.array_equal(r.selection, tr.mask(raw2, 4))


def test_before_any_selection_the_tier_counters_are_zero_and_other_names_are_refused():
    r = Renderer(cornell_box("v3"), Config.cornell_v3(16, 16, 0, 3))
    assert [r.counter("select_tier%d" % t) for t in range(8)] == [0] * 8
    for name in ("select_tier8", "select_tier", "select_tier00"):
        assert ck.code(lambda: r.counter(name)) == ck.EINVAL
    for key, bad in (("select_tiers", 0), ("select_tiers", 9), ("select_batch", 0), ("select_batch", 65537)):
        assert ck.code(lambda: r.set_option(key, bad)) == ck.EINVAL


# ------------------------------------------------------------------ 5. render_adaptive(tiers=4)
def test_render_adaptive_with_tiers_is_its_calls_one_by_one():
    scene, cfg = cornell_box("v3"), Config.cornell_v3(64, 64, 0, 3)
    noise, budget, batch, dilate, tiers = 0.1, 288, 32, 1, 4
    a = Renderer(scene, cfg)
    a.refresh()
    traced, st = a.render_adaptive(noise, budget, batch_spp=batch, dilate=dilate, tiers=tiers)
    assert a.select_tiers == (1, 16)
    b = Renderer(scene, cfg)
    b.refresh()
    b.set_select_tiers(tiers, batch)
    want_traced, used, seen = 0, 0, set()
    for _ in range(2):
        b.sample(batch)
        b.noise_update()
        want_traced, used = want_traced + 64 * 64 * batch, used + batch
    while used + batch <= budget:
        n_sel = b.select_noisy(noise, dilate)
        sel = b.selection
        want = tr.select(b.noise, b.image_buffer[..., 3], noise, dilate, tiers, batch)
        assert np.array_equal(sel, want) and n_sel == int((want != 0).sum()) and b.selection_tiers == tr.counts(want, tiers)
        if n_sel == 0:
            break
        seen |= set(np.unique(want).tolist())
        b.sample_selected(batch)
        _check_counters(b, batch, want, tiers)
        b.noise_update()
        want_traced, used = want_traced + tr.traced(batch, tr.counts(want, tiers)), used + batch
    ck.same(a.image_buffer, b.image_buffer, "image_buffer")
    ck.same(a.moments, b.moments, "moments")
    assert traced == want_traced == int(a.image_buffer[..., 3].astype(np.float64).sum())
    assert seen >= {1, 2}, seen                # the loop gave out more than one share
    print(f"render_adaptive(tiers=4): {traced} pixel-samples, {used // batch - 2} selected rounds, {st.pixels_above} pixels above")


# ------------------------------------------------------------------ 6. one random call sequence
def test_a_random_call_sequence_against_the_composed_oracle():
    """32 calls, fixed seed.  The oracle has no reprojection: after reproject() it takes the device's image buffer and the new
    camera (the reprojection is not what this test is about; that a selection and its tiers survive it is)."""
    w, h = 40, 30
    scene, cfg = cornell_box("v3", aspect=w / h), Config.cornell_v3(w, h, 0, 3)
    r, o = Renderer(scene, cfg), OracleRenderer(scene, cfg)
    rng = np.random.default_rng(60)
    base, tiers, batch, sel, sel_tiers = 0, 1, 16, None, 1
    cams = [rp.MOVES["translate"](scene.camera)[1], scene.camera]
    log = []

    def read(what):
        ck.same(r.image_buffer, o.image_buffer, f"image_buffer after {what} (calls so far: {log})")

    r.refresh()                 # (a reprojection wants the image buffer to be a history of this scene)
    o.refresh()
    r.sample(2)
    r.noise_update()
    _oracle_sample(o, 0, 2)
    base = 2
    ops = ["tiers", "batch", "mask", "noisy", "selected", "selected", "sample", "refresh", "reproject"]
    for step in range(32):
        op = ops[int(rng.integers(len(ops)))] if step not in (0, 1) else ("tiers", "mask")[step]
        if op in ("selected", "noisy") and (sel is None if op == "selected" else False):
            op = "mask"
        log.append(op)
        if op == "tiers":
            tiers = int(rng.choice([1, 2, 4, 8])) if step else 4
            r.set_option("select_tiers", tiers)
        elif op == "batch":
            batch = int(rng.choice([4, 16, 64]))
            r.set_option("select_batch", batch)
        elif op == "mask":
            raw = _raw_mask(w, h, 100 + step, 8, 0.5)
            sel, sel_tiers = tr.mask(raw, tiers), tiers
            assert r.select_mask(raw, raw=True) == int((sel != 0).sum()) and np.array_equal(r.selection, sel)
        elif op == "noisy":
            dilate = int(rng.integers(0, 3))
            n = r.select_noisy(0.05, dilate)
            sel, sel_tiers = tr.select(r.noise, r.image_buffer[..., 3], 0.05, dilate, tiers, batch), tiers
            assert np.array_equal(r.selection, sel) and n == int((sel != 0).sum())
        elif op == "selected":
            n = int(rng.choice([0, 1, 3, 8, 13]))
            r.sample_selected(n)
            r.noise_update()
            _check_counters(r, n, sel, sel_tiers)
            _oracle_selected(o, base, n, sel, sel_tiers)
            base += n
            read(f"sample_selected({n})")
        elif op == "sample":
            n = int(rng.integers(1, 4))
            r.sample(n)
            r.noise_update()
            _oracle_sample(o, base, n)
            base += n
            read(f"sample({n})")
        elif op == "refresh":
            r.refresh()
            o.refresh()
            read("refresh")
        else:
            cam = cams[0]
            cams.reverse()
            r.reproject(cam, max_history=8.0)
            o.set_camera(cam)
            o.image_buffer = r.image_buffer
        if sel is not None:
            assert tuple(r.counter("select_tier%d" % t) for t in range(sel_tiers)) == tr.counts(sel, sel_tiers)
    read("the last call")
    assert {"selected", "noisy", "mask", "sample"} <= set(log)
