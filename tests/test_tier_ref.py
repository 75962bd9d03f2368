"""The tier rule and the stage plan of the tiered selection restated in numpy (tests/tier_ref_lib.py): known answers, the
properties the header promises, the two options' bounds on a context without a device, and what the new Renderer methods hand
across the C ABI (over the recording stand-in of test_renderer_marshalling)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import select_ref_lib as sr
import tier_ref_lib as tr
from raytracingpbr_amd import Renderer
from test_renderer_marshalling import H, W, Recorder, new_renderer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _random_maps(seed, w=13, h=10):
    rng = np.random.default_rng(seed)
    plane = rng.random((w, h), dtype=f32)
    count = np.floor(rng.random((w, h)) * 40).astype(f32) * (rng.random((w, h)) > 0.1)
    return plane, count


# ------------------------------------------------------------------ the rule
@pytest.mark.parametrize("dilate", [0, 1, 3])
def test_one_tier_is_the_binary_rule(dilate):
    plane, count = _random_maps(1)
    for thr in (0.0, 0.5, 0.9):
        got = tr.select(plane, count, thr, dilate, 1, 16)
        assert np.array_equal(got, sr.select(plane, count, thr, dilate))
        assert np.array_equal(tr.ordered_list(got), sr.ordered_list(got))
    raw = np.random.default_rng(2).integers(0, 256, (7, 5)).astype(np.uint8)
    assert np.array_equal(tr.mask(raw, 1), (raw != 0).astype(np.uint8))


@pytest.mark.parametrize("tiers", [2, 4, 8])
def test_membership_does_not_depend_on_the_tiers(tiers):
    plane, count = _random_maps(3)
    for d in range(4):
        got = tr.select(plane, count, 0.8, d, tiers, 64)
        assert np.array_equal(got != 0, sr.select(plane, count, 0.8, d) != 0)
        assert got.max() <= tiers


def test_known_answers():
    # threshold 0.5, 10 samples: need = 10 (r^2 - 1); batch 64, 4 tiers: the bounds are 32, 16, 8
    plane = np.array([[0.5, 0.51, 0.75, 1.0, 1.5, 3.0]], f32)
    count = np.full((1, 6), 10, f32)
    r = plane / f32(0.5)
    need = count * (r * r - f32(1))
    assert np.allclose(need, [0, 0.404, 12.5, 30, 80, 350])
    assert tr.bounds(4, 64) == [32, 16, 8]
    #   not above | need 0.4: all three bounds hold, tier 3 | 12.5 <= 32, 16: tier 2 | 30 <= 32: tier 1 | 80, 350: the full share
    assert tr.select(plane, count, 0.5, 0, 4, 64).tolist() == [[0, 4, 3, 2, 1, 1]]
    assert tr.select(plane, count, 0.5, 0, 2, 64).tolist() == [[0, 2, 2, 2, 1, 1]]
    # a batch that runs out of halves: B = 2, T = 4: the bounds are 1, 1, 1
    assert tr.bounds(4, 2) == [1, 1, 1] and tr.bounds(8, 65536)[-1] == 512
    assert tr.select(plane, count, 0.5, 0, 4, 2).tolist() == [[0, 4, 1, 1, 1, 1]]
    # need equal to a bound takes the smaller share (<=)
    exact = tr.select(np.array([[1.0]], f32), np.array([[8.0 / 3.0]], f32), 0.5, 0, 4, 64)
    assert f32(8.0 / 3.0) * f32(3) == f32(8) and exact.tolist() == [[4]]


def test_pixels_selected_without_the_plane_take_the_full_share():
    plane = np.full((3, 3), 0.6, f32)
    count = np.full((3, 3), 100, f32)
    count[0, 0], count[1, 1], count[2, 2] = 0, np.nan, 3
    half = np.full((3, 3), 50, f32)
    half[0, 1], half[1, 2] = 0, 100          # half A empty, half B empty
    got = tr.select(plane, count, 0.5, 1, 4, 256, min_samples=4, half_count=half)
    need = f32(100) * ((f32(0.6) / f32(0.5)) ** 2 - f32(1))        # 44: <= 128, 64 only
    assert 32 < need <= 64
    want = np.full((3, 3), 3, np.uint8)
    for p in ((0, 0), (1, 1), (2, 2), (0, 1), (1, 2)):
        want[p] = 1
    assert np.array_equal(got, want)


def test_the_window_maximum_sets_the_tier_of_the_neighbours():
    plane = np.zeros((9, 9), f32)
    count = np.full((9, 9), 10, f32)
    plane[4, 4] = 5.0            # need 990: the full share
    plane[0, 0] = 0.55           # need 2.1
    got = tr.select(plane, count, 0.5, 2, 4, 64)
    assert (got[2:7, 2:7] == 1).all() and (got[0:3, 0:3][got[0:3, 0:3] != 1] == 4).all() and got[0, 0] == 4 and got[2, 2] == 1
    assert got[8, 0] == 0 and int((got != 0).sum()) == 25 + 9 - 1


def test_tiers_are_monotone_in_the_plane_and_in_the_count():
    values = np.sort(np.random.default_rng(5).random(200).astype(f32) * 4)[None, :]
    for cnt in (1, 7, 100):
        got = tr.select(values, np.full(values.shape, cnt, f32), 0.3, 0, 8, 256).astype(int)[0]
        sel = got[got != 0]
        assert (np.diff(sel) <= 0).all() and (got[values[0] <= f32(0.3)] == 0).all()      # noisier: never a smaller share
    cnts = np.arange(1, 400, dtype=f32)[None, :]
    got = tr.select(np.full(cnts.shape, 0.45, f32), cnts, 0.3, 0, 8, 256).astype(int)[0]
    assert (got != 0).all() and (np.diff(got) <= 0).all() and got[0] == 8 and got[-1] == 1  # more samples behind the same noise: more to add


def test_zero_threshold_nan_and_infinity():
    plane = np.array([[0.0, 0.2, np.nan, np.inf, 0.2]], f32)
    count = np.array([[5, 5, 5, 5, np.inf]], f32)
    # threshold 0: r = m / 0 is infinite: the full share; the NaN is not above
    assert tr.select(plane, count, 0.0, 0, 8, 256).tolist() == [[0, 1, 0, 1, 1]]
    # need = 5 (2^2 - 1) = 15 <= 128, 64, 32, 16: tier 4; an infinite plane value, an infinite count: need is infinite: the full share
    assert tr.select(plane, count, 0.1, 0, 8, 256).tolist() == [[0, 5, 0, 1, 1]]
    # the NaN does not enter its neighbours' maximum
    assert tr.select(plane[:, :3], count[:, :3], 0.1, 1, 8, 256).tolist() == [[5, 5, 5]]
    # need = inf * 0 is NaN when r rounds to 1: no comparison holds
    thr = f32(2) - f32(2) ** -22
    one = np.array([[np.nextafter(thr, f32(3))]], f32)
    if one[0, 0] / thr == f32(1):
        assert tr.select(one, np.array([[np.inf]], f32), thr, 0, 4, 16).tolist() == [[1]]


def test_mask_bytes_are_tiers():
    raw = np.array([[0, 1, 2, 3, 4, 5, 200, 255]], np.uint8)
    assert tr.mask(raw, 4).tolist() == [[0, 1, 2, 3, 4, 4, 4, 4]]
    assert tr.mask(raw, 8).tolist() == [[0, 1, 2, 3, 4, 5, 8, 8]]
    assert tr.mask(raw, 2).tolist() == [[0, 1, 2, 2, 2, 2, 2, 2]]
    with pytest.raises(ValueError):
        tr.mask(raw.astype(np.int32), 4)


def test_the_list_is_tier_major_and_ascending_within_a_tier():
    sel = np.random.default_rng(7).integers(0, 5, (11, 7)).astype(np.uint8)
    lst = tr.ordered_list(sel)
    flat = sel.reshape(-1)
    assert sorted(lst.tolist()) == np.flatnonzero(flat).tolist() and lst.dtype == np.uint32
    key = [(int(flat[i]), int(i)) for i in lst]
    assert key == sorted(key)
    c = tr.counts(sel, 4)
    assert sum(c) == len(lst) and c == tuple(int((flat == k).sum()) for k in (1, 2, 3, 4))
    for t in range(4):      # the pixels of tiers 0 .. t are a prefix
        assert set(lst[:sum(c[:t + 1])].tolist()) == set(np.flatnonzero((flat != 0) & (flat <= t + 1)).tolist())
    assert tr.ordered_list(np.zeros((3, 3), np.uint8)).tolist() == []


def test_bad_arguments():
    plane, count = _random_maps(1)
    for bad in ({"dilate": 4}, {"tiers": 0}, {"tiers": 9}, {"batch": 0}, {"batch": 65537}, {"threshold": -1.0}):
        kw = {"threshold": 0.5, "dilate": 0, "tiers": 4, "batch": 16, **bad}
        with pytest.raises(ValueError):
            tr.select(plane, count, **kw)


# ------------------------------------------------------------------ the stage plan
def test_the_example_of_five_samples_in_four_tiers():
    assert tr.shares(5, 4) == (5, 2, 1, 1)
    #   stage 3: index 0 through everything; stage 2: s_2 = s_3, skipped; stage 1: index 1 through tiers 0..1; stage 0: 2..4
    assert tr.stage_plan(5, (10, 20, 30, 40)) == [(3, 0, 1, 100), (1, 1, 2, 30), (0, 2, 5, 10)]
    assert tr.traced(5, (10, 20, 30, 40)) == 50 + 40 + 30 + 40


@pytest.mark.parametrize("tiers", [1, 2, 4, 8])
@pytest.mark.parametrize("n", [0, 1, 5, 16, 255])
def test_the_stage_plan_against_a_count_per_pixel(n, tiers):
    rng = np.random.default_rng(100 * tiers + n)
    for trial in range(4):
        sel = rng.integers(0, tiers + 1, 60).astype(np.uint8)
        if trial == 1:
            sel[sel == 1] = 0                    # tier 0 empty
        if trial == 2:
            sel[(sel != 0) & (sel != tiers)] = 0    # only the last tier
        if trial == 3:
            sel[:] = 0
        cnt, lst = tr.counts(sel, tiers), tr.ordered_list(sel)
        got = np.zeros(60, int)
        indices = [[] for _ in range(60)]
        plan = tr.stage_plan(n, cnt)
        for t, lo, hi, L in plan:
            assert lo < hi and L > 0 and L == sum(cnt[:t + 1])
            for p in lst[:L]:
                got[p] += hi - lo
                indices[p] += list(range(lo, hi))
        # brute force: a pixel of tier t receives the indices 0 .. max(1, n >> t) - 1, in ascending order, nothing when n = 0
        for p in range(60):
            want = 0 if sel[p] == 0 or n == 0 else max(1, n >> (int(sel[p]) - 1))
            assert got[p] == want and indices[p] == list(range(want)), (p, sel[p])
        assert tr.traced(n, cnt) == int(got.sum())
        assert [t for t, _, _, _ in plan] == sorted((t for t, _, _, _ in plan), reverse=True)
        if n == 0 or not sel.any():
            assert plan == []
    assert tr.shares(n, tiers)[0] == n and (tiers == 1 or n == 0 or tr.shares(n, tiers)[-1] == max(1, n >> (tiers - 1)))


# ------------------------------------------------------------------ the header and the options
def test_the_header_carries_the_rule():
    hdr = " ".join(open(os.path.join(ROOT, "include", "rtpbr.h")).read().replace("*", " ").split())
    for text in ('"select_tiers" = T (1..8, default 1', '"select_batch" = B (1..65536, default 16', "t = min(b, T) - 1",
                 "m = fmaxf over the pixels q inside the frame with max(|dx|, |dy|) <= dilate and plane[q] > threshold, of plane[q]",
                 "r = m / threshold", "need = b.w (r r - 1.0f)", "t = the number of k in 1 .. T - 1 with need <= (float)max(1, B >> k)",
                 "RTPBR_BUF_SELECTION holds 0 or 1 + t", "ordered by tier, then by ascending buffer index within a tier",
                 "s_t = max(1, n >> t)", '"select_tier0" .. "select_tier7"',
                 "samples = deposits = the sum over t of (pixels in tier t) s_t"):
        assert text in hdr, text


TIERS_MESSAGE = ("select_tiers must be 1 (every selected pixel takes the whole batch of rtpbr_sample_selected) .. 8 (the select calls give "
                 "every selected pixel one of that many shares of it)")
BATCH_MESSAGE = ("select_batch must be 1 .. 65536 (the n the host will pass to rtpbr_sample_selected: with select_tiers > 1 the "
                 "noise-driven select calls size the shares by it)")


def test_the_two_options_keep_their_bounds_and_messages(tmp_path, monkeypatch):
    """on a context without a device (test_host_logic.test_every_option_keeps_its_bounds_and_messages has the pattern)"""
    from raytracingpbr_amd import dataclass as dc
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
    for key, lo, hi, msg in (("select_tiers", 1, 8, TIERS_MESSAGE), ("select_batch", 1, 65536, BATCH_MESSAGE)):
        for value in (lo - 1, hi + 1, -5):
            assert answer("%s=%d nosuchkey=0" % (key, value)) == (-1, msg), (key, value)
        for value in (lo, hi):
            assert answer("%s=%d nosuchkey=0" % (key, value)) == unknown, (key, value)
    assert not list(tmp_path.iterdir())                        # nothing was compiled


def test_the_capi_source_declares_both_rows_beside_their_neighbours():
    src = open(os.path.join(ROOT, "raytracingpbr_amd", "csrc", "rt_capi.hip")).read()
    assert re.search(r"OPTION\(select_tiers, 1, 8, false,", src) and re.search(r"OPTION\(select_batch, 1, 65536, false,", src)


# ------------------------------------------------------------------ what the Python methods hand across
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


def _option(key, value):
    return ("set_option", "ctx", key.encode(), value)


def _tier_reads(tiers):
    return [("get_counter", "ctx", b"select_tier%d" % t, ("ref", bytes(8))) for t in range(tiers)]


def test_set_select_tiers_and_selection_tiers():
    from raytracingpbr_amd import Config, cornell_box
    api = Counting({"select_tier%d" % t: 10 * t + 1 for t in range(8)})
    r = Renderer(cornell_box("v3"), Config.cornell_v3(W, H, 0, 3), api=api)
    assert r.select_tiers == (1, 16) and not any(c[0] == "set_option" for c in api.calls)
    del api.calls[:]
    assert r.selection_tiers == (1,)
    r.set_select_tiers(4, 256)
    assert r.select_tiers == (4, 256) and r.selection_tiers == (1, 11, 21, 31)
    r.set_select_tiers()
    assert api.calls == (_tier_reads(1) + [_option("select_tiers", 4), _option("select_batch", 256)] + _tier_reads(4)
                         + [_option("select_tiers", 1), _option("select_batch", 16)])
    assert Renderer.tier_shares(5, 4) == (5, 2, 1, 1) and Renderer.tier_shares(0, 3) == (0, 0, 0) and Renderer.tier_shares(16, 1) == (16,)


def test_select_mask_raw_passes_the_bytes_through():
    r, api = new_renderer(script={"select_mask": [5, 7]})
    raw = np.arange(W * H, dtype=np.uint8).reshape(W, H) * 9
    assert r.select_mask(raw) == 5 and r.select_mask(raw, raw=True) == 7
    assert api.calls == [("select_mask", "ctx", (raw != 0).astype(np.uint8).tobytes(), W * H, ("ref", bytes(4))),
                         ("select_mask", "ctx", raw.tobytes(), W * H, ("ref", bytes(4)))]
    with pytest.raises(TypeError):
        r.select_mask(raw.astype(np.int32), raw=True)
    with pytest.raises(ValueError):
        r.select_mask(raw.T, raw=True)
    assert len(api.calls) == 2


def _adaptive_calls(tiers, batch, rounds, per_sample=False):
    """render_adaptive's calls with ``rounds`` selections that found pixels and one that found none"""
    calls = []
    if tiers != 1:
        calls += [_option("select_tiers", tiers), _option("select_batch", batch)]
    for _ in range(2):
        calls += [("sample", "ctx", batch), ("noise_update", "ctx")]
    for k in range(rounds + 1):
        calls.append(("select_noisy", "ctx", 0.25, 1, ("ref", bytes(4))))
        if k < rounds:
            calls += [("sample_selected", "ctx", batch), ("noise_update", "ctx")]
            if tiers != 1:
                calls += _tier_reads(tiers)
    calls.append(("noise_estimate", "ctx", 0.25, ("ref", bytes(12))))
    if tiers != 1:
        calls += [_option("select_tiers", 1), _option("select_batch", 16)]
    return calls


def test_render_adaptive_sets_the_tiers_for_the_call_and_counts_what_was_traced():
    counters = {"select_tier0": 3, "select_tier1": 2, "select_tier2": 0, "select_tier3": 4}
    api = Counting(counters, script={"select_noisy": [9, 9, 0]})
    from raytracingpbr_amd import Config, cornell_box
    r = Renderer(cornell_box("v3"), Config.cornell_v3(W, H, 0, 3), api=api)
    del api.calls[:]
    traced, _ = r.render_adaptive(0.25, 1000, batch_spp=20, dilate=1, tiers=4)
    assert api.calls == _adaptive_calls(4, 20, 2)
    assert traced == 2 * 20 * W * H + 2 * (3 * 20 + 2 * 10 + 0 * 5 + 4 * 2)
    assert r.select_tiers == (1, 16)
    # one tier: exactly the calls of the binary loop
    api.script["select_noisy"] = [9, 9, 0]
    del api.calls[:]
    traced, _ = r.render_adaptive(0.25, 1000, batch_spp=20, dilate=1)
    assert api.calls == _adaptive_calls(1, 20, 2) and traced == 2 * 20 * W * H + 2 * 9 * 20
    # what set_select_tiers had set before comes back, however the loop ends
    r.set_select_tiers(2, 64)
    api.script["select_noisy"] = [9]
    api.fail = ("sample_selected", api.seen["sample_selected"] + 1)
    del api.calls[:]
    from test_renderer_marshalling import Scripted
    with pytest.raises(Scripted):
        r.render_adaptive(0.25, 1000, batch_spp=20, dilate=1, tiers=8)
    assert api.calls[:2] == [_option("select_tiers", 8), _option("select_batch", 20)]
    assert api.calls[-2:] == [_option("select_tiers", 2), _option("select_batch", 64)] and r.select_tiers == (2, 64)


def test_render_adaptive_denoised_sets_the_tiers_for_the_call():
    counters = {"select_tier0": 1, "select_tier1": 5}
    api = Counting(counters, script={"denoise_error": [(W * H, 3, 0.5), (W * H, 0, 0.0)], "select_error": [6]})
    from raytracingpbr_amd import Config, cornell_box
    r = Renderer(cornell_box("v3"), Config.cornell_v3(W, H, 0, 3), api=api)
    del api.calls[:]
    traced, _ = r.render_adaptive_denoised(0.25, 1000, batch_spp=8, tiers=2)
    names = [c[0] for c in api.calls]
    assert names == ["set_option", "set_option", "sample", "half_update", "sample", "half_update", "denoise_error", "select_error",
                     "sample_selected", "half_update", "get_counter", "get_counter", "denoise_error", "denoise", "set_option", "set_option"]
    assert api.calls[:2] == [_option("select_tiers", 2), _option("select_batch", 8)]
    assert api.calls[-2:] == [_option("select_tiers", 1), _option("select_batch", 16)]
    assert traced == 2 * 8 * W * H + 1 * 8 + 5 * 4
    del api.calls[:]
    api.script.update({"denoise_error": [(W * H, 3, 0.5), (W * H, 0, 0.0)], "select_error": [6]})
    traced, _ = r.render_adaptive_denoised(0.25, 1000, batch_spp=8)
    assert "set_option" not in [c[0] for c in api.calls] and "get_counter" not in [c[0] for c in api.calls]
    assert traced == 2 * 8 * W * H + 6 * 8
