"""The lattice selection built on the device (option select_lattice; include/rtpbr.h) on the GPU.  Every case runs a twin context
that makes the same calls with rtpbr_select_mask and the lattice's mask in place of the option, and every comparison is ``==`` on
bit patterns: the option promises exactly the state select_mask leaves.  The list is not readable, and its order may differ from
the twin's (a build with RT_LATTICE_ORDER=1 orders it in blocks of 8 x 8 lattice pixels); what no order may change is checked: a
duplicate or a missing entry shows in image_buffer's count channel, a wrong index in every buffer.

Work counters compared: all six of rtpbr_get_counters (checks.COUNTERS: samples, raycasts, march_steps, hits, sky_lookups,
deposits) — they count rays, bounces and march iterations per path, whichever wave traces it.  Left out: the named counters beyond
them (mlp_wave_evals, mlp_lane_evals, dense_launches, jit_active), which count waves and launches, and the timings: those depend
on which pixels share a wave, which is what the list's order changes."""
import numpy as np
import pytest

import checks as ck
import test_gpu_reproject as rp
from checks import EINVAL, ESTATE
from raytracingpbr_amd import Config, Renderer, cornell_box
from raytracingpbr_amd._capi import RtpbrError
from raytracingpbr_amd.renderer import BUF_HALF_BUFFER, BUF_IMAGE_BUFFER, BUF_IMAGE_PIXELS, BUF_MOMENTS, BUF_SELECTION

pytestmark = pytest.mark.gpu

FRAMES = [(48, 40), (33, 17), (7, 5)]
LATTICES = [((2, 2), (0, 0)), ((2, 2), (1, 0)), ((2, 2), (0, 1)), ((2, 2), (1, 1)), ((4, 4), (3, 1)), ((3, 2), (2, 1)), ((8, 8), (7, 4)),
            ((1, 1), (0, 0))]
CASES = [(f, l) for f in FRAMES for l in LATTICES] + [((7, 5), ((8, 8), (7, 7)))]      # the last: an empty lattice


def lattice_mask(w, h, period, phase):
    return np.logical_and.outer(np.arange(w) % period[0] == phase[0], np.arange(h) % period[1] == phase[1])


def code_of(period, phase):
    return period[0] + 16 * period[1] + 256 * phase[0] + 4096 * phase[1]


def twins(w, h, tracked=True):
    """(the context under test, its twin), Cornell v3, with per-sample noise tracking and per-sample halves"""
    scene, cfg = cornell_box("v3", aspect=w / h), Config.cornell_v3(w, h, 0, 3)
    pair = Renderer(scene, cfg), Renderer(scene, cfg)
    for r in pair:
        if tracked:
            r.set_noise_tracking(True)
            r.set_half_mode(per_sample=True)
    return pair


def select(pair, period, phase):
    """the option on the first, select_mask with the lattice's mask on the twin; the count"""
    a, b = pair
    w, h = a.config.width, a.config.height
    n = a.select_lattice(period, phase, device=True)
    assert n == b.select_mask(lattice_mask(w, h, period, phase)) == int(lattice_mask(w, h, period, phase).sum())
    return n


def same_selection(pair, what):
    a, b = pair
    ck.same(a.selection, b.selection, f"selection {what}")
    assert [a.counter("select_tier%d" % t) for t in range(8)] == [b.counter("select_tier%d" % t) for t in range(8)], what
    assert a.selection_tiers == b.selection_tiers, what


def same_frame(pair, what):
    a, b = pair
    ck.same(a.image_buffer, b.image_buffer, f"image_buffer {what}")
    ck.same(a.moments, b.moments, f"moments {what}")
    ck.same(a.half_buffer, b.half_buffer, f"half A {what}")


@pytest.mark.parametrize("frame,lattice", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v[0], int) else "%dx%d@%d,%d" % (v[0] + v[1]))
def test_the_option_leaves_the_state_of_select_mask_and_the_launches_their_bits(frame, lattice):
    (w, h), (period, phase) = frame, lattice
    pair = twins(w, h)
    a, b = pair
    mask = lattice_mask(w, h, period, phase)
    for tiers in (4, 1):
        for r in pair:
            r.set_select_tiers(tiers, 8)
        n = select(pair, period, phase)
        same_selection(pair, f"with select_tiers = {tiers}")
        assert np.array_equal(a.selection, mask.astype(np.uint8)) and a.selection_tiers == (n,) + (0,) * (tiers - 1)
    for r in pair:
        r.refresh()
        r.sample_selected(2)
    assert ck.counters(a) == ck.counters(b) and a.counters().samples == a.counters().deposits == 2 * n
    same_frame(pair, "after refresh + sample_selected(2)")
    for r in pair:
        r.sample_selected(3)
    assert ck.counters(a) == ck.counters(b) and a.counters().samples == 3 * n
    same_frame(pair, "after a second sample_selected(3)")
    assert np.array_equal(a.image_buffer[..., 3], 5 * mask.astype(np.float32))      # every lattice pixel once in the list, nobody else
    # the sparse frame completed and displayed
    assert a.denoise_fill() == b.denoise_fill()
    ck.same(a.denoised_pixels, b.denoised_pixels, "denoised_pixels after denoise_fill")
    for r in pair:
        r.present("denoised")
    ck.same(a.presented, b.presented, "the presented frame")


@pytest.mark.parametrize("frame", FRAMES[:2], ids=lambda f: "%dx%d" % f)
def test_a_tiered_launch_on_the_lattice(frame):
    """set_select_tiers(4, 8): every lattice pixel is in tier 0 and takes the whole batch, in the stages of the tiered launch"""
    w, h = frame
    pair = twins(w, h)
    a, b = pair
    for r in pair:
        r.set_select_tiers(4, 8)
        r.sample(1)
    n = select(pair, (2, 2), (1, 0))
    same_selection(pair, "tiered")
    assert a.selection_tiers == (n, 0, 0, 0)
    for r in pair:
        r.sample_selected(8)
    assert ck.counters(a) == ck.counters(b) and a.counters().samples == 8 * n
    assert a.last_sample_ms()[2] == b.last_sample_ms()[2]
    same_frame(pair, "after the tiered sample_selected(8)")
    assert np.array_equal(a.image_buffer[..., 3], 1 + 8 * lattice_mask(w, h, (2, 2), (1, 0)).astype(np.float32))


def test_a_random_call_sequence_against_the_twin():
    """40 calls, fixed seed: the option between select_noisy, select_mask, reproject, refresh, a configuration of another size and
    back, and selected launches.  A later selection replaces the lattice, the lattice replaces an earlier selection, a new
    resolution drops it."""
    w, h = 40, 30
    scene, cfg = cornell_box("v3", aspect=w / h), Config.cornell_v3(w, h, 0, 3)
    other = Config.cornell_v3(23, 19, 0, 3)
    pair = twins(w, h)
    a, b = pair
    rng = np.random.default_rng(71)
    cams = [rp.MOVES["translate"](scene.camera)[1], scene.camera]
    for r in pair:
        r.refresh()
        r.sample(2)
    have, size, log = False, (w, h), []
    ops = ["lattice", "lattice", "lattice", "noisy", "mask", "selected", "selected", "selected", "refresh", "reproject", "config"]
    forced = {0: "lattice", 1: "selected", 2: "mask", 3: "lattice", 4: "selected", 5: "noisy", 6: "lattice", 7: "selected", 8: "config"}
    for step in range(40):
        op = forced.get(step) or ops[int(rng.integers(len(ops)))]
        if op == "selected" and not have:
            op = "lattice"
        log.append(op)
        if op == "lattice":
            period = (int(rng.integers(1, 9)), int(rng.integers(1, 9)))
            phase = (int(rng.integers(period[0])), int(rng.integers(period[1])))
            tiers = int(rng.choice([1, 1, 4]))
            for r in pair:
                r.set_select_tiers(tiers, 8)
            select(pair, period, phase)
            have = True
        elif op == "noisy":
            dilate = int(rng.integers(0, 3))
            assert a.select_noisy(0.05, dilate) == b.select_noisy(0.05, dilate)
            have = True
        elif op == "mask":
            m = rng.random(size) < 0.4
            assert a.select_mask(m) == b.select_mask(m)
            have = True
        elif op == "selected":
            n = int(rng.choice([0, 1, 3, 8]))
            for r in pair:
                r.sample_selected(n)
            assert ck.counters(a) == ck.counters(b), log
        elif op == "refresh":
            for r in pair:
                r.refresh()
        elif op == "reproject":
            cam = cams[0]
            cams.reverse()
            for r in pair:
                r.reproject(cam, max_history=8.0)
        else:
            size = (23, 19) if size == (w, h) else (w, h)
            for r in pair:
                r.set_config(other if size == (23, 19) else cfg)
                r.refresh()
                r.sample(1)
            have = False
            assert ck.code(lambda: a.sample_selected(1)) == ESTATE
        if have:
            same_selection(pair, f"after {log}")
        same_frame(pair, f"after {log}")
    assert {"lattice", "noisy", "mask", "selected", "refresh", "reproject", "config"} <= set(log)


def _state(r):
    buffers = (BUF_IMAGE_BUFFER, BUF_IMAGE_PIXELS, BUF_MOMENTS, BUF_HALF_BUFFER, BUF_SELECTION)
    return {b: r._read(b) for b in buffers}, ck.counters(r), [r.counter("select_tier%d" % t) for t in range(8)]


def _unchanged(r, state, what):
    buffers, counters, tiers = state
    assert ck.counters(r) == counters and [r.counter("select_tier%d" % t) for t in range(8)] == tiers, what
    for b, want in buffers.items():
        ck.same(r._read(b), want, f"buffer {b} after {what}")


def test_refused_values_value_0_and_tiles_change_nothing():
    w, h = 33, 17
    pair = twins(w, h)
    a, b = pair
    m = np.random.default_rng(72).random((w, h)) < 0.3
    for r in pair:
        r.set_select_tiers(4, 8)
        r.sample(2)
        r.select_mask(m.astype(np.uint8) * 2, raw=True)      # an earlier selection, in tier 1
        r.sample_selected(4)
        r.post_process()
    state = _state(a)
    for value in (0x10, 0x01, 0x19, 0x91, 0x222, 0x2022, 0x10022, -1, -0x22, 1 << 40):
        with pytest.raises(RtpbrError, match=r"select_lattice must be 0 \(nothing\) or px \+ 16 \* py") as e:
            a.set_option("select_lattice", value)
        assert e.value.code == EINVAL, hex(value)
    _unchanged(a, state, "invalid values")
    a.set_option("select_lattice", 0)
    _unchanged(a, state, "value 0")
    a.set_tiles(16, 16, 0, 2)
    with pytest.raises(RtpbrError, match="not with tiles of world > 1") as e:
        a.set_option("select_lattice", 0x22)
    assert e.value.code == ESTATE
    a.set_option("select_lattice", 0)                          # still nothing
    a.set_tiles(0, 0, 0, 1)
    _unchanged(a, state, "the refusal with tiles")
    # ... and the earlier selection still traces: the twin made the accepted calls only
    for r in pair:
        r.sample_selected(4)
    assert ck.counters(a) == ck.counters(b)
    same_frame(pair, "after the next selected launch")
    # the lattice replaces it
    select(pair, (3, 2), (2, 1))
    same_selection(pair, "the lattice over the earlier selection")
    for r in pair:
        r.sample_selected(2)
    same_frame(pair, "after the lattice's launch")
