"""Adaptive sampling of the complete-path form on the GPU (rtpbr_select_mask, rtpbr_select_noisy, rtpbr_sample_selected,
Renderer.render_adaptive).  Every comparison is ``==`` on bit patterns: a selected launch against image buffers composed from
the unchanged CPU oracle (full-frame samples at the same sample base, ``np.where(mask, after, before)``), the selection against
the numpy restatement of the rule (tests/select_ref_lib.py) on the GPU's own noise buffer."""
import numpy as np
import pytest

import checks as ck
import select_ref_lib as sr
import test_gpu_features_denoise as fd
import test_gpu_reproject as rp
from cases import all_cases
from checks import EINVAL, ESTATE
from oracle_backend import OracleRenderer
from raytracingpbr_amd import Config, Renderer, cornell_box, src_scene
from raytracingpbr_amd._capi import RtpbrError
from raytracingpbr_amd.renderer import (BUF_DIFF_BUFFER, BUF_DIFF_PIXELS, BUF_IMAGE_BUFFER, BUF_IMAGE_PIXELS, BUF_MOMENTS, BUF_NOISE,
                                        BUF_RAY_BUFFER, BUF_SELECTION)

pytestmark = pytest.mark.gpu


def _small_cases():
    """every complete-path case of tests/cases.py, 40 pixels wide"""
    out = {}
    for c in all_cases():
        if c.cfg.kernel_form == 0:
            h = max(8, round(c.cfg.height * 40 / c.cfg.width))
            out[c.name] = (c, c.cfg.copy(width=40, height=h))
    return out


def _random_mask(w, h, seed, share=0.3):
    return (np.random.default_rng(seed).random((w, h)) < share).astype(np.uint8)


def _run(r, steps, oracle):
    """steps: ("sample", n) | ("select", mask) | ("selected", n).  On the oracle a selected launch is: keep the buffer, sample the
    full frame at the same sample base, take the new values where the mask is set.  Returns image_buffer."""
    base, mask = 0, None
    for s in steps:
        if s[0] == "select":
            mask = s[1]
            if not oracle:
                assert r.select_mask(mask) == int((mask != 0).sum())
                assert np.array_equal(r.selection, (mask != 0).astype(np.uint8))
        elif oracle:
            before = r.image_buffer
            r.set_sample_base(base)
            r.sample(s[1])
            if s[0] == "selected":
                r.image_buffer = np.where((mask != 0)[..., None], r.image_buffer, before)
            base += s[1]
        elif s[0] == "sample":
            r.sample(s[1])
        else:
            r.sample_selected(s[1])
            c = r.counters()
            assert c.samples == c.deposits == int((mask != 0).sum()) * s[1]
    return r.image_buffer


def _sequence(w, h, seed=1):
    a, b = _random_mask(w, h, seed), _random_mask(w, h, seed + 100, 0.5)
    return [("sample", 4), ("select", a), ("selected", 3), ("sample", 2), ("select", b), ("selected", 5)]


_expected = {}


def _oracle_image(name, steps_key, steps):
    if (name, steps_key) not in _expected:
        case, cfg = _small_cases()[name]
        _expected[name, steps_key] = _run(case.setup(OracleRenderer(case.scene, cfg)), steps, True)
    return _expected[name, steps_key]


# ------------------------------------------------------------------ 1. host masks against the oracle
@pytest.mark.parametrize("name", list(_small_cases()))
def test_host_masks_bit_identical_to_composed_oracle(name):
    case, cfg = _small_cases()[name]
    steps = _sequence(cfg.width, cfg.height)
    got = _run(case.setup(Renderer(case.scene, cfg)), steps, False)
    ck.same(got, _oracle_image(name, "seq", steps), "image_buffer")
    assert len(np.unique(got[..., 3])) >= 3      # pixels with 6, 9, 11 and 14 samples


CORNELL = "c1_cornell_v3_256_16spp_4b"


def _special_masks(w, h):
    one = np.zeros((w, h), np.uint8)
    one[w // 3, h - 2] = 200                      # any nonzero byte selects
    column = np.zeros((w, h), np.uint8)
    column[w - 1, :] = 1                          # the last column: the end of the buffer
    row = np.zeros((w, h), np.uint8)
    row[:, 0] = 1                                 # y = 0 of every column: one entry per 'height' indices
    return {"empty": np.zeros((w, h), np.uint8), "full": np.ones((w, h), np.uint8), "one_pixel": one, "edge_column": column,
            "bottom_row": row}


@pytest.mark.parametrize("which", ["empty", "full", "one_pixel", "edge_column", "bottom_row"])
def test_special_masks(which):
    case, cfg = _small_cases()[CORNELL]
    mask = _special_masks(cfg.width, cfg.height)[which]
    steps = [("sample", 4), ("select", mask), ("selected", 3), ("sample", 2)]       # (the last step: sample_base advanced for everybody)
    r = case.setup(Renderer(case.scene, cfg))
    got = _run(r, steps[:3], False)
    sel_counters = ck.counters(r)
    ck.same(got, _oracle_image(CORNELL, which + "/3", steps[:3]), "image_buffer after the selected launch")
    r.sample(2)
    ck.same(r.image_buffer, _oracle_image(CORNELL, which + "/4", steps), "image_buffer after the next full-frame launch")
    if which == "empty":
        assert sel_counters == [0] * 6
    if which == "full":           # rtpbr_sample itself, counters included (HIP and oracle)
        plain = case.setup(Renderer(case.scene, cfg))
        plain.sample(4)
        plain.sample(3)
        ck.same(got, plain.image_buffer, "image_buffer against rtpbr_sample")
        assert sel_counters == ck.counters(plain)
        o = case.setup(OracleRenderer(case.scene, cfg))
        o.sample(4)
        o.sample(3)
        assert sel_counters == ck.counters(o)


def test_a_selection_survives_full_frame_calls_and_is_replaced_by_the_next():
    case, cfg = _small_cases()[CORNELL]
    a, b = _random_mask(cfg.width, cfg.height, 5), _random_mask(cfg.width, cfg.height, 6)
    steps = [("select", a), ("selected", 2), ("sample", 1), ("selected", 2), ("select", b), ("selected", 1)]
    got = _run(case.setup(Renderer(case.scene, cfg)), steps, False)
    ck.same(got, _oracle_image(CORNELL, "survives", steps), "image_buffer")


# ------------------------------------------------------------------ 2. options that must neither fail a selected launch nor change its bits
OPTION_SETS = [{"scheduler": 0}, {"scheduler": 1}, {"primary_split": 0}, {"primary_split": 2}, {"stage_dense": 1}, {"chunk": 7},
               {"staging_bytes": 1 << 20}, {"specialize": 0}, {"jit": 0}, {"jit": 1}, {"jit": 1, "jit_bake": 1}, {"jit": 1, "stage_dense": 1}]


@pytest.mark.parametrize("options", OPTION_SETS, ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_options_do_not_change_the_bits(options):
    case, cfg = _small_cases()[CORNELL]
    steps = _sequence(cfg.width, cfg.height)
    r = case.setup(Renderer(case.scene, cfg))
    for k, v in options.items():
        r.set_option(k, v)
    ck.same(_run(r, steps, False), _oracle_image(CORNELL, "seq", steps), f"image_buffer with {options}")


def test_many_sub_launches_of_a_selected_call():
    """a staging budget of 1 MiB holds ~74 898 items: 1300 selected pixels x 200 samples run as four sub-launches"""
    scene, cfg = cornell_box("v3"), Config.cornell_v3(64, 64, 0, 3)
    mask = _random_mask(64, 64, 9, 0.32)
    got = []
    for budget in (1 << 20, 1 << 30):
        r = Renderer(scene, cfg)
        r.set_option("staging_bytes", budget)
        r.sample(1)
        r.select_mask(mask)
        r.sample_selected(200)
        c = r.counters()
        assert c.samples == c.deposits == int(mask.sum()) * 200
        r.sample(1)                       # the context's own geometry is back: the full frame, sample 201
        got.append(r.image_buffer)
    ck.same(got[0], got[1], "image_buffer, four sub-launches against one")
    assert np.array_equal(got[0][..., 3], np.where(mask != 0, 202, 2))


# ------------------------------------------------------------------ 3. select_noisy against the numpy rule
def _check_noisy(r, quantile, dilate, trace):
    r.noise_estimate(0.0)
    noise = r.noise
    thr = float(np.quantile(noise[noise > 0], quantile)) if (noise > 0).any() else 0.0
    n = r.select_noisy(thr, dilate)
    ib = r.image_buffer
    ck.same(r.noise, noise, "noise written by select_noisy")
    want = sr.select(r.noise, ib[..., 3], thr, dilate)
    got = r.selection
    assert got.dtype == np.uint8 and np.array_equal(got, want), f"{int((got != want).sum())} pixels differ"
    assert n == int(want.sum())
    if trace:
        # the device list covers exactly the mask: one more sample where it is set, the same bits elsewhere
        r.sample_selected(1)
        after = r.image_buffer
        assert np.array_equal(after[..., 3] - ib[..., 3], want.astype(np.float32))
        keep = want == 0
        assert np.array_equal(ck.bits(after)[keep], ck.bits(ib)[keep])
        c = r.counters()
        assert c.samples == c.deposits == n
    return want


@pytest.mark.parametrize("name", list(fd._scenes(fd.W, fd.H)))
def test_select_noisy_on_every_scene_kind(name):
    scene, cfg = fd._scenes(fd.W, fd.H)[name]
    r = fd._renderer(scene, cfg)
    complete = cfg.kernel_form == 0
    for _ in range(3):
        r.sample(2 if complete else 6)
        r.noise_update()
    sizes = []
    for dilate in range(4):
        sizes.append(int(_check_noisy(r, 0.8, dilate, complete).sum()))
    print(name, "selected with dilate 0..3:", sizes)
    assert 0 < sizes[0] < fd.W * fd.H and sizes == sorted(sizes)
    if not complete:
        with pytest.raises(RtpbrError) as e:
            r.sample_selected(1)
        assert e.value.code == ESTATE


def test_select_noisy_at_1080p():
    scene, cfg = cornell_box("v3", aspect=1920 / 1080), Config.cornell_v3(1920, 1080, 0, 3)
    r = fd._renderer(scene, cfg)
    for _ in range(2):
        r.sample(2)
        r.noise_update()
    want = _check_noisy(r, 0.9, 1, True)
    assert 0 < int(want.sum()) < 1920 * 1080


def test_pixels_without_history_are_selected_after_a_reprojection():
    scene, cfg = cornell_box("v3", aspect=fd.W / fd.H), Config.cornell_v3(fd.W, fd.H, 0, 3)
    old, new = rp.MOVES["translate"](scene.camera)
    r = rp._with_history(scene, cfg, old, 0)
    for _ in range(3):
        r.sample(2)
        r.noise_update()
    r.reproject(new, max_history=5.0)
    empty = ~(r.image_buffer[..., 3] > 0)
    assert empty.any() and not empty.all()
    want = _check_noisy(r, 0.95, 0, True)
    assert (want[empty] == 1).all() and int(want.sum()) > int(empty.sum())
    assert (r.image_buffer[..., 3][empty] == 1).all()


# ------------------------------------------------------------------ 4. render_adaptive
def test_render_adaptive_holds_a_prefix_of_every_pixels_samples():
    """Cornell v3 256x256 to noise 0.1 in batches of 16, dilate 0: the active set only shrinks (a deselected pixel's moments no
    longer change), so every pixel holds the first `count` samples of its own sequence — the oracle's image_buffer after `count`
    samples of the same seed, compared by groups of equal count at the batch boundaries."""
    scene, cfg = cornell_box("v3"), Config.cornell_v3(256, 256, 0, 3)
    noise, max_spp, batch = 0.1, 2048, 16
    r = Renderer(scene, cfg)
    r.refresh()
    traced, st = r.render_adaptive(noise, max_spp, batch_spp=batch, dilate=0)
    ib = r.image_buffer
    count = ib[..., 3]
    counts = np.unique(count)
    print(f"render_adaptive: {traced} pixel-samples, counts {counts.min():.0f}..{counts.max():.0f} in {len(counts)} groups, "
          f"{st.pixels_above} pixels above, max noise {st.max_noise:.4f}")
    assert st.pixels_above == 0
    assert traced == int(count.astype(np.float64).sum())
    assert counts.min() >= 2 * batch and (counts % batch == 0).all() and counts.max() <= max_spp
    u = Renderer(scene, cfg)
    u.refresh()
    spp, ust = u.render_until(noise, max_spp, batch_spp=batch)
    print(f"render_until: {spp} spp = {spp * 256 * 256} pixel-samples, {ust.pixels_above} pixels above")
    assert traced < spp * 256 * 256
    o = OracleRenderer(scene, cfg)
    done = 0
    for c in counts:
        while done < int(c):
            o.sample(batch)
            done += batch
        group = count == c
        bad = ck.bits(ib)[group] != ck.bits(o.image_buffer)[group]
        assert not bad.any(), f"pixels with {int(c)} samples: {int(bad.any(axis=-1).sum())} of {int(group.sum())} differ from the oracle"


def test_render_adaptive_with_dilation_and_a_budget():
    scene, cfg = cornell_box("v3"), Config.cornell_v3(64, 64, 0, 3)
    r = Renderer(scene, cfg)
    r.refresh()
    r.track_noise = True
    traced, st = r.render_adaptive(0.05, 100, batch_spp=16, dilate=1)       # 100 spp do not reach 0.05: the budget ends it
    count = r.image_buffer[..., 3]
    assert r.track_noise is True
    assert count.max() == 96 and count.min() >= 32 and traced == int(count.sum())
    assert st.pixels_above > 0
    with pytest.raises(ValueError):
        r.render_adaptive(0.05, 0)


def test_sample_selected_honours_track_noise():
    scene, cfg = cornell_box("v3"), Config.cornell_v3(48, 32, 0, 3)
    r = Renderer(scene, cfg)
    r.track_noise = True
    r.sample(2)
    mask = _random_mask(48, 32, 2)
    r.select_mask(mask)
    r.sample_selected(3)
    K = r.moments[..., 3]
    assert np.array_equal(K, np.where(mask != 0, 2, 1).astype(np.float32))


# ------------------------------------------------------------------ 5. errors; a refused call changes nothing
def _code(call, *a):
    with pytest.raises(RtpbrError) as e:
        call(*a)
    return e.value.code


def test_state_rules():
    scene, cfg = cornell_box("v3"), Config.cornell_v3(32, 24, 0, 3)
    r = Renderer(scene, cfg)
    assert _code(r._read, BUF_SELECTION) == ESTATE                   # not allocated before the first select call
    assert _code(r.sample_selected, 1) == ESTATE                     # no selection yet
    assert r.image_buffer[..., 3].max() == 0
    mask = _random_mask(32, 24, 3)
    assert r.select_mask(mask) == int(mask.sum())
    assert _code(r._write, BUF_SELECTION, mask) == EINVAL            # an output only
    r.sample_selected(2)
    # the same resolution keeps the selection, a new one frees the buffer and drops it
    r.set_config(cfg.copy(seed=5))
    r.sample_selected(1)
    assert np.array_equal(r.image_buffer[..., 3], 3 * mask.astype(np.float32))
    r.set_config(Config.cornell_v3(40, 24, 0, 3))
    assert _code(r._read, BUF_SELECTION) == ESTATE
    assert _code(r.sample_selected, 1) == ESTATE
    assert r.select_noisy(0.0) == 40 * 24 and r.selection.shape == (40, 24)      # no samples anywhere: everything is selected


def test_errors_and_a_refused_call_changes_nothing():
    import ctypes as C
    scene, cfg = cornell_box("v3"), Config.cornell_v3(32, 24, 0, 3)
    r = Renderer(scene, cfg)
    for _ in range(2):
        r.sample(2)
        r.noise_update()
    mask = _random_mask(32, 24, 4)
    r.select_noisy(0.05, 1)
    r.select_mask(mask)
    r.sample_selected(1)
    r.post_process()
    buffers = (BUF_IMAGE_BUFFER, BUF_IMAGE_PIXELS, BUF_RAY_BUFFER, BUF_DIFF_BUFFER, BUF_DIFF_PIXELS, BUF_MOMENTS, BUF_NOISE, BUF_SELECTION)
    keep = {b: r._read(b) for b in buffers}
    counters = ck.counters(r)
    nan = float("nan")
    n = C.c_uint32(77)
    m = np.ascontiguousarray(mask)
    ptr = m.ctypes.data_as(C.c_void_p)
    raw = r.api.fn
    assert raw["select_mask"](r._ctx, None, m.nbytes, C.byref(n)) == EINVAL
    assert raw["select_mask"](r._ctx, ptr, m.nbytes, None) == EINVAL
    assert raw["select_mask"](None, ptr, m.nbytes, C.byref(n)) == EINVAL
    for nbytes in (m.nbytes - 1, m.nbytes + 1, 0):
        assert raw["select_mask"](r._ctx, ptr, nbytes, C.byref(n)) == EINVAL
    assert raw["select_noisy"](r._ctx, 0.1, 0, None) == EINVAL
    assert raw["select_noisy"](None, 0.1, 0, C.byref(n)) == EINVAL
    assert raw["sample_selected"](None, 1) == EINVAL
    for thr in (-1.0, nan):
        assert _code(r.select_noisy, thr, 0) == EINVAL
    for dilate in (-1, 4):
        assert _code(r.select_noisy, 0.1, dilate) == EINVAL
    assert _code(r.sample_selected, -1) == EINVAL
    with pytest.raises(ValueError):
        r.select_mask(np.zeros((24, 32), np.uint8))
    assert n.value == 77
    r.set_tiles(16, 16, 0, 2)
    assert _code(r.select_mask, mask) == ESTATE
    assert _code(r.select_noisy, 0.1) == ESTATE
    assert _code(r.sample_selected, 1) == ESTATE
    r.set_tiles(0, 0, 0, 1)
    r.set_option("precision", 1)
    assert _code(r.sample_selected, 1) == ESTATE
    r.set_option("precision", 0)
    assert ck.counters(r) == counters
    for b, a in keep.items():
        ck.same(r._read(b), a, f"buffer {b} after refused calls")
    # ... and the sample index did not move: the next selected launch gives what it gives on a context that made the accepted calls only
    twin = Renderer(scene, cfg)
    for _ in range(2):
        twin.sample(2)
    twin.select_mask(mask)
    twin.sample_selected(1)
    for x in (r, twin):
        x.sample_selected(1)
    ck.same(r.image_buffer, twin.image_buffer, "image_buffer one selected launch after the refused calls")


def test_refused_before_the_context_is_set_up():
    import ctypes as C
    from raytracingpbr_amd import _capi
    api = _capi.hip_api()
    ctx = C.c_void_p()
    api.call("create", 0, C.byref(ctx))
    try:
        n = C.c_uint32()
        m = np.zeros(16, np.uint8)
        assert api.fn["select_mask"](ctx, m.ctypes.data_as(C.c_void_p), 16, C.byref(n)) == ESTATE
        assert api.fn["select_noisy"](ctx, 0.1, 0, C.byref(n)) == ESTATE
        assert api.fn["sample_selected"](ctx, 1) == ESTATE
        cfg = Config.cornell_v3(4, 4, 0, 3)
        api.call("set_config", ctx, C.byref(cfg))
        assert api.fn["select_mask"](ctx, m.ctypes.data_as(C.c_void_p), 16, C.byref(n)) == ESTATE      # no scene, no camera
        assert api.fn["sample_selected"](ctx, 1) == ESTATE
    finally:
        api.call("destroy", ctx)


def test_persistent_form_is_refused():
    scene, cfg = src_scene(aspect=40 / 24), Config.src(40, 24, 7, steps_per_launch=1)
    r = fd._renderer(scene, cfg)
    r.sample(2)
    assert r.select_mask(np.ones((40, 24), np.uint8)) == 40 * 24
    before = r.image_buffer
    assert _code(r.sample_selected, 1) == ESTATE
    ck.same(r.image_buffer, before, "image_buffer")


def test_selected_launches_are_timed_and_asynchronous_reads_are_respected():
    scene, cfg = cornell_box("v3"), Config.cornell_v3(128, 128, 0, 3)
    r = Renderer(scene, cfg)
    r.sample(2)
    mask = _random_mask(128, 128, 8)
    r.select_mask(mask)
    host = r.host_array(BUF_IMAGE_BUFFER)
    before = r.image_buffer
    t = r.read_async(BUF_IMAGE_BUFFER, host)       # the selected launch that follows must not overtake this copy
    r.sample_selected(4)
    r.read_wait(t)
    ck.same(host, before, "asynchronously read image_buffer")
    trace_ms, total_ms, launches = r.last_sample_ms()
    assert launches == 1 and 0 < trace_ms <= total_ms
    r.select_mask(np.zeros((128, 128), np.uint8))
    r.sample_selected(4)
    assert r.last_sample_ms()[2] == 0
