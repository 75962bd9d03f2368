"""State changes between C-ABI calls, HIP against the CPU oracle (run with -m gpu): the random call sequences of
tests/call_sequences.py in lock step, the post sequences (reproject, noise, selection, present) and the motion sequences
(reproject_scene, set_noise_tracking, tracked sample calls) against the models of tests/post_model.py, one sequence of each kind
through the run-time compiled instances, and named regressions for what such sequences found.  Frames are tiny and max_raytrace <= 4, so the oracle answers every observation in milliseconds."""
import numpy as np
import pytest

import call_sequences as cs
import post_model as pm
from oracle_backend import OracleRenderer
from raytracingpbr_amd import Renderer
from raytracingpbr_amd.ibl import synthetic_env

pytestmark = pytest.mark.gpu


def _pair(s):
    return cs.new_renderer(s, Renderer), cs.new_renderer(s, OracleRenderer)


@pytest.mark.parametrize("seed", range(24))
def test_random_call_sequence_matches_oracle(seed):
    """~60 random operations over configuration, scene, camera, environment, tiles, buffers written back, sample_base and HIP-only
    options: every observation bit for bit the oracle's, every refused call refused alike, features and denoise equal to the CPU
    reference of the state at the time"""
    s = cs.script(seed)
    a, b = _pair(s)
    try:
        seen = cs.run(s, a, b)
    finally:
        a.close()
        b.close()
    assert any(k == "counters" for _, k, _ in seen)


def test_jit_call_sequence_matches_oracle(tmp_path, monkeypatch):
    """jit = -1 over two scenes that no ahead-of-time specialisation serves (7 and 8 mixed shapes), persistent-ray form: the run-time
    instance is acquired and released at scene changes, with lazy shadings of one-step launches pending across them"""
    monkeypatch.setenv("RTPBR_JIT_CACHE", str(tmp_path))
    s = cs.script(1001, n_ops=50, jit=-1, scenes=("mixed7", "mixed8"), forms=(1,))
    a, b = _pair(s)
    try:
        cs.run(s, a, b)
        a.set_option("scheduler", -1)
        a.set_tiles(0, 0, 0, 1)
        a.set_config(a.config.copy(sky_kind=2))
        a.sample(1)
        assert a.counter("jit_active") == 1
    finally:
        a.close()
        b.close()


def _run_post(s):
    a, b = cs.new_renderer(s, Renderer), pm.model(s)
    try:
        return cs.run_post(s, a, b), a
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("seed", range(24))
def test_random_post_sequence_matches_model(seed):
    """~60 random operations, half of them those of the sequences above, half rtpbr_reproject, the noise calls, the estimator
    setting, the select calls, rtpbr_sample_selected, rtpbr_present and reads of the buffers they own: every call refused or
    accepted as include/rtpbr.h says, every value it returns or leaves behind bit for bit the model's"""
    seen, _ = _run_post(cs.post_script(seed))
    assert any(k == "image_buffer" for _, k, _ in seen) and any(k == "presented" or k == "moments" for _, k, _ in seen)


def test_jit_post_sequence_matches_model(tmp_path, monkeypatch):
    """the same through run-time compiled instances (jit = -1, 7 and 8 mixed shapes, both kernel forms)"""
    monkeypatch.setenv("RTPBR_JIT_CACHE", str(tmp_path))
    seen, _ = _run_post(cs.jit_post_script())
    assert any(k == "motion" for _, k, _ in seen)


@pytest.mark.parametrize("seed", range(24))
def test_random_motion_sequence_matches_model(seed):
    """~60 random operations, a third of them those of the first sequences, a third those of the post sequences, a third
    rtpbr_reproject_scene on an accumulating pose (fuzz scenes, both normal spaces, tables that are no rigid motion),
    rtpbr_set_noise_tracking and tracked rtpbr_sample / rtpbr_sample_selected calls with what they refuse: every call refused or
    accepted as include/rtpbr.h says, every value it returns or leaves behind bit for bit the model's"""
    seen, _ = _run_post(cs.motion_script(seed))
    assert any(k == "image_buffer" for _, k, _ in seen) and any(k == "moments" for _, k, _ in seen)


def test_jit_motion_sequence_matches_model(tmp_path, monkeypatch):
    """the same through run-time compiled instances (jit = -1, 7 and 8 mixed shapes, both kernel forms): a moved table is a scene
    the instance was not acquired for"""
    monkeypatch.setenv("RTPBR_JIT_CACHE", str(tmp_path))
    seen, _ = _run_post(cs.jit_motion_script())
    assert any(k == "motion" for _, k, _ in seen) and any(k == "moments" for _, k, _ in seen)


def _counters(r):
    c = r.counters()
    return tuple(getattr(c, k) for k in cs.COUNTERS)


@pytest.mark.parametrize("steps", [0, -1])
@pytest.mark.parametrize("first", ["complete_path", "persistent_ray"])
def test_persistent_call_without_bounce_steps_leaves_the_counters_dirty(first, steps):
    """rtpbr_sample() marked the next counter buffer as zeroed after every persistent-ray call with n > 0, but a call with
    steps_per_launch <= 0 enqueues no kernel to zero it: the call after it then started from an earlier call's work counters and
    claim counter (complete path: its waves found the queue drained and the accumulate pass re-added old staging).  Three calls —
    `first` form, the persistent-ray form with no bounce-steps, `first` form again — image_buffer and counters after every one
    bit for bit the oracle's."""
    sc = cs.scene("src")
    form = 0 if first == "complete_path" else 1
    cfg = cs.base_config("src", 40, 24, 3).copy(kernel_form=form, steps_per_launch=2)
    g, o = Renderer(sc, cfg), OracleRenderer(sc, cfg)
    g.set_option("jit", 0)
    try:
        for r in (g, o):
            r.set_env(synthetic_env(64, 32, seed=0), 1.4, 2.2)
        for i, (c, n) in enumerate(((cfg, 3), (cfg.copy(kernel_form=1, steps_per_launch=steps), 1), (cfg, 3))):
            for r in (g, o):
                r.set_config(c)
                r.sample(n)
            assert _counters(g) == _counters(o), (i, _counters(g), _counters(o))
            assert np.array_equal(g.image_buffer.view(np.uint32), o.image_buffer.view(np.uint32)), i
        assert np.array_equal(g.ray_buffer.view(np.uint32), o.ray_buffer.view(np.uint32))
    finally:
        g.close()
        o.close()


@pytest.mark.parametrize("launch", ["one_step", "fused"])
@pytest.mark.parametrize("scene", ["src", "mixed10"])
def test_src_op_bits_are_independent(scene, launch):
    """option src_op 0..7 (object-parallel evaluation, pool-kernel variant, per-lane lean loop) on a scene of <= 8 and one of > 8
    objects, in one-step (wavefront split) and fused launches: image_buffer, ray_buffer and the counters are the oracle's"""
    sc = cs.scene(scene)
    cfg = cs.base_config("src", 40, 24, 11).copy(steps_per_launch=1 if launch == "one_step" else 4)
    calls = (1, 1, 1, 2, 1) if launch == "one_step" else (2, 3)

    def go(r):
        for n in calls:
            r.sample(n)
        return r.image_buffer, r.ray_buffer, _counters(r)

    want = go(OracleRenderer(sc, cfg))
    for op in range(8):
        g = Renderer(sc, cfg)
        g.set_option("jit", 0)
        g.set_option("src_op", op)
        got = go(g)
        g.close()
        assert got[2] == want[2], (op, got[2], want[2])
        for k, x, y in zip(("image_buffer", "ray_buffer"), got[:2], want[:2]):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (op, k)
