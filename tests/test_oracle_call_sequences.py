"""The call-sequence generator of tests/call_sequences.py on the CPU alone: scripts are reproducible from their seed, every
operation is legal where it is meant to be, the illegal ones are refused with the code the script expects, and two oracles of
different thread counts driven in lock step observe the same bits throughout."""
import numpy as np
import pytest

import call_sequences as cs
from oracle_backend import OracleRenderer
from raytracingpbr_amd import Config, cornell_box
from raytracingpbr_amd._capi import RtpbrError


def test_scripts_are_reproducible_from_their_seed():
    for seed in range(8):
        a, b = cs.script(seed), cs.script(seed)
        assert [repr(o) for o in a.ops] == [repr(o) for o in b.ops] and bytes(a.base) == bytes(b.base)
    assert [repr(o) for o in cs.script(1).ops] != [repr(o) for o in cs.script(2).ops]


def test_the_grammar_is_covered():
    """over the seeds the GPU tier runs, every kind of operation, both kernel forms, steps_per_launch 0, every resolution, every
    scene of the pool, every HIP-only option and every kind of refused call appear"""
    kinds, over, scenes, options, errors = set(), [], set(), set(), set()
    for seed in range(24):
        s = cs.script(seed)
        scenes.add(s.scene0)
        for o in s.ops:
            kinds.add(o.kind)
            if o.kind == "set_config":
                over.append(o.args["over"])
            if o.kind == "set_scene":
                scenes.add(o.args["name"])
            if o.kind == "option":
                options.add(o.args["key"])
            if o.expect is not None:
                errors.add((o.kind, o.expect))
    assert kinds >= {"set_config", "set_scene", "set_camera", "set_env", "set_shape_data", "set_tiles", "refresh", "sample",
                     "post_process", "write_image", "write_rays", "sample_base", "option", "observe", "features", "denoise", "bad_scene"}
    assert {d.get("kernel_form", None) for d in over} >= {0, 1} and any(d.get("steps_per_launch", 1) == 0 for d in over)
    assert {(d.get("width"), d.get("height")) for d in over if "width" in d} >= {(w, h) for w, h in cs.SIZES} - {(None, None)}
    assert scenes == set(cs.SCENES) and options == set(cs.OPTIONS)
    assert errors >= {("sample", cs.EINVAL), ("sample", cs.ESTATE), ("set_config", cs.EINVAL), ("set_tiles", cs.EINVAL),
                      ("set_shape_data", cs.EINVAL), ("set_env", cs.EINVAL), ("bad_scene", cs.EINVAL), ("denoise", cs.ESTATE)}


@pytest.mark.parametrize("seed", [0, 3, 5, 10])
def test_two_oracles_agree_along_a_script(seed):
    """lock step of a 1-thread and a 4-thread oracle: same codes for every refused call, same bits at every observation; and the
    same script run again observes the same values (determinism)"""
    s = cs.script(seed, n_ops=40)
    a, b = cs.new_renderer(s, OracleRenderer, threads=1), cs.new_renderer(s, OracleRenderer, threads=4)
    seen = cs.run(s, a, b)
    assert any(k == "counters" for _, k, _ in seen)
    again = cs.run(s, cs.new_renderer(s, OracleRenderer, threads=3), cs.new_renderer(s, OracleRenderer, threads=2))
    assert [(i, k) for i, k, _ in again] == [(i, k) for i, k, _ in seen]
    for (_, k, x), (_, _, y) in zip(seen, again):
        assert cs._first_diff(x, y) is None, k


def test_a_mismatch_report_names_seed_operation_and_replay():
    """the report of a difference: seed, operation index, the operations since the last observation that matched, which buffer,
    how many words and where"""
    s = cs.script(3, n_ops=30)
    a, b = cs.new_renderer(s, OracleRenderer), cs.new_renderer(s, OracleRenderer)
    b.set_sample_base(12345)         # b draws other random numbers from here on
    with pytest.raises(cs.Mismatch) as e:
        cs.run(s, a, b)
    msg = str(e.value)
    assert "call sequence seed 3, operation #" in msg and "words differ, first at" in msg
    assert "BASE = Config.from_buffer_copy" in msg and "replay: call_sequences.replay(" in msg


def test_refused_set_config_keeps_the_renderer_usable():
    """Renderer.set_config kept the new configuration before the library had accepted it: after a refused one (width 0) every
    buffer read failed on a size mismatch.  The refused call must leave the renderer as it was."""
    cfg = Config.cornell_v3(23, 17, 0, 3)
    r = OracleRenderer(cornell_box("v3"), cfg)
    r.sample(1)
    before = r.image_buffer
    with pytest.raises(RtpbrError) as e:
        r.set_config(cfg.copy(width=0))
    assert e.value.code == cs.EINVAL
    assert r.config.width == 23 and np.array_equal(r.image_buffer.view(np.uint32), before.view(np.uint32))


@pytest.mark.parametrize("steps", [0, -1, -3])
def test_oracle_call_without_bounce_steps_changes_nothing(steps):
    """steps_per_launch <= 0 means no bounce-steps (include/rtpbr.h; the HIP library enqueues nothing): the oracle moved the sample
    index back by n * steps_per_launch when that product was negative, so every later call drew other random numbers than the
    HIP library's.  A call of no bounce-steps leaves image_buffer, ray_buffer and the sample index as they were and counts nothing."""
    sc = cs.scene("src")
    cfg = cs.base_config("src", 23, 17, 4).copy(steps_per_launch=2)
    a, b = OracleRenderer(sc, cfg), OracleRenderer(sc, cfg)
    a.sample(2)
    b.sample(2)
    before = (a.image_buffer, a.ray_buffer)
    a.set_config(cfg.copy(steps_per_launch=steps))
    a.sample(3)
    assert all(v == 0 for v in (getattr(a.counters(), k) for k in cs.COUNTERS))
    assert np.array_equal(a.image_buffer.view(np.uint32), before[0].view(np.uint32))
    assert np.array_equal(a.ray_buffer.view(np.uint32), before[1].view(np.uint32))
    a.set_config(cfg)
    a.sample(2)
    b.sample(2)
    assert np.array_equal(a.image_buffer.view(np.uint32), b.image_buffer.view(np.uint32))
    assert np.array_equal(a.ray_buffer.view(np.uint32), b.ray_buffer.view(np.uint32))
