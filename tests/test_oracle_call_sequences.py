"""The call-sequence generator of tests/call_sequences.py on the CPU alone: scripts are reproducible from their seed, every
operation is legal where it is meant to be, the illegal ones are refused with the code the script expects, and two oracles of
different thread counts driven in lock step observe the same bits throughout.  The post scripts (reproject, noise, selection,
present) and the motion scripts (reproject_scene, set_noise_tracking and the tracked sample calls) run on the models of
tests/post_model.py alone: they are executable, deterministic and independent of the oracle's thread count, the 24 committed seeds
of each meet their coverage conditions, and three deliberately wrong models show that the motion scripts observe the state in
question."""
import hashlib

import numpy as np
import pytest

import call_sequences as cs
import post_model as pm
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


# ------------------------------------------------------------------ the post scripts on the model alone
# sha256 over repr() of every operation of script(0..23) and of the JIT script, one per line, computed at the commit before
# post_script existed (dced5ff): the old scripts draw what they drew.
OLD_SCRIPTS_SHA256 = "e199981cde07179b809aa7b220afd0c7753f1efd5243eb1245396f51c893b6d4"
# the same over post_script(0..23) and jit_post_script(), computed at the commit before motion_script existed (91e0d4b), whose
# draws moved into _Grammar.post_op() unchanged
POST_SCRIPTS_SHA256 = "92f29685c2e9a9d3d7d21dab889d2e7efb5bcb944f4b9ddc0993dc738306819b"
POST_SEEDS = range(24)
MOTION_SEEDS = range(24)


def test_the_old_scripts_are_unchanged():
    h = hashlib.sha256()
    for s in [cs.script(seed) for seed in range(24)] + [cs.script(1001, n_ops=50, jit=-1, scenes=("mixed7", "mixed8"), forms=(1,))]:
        h.update(("\n".join(repr(o) for o in s.ops) + "\n").encode())
    assert h.hexdigest() == OLD_SCRIPTS_SHA256


def test_the_post_scripts_are_unchanged():
    h = hashlib.sha256()
    for s in [cs.post_script(seed) for seed in range(24)] + [cs.jit_post_script()]:
        h.update(("\n".join(repr(o) for o in s.ops) + "\n").encode())
    assert h.hexdigest() == POST_SCRIPTS_SHA256


def _model_run(s, threads, cls=None):
    m = (cls or pm.model)(s, threads)
    try:
        return cs.run_post(s, None, m), m.events
    finally:
        m.close()


_runs = {}


def _run(seed):
    """(script, expected values, events) of a committed seed on a 1-thread model, computed once"""
    if seed not in _runs:
        s = cs.post_script(seed)
        _runs[seed] = (s,) + _model_run(s, 1)
    return _runs[seed]


@pytest.mark.parametrize("seed", POST_SEEDS)
def test_post_model_is_deterministic_across_thread_counts(seed):
    """every expected output and every expected refusal of a post script is the same on a 1-thread and a 4-thread oracle, and
    the script is reproducible from its seed"""
    s, seen, events = _run(seed)
    again = cs.post_script(seed)
    assert [repr(o) for o in again.ops] == [repr(o) for o in s.ops] and bytes(again.base) == bytes(s.base)
    seen4, events4 = _model_run(again, 4)
    assert [(i, k) for i, k, _ in seen4] == [(i, k) for i, k, _ in seen] and events4 == events
    for (i, k, x), (_, _, y) in zip(seen, seen4):
        assert cs._first_diff(x, y) is None, (i, k)
    assert {k for _, k, _ in seen} >= {"image_buffer", "counters"}


def test_the_jit_post_script_runs_on_the_model():
    """... and holds what it is there for: selected launches and reprojections that succeed, in both kernel forms"""
    s = cs.jit_post_script()
    seen, _ = _model_run(s, 2)
    assert sum(o.kind == "sample_selected" and o.expect is None for o in s.ops) >= 2
    assert sum(o.kind == "reproject" and o.expect is None for o in s.ops) >= 2
    assert {s.base.kernel_form} | {o.args["over"].get("kernel_form", s.base.kernel_form) for o in s.ops if o.kind == "set_config"} == {0, 1}
    assert s.jit == -1 and {o.args["name"] for o in s.ops if o.kind == "set_scene"} <= {"mixed7", "mixed8"} and seen


def test_a_post_mismatch_report_names_seed_operation_and_replay():
    """the report of a difference, on a script whose expectation is edited by hand: seed, operation index, the operations up to
    it as replayable statements, and the replay call"""
    s = cs.post_script(0, n_ops=30)
    i = next(i for i, o in enumerate(s.ops) if o.kind in cs.POST_KINDS and o.expect is None)
    s.ops[i].expect = cs.EINVAL
    m = pm.PostModel(s, 1)
    with pytest.raises(cs.Mismatch) as e:
        cs.run_post(s, None, m)
    m.close()
    msg = str(e.value)
    assert f"post call sequence seed 0, operation #{i}: {s.ops[i].kind}" in msg and "BASE = Config.from_buffer_copy" in msg
    assert f"replay: call_sequences.replay(call_sequences.post_script(0, ...), upto={i + 1})" in msg and f"[{i}] r." in msg


def _wanted_refusals():
    """every refusal reason of the sentences of include/rtpbr.h, as (operation, reason)"""
    want = {("reproject", f"dirty:{d}") for d in pm.DIRTY_BY} | {("present", "no_denoised")}
    want |= {("sample_selected", w) for w in ("persistent", "no_selection", "tiles")}
    want |= {(k, "tiles") for k in ("reproject", "noise_update", "noise_estimate", "denoise_guided", "select_mask", "select_noisy")}
    return want | {(k, "argument") for k in ("set_noise_estimator", "noise_estimate", "denoise_guided", "select_noisy", "sample_selected", "reproject")}


def _coverage():
    """{condition: (figure, minimum)} over the 24 committed seeds; figures count scripts unless the name says otherwise"""
    scripts = [_run(seed) for seed in POST_SEEDS]
    new = [o for s, _, _ in scripts for o in s.ops if o.kind in cs.POST_KINDS]
    refused = [o for o in new if o.expect is not None]

    def count(pred):
        return sum(1 for s, _, ev in scripts if pred(s, ev))

    def rep(ev):                # (kind, kept any, lost any, cap applied, with moments)
        return [e for e in ev if e[0] == "reproject"]

    out = {f"{kind} succeeds": (count(lambda s, ev: any(o.kind == kind and o.expect is None for o in s.ops)), 8) for kind in cs.POST_KINDS}
    out["observe post"] = (count(lambda s, ev: any(o.kind == "observe" and o.args["what"] == "post" for o in s.ops)), 8)
    reasons = {(o.kind, w) for o in refused for w in o.why}
    out["refusal reasons missing: " + repr(sorted(_wanted_refusals() - reasons))] = (-len(_wanted_refusals() - reasons), 0)
    # ... one cause at a time for the reproject rule, and present is the call that tiles do not refuse
    alone = {o.why for o in refused if o.kind == "reproject"}
    out["reproject refused for each single cause (causes)"] = (sum((f"dirty:{d}",) in alone for d in pm.DIRTY_BY), 4)
    out["present succeeds with tiles of world > 1 (operations)"] = (sum(o.kind == "present" and o.expect is None and _tiled(s, i) for s, _, _ in scripts
                                                                      for i, o in enumerate(s.ops)), 1)
    out["new operations that succeed per refusal (x 3 at least)"] = (len(new) - len(refused), 3 * len(refused))
    sizes = {(s.base.width, s.base.height) for s, _, _ in scripts}
    sizes |= {_size_after(s, o) for s, _, _ in scripts for o in s.ops if o.kind == "set_config" and o.expect is None}
    out["frame sizes"] = (len(sizes & set(cs.POST_SIZES)), len(cs.POST_SIZES))
    out["reproject keeps some pixels and loses some"] = (count(lambda s, ev: any(e[1] and e[2] for e in rep(ev))), 6)
    out["reproject applies the max_history cap"] = (count(lambda s, ev: any(e[3] for e in rep(ev))), 3)
    out["reproject with moments, then noise_update + noise_estimate"] = (count(_reproject_then_batch_and_estimate), 3)
    out["pooling changes a noise value"] = (count(lambda s, ev: ("pooling_changed_noise",) in ev), 4)
    out["select_noisy selects a part"] = (count(lambda s, ev: any(e[0] == "select_noisy" and 0 < e[1] < e[2] for e in ev)), 6)
    out["sample_selected on a partial selection"] = (count(lambda s, ev: any(e[0] == "sample_selected" and 0 < e[1] < e[2] and e[3] > 0 for e in ev)), 6)
    out["present(denoised) after a guided denoise"] = (count(lambda s, ev: ("present_denoised_after_guided",) in ev), 4)
    out["new resolution with moments, selection and presented frame"] = (count(lambda s, ev: ("new_resolution_with_moments_selection_presented",) in ev), 4)
    return out


def test_the_post_grammar_meets_its_coverage_conditions():
    """Conditions over the 24 committed seeds; the generator's weights were tuned until the model run met them."""
    cov = _coverage()
    print("\n".join(f"{v:4d} >= {lo:3d}  {k}" for k, (v, lo) in cov.items()))
    assert not [k for k, (v, lo) in cov.items() if v < lo], {k: v for k, v in cov.items() if v[0] < v[1]}


def _tiled(s, i):
    """tiles of world > 1 are set when operation i runs"""
    tiles = [o.args["tiles"] for o in s.ops[:i] if o.kind == "set_tiles" and o.expect is None]
    return bool(tiles) and tiles[-1][3] > 1


def _reproject_then_batch_and_estimate(s, ev):
    """a reproject that ran with moments present, followed by noise_update and noise_estimate before the next refresh, reproject
    or new resolution"""
    with_moments = iter([e[4] for e in ev if e[0] == "reproject"])
    ops = [o for o in s.ops if o.expect is None]
    for i, o in enumerate(ops):
        if o.kind == "reproject" and next(with_moments):
            tail = []
            for q in ops[i + 1:]:
                if q.kind in ("refresh", "reproject") or (q.kind == "set_config" and _size_after(s, q) != _size_before(s, q)):
                    break
                tail.append(q.kind)
            if "noise_update" in tail and "noise_estimate" in tail[tail.index("noise_update"):]:
                return True
    return False


def _size_after(s, op):
    return op.args["over"].get("width", s.base.width), op.args["over"].get("height", s.base.height)


def _size_before(s, op):
    size = s.base.width, s.base.height
    for o in s.ops:
        if o is op:
            return size
        if o.kind == "set_config" and o.expect is None:
            size = _size_after(s, o)
    return size


# ------------------------------------------------------------------ the motion scripts on the model alone
_motion_runs = {}


def _motion(seed):
    """(script, expected values, events) of a committed motion seed on a 1-thread model, computed once"""
    if seed not in _motion_runs:
        s = cs.motion_script(seed)
        _motion_runs[seed] = (s,) + _model_run(s, 1)
    return _motion_runs[seed]


@pytest.mark.parametrize("seed", MOTION_SEEDS)
def test_motion_model_is_deterministic_across_thread_counts(seed):
    """as for the post scripts: reproducible from the seed, same expected values, refusals and events on 1 and 4 threads"""
    s, seen, events = _motion(seed)
    again = cs.motion_script(seed)
    assert [repr(o) for o in again.ops] == [repr(o) for o in s.ops] and bytes(again.base) == bytes(s.base)
    seen4, events4 = _model_run(again, 4)
    assert [(i, k) for i, k, _ in seen4] == [(i, k) for i, k, _ in seen] and events4 == events
    for (i, k, x), (_, _, y) in zip(seen, seen4):
        assert cs._first_diff(x, y) is None, (i, k)
    assert {k for _, k, _ in seen} >= {"image_buffer", "counters"}


def test_the_jit_motion_script_runs_on_the_model():
    """... and holds what it is there for: two reproject_scene calls that succeed, both kernel forms, tracked samples"""
    s = cs.jit_motion_script()
    seen, events = _model_run(s, 2)
    assert sum(o.kind == "reproject_scene" and o.expect is None for o in s.ops) >= 2
    assert {s.base.kernel_form} | {o.args["over"].get("kernel_form", s.base.kernel_form) for o in s.ops if o.kind == "set_config"} == {0, 1}
    assert any(e[0] == "tracked" and e[2] > 0 and e[3] > 0 for e in events)
    assert s.jit == -1 and s.motion and {o.args["name"] for o in s.ops if o.kind == "set_scene"} <= {"mixed7", "mixed8"} and seen


def test_a_motion_mismatch_report_names_motion_script():
    s = cs.motion_script(0, n_ops=30)
    i = next(i for i, o in enumerate(s.ops) if o.kind in cs.MOTION_KINDS and o.expect is None)
    s.ops[i].expect = cs.EINVAL
    m = pm.model(s, 1)
    with pytest.raises(cs.Mismatch) as e:
        cs.run_post(s, None, m)
    m.close()
    assert f"replay: call_sequences.replay(call_sequences.motion_script(0, ...), upto={i + 1})" in str(e.value)


def _wanted_motion_refusals():
    want = {("reproject_scene", f"dirty:{d}") for d in pm.DIRTY_BY} | {("reproject_scene", "tiles"), ("reproject_scene", "argument")}
    want |= {("reproject_scene", f"table:{t}") for t in ("count", "scale", "material", "type")}
    want |= {("set_noise_tracking", "tiles"), ("set_noise_tracking", "argument")}
    return want | {("sample", "tracked:persistent"), ("sample", "tracked:tiles"), ("sample_selected", "tracked:tiles")}


def _is_new(s, i):
    """operation i is one of the new kinds: reproject_scene, set_noise_tracking, or a sample call drawn while tracked mode is on"""
    o = s.ops[i]
    if o.kind in cs.MOTION_KINDS:
        return True
    if o.kind not in ("sample", "sample_selected"):
        return False
    modes = [q.args["mode"] for q in s.ops[:i] if q.kind == "set_noise_tracking" and q.expect is None]
    return bool(modes) and modes[-1] == 1


def _motion_coverage():
    """{condition: (figure, minimum)} over the 24 committed motion seeds; figures count scripts unless the name says otherwise"""
    scripts = [_motion(seed) for seed in MOTION_SEEDS]
    new = [(s, i, o) for s, _, _ in scripts for i, o in enumerate(s.ops) if _is_new(s, i)]
    refused = [o for _, _, o in new if o.expect is not None]

    def count(pred):
        return sum(1 for s, _, ev in scripts if pred(s, ev))

    def rs_(ev):
        return [e[1] for e in ev if e[0] == "reproject_scene"]

    def tr(ev):                 # (kind, call, n, n_selected, pixels, what ran since the last tracked call, tracked calls before)
        return [e for e in ev if e[0] == "tracked"]

    out = {}
    for kind in ("reproject_scene", "set_noise_tracking", "sample", "sample_selected"):
        out[f"{kind} succeeds" + ("" if kind in cs.MOTION_KINDS else " in tracked mode")] = (
            count(lambda s, ev: any(o.kind == kind and o.expect is None and _is_new(s, i) and (kind != "set_noise_tracking" or o.args["mode"] == 1)
                                    for i, o in enumerate(s.ops))), 8)
    out["set_noise_tracking off succeeds"] = (count(lambda s, ev: any(o.kind == "set_noise_tracking" and o.expect is None and o.args["mode"] == 0 for o in s.ops)), 8)
    reasons = {(o.kind, w) for o in refused for w in o.why}
    out["refusal reasons missing: " + repr(sorted(_wanted_motion_refusals() - reasons))] = (-len(_wanted_motion_refusals() - reasons), 0)
    alone = {o.why for o in refused if o.kind == "reproject_scene"}
    out["reproject_scene refused for each single cause (causes)"] = (sum((f"dirty:{d}",) in alone for d in pm.DIRTY_BY), 4)
    out["new operations that succeed per refusal (x 3 at least)"] = (len(new) - len(refused), 3 * len(refused))
    out["reproject_scene keeps some pixels and loses some"] = (count(lambda s, ev: any(e["kept"] and e["lost"] for e in rs_(ev))), 6)
    out["a moved object keeps history"] = (count(lambda s, ev: any(e["moved_kept"] for e in rs_(ev))), 6)
    out["reproject_scene applies the max_history cap"] = (count(lambda s, ev: any(e["cap"] for e in rs_(ev))), 3)
    out["reproject_scene with moments"] = (count(lambda s, ev: any(e["moments"] for e in rs_(ev))), 6)
    out["reproject_scene with moments made by tracked samples"] = (count(lambda s, ev: any(e["tracked_moments"] for e in rs_(ev))), 3)
    out["normal_space LOCAL and a moved object keeps history"] = (count(lambda s, ev: any(e["local"] and e["moved_kept"] for e in rs_(ev))), 2)
    out["an empty move equals reproject"] = (count(lambda s, ev: any(e["empty"] for e in rs_(ev))), 2)
    out["a turn of +360 degrees"] = (count(lambda s, ev: any(e["full_turn"] for e in rs_(ev))), 2)
    out["a scene other than cornell or src is moved"] = (count(lambda s, ev: any(any(e["moved"]) and not e["scene"].startswith(("cornell", "src")) for e in rs_(ev))), 6)
    out["a second reproject_scene on an accumulated pose"] = (count(lambda s, ev: any(e["accumulated"] and any(e["moved"]) for e in rs_(ev))), 4)
    out["a tracked sample with n >= 8"] = (count(lambda s, ev: any(e[1] == "sample" and e[2] >= 8 for e in tr(ev))), 6)
    out["a tracked sample_selected on a partial selection"] = (count(lambda s, ev: any(e[1] == "sample_selected" and 0 < e[3] < e[4] for e in tr(ev))), 4)
    for what in ("write_image", "refresh", "new_resolution"):
        out[f"a tracked sample after {what}"] = (count(lambda s, ev: any(what in e[5] for e in tr(ev))), 2)
    out["noise_update between tracked calls"] = (count(lambda s, ev: any("noise_update" in e[5] and e[6] > 0 for e in tr(ev))), 3)
    out["pooling changes a noise value while tracking is on"] = (count(lambda s, ev: ("pooling_changed_noise_while_tracking",) in ev), 2)
    return out


def test_the_motion_grammar_meets_its_coverage_conditions():
    """Conditions over the 24 committed seeds; the generator's weights were tuned until the model run met them.  The events of a
    turn of +360 degrees report what reproject_scene_ref_lib.moved said of it."""
    cov = _motion_coverage()
    print("\n".join(f"{v:4d} >= {lo:3d}  {k}" for k, (v, lo) in cov.items()))
    assert not [k for k, (v, lo) in cov.items() if v < lo], {k: v for k, v in cov.items() if v[0] < v[1]}
    for _, _, ev in (_motion(seed) for seed in MOTION_SEEDS):
        assert all(isinstance(e[1]["moved"], tuple) for e in ev if e[0] == "reproject_scene" and e[1]["full_turn"])


# Three models that are wrong on purpose: each must expect something else than the true model somewhere in at least 4 of the 24
# scripts, or the scripts would not notice a library that made the same mistake.
class _KeepsTheOldFeatures(pm.MotionModel):
    """after reproject_scene the features stay those of the old pose until something renders them again"""
    stale = None

    def apply(self, op):
        if op.kind in ("set_config", "set_scene", "set_camera", "set_shape_data", "features", "reproject", "reproject_scene"):
            self.stale = None
        return super().apply(op)

    def _features(self, cam=None, scene=None):
        return super()._features(cam, self.stale if scene is None and self.stale is not None else scene)

    def _do_reproject_scene(self, op):
        old = self._scene()
        out = super()._do_reproject_scene(op)
        self.stale = old
        return out


class _KeepsTheOldSnapshot(pm.MotionModel):
    """reproject_scene warps the moments and leaves the snapshot as it was"""

    def _do_reproject_scene(self, op):
        keep = None if self.tracker is None else self.tracker.snapshot.copy()
        out = super()._do_reproject_scene(op)
        if keep is not None:
            self.tracker.snapshot[:] = keep
        return out


class _FoldsOneBatch(pm.MotionModel):
    """a tracked call of n samples folds them as one batch of n, as rtpbr_noise_update would"""

    def _fold(self, colours, before, mask):
        import noise_ref_lib as nr
        M, s, b = super()._fold(colours, before, mask)
        t = nr.Tracker(*self._size())
        t.moments[:], t.snapshot[:] = self.tracker.moments, before
        return t.update(b).copy(), s, b


@pytest.mark.parametrize("wrong", [_KeepsTheOldFeatures, _KeepsTheOldSnapshot, _FoldsOneBatch], ids=lambda c: c.__name__.strip("_"))
def test_the_motion_scripts_tell_a_wrong_model_from_the_true_one(wrong):
    differ = []
    for seed in MOTION_SEEDS:
        s, seen, _ = _motion(seed)
        got, _ = _model_run(s, 1, wrong)
        assert [(i, k) for i, k, _ in got] == [(i, k) for i, k, _ in seen]
        if any(cs._first_diff(x, y) is not None for (_, _, x), (_, _, y) in zip(seen, got)):
            differ.append(seed)
    print(f"{wrong.__name__}: differs on seeds {differ}")
    assert len(differ) >= 4, differ
