"""The call sequences of tests/blend_error_sequences.py on the model alone (no GPU): every script's expected codes are the
model's, and the draws reach what they are meant to reach."""
import collections

import pytest

import blend_error_sequences as bs

SEEDS = range(6)


@pytest.fixture(scope="module")
def runs():
    out = []
    for seed in SEEDS:
        s = bs.blend_script(seed)
        m = bs.model(s)
        try:
            seen, events = bs.run(s, None, m)
        finally:
            m.close()
        out.append((s, seen, list(events)))
    return out


def test_scripts_are_reproducible():
    a, b = bs.blend_script(3), bs.blend_script(3)
    assert [repr(x) for x in a.ops] == [repr(x) for x in b.ops] and bytes(a.base) == bytes(b.base)


def test_the_model_agrees_with_every_script_and_the_draws_cover_the_calls(runs):
    events = [e for _, _, ev in runs for e in ev]
    count = collections.Counter(e[0] for e in events)
    refused = collections.Counter((op.kind, op.expect) for s, _, _ in runs for op in s.ops if op.expect is not None)
    why = {w for s, _, _ in runs for op in s.ops for w in op.why}
    seen = {k for _, sn, _ in runs for _, k, _ in sn}
    assert {"blend_error_map", "blend_weight", "blend_depth", "denoised_pixels", "selection", "half_buffer", "image_buffer"} <= seen
    assert count["blend_error"] >= 12 and count["select_blend_error"] >= 6
    # estimates with every pixel valid, with some not (an empty half after a reprojection or a refresh), with levels refused and
    # with a bias term; selections that take a part of the frame
    blends = [e for e in events if e[0] == "blend_error"]
    assert any(e[1] == e[2] for e in blends) and any(0 < e[1] < e[2] for e in blends) and any(e[1] == 0 for e in blends)
    assert any(e[3] > 0 for e in blends) and any(e[4] for e in blends)
    assert any(0 < e[1] < e[2] for e in events if e[0] == "select_blend_error")
    assert refused[("blend_error", bs.EINVAL)] >= 1 and refused[("blend_error", bs.ESTATE)] >= 1
    assert refused[("select_blend_error", bs.ESTATE)] >= 1
    assert {"no_halves", "no_blend_error"} <= why
    assert len({(s.base.width, s.base.height) for s, _, _ in runs}) == 2
