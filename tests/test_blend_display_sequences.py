"""The call sequences of tests/blend_display_sequences.py on the model alone (no GPU): every script's expected codes are the
model's, and the draws reach both estimate calls, either order of the pair on one state, and their refusals."""
import collections

import numpy as np
import pytest

import blend_display_sequences as ds

SEEDS = (0, 1, 2, 8, 9, 10)      # 9 and 10 draw the display call before half A exists and with tiles


@pytest.fixture(scope="module")
def runs():
    out = []
    for seed in SEEDS:
        s = ds.display_script(seed)
        m = ds.model(s)
        try:
            seen, events = ds.run(s, None, m)
        finally:
            m.close()
        out.append((s, seen, list(events)))
    return out


def test_scripts_are_reproducible():
    a, b = ds.display_script(3), ds.display_script(3)
    assert [repr(x) for x in a.ops] == [repr(x) for x in b.ops] and bytes(a.base) == bytes(b.base)


def test_the_model_agrees_with_every_script_and_the_draws_cover_both_calls(runs):
    events = [e for _, _, ev in runs for e in ev]
    count = collections.Counter(e[0] for e in events)
    refused = collections.Counter((op.kind, op.expect) for s, _, _ in runs for op in s.ops if op.expect is not None)
    seen = {k for _, sn, _ in runs for _, k, _ in sn}
    assert {"blend_error_map", "blend_weight", "blend_depth", "denoised_pixels", "selection", "half_buffer", "image_buffer"} <= seen
    assert count[ds.DISPLAY] >= 10 and count["blend_error"] >= 10 and count["select_blend_error"] >= 6
    shows = [e for e in events if e[0] == ds.DISPLAY]
    assert any(e[1] == e[2] for e in shows) and any(e[1] < e[2] for e in shows)      # every pixel valid, and some not
    assert any(e[3] > 0 for e in shows) and any(e[4] for e in shows)                 # levels refused, a bias term
    assert refused[(ds.DISPLAY, ds.EINVAL)] >= 1 and refused[(ds.DISPLAY, ds.ESTATE)] >= 1
    # the pair on one state, either way round, with planes that differ: the second call is seen to replace the first's
    pairs = collections.Counter()
    for s, sn, _ in runs:
        plane = {i: y for i, k, y in sn if k == "blend_error_map" and isinstance(y, np.ndarray)}
        ops = s.ops
        for i in range(len(ops) - 2):
            a, b = ops[i], ops[i + 2]
            if {a.kind, b.kind} == {ds.DISPLAY, "blend_error"} and a.args == b.args and a.expect is None and b.expect is None \
                    and i in plane and i + 2 in plane and not np.array_equal(plane[i], plane[i + 2]):
                pairs[a.kind] += 1
    assert pairs[ds.DISPLAY] >= 1 and pairs["blend_error"] >= 1
