"""The call sequences of tests/half_sequences.py on the model alone (no GPU): every script's expected codes are the model's, the
model's own cross-checks hold (the fold's image_buffer is the oracle's, the gather of half A agrees with the image's gather), and
the draws reach what they are meant to reach."""
import collections

import pytest

import half_sequences as hs

SEEDS = range(8)


@pytest.fixture(scope="module")
def runs():
    out = []
    for seed in SEEDS:
        s = hs.half_script(seed)
        m = hs.model(s)
        try:
            seen, events = hs.run_half(s, None, m)
        finally:
            m.close()
        out.append((s, seen, list(events)))
    return out


def test_scripts_are_reproducible():
    a, b = hs.half_script(3), hs.half_script(3)
    assert [repr(x) for x in a.ops] == [repr(x) for x in b.ops] and bytes(a.base) == bytes(b.base)


def test_the_model_agrees_with_every_script_and_the_draws_cover_the_mode(runs):
    events = collections.Counter(e[0] for _, _, ev in runs for e in ev)
    refused = collections.Counter((op.kind, op.expect) for s, _, _ in runs for op in s.ops if op.expect is not None)
    why = {w for s, _, _ in runs for op in s.ops for w in op.why}
    seen = {k for _, sn, _ in runs for _, k, _ in sn}
    assert {"half_buffer", "denoised_error", "selection", "moments", "motion", "image_buffer"} <= seen
    assert events["dealt"] >= 10 and events["warped_halves"] >= 4 and events["denoise_error"] >= 4
    # a warped move that keeps pixels with both halves filled, and dealing with noise tracking on in the same pass
    assert any(e[0] == "warped_halves" and e[1] for _, _, ev in runs for e in ev)
    assert any(e[0] == "dealt" and e[4] for _, _, ev in runs for e in ev)
    assert any(e[0] == "dealt" and e[1] == "sample_selected" for _, _, ev in runs for e in ev)
    assert refused[("set_half_mode", hs.EINVAL)] >= 1 and refused[("sample", hs.ESTATE)] >= 1
    assert {"dealt:persistent", "dealt:tiles", "no_halves"} & why == {"dealt:persistent", "dealt:tiles", "no_halves"}
    assert {s.base.kernel_form for s, _, _ in runs} == {0, 1}
