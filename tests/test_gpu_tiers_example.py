"""examples/adaptive_tiers.py at a small size (run with -m gpu): the three loops end, and the tiered one reports its rounds."""
import re

import pytest

from test_gpu_examples import run

pytestmark = pytest.mark.gpu


def test_adaptive_tiers_example():
    s = run("adaptive_tiers.py", "--size", 48, 48, "--noise", 0.15, "--max-spp", 256, "--batch", 32, "--tiers", 4, "--truth-spp", 256)
    rows = [l for l in s.split("\n") if " rounds, " in l]
    assert [l.split(":")[0] for l in rows] == ["binary, batch 16", "binary, batch 32", "4 tiers, batch 32"], s
    for l in rows:
        rounds, traced = map(int, re.search(r"(\d+) rounds, (\d+) pixel-samples", l).groups())
        assert rounds >= 1 and traced >= 2 * 16 * 48 * 48 and "RMSE" in l
