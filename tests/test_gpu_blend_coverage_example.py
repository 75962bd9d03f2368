"""examples/denoise_levels.py --coverage and examples/adaptive_denoised.py --coverage at a small size (run with -m gpu), in the
pattern of tests/test_gpu_examples.py."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(script, *args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", script), *map(str, args)], capture_output=True, text=True,
                         timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout


def test_denoise_levels_example_with_coverage(tmp_path):
    s = run("denoise_levels.py", "--size", 64, 64, "--spp", 32, 64, "--ref-spp", 256, "--coverage", "--depth-map", tmp_path / "depth.png")
    assert len(re.findall(r"^\s+\d+ \+ \d+\s", s, flags=re.M)) == 2, s
    rows = re.findall(r"^\s+(frame|coverage below 1|interior) \((\d+) px\): denoise ([0-9.]+)  levels ([0-9.]+)  coverage ([0-9.]+)  new ([0-9.]+)"
                      r"\s+new / levels ([0-9.]+)\s+new / coverage ([0-9.]+)\s*$", s, flags=re.M)
    assert [r[0] for r in rows] == ["frame", "coverage below 1", "interior"] * 2, s
    for name, px, den, lev, cov, new, nl, nc in rows:
        assert 0 < int(px) <= 64 * 64 and (name != "frame" or int(px) == 64 * 64)
        assert all(float(v) > 0 for v in (den, lev, cov, new))
        assert abs(float(nl) - float(new) / float(lev)) <= 0.02 and abs(float(nc) - float(new) / float(cov)) <= 0.02
    resolved = [int(v) for v in re.findall(r"pixels resolved: (\d+)", s)]
    assert len(resolved) == 2 and resolved[0] == resolved[1] > 0      # the resolve is geometric: the same pixels at every sample count
    assert os.path.getsize(tmp_path / "depth.png") > 0


def test_adaptive_denoised_example_with_coverage():
    s = run("adaptive_denoised.py", "--size", 64, 64, "--max-spp", 32, "--ref-spp", 256, "--coverage")
    m = re.search(r"the loop ended with denoise_blend_levels_coverage: (\d+) pixels resolved, mean depth ([0-9.]+)", s)
    assert m and int(m.group(1)) > 0 and 0.0 <= float(m.group(2)) <= 4.0, s
    assert re.search(r"render_adaptive_denoised\([0-9.]+\): \d+ pixel-samples", s) and "samples spent, denoised loop / raw loop" in s
