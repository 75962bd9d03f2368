"""examples/blend_error.py at a small size (run with -m gpu), in the pattern of tests/test_gpu_examples.py."""
import os
import re
import subprocess
import sys

import pytest

from raytracingpbr_amd.imageio import imread

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(script, *args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", script), *map(str, args)], capture_output=True, text=True,
                         timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout


def test_blend_error_example(tmp_path):
    frame, emap = tmp_path / "frame.png", tmp_path / "error.png"
    s = run("blend_error.py", "--size", 64, 64, "--spp", 32, 64, "--ref-spp", 256, "--out", frame, "--error-map", emap)
    rows = re.findall(r"^\s+(\d+) \+ (\d+)\s+([0-9.]+)\s+([0-9.]+)\s+([0-9.]+)\s+([0-9.]+)\s+([0-9.]+)\s*$", s, flags=re.M)
    assert [(int(r[0]), int(r[1])) for r in rows] == [(16, 16), (32, 32)], s
    for r in rows:
        est, true, ratio = float(r[2]), float(r[3]), float(r[4])
        assert est > 0 and true > 0 and abs(ratio - est / true) <= 0.02 * ratio + 0.01
    a, b = imread(str(frame)), imread(str(emap))
    assert a.shape == b.shape == (64, 64, 3) and a.std() > 5 and b.max() > 0
