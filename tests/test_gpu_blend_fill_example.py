"""examples/sparse_preview.py --blend and examples/adaptive_flythrough.py --show-moves at 32x32, headless (run with -m gpu), in the
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


@pytest.mark.parametrize("extra", [(), ("--coverage-fill",)])
def test_sparse_preview_example_with_the_filling_blend(tmp_path, extra):
    s = run("sparse_preview.py", "--size", 32, 32, "--spp", 4, "--blend", *extra, "--out", tmp_path / "sparse")
    rows = re.findall(r"^(first|moved|frame\d): (\d+) pixels filled, (\d+) still empty, deepest level (\d+), mean blend depth ([0-9.]+)$", s,
                      flags=re.M)
    assert [r[0] for r in rows] == ["first", "moved", "frame0", "frame1", "frame2", "frame3"], s
    assert int(rows[0][1]) + int(rows[0][2]) == 32 * 32 * 3 // 4 and int(rows[0][1]) > 0      # the (2,2) lattice leaves three of four
    assert int(rows[-1][1]) == int(rows[-1][2]) == 0           # after the rotation every pixel has samples
    assert all(0.0 <= float(r[4]) <= 4.0 for r in rows)
    for step in ("first", "moved", "frame3"):
        for kind in ("filled", "holes"):
            assert os.path.getsize(tmp_path / f"sparse_{step}_{kind}.png") > 0


def test_adaptive_flythrough_example_shows_the_moved_frames():
    s = run("adaptive_flythrough.py", "--size", 32, 32, "--frames", 3, "--ref-spp", 64, "--max-spp", 8, "--show-moves")
    assert "right after each move, before any new sample" in s
    rows = re.findall(r"^move\s+(\d+):\s+(\d+) /\s+(\d+) /\s+(\d+)\s+([0-9.]+)\s+([0-9.]+)\s+([0-9.]+)$", s, flags=re.M)
    assert [int(r[0]) for r in rows] == [1, 2], s
    for _, without, filled, empty, e_holes, e_fill, e_new in rows:
        assert int(filled) + int(empty) == int(without)
        assert all(0.0 < float(v) < 1.0 for v in (e_holes, e_fill, e_new))
