"""The adaptive loop with and without tiers on the CPU oracle (tests/tier_loop_ref.py): deterministic, fixed seeds.  What is
asserted is only the direction observed on this run (DESIGN.md section 6u has the whole table): the tiered loop traces fewer
pixel-samples than the binary loop at the same batch, and takes fewer rounds than the binary loop in batches of 16."""
import numpy as np

import tier_loop_ref as tl
from raytracingpbr_amd import Config, cornell_box

W = H = 64
NOISE, DILATE, BUDGET, TRUTH_SPP = 0.1, 1, 2048, 1024


def test_the_three_loops_on_cornell_v3():
    """Cornell v3 64x64, noise 0.1, dilate 1, at most 2048 spp per pixel.  Measured (truth: 2048 spp of other indices; this test
    takes 1024 to stay short, which moves the two error columns it prints and nothing it asserts):

        loop                  rounds  pixel-samples  spp range   display RMSE  mean error, first half
        binary, batch 16        49      1 239 888    32..816       0.1033         -0.0291
        binary, batch 128        8      2 067 584    256..1280     0.0804         -0.0123
        6 tiers, batch 128      10      2 011 600    256..1536     0.0810         -0.0127

    The tiered loop saves 2.7 % of the binary loop's samples at the same batch and needs two rounds more (a pixel that took a small
    share and is still above the threshold comes back); both large-batch loops trace 1.6 x the samples of the loop in batches of 16."""
    scene, cfg = cornell_box("v3"), Config.cornell_v3(W, H, 0, 3)
    truth = tl.truth(scene, cfg, TRUTH_SPP).astype(np.float64)
    rows = {}
    for label, batch, tiers in (("binary 16", 16, 1), ("binary 128", 128, 1), ("6 tiers 128", 128, 6)):
        ib, traced, rounds = tl.adaptive(scene, cfg, NOISE, BUDGET, batch, DILATE, tiers)
        cnt = ib[..., 3]
        assert traced == int(cnt.astype(np.float64).sum())
        e = tl.display(scene, cfg, ib).astype(np.float64) - truth
        low = cnt <= np.quantile(cnt, 0.5)
        rows[label] = (rounds, traced)
        print(f"{label}: {rounds} rounds, {traced} pixel-samples ({cnt.min():.0f}..{cnt.max():.0f}), RMSE {np.sqrt(np.mean(e ** 2)):.4f}, "
              f"mean error of the half that stopped first {e[low].mean():+.4f}")
    assert rows["6 tiers 128"][1] < rows["binary 128"][1]
    assert rows["6 tiers 128"][0] < rows["binary 16"][0]
