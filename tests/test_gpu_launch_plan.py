"""The wiring of the launch plans (raytracingpbr_amd/csrc/rt_launch_plan.hpp) on the device: tests/test_launch_plan_host.py holds the
plans to their restatement, this holds the launches to the plans, with what the context reports of a call — the number of
sub-launches (rtpbr_last_sample_ms) and whether one staged densely (counter dense_launches) — and the image's bits, which no plan
may change."""
import numpy as np
import pytest

import launch_plan_ref as ref
from raytracingpbr_amd import Config, Renderer, cornell_box

pytestmark = pytest.mark.gpu

N_CU = 256      # (only the 32-bit margin of the budget depends on it: far from these frames)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def render(scene, cfg, spp, **options):
    r = Renderer(scene, cfg)
    for k, v in options.items():
        r.set_option(k, v)
    r.sample(spp)
    image, launches, dense = bits(r.image_buffer).copy(), r.last_sample_ms()[2], r.counter("dense_launches")
    r.close()
    return image, launches, dense


def test_the_staging_budget_splits_a_call_into_the_plans_sub_launches():
    """128 x 64 at 16 spp on 1 MiB of staging: 14 bytes an item give 9 + 7 samples per pixel, 19 (with primary records) 6 + 6 + 4"""
    cfg, scene = Config.cornell_v3(128, 64, 0, 2), cornell_box("v3", aspect=128 / 64)
    want, launches, _ = render(scene, cfg, 16)
    assert launches == 1
    for primary_split, plan in ((0, [9, 7]), (2, [6, 6, 4])):
        assert ref.sub_launches(128 * 64, 16, 1 << 20, N_CU, primary_split != 0, False, primary_split) == plan
        image, launches, _ = render(scene, cfg, 16, staging_bytes=1 << 20, primary_split=primary_split)
        assert launches == len(plan), primary_split
        assert np.array_equal(image, want), primary_split


def test_dense_staging_takes_the_claim_size_the_plan_finds_or_declines():
    """24 x 16 at 12 spp: claims of 120 (from 128), 36 and 240 are whole multiples of a pixel's 12 samples; 257 does not fit the
    record's one-byte offset"""
    cfg, scene = Config.cornell_v3(24, 16, 3, 8), cornell_box("v3", aspect=24 / 16)
    want, _, dense = render(scene, cfg, 12)
    assert dense == 0
    for chunk in (0, 36, 240, 257):
        on = ref.dense_plan(24 * 16 * 12, 12, ref.claim_plan(24 * 16 * 12, 18, chunk), chunk)[0]
        assert on == (chunk != 257)
        image, launches, dense = render(scene, cfg, 12, stage_dense=1, jit=2, chunk=chunk)
        assert (launches, dense) == (1, int(on)), chunk
        assert np.array_equal(image, want), chunk
