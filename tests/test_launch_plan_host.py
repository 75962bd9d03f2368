"""The launch geometry of the sample calls (raytracingpbr_amd/csrc/rt_launch_plan.hpp) on the host: the header is compiled by the
host compiler behind a shim (tests/launch_plan/launch_plan.cpp) and every output field of every plan is compared with a restatement
in Python integers (tests/launch_plan_ref.py, written from the scheduler's text before the header existed) over a sweep of frames,
devices, occupancies and options, and with rows worked out by hand from that text and DESIGN.md's account of it.  The image depends
on none of these numbers (tests/test_gpu_parity.py), so this is the only place a grid capped at the wrong multiple or a claim size
of 256 for 128 can show.  tests/launch_plan/san_main.cpp walks the same inputs as a stand-alone program for the sanitizers."""
import ctypes as C
import itertools
import os

import pytest

import launch_plan_ref as ref
import tier_ref_lib
from ref_build import I, P, ROOT
from test_lattice_rank import CxxLibrary

LL = C.c_longlong
LAUNCH_PLAN = CxxLibrary("launch_plan", {
    "lp_scalars": [I, I, I, LL, P], "lp_staging": [LL, LL, LL, I, I, I, I, P], "lp_claim": [LL, LL, I, P], "lp_dense": [LL, I, LL, I, P],
    "lp_pool": [LL, I, I, I, I, I, I, P], "lp_march": [LL, I, I, I, I, I, I, I, I, P], "lp_tier": [I, I, I, P],
}, deps=[os.path.join(ROOT, "raytracingpbr_amd", "csrc", "rt_launch_plan.hpp")])

NP = (1, 255, 256, 257, 384, 4096, 65536, 331776, 589824, 2073600, 2500000, 2500001, 3686400, 33177600)
N_CU = (1, 8, 256, 304)
PER_CU = (0, 1, 2, 4, 5, 8)
SPP = (1, 2, 3, 12, 16, 27, 256, 4096)
CHUNK = (0, 31, 32, 36, 96, 240, 256, 257, 777, 8192)
STAGING = (1 << 20, 16 << 30)
WAVES_PER_CU = (0, 1, 7, 32)
GRID_BLOCKS = (0, 1, 65535)
BOOL = (0, 1)
GiB16 = 16 << 30


@pytest.fixture(scope="module")
def plan():
    lib = LAUNCH_PLAN.lib()
    out = (LL * 8)()

    def plan(name, *args):
        n = getattr(lib, "lp_" + name)(*args, C.cast(out, C.c_void_p))
        return tuple(out[:n])

    return plan


def same(got, want):
    """field by field, booleans as 0 / 1"""
    return tuple(got) == tuple(int(v) for v in want)


def test_scalars_and_the_shared_clamp(plan):
    for q, w, n_cu, np in itertools.product(PER_CU + (-3,), WAVES_PER_CU, N_CU + (0,), NP):
        for items in (np, np * 16):
            per_cu = ref.blocks_per_cu(q, w)
            want = (per_cu, ref.capped_grid(per_cu, n_cu, items), ref.work_margin(n_cu), ref.capped_grid(ref.PRIMARY_BLOCKS_PER_CU, n_cu, items))
            assert same(plan("scalars", q, w, n_cu, items), want), (q, w, n_cu, items)
    # a device of no CUs and a kernel without occupancy still launch one block; the margin falls back to the MI355X's 256 CUs
    assert plan("scalars", 0, 0, 0, 1 << 20) == (2, 1, 256 * 32 * 8192, 1)
    assert plan("scalars", 5, 7, 256, 1 << 30) == (2, 512, 1 << 26, 2048)


def test_staging_budget(plan):
    for args in itertools.product(NP, SPP, STAGING, N_CU, BOOL, BOOL, (0, 1, 2)):
        got = plan("staging", *args)
        assert same(got, ref.staging_plan(*args)), args
        assert 1 <= got[1] <= args[1] and got[3] == args[0] * got[1]      # the launch's items fit 32 bits as they are


def test_claim_size_and_dense_staging(plan):
    on = off = 0
    for np, K, per_cu, w, n_cu in itertools.product(NP, SPP, PER_CU, WAVES_PER_CU, N_CU):
        total = np * K
        if total + ref.work_margin(n_cu) > 0xFFFFFFFF:      # (staging_plan never makes such a launch)
            continue
        grid = ref.capped_grid(ref.blocks_per_cu(per_cu, w), n_cu, total)
        for opt in CHUNK:
            chunk = ref.claim_plan(total, grid, opt)
            assert plan("claim", total, grid, opt) == (chunk,), (total, grid, opt)
            want = ref.dense_plan(total, K, chunk, opt)
            assert same(plan("dense", total, K, chunk, opt), want), (total, K, chunk, opt)
            on, off = on + want[0], off + (not want[0])
    assert on > 0 and off > 0


def test_pool_grid(plan):
    for args in itertools.product(NP, PER_CU, N_CU, (0, 1, 1024, 2048), BOOL, BOOL, GRID_BLOCKS):
        assert same(plan("pool", *args), ref.pool_plan(*args)), args


def test_march_grid(plan):
    for args in itertools.product(NP, PER_CU, N_CU + (2048,), WAVES_PER_CU, GRID_BLOCKS, (-1, 0, 1), (24, 8, 64), (0, 1), (8, 9)):
        assert same(plan("march", *args), ref.march_plan(*args)), args


def test_tier_stages_are_the_stage_plan_of_the_tier_restatement(plan):
    for n, T in itertools.product(range(1, 71), range(1, 9)):
        stages = [(t,) + plan("tier", n, t, T) for t in range(T - 1, -1, -1)]
        for t, lo, hi in stages:
            assert (lo, hi) == ref.tier_stage(n, t, T), (n, t, T)
        assert [(t, lo, hi, t + 1) for t, lo, hi in stages if hi != lo] == tier_ref_lib.stage_plan(n, (1,) * T), (n, T)


# ---- rows worked out by hand: 256 CUs, 16 GiB of staging, option chunk 0, primary_split 1 unless stated ---------------------------

def complete_path(plan, np, n, per_cu=2, split_ok=1, chunk_option=0, n_cu=256, staging=GiB16):
    """what sample_complete_path decides for its first sub-launch: (K, split, items, grid, claim)"""
    _, K, split, items = plan("staging", np, n, staging, n_cu, split_ok, 0, 1)
    grid = plan("scalars", per_cu, 0, n_cu, items)[1]
    return K, split, items, grid, plan("claim", items, grid, chunk_option)[0]


def test_complete_path_rows(plan):
    assert complete_path(plan, 1920 * 1080, 256) == (256, 1, 530841600, 512, 1024)
    assert plan("dense", 530841600, 256, 1024, 0)[:5] == (1, 256, 4096, 16777217, 16777217)
    assert complete_path(plan, 7680 * 4320, 256) == (27, 1, 27 * 7680 * 4320, 512, 1024)      # 27: what 16 GiB hold at 19 bytes an item
    assert complete_path(plan, 256 * 256, 16, per_cu=2) == (16, 0, 1 << 20, 512, 256)
    assert complete_path(plan, 256 * 256, 16, per_cu=8)[3:] == (2048, 128)
    # 24 x 16 at 12 spp: 4608 items on 18 blocks
    for option, claim, dense in ((0, 128, (1, 120, 4080, 357913942, 35791395)), (36, 36, (1, 36, 4068, 357913942, 119304648)),
                                 (240, 240, (1, 240, 4080, 357913942, 17895698)), (31, 31, (0, 0, 0, 0, 0)), (257, 257, (0, 0, 0, 0, 0))):
        K, split, items, grid, chunk = complete_path(plan, 24 * 16, 12, chunk_option=option)
        assert (K, items, grid, chunk) == (12, 4608, 18, claim), option
        assert plan("dense", items, K, chunk, option)[:5] == dense, option


def test_pool_grid_rows(plan):
    def pool(np, candidate=1, room=0):
        return plan("pool", np, 5, 256, 1024, candidate, room, 0)

    assert pool(1920 * 1080)[:4] == (1024, 1024, 256, 1)
    assert pool(768 * 432)[:2] == (768, 512) and pool(768 * 432, room=1)[0] == 512
    assert pool(1024 * 576)[:2] == (1024, 768) and pool(1024 * 576, room=1)[0] == 768
    assert pool(2560 * 1440, candidate=0)[:4] == (1280, 1280, 256, 0)      # above chain_np_max: the whole device, no chain kernel
    assert pool(64 * 64)[0] == 16
    assert pool(16 * 16)[0] == 1
