// Test shim of raytracingpbr_amd/csrc/rt_launch_plan.hpp (test infrastructure): the header as the host compiler takes it, behind C
// functions that write a plan's fields, in the order of the struct, into out[] and return how many.  tests/test_launch_plan_host.py
// loads it; tests/launch_plan/san_main.cpp includes it.
#include "../../raytracingpbr_amd/csrc/rt_launch_plan.hpp"

#define EXPORT extern "C" __attribute__((visibility("default")))

EXPORT int lp_scalars(int queried, int waves_per_cu, int n_cu, long long items, long long* out) {
    out[0] = rt::blocks_per_cu(queried, waves_per_cu);
    out[1] = rt::capped_grid(rt::blocks_per_cu(queried, waves_per_cu), n_cu, items);
    out[2] = rt::work_margin(n_cu);
    out[3] = rt::capped_grid(rt::tune::PRIMARY_BLOCKS_PER_CU, n_cu, items);
    return 4;
}

EXPORT int lp_staging(long long np, long long left, long long staging_bytes, int n_cu, int split_ok, int unstaged, int primary_split, long long* out) {
    const rt::StagingPlan s = rt::staging_plan(np, left, staging_bytes, n_cu, split_ok != 0, unstaged != 0, primary_split);
    out[0] = s.per_spp, out[1] = s.K, out[2] = s.split, out[3] = s.total_items;
    return 4;
}

EXPORT int lp_claim(long long total_items, long long grid, int chunk_option, long long* out) {
    out[0] = rt::claim_plan((uint32_t)total_items, grid, chunk_option);
    return 1;
}

EXPORT int lp_dense(long long total_items, int K, long long chunk, int chunk_option, long long* out) {
    const rt::DensePlan d = rt::dense_plan((uint32_t)total_items, K, chunk, chunk_option);
    out[0] = d.on, out[1] = d.chunk, out[2] = d.acc_batch, out[3] = d.acc_magic_k, out[4] = d.acc_magic_chunk, out[5] = (long long)d.n_fill;
    return 6;
}

EXPORT int lp_pool(long long np, int per_cu, int n_cu, int chain_waves, int chain_candidate, int chain_room, int grid_blocks, long long* out) {
    const rt::PoolPlan p = rt::pool_plan(np, per_cu, n_cu, chain_waves, chain_candidate != 0, chain_room != 0, grid_blocks);
    out[0] = p.grid, out[1] = p.grid_room, out[2] = p.chain_blocks, out[3] = p.chain_fits, out[4] = p.n_cls;
    return 5;
}

EXPORT int lp_march(long long np, int per_cu, int n_cu, int waves_per_cu, int grid_blocks, int split_head, int sparse_lanes, int src_op, int n_obj,
                    long long* out) {
    const rt::MarchPlan m = rt::march_plan(np, per_cu, n_cu, waves_per_cu, grid_blocks, split_head, sparse_lanes, src_op, n_obj);
    out[0] = m.grid, out[1] = m.need, out[2] = m.n_teams, out[3] = m.split_head, out[4] = m.sparse_lanes;
    return 5;
}

EXPORT int lp_tier(int n, int t, int T, long long* out) {
    const rt::TierStage s = rt::tier_stage(n, t, T);
    out[0] = s.lo, out[1] = s.hi;
    return 2;
}
