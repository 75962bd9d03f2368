// rt_launch_plan.hpp — the geometry of the sample calls' launches, decided on the host: how many samples a sub-launch stages, how
// many blocks a kernel gets, how many items a wave claims.  Plain C++17 without a HIP include (as rt_dispatch.hpp and rt_lattice.hpp):
// plain numbers in, a plain struct out, so the host compiler takes it behind a shim and tests/test_launch_plan_host.py holds every
// function to a restatement and to rows worked out by hand.  By design the image depends on none of this — a slip here costs speed
// on one workload and no parity test sees it.  rt_capi.hip gets a plan, copies it into Params, allocates and launches.
#pragma once
#include <stdint.h>

namespace rt {

// ------------------------------------------------------------------------------------------------------------------------
// THE HOST SCHEDULER'S CONSTANTS, in one place.  Everything below that is a number was MEASURED on one MI355X (256 CUs, 4 SIMDs
// per CU, 160 KB of LDS per CU); what follows from the device is read from hipDeviceProp (c->n_cu) or from the kernels'
// occupancy (hipOccupancyMaxActiveBlocksPerMultiprocessor / the run-time module's own query).  Option defaults — the numbers a
// caller can change — live in rt_ctx.hpp next to the option they belong to; rtpbr.h documents them.  On another SKU or a
// partitioned device (CPX) these are the lines to re-measure (tools/gpu_src_grid.py, tools/gpu_src_1step.py sweep them).
namespace tune {
constexpr int WAVES_PER_BLOCK = 4;              // 256 threads: one wave per SIMD of a CU
constexpr int CTX_PER_WAVE = 128;               // src/ pool kernel: 64 lanes + 64 LDS slots (rt_persistent.hpp)
constexpr int MAX_FUSED_STEPS = 256;            // bounce-steps per fused src/ launch (G_META holds 9 bits)
// --- src/ pool kernel (fused launches) -----------------------------------------------------------------------------------
constexpr int POOL_MIN_PIX_PER_WAVE = 64;       // a wave never owns fewer pixels than it has lanes (grid <= np / 256)
// beside the chain kernel a pool wave should own ~190 pixels, in whole blocks per CU, at least two (two waves of 162 contexts
// march with 54-57 of 64 lanes, three of 108 with 34; a wave issues one instruction per ~6.5 cycles whatever it carries):
// 1024x576 four -> three blocks per CU 30.8 -> 27.3 ms, 960x540 29.5 -> 24.2, 768x432 three -> two 22.7 -> 22.3 (round 5)
constexpr int CHAIN_POOL_PIX_PER_BLOCK = 760;
constexpr int CHAIN_POOL_MIN_BLOCKS_PER_CU = 2;
constexpr int CHAIN_GRID_BLOCKS = 512;          // chain kernel: 2048 waves = the largest chain set a plan can make (waves without an entry leave at once)
// --- src/ wavefront split (launches of <= src_split steps) -----------------------------------------------------------------
// waves per SIMD of the march kernel: 2 / 3 / 4 / 5 / 8 = 0.53 / 0.51 / 0.51 / 0.55 / 0.59 ms per 1080p launch (the arbiter
// serves the oldest wave first: with more the youngest starve and end last)
constexpr int MARCH_MAX_BLOCKS_PER_CU = 4;
// small frames are all tail: two waves per SIMD (640x360 0.230 / 0.236 / 0.240 ms at 2 / 3 / 4, 768x432 0.258 / 0.261 / 0.270,
// no difference from 1024x576 on) and the list's heavy head interleaved over the groups (768x432 0.2375 -> 0.224; 1080p loses)
constexpr long long MARCH_SMALL_FRAME_PIXELS = 600000;
constexpr int MARCH_SMALL_BLOCKS_PER_CU = 2;
constexpr int MARCH_MAX_TEAMS = 1024;           // team counters allocated (rtpbr_create)
constexpr int SPARSE_LANES_DEFAULT = 24;        // option sparse_lanes as rt_ctx.hpp sets it (fused pool kernel: tracked march when <= 24 lanes march)
constexpr int SPLIT_SPARSE_LANES = 8;           // ... the split march kernel with the object-parallel evaluation: from 8 lanes down
// --- complete-path form ----------------------------------------------------------------------------------------------------
constexpr long long PRIMARY_SPLIT_MIN_ITEMS = 1LL << 23;    // the separate primary kernel costs ~0.3 ms per launch: below ~8 M items the fused kernel wins
// work items a wave claims per atomic: total / (waves x 64) clamped to [256, 1024]; 128 when a launch has fewer than 256 per wave
// (1080p x 16 spp: 64 / 128 / 256 / 512 items = 10.6 / 9.6 / 9.2 / 9.3 ms; 4096 cost 2 % on the Cornell frame and 18 % on the
// glass bunny — a wave that claims the last chunk works it off 128 paths at a time; C1: 1407 -> 1492 Msamples/s with 128)
constexpr long long CHUNK_MIN = 256, CHUNK_MAX = 1024, CHUNK_TINY = 128;
constexpr int PRIMARY_BLOCKS_PER_CU = 8;        // the primary kernel needs ~57 VGPRs: 32 waves per CU (plan_hist, plan_scatter and accumulate_dense take the same grid)
}  // namespace tune

// Staging (one 12-byte StageRec per item) and, for the primary split, the primary records (5 bytes per item: a float, then a byte).
constexpr uint64_t PRIMARY_REC_BYTES = 5;     // float t_eval + one byte of idx | state
// staging of `items` samples: the 12-byte records, then (dense staging) one fill count per chunk of >= 32 items and one byte per record
constexpr uint64_t STAGE_ITEM_BYTES = 14;     // what a sample is budgeted at (12 + 1 + 4 / 32, rounded up)
constexpr uint32_t DENSE_CHUNK_MIN = 32, DENSE_CHUNK_MAX = 256, DENSE_BATCH_MAX = 4096;

// blocks of 256 threads a kernel gets per CU: what its occupancy query said (2 where the query failed), or option waves_per_cu
constexpr int blocks_per_cu(int queried, int waves_per_cu) { return waves_per_cu > 0 ? (waves_per_cu + 3) / 4 : queried > 0 ? queried : 2; }
constexpr int cus_or_default(int n_cu) { return n_cu > 0 ? n_cu : 256; }      // (a caller without a device count plans for the MI355X)

// blocks per CU x CUs, at most `need` blocks, at least one; capped_grid: `need` = one thread per item
constexpr long long capped_blocks(int per_cu, int n_cu, long long need) {
    const long long grid = (long long)per_cu * n_cu < need ? (long long)per_cu * n_cu : need;
    return grid < 1 ? 1 : grid;
}
constexpr long long capped_grid(int per_cu, int n_cu, long long items) { return capped_blocks(per_cu, n_cu, (items + 255) / 256); }

// Room kept free below 2^32 for the claims the last waves make past the end of the work (one failing claim per wave):
// at most 32 waves per CU, at most 8192 items per claim (option "chunk" is clamped to that).
constexpr long long work_margin(int n_cu) { return (long long)cus_or_default(n_cu) * 32LL * 8192LL; }

// ---- complete-path form: one sub-launch of K samples per pixel ---------------------------------------------------------------
// per_spp: bytes one sample per pixel is budgeted at; K: samples per pixel of this sub-launch = min(left, what staging_bytes holds,
// what 32 bits hold), >= 1; split: the primary rays get a kernel of their own; total_items = np * K
struct StagingPlan {
    long long per_spp, K;
    bool split;
    uint32_t total_items;
};
// `left` samples per pixel are still to trace (>= 1); split_ok: the launch could split its primary rays off; unstaged: it keeps no
// records (the tolerance flavour accumulates in LDS and adds to image_buffer directly: no staging, no accumulate kernel)
inline StagingPlan staging_plan(long long np, long long left, long long staging_bytes, int n_cu, bool split_ok, bool unstaged, int primary_split) {
    long long per_spp = np * (long long)((unstaged ? 0 : STAGE_ITEM_BYTES) + (split_ok ? PRIMARY_REC_BYTES : 0));
    if (per_spp < 1) per_spp = 1;
    long long kmax = staging_bytes / per_spp;
    if (kmax < 1) kmax = 1;
    // keep total_items within 32 bits (minus the chunks the last waves claim past the end: the work counter must not wrap)
    long long k32 = (0xFFFFFFFFLL - work_margin(n_cu)) / np;
    if (k32 < 1) k32 = 1;
    if (kmax > k32) kmax = k32;
    const long long K = left < kmax ? left : kmax;
    return {per_spp, K, split_ok && (primary_split == 2 || np * K >= tune::PRIMARY_SPLIT_MIN_ITEMS), (uint32_t)(np * K)};
}

// work items a wave claims per atomic (tune::CHUNK_*), or option chunk
inline long long claim_plan(uint32_t total_items, long long grid, int chunk_option) {
    const long long waves = grid * tune::WAVES_PER_BLOCK;
    long long chunk = (long long)total_items / (waves * 64);
    if (chunk < tune::CHUNK_MIN) chunk = (long long)total_items < waves * tune::CHUNK_MIN ? tune::CHUNK_TINY : tune::CHUNK_MIN;
    if (chunk > tune::CHUNK_MAX) chunk = tune::CHUNK_MAX;
    if (chunk_option > 0) chunk = chunk_option;
    return chunk;
}

// dense staging (rt_trace.hpp stage_sample, accumulate_dense): the claim must be whole pixels or a whole fraction of one, and
// fit the record's one-byte offset; a launch that has no such claim size near the one wanted keeps the item-linear records
struct DensePlan {
    bool on;
    uint32_t chunk, acc_batch, acc_magic_k, acc_magic_chunk;      // (all 0 when off)
    uint64_t n_fill;                                              // fill counters behind the records
};
inline DensePlan dense_plan(uint32_t total_items, int K, long long chunk, int chunk_option) {
    long long lo = DENSE_CHUNK_MIN, hi = chunk < 64 ? 64 : chunk > (long long)DENSE_CHUNK_MAX ? (long long)DENSE_CHUNK_MAX : chunk, cc = 0;
    if (chunk_option > 0) lo = hi = chunk_option;       // a claim size that was asked for is kept as it is (or the records stay item-linear)
    if (lo >= (long long)DENSE_CHUNK_MIN && hi <= (long long)DENSE_CHUNK_MAX)
        for (long long t = hi; t >= lo; t--)
            if (t % K == 0 || K % t == 0) { cc = t; break; }
    const long long unit = cc > K ? cc : K;      // one divides the other: their least common multiple
    if (cc <= 0 || unit > (long long)DENSE_BATCH_MAX) return {};
    return {true, (uint32_t)cc, (uint32_t)(unit * ((long long)DENSE_BATCH_MAX / unit)),
            K > 1 ? (uint32_t)(0x100000000ULL / (unsigned long long)K) + 1u : 0u, (uint32_t)(0x100000000ULL / (unsigned long long)cc) + 1u,
            (uint64_t)total_items / (uint64_t)cc + 1};
}

// selected call on a tiered selection: stage t of T traces the sample indices base + lo .. base + hi - 1 (shares max(1, n >> t))
struct TierStage { int lo, hi; };
inline TierStage tier_stage(int n, int t, int T) {
    const int hi = (n >> t) > 1 ? n >> t : 1;
    const int lo = t + 1 == T ? 0 : (n >> (t + 1)) > 1 ? n >> (t + 1) : 1;
    return {lo, hi};
}

// ---- src/ persistent-ray form: the fused pool kernel's grid ------------------------------------------------------------------
// grid: blocks of the pool kernel; grid_room: ... of the grid a plan decides "chain-bound" against; chain_fits: the device holds the
// pool grid and the chain kernel together; n_cls: blocks per CU of `grid`, rounded up
struct PoolPlan {
    long long grid, grid_room, chain_blocks;
    bool chain_fits;
    int n_cls;
};
// per_cu: blocks_per_cu() of the pool kernel.  chain_candidate: the launch may get a chain set (options src_chain and src_plan, no
// grid_blocks, a frame of at most chain_np_max pixels); chain_room: ... and the last plan made one (or src_chain = 2).
inline PoolPlan pool_plan(long long np, int per_cu, int n_cu, int chain_waves, bool chain_candidate, bool chain_room, int grid_blocks) {
    // Static ownership (persistent_pool_impl): every resident wave owns np / waves pixels.  A wave holds 128 contexts:
    // when the frame fits (np <= 128 x resident waves) the grid is sized so that every wave owns <= 128 pixels and
    // keeps them for the whole launch, in whole multiples of the CU count (every CU the same number of blocks), but
    // never fewer than 64 pixels per wave; larger frames use every resident wave and walk their pixels in
    // residencies of `residency` bounce-steps.
    const long long max_blocks = (long long)per_cu * n_cu;
    const long long ctx_per_block = (long long)tune::CTX_PER_WAVE * tune::WAVES_PER_BLOCK;
    long long grid = (np + ctx_per_block - 1) / ctx_per_block;
    if (grid >= max_blocks) {
        grid = max_blocks;
    } else {
        grid = (grid + n_cu - 1) / n_cu * n_cu;
        if (grid > max_blocks) grid = max_blocks;
        const long long dense = np / (tune::POOL_MIN_PIX_PER_WAVE * tune::WAVES_PER_BLOCK);
        if (grid > dense) grid = dense;
    }
    // The chain kernel (rt_chain.hpp) runs BESIDE the pool kernel and needs wave slots of its own.  Frames up to about
    // 1080p may be chain-bound (plan_scan decides, on the device, against the grid the pool kernel has beside the chain kernel);
    // when the last plan made a chain set the pool grid makes room — whole multiples of the CU count: an uneven grid
    // costs more than it gives (1024x576 42.8 -> 30 ms, 1280x720 46 -> 40, 1600x900 54.7 -> 50.4, 1080p 58.6 -> 57.3) —
    // and is sized for ~190 pixels per wave.  Larger frames are throughput-bound and keep the whole device for the pool
    // kernel (2560x1440: 97.2 against 100.3 ms).
    const long long chain_blocks = (chain_waves + tune::WAVES_PER_BLOCK - 1) / tune::WAVES_PER_BLOCK;
    // (the grid WITH room is computed whether or not room is made: it is what the plan decides "chain-bound" against, so that
    // the decision is the same before and after — the host makes room only once a plan has said so)
    // Two separate things (round 6 took them apart: `src_chain = 0 / 1 / 2` at 1080p = 56.3 / 56.5 / 53.4 ms showed that what
    // helps there is the GRID, the plan never finds 1080p chain-bound): (a) a frame that may get a chain set leaves one block
    // per CU free — four blocks per CU instead of five are faster at these sizes with or without a chain kernel beside them
    // (1080p 56 -> 53.4 ms); (b) the ~190 pixels per wave of a small frame pay only BESIDE a chain kernel (without one the
    // heaviest pixels need the larger grid: 768x432 26 against 36 ms) — applied once a plan has produced a chain set.
    long long grid_room = grid;
    if (chain_candidate) {
        if (grid_room + chain_blocks > max_blocks && max_blocks - chain_blocks >= n_cu) grid_room = (max_blocks - chain_blocks) / n_cu * n_cu;
        if (grid_room < 1) grid_room = 1;
        grid = grid_room;                                                     // (a)
        long long want = (np / tune::CHAIN_POOL_PIX_PER_BLOCK + n_cu / 2) / n_cu * n_cu;
        if (want < (long long)tune::CHAIN_POOL_MIN_BLOCKS_PER_CU * n_cu) want = (long long)tune::CHAIN_POOL_MIN_BLOCKS_PER_CU * n_cu;
        if (grid_room > want) grid_room = want;                               // (b): what the plan decides "chain-bound" against
    }
    if (chain_room) grid = grid_room;
    if (grid_blocks > 0) grid = grid_blocks;
    if (grid < 1) grid = 1;
    // the chain kernel is launched only when the device has room for both: more resident waves than it holds just queue
    // the pool's last blocks behind the chain waves (measured -12 % at 720p)
    return {grid, grid_room, chain_blocks, chain_candidate && grid + chain_blocks <= max_blocks, (int)((grid + n_cu - 1) / n_cu)};
}

// ---- src/ wavefront split: the march kernel's grid ---------------------------------------------------------------------------
// grid: blocks of the march kernel; need: blocks of the gen and shade kernels, one thread per pixel; n_teams: teams of blocks that
// share a claim counter: the blocks resident on one CU (blocks are placed round-robin)
struct MarchPlan {
    long long grid, need;
    int n_teams, split_head, sparse_lanes;
};
// per_cu: the march kernel's occupancy as queried; the options as the context holds them
inline MarchPlan march_plan(long long np, int per_cu, int n_cu, int waves_per_cu, int grid_blocks, int split_head_option, int sparse_lanes_option,
                            int src_op, int n_obj) {
    MarchPlan m{};
    // with the object-parallel evaluation the tracked forms pay from 8 marching lanes down; between 9 and 24 a wave's lanes rarely
    // share an object and the three-smallest evaluation (2.7 kcycles per call in the tails) only replaces a plain step (1.1 k):
    // 768x432 0.2125 -> 0.205 ms per launch, 1080p 0.454 -> 0.450.  (An explicit sparse_lanes — the tests force 64 — is respected.)
    m.sparse_lanes = sparse_lanes_option == tune::SPARSE_LANES_DEFAULT && (src_op & 1) && n_obj <= 8 ? tune::SPLIT_SPARSE_LANES : sparse_lanes_option;
    int mper = blocks_per_cu(per_cu, 0);
    if (mper > tune::MARCH_MAX_BLOCKS_PER_CU) mper = tune::MARCH_MAX_BLOCKS_PER_CU;
    const bool small = np <= tune::MARCH_SMALL_FRAME_PIXELS;
    if (small && mper > tune::MARCH_SMALL_BLOCKS_PER_CU) mper = tune::MARCH_SMALL_BLOCKS_PER_CU;
    m.split_head = split_head_option >= 0 ? split_head_option : (small ? 1 : 0);
    mper = blocks_per_cu(mper, waves_per_cu);
    m.need = (np + 255) / 256;
    m.grid = grid_blocks > 0 ? grid_blocks : capped_grid(mper, n_cu, np);
    m.n_teams = (int)(m.grid < n_cu ? m.grid : n_cu);
    if (m.n_teams > tune::MARCH_MAX_TEAMS) m.n_teams = tune::MARCH_MAX_TEAMS;
    return m;
}

}  // namespace rt
