// rt_select.hip — kernels of rtpbr_select_mask / rtpbr_select_noisy / rtpbr_select_error (see rt_select.hpp).
#include <hip/hip_runtime.h>

#include "rt_select.hpp"
#include "rt_device.hpp"

namespace rt {

RT_D uint32_t sel_rank(unsigned long long m) {      // set bits below this lane
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
}

// One lane per pixel, i = x * H + y.  SELECT_NOISY: the rule of rtpbr_select_noisy (include/rtpbr.h) — comparisons only; the
// neighbourhood is walked along y (the contiguous index) in the inner loop, at most 49 4-byte loads, and left at the first hit.
// SELECT_ERROR: the rule of rtpbr_select_error — the same on RTPBR_BUF_DENOISED_ERROR, and a pixel with an empty half is selected
// as one without samples is (16 more bytes read per pixel: half A's texel).
template <int RULE>
__global__ void __launch_bounds__(256) select_mark(const SelectArgs A) {
    __shared__ uint32_t wcnt[4];
    const int H = A.height, W = A.width;
    const uint32_t n = (uint32_t)W * (uint32_t)H;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool sel = false;
    if (i < n) {
        if constexpr (RULE != SELECT_MASK) {
            const float cnt = A.image_buffer[i].w;
            sel = !(cnt > 0.0f) || cnt < A.min_samples;
            if constexpr (RULE == SELECT_ERROR) {
                const float ca = A.half_a[i].w;
                sel = sel || !(ca > 0.0f) || !(cnt - ca > 0.0f);
            }
            if (!sel) {
                const int x = (int)(i / (uint32_t)H), y = (int)(i - (uint32_t)x * (uint32_t)H);
                const int d = A.dilate;
                for (int dx = -d; dx <= d && !sel; dx++) {
                    const int xq = x + dx;
                    if (xq < 0 || xq >= W) continue;
                    for (int dy = -d; dy <= d; dy++) {
                        const int yq = y + dy;
                        if (yq < 0 || yq >= H) continue;
                        if (A.noise[(size_t)xq * (size_t)H + (size_t)yq] > A.threshold) {
                            sel = true;
                            break;
                        }
                    }
                }
            }
        } else {
            sel = A.host_mask[i] != 0;
        }
        A.mask[i] = sel ? (uint8_t)1 : (uint8_t)0;
    }
    const unsigned long long m = __ballot(sel);
    if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) A.blocks[blockIdx.x] = (wcnt[0] + wcnt[1]) + (wcnt[2] + wcnt[3]);
}

// One block: blocks[0 .. nb) counts -> exclusive prefix sums, blocks[nb] = the total.
__global__ void __launch_bounds__(256) select_scan(uint32_t* blocks, uint32_t nb) {
    __shared__ uint32_t wsum[4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < nb; base += 256u) {
        const uint32_t j = base + threadIdx.x;
        const uint32_t v = j < nb ? blocks[j] : 0u;
        uint32_t incl = v;
#pragma unroll
        for (uint32_t off = 1; off < 64u; off <<= 1) {
            const uint32_t t = (uint32_t)__shfl_up((int)incl, off, 64);
            if (lane >= off) incl += t;
        }
        if (lane == 63u) wsum[wave] = incl;
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (uint32_t w = 0; w < 4u; w++) {
            before += w < wave ? wsum[w] : 0u;
            total += wsum[w];
        }
        if (j < nb) blocks[j] = carry + before + (incl - v);
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) blocks[nb] = carry;
}

// One lane per pixel: list[start of the block + selected pixels of the block below this one] = i.
__global__ void __launch_bounds__(256) select_scatter(const SelectArgs A) {
    __shared__ uint32_t wcnt[4];
    const uint32_t n = (uint32_t)A.width * (uint32_t)A.height;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool sel = i < n && A.mask[i] != 0;
    const unsigned long long m = __ballot(sel);
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) wcnt[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    if (!sel) return;
    uint32_t at = A.blocks[blockIdx.x];
    for (uint32_t w = 0; w < wave; w++) at += wcnt[w];
    A.list[at + sel_rank(m)] = i;      // at + rank < the total <= n: the list has n entries of room
}

// ---- the tiered selection (option select_tiers = T > 1; the rule: include/rtpbr.h): new instances, the three above are what T = 1 runs.

// The tier of one pixel, -1 = not selected.  Membership is select_mark's; where the plane decides, the window is walked to its end
// (the maximum is wanted, not the first hit).  Every operation is a single exactly rounded f32 one (the library is built without
// contraction, and the rounding intrinsics say so where it matters).
// STAGED: the block's window of the plane is in `tile` (select_stage_window); otherwise every value is a load of its own.
constexpr int SELECT_TILE_RUN = 256 + 6;      // words per row of the tile: the block's 256 indices and dilate <= 3 on either side
template <int RULE, bool STAGED>
RT_D int select_tier_of(const SelectTierArgs& S, uint32_t i, const float* tile) {
    const SelectArgs& A = S.A;
    const int T = S.tiers;
    if constexpr (RULE == SELECT_MASK) {
        const int b = A.host_mask[i];
        return (b < T ? b : T) - 1;
    } else {
        const int H = A.height, W = A.width;
        const float cnt = A.image_buffer[i].w;
        bool young = !(cnt > 0.0f) || cnt < A.min_samples;
        if constexpr (RULE == SELECT_ERROR) {
            const float ca = A.half_a[i].w;
            young = young || !(ca > 0.0f) || !(cnt - ca > 0.0f);
        }
        if (young) return 0;
        const int x = (int)(i / (uint32_t)H), y = (int)(i - (uint32_t)x * (uint32_t)H);
        const int d = A.dilate;
        float m = 0.0f;      // every value that counts is > threshold >= 0, so 0 stands for "none yet"
        for (int dx = -d; dx <= d; dx++) {
            const int xq = x + dx;
            if (xq < 0 || xq >= W) continue;
            for (int dy = -d; dy <= d; dy++) {
                const int yq = y + dy;
                if (yq < 0 || yq >= H) continue;
                const float v = STAGED ? tile[(dx + d) * SELECT_TILE_RUN + (int)threadIdx.x + d + dy] : A.noise[(size_t)xq * (size_t)H + (size_t)yq];
                if (v > A.threshold) m = fmaxf(m, v);      // (NaN compares false and never gets here)
            }
        }
        if (!(m > 0.0f)) return -1;
        const float r = __fdiv_rn(m, A.threshold);
        const float need = __fmul_rn(cnt, __fsub_rn(__fmul_rn(r, r), 1.0f));
        int t = 0;
        for (int k = 1; k < T; k++) t += need <= S.bound[k - 1] ? 1 : 0;      // NaN and infinity: no comparison holds, tier 0
        return t;
    }
}

// The per-tier counts of a block of 256 lanes: one ballot + popcount per tier and wave into wcnt[wave][tier]; returns the ballot
// of this lane's own tier (0 for a lane that is not selected).
RT_D unsigned long long select_tier_ballots(int tier, int T, uint32_t (*wcnt)[SELECT_MAX_TIERS]) {
    unsigned long long mine = 0;
    for (int t = 0; t < T; t++) {
        const unsigned long long m = __ballot(tier == t);
        if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6][t] = (uint32_t)__popcll(m);
        if (tier == t) mine = m;
    }
    return mine;
}

// The window of a block of 256 consecutive indices i0 .. i0 + 255 in LDS: the neighbour (x + dx, y + dy) of index i is index
// i + dx * H + dy, so row dx of the window is the contiguous run i0 + dx * H - d .. i0 + dx * H + 255 + d of the plane:
// tile[(dx + d) * SELECT_TILE_RUN + j] = plane[i0 + dx * H - d + j], 0 (never above a threshold) outside the buffer.  A run crosses
// column ends; the walk's own tests of xq and yq keep a lane from reading a value that is not its neighbour's.  2 d + 1 runs of
// 256 + 2 d words: 7.2 loads per lane at dilate 3 against 49.
RT_D void select_stage_window(const SelectArgs& A, float* tile) {
    const int d = A.dilate, run = 256 + 2 * d;
    const long long n = (long long)A.width * A.height, i0 = (long long)blockIdx.x * 256;
    for (int dx = -d; dx <= d; dx++) {
        const long long g0 = i0 + (long long)dx * A.height - d;
        for (int j = threadIdx.x; j < run; j += 256) {
            const long long g = g0 + j;
            tile[(dx + d) * SELECT_TILE_RUN + j] = g >= 0 && g < n ? A.noise[g] : 0.0f;
        }
    }
    __syncthreads();
}

// One lane per pixel: the byte 1 + tier (0 = not selected), and the block's count of every tier into blocks[t * nb + block]
// (tier-major, so that one scan over T * nb entries gives every (tier, block) its start in the tier-major list).
template <int RULE, bool STAGED>
__global__ void __launch_bounds__(256) select_mark_tiered(const SelectTierArgs S) {
    __shared__ uint32_t wcnt[4][SELECT_MAX_TIERS];
    __shared__ float tile[STAGED ? 7 * SELECT_TILE_RUN : 1];
    const uint32_t n = (uint32_t)S.A.width * (uint32_t)S.A.height;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if constexpr (STAGED) select_stage_window(S.A, tile);
    int tier = -1;
    if (i < n) {
        tier = select_tier_of<RULE, STAGED>(S, i, tile);
        S.A.mask[i] = (uint8_t)(tier + 1);
    }
    select_tier_ballots(tier, S.tiers, wcnt);
    __syncthreads();
    if ((int)threadIdx.x < S.tiers) {
        const uint32_t t = threadIdx.x;
        S.A.blocks[t * gridDim.x + blockIdx.x] = (wcnt[0][t] + wcnt[1][t]) + (wcnt[2][t] + wcnt[3][t]);
    }
}

// One lane per pixel: list[start of (tier, block) + lanes of the same tier in the block below this one] = i.
__global__ void __launch_bounds__(256) select_scatter_tiered(const SelectTierArgs S) {
    __shared__ uint32_t wcnt[4][SELECT_MAX_TIERS];
    const uint32_t n = (uint32_t)S.A.width * (uint32_t)S.A.height;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    int tier = -1;
    if (i < n) {
        const int b = S.A.mask[i];
        tier = (b < S.tiers ? b : S.tiers) - 1;      // (the mark pass wrote no byte above T: the clamp keeps the index into blocks inside whatever it reads)
    }
    const unsigned long long mine = select_tier_ballots(tier, S.tiers, wcnt);
    __syncthreads();
    if (tier < 0) return;
    const uint32_t wave = threadIdx.x >> 6;
    uint32_t at = S.A.blocks[(uint32_t)tier * gridDim.x + blockIdx.x];
    for (uint32_t w = 0; w < wave; w++) at += wcnt[w][tier];
    S.A.list[at + sel_rank(mine)] = i;      // at + rank < the total <= n: the list has n entries of room
}

// The cumulative counts L_t = blocks[(t + 1) * nb] (the start of tier t + 1's first block; the total for the last tier), gathered
// behind the total so that one copy of T words brings them to the host.
__global__ void select_tier_counts(uint32_t* blocks, uint32_t nb, uint32_t tiers) {
    if (threadIdx.x < tiers) blocks[tiers * nb + 1u + threadIdx.x] = blocks[(threadIdx.x + 1u) * nb];
}

// 1080p, 4 tiers, direct / staged: 21.1 / 23.0 us at dilate 1, 37.7 / 34.6 at 2, 61.1 / 51.2 at 3 (the staging pays from 25 taps on)
#ifndef RT_SELECT_STAGE_MIN_DILATE
#define RT_SELECT_STAGE_MIN_DILATE 2
#endif
constexpr int SELECT_STAGE_MIN_DILATE = RT_SELECT_STAGE_MIN_DILATE;      // (1: wherever there is a window, 4: never — the builds of the comparison)

void launch_select_tiered(const SelectTierArgs& S, int rule, hipStream_t st) {
    const uint32_t nb = select_blocks(S.A.width, S.A.height);
    // the window from LDS where that is faster (dilate >= SELECT_STAGE_MIN_DILATE); measured on the MI355X: DESIGN.md 6u
    const bool staged = rule != SELECT_MASK && S.A.dilate >= SELECT_STAGE_MIN_DILATE;
    if (rule == SELECT_NOISY && staged) hipLaunchKernelGGL((select_mark_tiered<SELECT_NOISY, true>), dim3(nb), dim3(256), 0, st, S);
    else if (rule == SELECT_NOISY) hipLaunchKernelGGL((select_mark_tiered<SELECT_NOISY, false>), dim3(nb), dim3(256), 0, st, S);
    else if (rule == SELECT_ERROR && staged) hipLaunchKernelGGL((select_mark_tiered<SELECT_ERROR, true>), dim3(nb), dim3(256), 0, st, S);
    else if (rule == SELECT_ERROR) hipLaunchKernelGGL((select_mark_tiered<SELECT_ERROR, false>), dim3(nb), dim3(256), 0, st, S);
    else hipLaunchKernelGGL((select_mark_tiered<SELECT_MASK, false>), dim3(nb), dim3(256), 0, st, S);
    hipLaunchKernelGGL(select_scan, dim3(1), dim3(256), 0, st, S.A.blocks, nb * (uint32_t)S.tiers);
    hipLaunchKernelGGL(select_scatter_tiered, dim3(nb), dim3(256), 0, st, S);
    hipLaunchKernelGGL(select_tier_counts, dim3(1), dim3(64), 0, st, S.A.blocks, nb, (uint32_t)S.tiers);
}

void launch_select(const SelectArgs& A, int rule, hipStream_t st) {
    const uint32_t nb = select_blocks(A.width, A.height);
    if (rule == SELECT_NOISY) hipLaunchKernelGGL(select_mark<SELECT_NOISY>, dim3(nb), dim3(256), 0, st, A);
    else if (rule == SELECT_ERROR) hipLaunchKernelGGL(select_mark<SELECT_ERROR>, dim3(nb), dim3(256), 0, st, A);
    else hipLaunchKernelGGL(select_mark<SELECT_MASK>, dim3(nb), dim3(256), 0, st, A);
    hipLaunchKernelGGL(select_scan, dim3(1), dim3(256), 0, st, A.blocks, nb);
    hipLaunchKernelGGL(select_scatter, dim3(nb), dim3(256), 0, st, A);
}

// ---- the lattice selection (option "select_lattice"; the rule and the two orders: rt_lattice.hpp)

// 0 (default): the ascending order, what select_mask makes of the same mask; 1: the tiled one — the build of the comparison.
// Measured on the MI355X: the tiled list's selected launches are not faster than the ascending one's, on the glass
// bunny's (2,2) lattice slower than the spread of the ascending list's own runs.
#ifndef RT_LATTICE_ORDER
#define RT_LATTICE_ORDER 0
#endif
constexpr int LATTICE_ORDER = RT_LATTICE_ORDER;

// One lane per word of the plane: the four pixels i0 .. i0 + 3 along i = x * H + y (they may cross a column end), their bytes in one
// store where all four are inside the frame (the plane is an allocation of its own, so i0 is word-aligned), and list[rank] = i for
// those on the lattice: x < W and x % px == phx give a = x / px < nx, likewise b < ny, so rank < nx * ny <= W * H, the list's room.
// Nothing is read, no lane waits for another.
__global__ void __launch_bounds__(256) select_lattice_build(const LatticeArgs A) {
    const uint32_t H = (uint32_t)A.height, n = (uint32_t)A.width * H;
    const uint32_t i0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4u;
    if (i0 >= n) return;
    const uint32_t px = (uint32_t)A.l.px, py = (uint32_t)A.l.py, phx = (uint32_t)A.l.phx, phy = (uint32_t)A.l.phy;
    const uint32_t left = n - i0 < 4u ? n - i0 : 4u;
    uint32_t x = i0 / H, y = i0 - x * H, word = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) {
        if (k < left && x % px == phx && y % py == phy) {
            word |= 1u << (8u * k);
            A.list[lattice_rank(LATTICE_ORDER, x / px, y / py, A.l.nx, A.l.ny)] = i0 + k;
        }
        if (++y == H) {
            y = 0;
            x++;
        }
    }
    if (left == 4u) {
        *reinterpret_cast<uint32_t*>(A.mask + i0) = word;
    } else {
        for (uint32_t k = 0; k < left; k++) A.mask[i0 + k] = (uint8_t)(word >> (8u * k));
    }
}

void launch_select_lattice(const LatticeArgs& A, hipStream_t st) {
    const uint32_t words = (uint32_t)(((size_t)A.width * (size_t)A.height + 3) / 4);
    hipLaunchKernelGGL(select_lattice_build, dim3((words + 255u) / 256u), dim3(256), 0, st, A);
}

}  // namespace rt
