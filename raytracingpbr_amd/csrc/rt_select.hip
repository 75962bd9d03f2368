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

void launch_select(const SelectArgs& A, int rule, hipStream_t st) {
    const uint32_t nb = select_blocks(A.width, A.height);
    if (rule == SELECT_NOISY) hipLaunchKernelGGL(select_mark<SELECT_NOISY>, dim3(nb), dim3(256), 0, st, A);
    else if (rule == SELECT_ERROR) hipLaunchKernelGGL(select_mark<SELECT_ERROR>, dim3(nb), dim3(256), 0, st, A);
    else hipLaunchKernelGGL(select_mark<SELECT_MASK>, dim3(nb), dim3(256), 0, st, A);
    hipLaunchKernelGGL(select_scan, dim3(1), dim3(256), 0, st, A.blocks, nb);
    hipLaunchKernelGGL(select_scatter, dim3(nb), dim3(256), 0, st, A);
}

}  // namespace rt
