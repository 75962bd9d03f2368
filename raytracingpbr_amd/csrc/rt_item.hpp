// rt_item.hpp — work item -> (local pixel, sample): item = q * K + k.
// K (samples per pixel of one sub-launch, Params::K) is a launch argument, and a 32-bit division by a run-time divisor is ~25
// vector instructions per sample in both complete-path kernels.  Launches nearly always use a power of two (256 spp per step,
// halved when the staging does not fit), so the host passes log2(K) beside K (Params::k_shift, -1 when K is no power of two) and
// the kernels shift and mask behind a wave-uniform branch; any other K keeps the division.  Plain integer arithmetic: both forms
// give the same (q, k) for every 32-bit item.  No device code in here: tests/test_item_split.py compiles it into a host program.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RT_ITEM_FN __host__ __device__ __forceinline__
#else
#define RT_ITEM_FN inline
#endif

namespace rt {

// log2(K) when K is a power of two (K = 1: 0), else -1
RT_ITEM_FN int32_t item_shift_of(int32_t K) {
    if (K <= 0 || (K & (K - 1)) != 0) return -1;
    int32_t s = 0;
    while ((1u << s) != (uint32_t)K) s++;
    return s;
}

// q = item / K, k = item % K; shift = item_shift_of(K) (wave-uniform on the device).  Returns true when the shift form was used.
RT_ITEM_FN bool item_split(uint32_t item, uint32_t K, int32_t shift, uint32_t& q, uint32_t& k) {
    if (shift >= 0) {
        q = item >> shift;
        k = item & (K - 1u);
        return true;
    }
    q = item / K;
    k = item - q * K;
    return false;
}

RT_ITEM_FN uint32_t item_pixel(uint32_t item, uint32_t K, int32_t shift) { return shift >= 0 ? item >> shift : item / K; }

}  // namespace rt
