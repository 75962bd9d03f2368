// rt_noise.hpp — per-pixel noise estimation (rtpbr_noise_update, rtpbr_noise_estimate).  The variance-guided a-trous of
// rtpbr_denoise_guided, which reads this estimate, is the GUIDED instance of atrous_level: rt_features.hpp / rt_features.hip.
//
//   noise_update        one lane per pixel along the contiguous index: the samples deposited into image_buffer since the
//                       snapshot are one batch; its mean's LINEAR luminance goes into the moments (sum c L, sum c L^2,
//                       sum c, K).  A streaming pass: 32 bytes read, 32 written per pixel.  (Moments of the compressed
//                       luminance r(mean) of each batch were measured first: they describe the mean of compressed batch means,
//                       not the displayed r(mean of everything), and under-estimate its variance 12-fold at 32 spp: DESIGN.md 6d.)
//   noise_estimate      the variance of the displayed luminance per pixel: from the moments (K >= 2) — the standard deviation
//                       of the mean linear luminance carried through r(c) = c / (1 + c) by its two sigma points, so the
//                       estimate is bounded by 1/4 whatever a firefly does to the moments —, else from the 7x7
//                       neighbourhood on the pixel's object (young pixels, as SVGF does); writes RTPBR_BUF_NOISE = sqrt(v), the
//                       filter's level-0 variance (v, -1 = pixel without samples) and the three statistics.
//   noise_estimate_pooled<R>  the same pass with rtpbr_set_noise_estimator's pooling on: a 2-D tile per block, (sum of squares,
//                       degrees of freedom, object) of the tile and an R-pixel halo staged in LDS once, and every young
//                       temporal pixel (2 <= K < pool_batches) takes max(own, pooled over its (2R+1)^2 window).  Every other
//                       pixel takes noise_estimate's path.  launch_noise_estimate picks it only when pool_batches > 0.
// The arithmetic is fixed operation by operation (include/rtpbr.h) so that a CPU restatement matches bit for bit
// (tests/post_ref/noise.h, tests/post_ref/filter.h).
#pragma once
#include "rt_types.hpp"

namespace rt {

// rtpbr_noise_stats as the kernel accumulates it: NOISE_SHARDS copies, one 128-byte line each, block b adds to shard b % 64 and
// the host folds them (sums and a maximum: still independent of the order).  One copy for all 8100 blocks of a 1080p frame
// serialised 24 300 atomics on one line: 0.23 ms for a pass that moves 40 bytes per pixel.
constexpr int NOISE_SHARDS = 64;
struct NoiseStats {
    uint32_t estimated, above, max_bits, pad[29];
};

// lum(c) of include/rtpbr.h
RT_D float nz_lum(vec3 c) { return (0.299f * c.x + 0.587f * c.y) + 0.114f * c.z; }

// the statistics, by every lane of the block (blk: three zeroed LDS words, a barrier since): per wave a ballot and a butterfly
// maximum, per block three LDS atomics per wave, then three global ones into the block's shard.  Shared by the estimate kernels
// here and half_error<R> (rt_half.hip).
RT_D void nz_stats(NoiseStats* stats, float threshold, uint32_t* blk, bool estimated, float noise, uint32_t block) {
    const bool above = estimated && noise > threshold;
    const unsigned long long m_est = __ballot(estimated), m_abv = __ballot(above);
    uint32_t mx = __float_as_uint(noise);       // >= +0: the bit patterns order like the values
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)mx, o, 64);
        mx = other > mx ? other : mx;
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&blk[0], (uint32_t)__popcll(m_est));
        atomicAdd(&blk[1], (uint32_t)__popcll(m_abv));
        atomicMax(&blk[2], mx);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        NoiseStats* s = stats + (block % NOISE_SHARDS);
        if (blk[0]) atomicAdd(&s->estimated, blk[0]);
        if (blk[1]) atomicAdd(&s->above, blk[1]);
        if (blk[2]) atomicMax(&s->max_bits, blk[2]);
    }
}

struct NoiseArgs {
    const float4* image_buffer;
    float4* snapshot;             // noise_update: in / out
    float4* moments;              // noise_update: in / out; noise_estimate: in
    const int32_t* object;        // noise_estimate: the spatial fallback's object test
    float* noise;                 // noise_estimate: out, sqrt(v)
    float* var0;                  // noise_estimate: out, v (-1: no samples)
    NoiseStats* stats;            // noise_estimate: out (zeroed before the launch)
    float threshold;
    int32_t width, height;
    int32_t pool_batches;         // noise_estimate: rtpbr_noise_estimator (0 = off: the plain kernel)
    int32_t pool_radius;          // 1..3
};

void launch_noise_update(const NoiseArgs& A, hipStream_t st);
void launch_noise_estimate(const NoiseArgs& A, hipStream_t st);

}  // namespace rt
