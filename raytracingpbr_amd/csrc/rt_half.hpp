// rt_half.hpp — the two-half error estimate of the denoised frame (rtpbr_half_update, rtpbr_denoise_error).
//
// The samples of image_buffer are kept in two independent halves: A is stored (RTPBR_BUF_HALF_BUFFER), B = image_buffer - A is
// not.  rtpbr_denoise's filter runs on each half (the existing atrous_level / atrous_none instances, rt_features.hip); the
// difference of the two results measures the variance of the filtered full frame, correlations between neighbours included.
//
//   half_update         one lane per pixel along the contiguous index: what was deposited into image_buffer since the snapshot
//                       is one batch, and goes to the half with fewer samples (A on a tie).  A streaming pass as noise_update:
//                       32 bytes read and 16 written per pixel, 32 more both ways where A takes the batch.
//   half_subtract       B = image_buffer - A per component into a buffer of its own: the filter takes its input as a pointer.
//   half_error<R>       e_q = (lum(DA_q) - lum(DB_q))^2 cA cB / (cA + cB)^2 per pixel with both halves filled, its mean over the
//                       (2R+1)^2 window on the pixel's object, the root of that into RTPBR_BUF_DENOISED_ERROR, and the three
//                       statistics of rtpbr_noise_estimate.  The layout of noise_estimate_pooled<R> (rt_noise.hip): a 2-D tile
//                       per block, (e_q, object) of the tile and an R-pixel halo staged in LDS once — e_q is computed while
//                       staging and never goes to memory —, then every lane walks its window in LDS.
// The arithmetic is fixed operation by operation (include/rtpbr.h) so that the CPU restatement matches bit for bit
// (tests/half_ref/half_ref.c).
#pragma once
#include "rt_noise.hpp"

namespace rt {

struct HalfArgs {
    const float4* image_buffer;
    float4* snapshot;             // half_update: in / out
    float4* half_a;               // half_update: in / out; half_subtract: in
    float4* half_b;               // half_subtract: out
    int32_t width, height;
};

struct ErrorArgs {
    const float* da;              // (W,H,3): the filter's display colour of half A
    const float* db;              // ... of half B
    const float4* half_a;         // the count words: cA
    const float4* half_b;         // ... cB (as half_subtract wrote it: image_buffer.w - A.w)
    const int32_t* object;        // RTPBR_BUF_FEAT_OBJECT
    float* error;                 // out: RTPBR_BUF_DENOISED_ERROR
    NoiseStats* stats;            // out (zeroed before the launch)
    float threshold;
    int32_t width, height;
    int32_t radius;               // 1..3
};

void launch_half_update(const HalfArgs& A, hipStream_t st);
void launch_half_subtract(const HalfArgs& A, hipStream_t st);
void launch_half_error(const ErrorArgs& A, hipStream_t st);

}  // namespace rt
