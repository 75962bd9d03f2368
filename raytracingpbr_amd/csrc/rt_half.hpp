// rt_half.hpp — the two-half error estimate of the denoised frame (rtpbr_half_update, rtpbr_denoise_error), the bias-aware
// blend of the denoised and the raw frame made from the same halves (rtpbr_denoise_blend), the same blend across the a-trous
// levels (rtpbr_denoise_blend_levels) and the error estimate of that level-blended frame (rtpbr_blend_error).
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
//   half_blend<R>       rtpbr_denoise_blend's window kernel, in half_error<R>'s layout.  From the LINEAR filter results of the full
//                       frame and of either half (atrous_level's LINEAR form, rt_features.hip) and the three raw averages it
//                       stages (a_q, q_q, x_q, object) — the regression's cross term, (filtered - raw)^2 and the product of the
//                       halves' (filtered - raw), whose expectation is bias^2 —, sums them over the window on the pixel's
//                       object, makes the weight t (RTPBR_BUF_BLEND_WEIGHT), blends the filtered and the raw colour, tone-maps
//                       and writes RTPBR_BUF_DENOISED_PIXELS; statistics through nz_stats.
//   level_blend<R,F,L>  rtpbr_denoise_blend_levels' window kernel, one launch per a-trous level k = 1..K, in half_blend<R>'s
//                       layout.  The non-last atrous_level instances run all K levels of the full frame and of either half in lock
//                       step, each chain in a ping-pong of its own, so the records of level k - 1 and k are both live (six float4
//                       planes).  The kernel applies half_blend's rule with the finer level in the place of the raw average
//                       (FIRST: level 0 from the (sum, count) buffers), makes t_k, and the lane updates its own pixel's running
//                       product T_k = T_{k-1} t_k, the depth sum of T_k and the colour c = c + T_k (FD_k - FD_{k-1}) in place
//                       (RTPBR_BUF_BLEND_WEIGHT, RTPBR_BUF_BLEND_DEPTH, RTPBR_BUF_DENOISED_PIXELS); LAST tone-maps and makes the
//                       statistics.  level_blend_none: K = 0.
//   level_blend<.., ERR> rtpbr_blend_error's instances of the same kernel: the lane also applies its T_k to either half's own ladder
//                       (XA, XB: two more float4 planes of running state, the centre pixel's four half records the only new
//                       loads: 64 bytes read and 32 read and written per pixel and level, where a kernel of its own per level
//                       would read T_k and the records again and launch K more times).  LAST leaves in the first plane what the
//                       window kernel stages — (lum XA, display lum XA, lum XB, display lum XB) — and in the error plane the
//                       slope s of the display luminance at the blended colour: the tone map runs four times per pixel here and
//                       never per staged entry.
//   level_blend<.., LIN> the last level of the three calls with option blend_coverage = 1 (the chains then ran atrous_level's COVER
//                       form): the blended linear colour — exactly the value the other form hands to tone_map, +0 for a pixel
//                       without samples — stays in `out`, for these calls a private (W,H,3) plane that carried the running colour of
//                       the levels before, from which cover_resolve (rt_coverage.hip) makes RTPBR_BUF_DENOISED_PIXELS.  Weight, depth, statistics and with ERR the slope and the four luminances are
//                       those of the pre-resolve colour, computed as without LIN.
//   level_blend<.., FILL> the last level of the three calls with option blend_fill = 1 (the chains then ran atrous_level's FILL form, or
//                       COVER and FILL: a pixel without samples takes a colour at the first level that reaches its object).  A pixel
//                       whose image_buffer count is 0 is shown from the last record of image_buffer's chain: a colour there is the
//                       remodulated F_K (weight 1, depth K — the running sums' values, the pixel was never usable), NO_SAMPLES
//                       leaves what post_process shows (weight 1, depth 0).  The lane counts both kinds into the call's shards
//                       (rt_features.hpp FILL_SHARDS; the levels raised the deepest level already) and, with LIN, writes the
//                       byte plane cover_resolve's FILL form reads.  The two pointers live in LevelsFillArgs, which only these
//                       instances take: LevelsArgs and every other instance's argument block stay as they were.  The levels before
//                       the last need no form of their own: what they leave of such a pixel the last level overwrites.
//   blend_error<R>      rtpbr_blend_error's window kernel, in half_error<R>'s layout with four planes (e_q, x_q, usable_q, object):
//                       e_q is half_error's with the blended halves' display luminances, x_q the product of the halves' (blended -
//                       raw) in linear luminance; the lane sums both over the window on its object and writes the root of
//                       variance + s^2 bias^2 into RTPBR_BUF_BLEND_ERROR; statistics through nz_stats.
//   blend_error<R, DISPLAY>  rtpbr_blend_error_display's instances: the staged x_q is (s_q s_q) x_q with the entry's own slope, read
//                       from a (W,H) plane of its own that the LAST ERR instance fills in the place of the error plane (a halo
//                       entry's slope belongs to a pixel whose error word another block may already have written), and the
//                       lane writes the root of variance + the window's mean of that.
// The arithmetic is fixed operation by operation (include/rtpbr.h) so that the CPU restatement matches bit for bit
// (tests/half_ref/half_ref.c, tests/post_ref/blend.h).
#pragma once
#include "rt_features.hpp"
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

struct BlendArgs {
    rtpbr_config cfg;             // tone map
    const float4* image_buffer;   // b
    const float4* half_a;         // A
    const float4* half_b;         // B as half_subtract wrote it
    const float* fd;              // (W,H,3): the filter's linear colour of image_buffer
    const float* fa;              // ... of half A
    const float* fb;              // ... of half B
    const int32_t* object;        // RTPBR_BUF_FEAT_OBJECT
    float* weight;                // out: RTPBR_BUF_BLEND_WEIGHT
    float* out;                   // out: RTPBR_BUF_DENOISED_PIXELS
    NoiseStats* stats;            // out (zeroed before the launch)
    float min_half;               // (float)min_half_samples
    float z2;                     // z * z
    int32_t width, height;
    int32_t radius;               // 1..3
};

struct LevelsArgs {
    rtpbr_config cfg;             // tone map (LAST)
    const float4* image_buffer;   // b: level 0 (FIRST), pixels without samples (LAST)
    const float4* half_a;         // A: the count words; level 0 (FIRST)
    const float4* half_b;         // B as half_subtract wrote it
    const float4* kd;             // level k's (colour, object word) of image_buffer; nullptr: K = 0
    const float4* ka;             // ... of half A
    const float4* kb;             // ... of half B
    const float4* pd;             // level k - 1's, of image_buffer (not FIRST)
    const float4* pa;             // ... of half A
    const float4* pb;             // ... of half B
    const float* albedo;          // (W,H,3): remodulation
    const int32_t* object;        // RTPBR_BUF_FEAT_OBJECT
    float* weight;                // in / out: the running T_k; RTPBR_BUF_BLEND_WEIGHT after LAST
    float* depth;                 // in / out: the running sum of T_k; RTPBR_BUF_BLEND_DEPTH
    float* out;                   // in / out: the running linear colour; LAST: RTPBR_BUF_DENOISED_PIXELS (LIN instances: a private plane that
                                  // stays linear, +0 without samples — the struct does not grow, so every other instance keeps its kernarg offsets)
    NoiseStats* stats;            // out (zeroed before the launches; LAST adds to it)
    float4* xa;                   // ERR instances, in / out: the running XA; after LAST (lum XA, display lum XA, lum XB, display lum XB)
    float4* xb;                   // ... the running XB
    float* slope;                 // ERR instances, LAST: out, s (the plane of RTPBR_BUF_BLEND_ERROR, which blend_error<R> then overwrites;
                                  // rtpbr_blend_error_display: a plane of its own)
    float min_half;               // (float)min_half_samples
    float z2;                     // z * z
    int32_t demodulate;
    int32_t width, height;
    int32_t radius;               // 1..3
};

// level_blend's FILL instances (last level, option blend_fill = 1): LevelsArgs and, behind it, what only they need
struct LevelsFillArgs : LevelsArgs {
    uint32_t* fill;               // the call's counts: FILL_SHARDS x FILL_SHARD_WORDS words (filled, empty, deepest level), as atrous_level's
    uint8_t* live;                // LIN: out, (W,H) 1 = the pixel has a colour (samples, or filled by level K), 0 = still empty (out takes +0)
};

struct BlendErrorArgs {
    const float4* lx;             // (W,H): (lum XA, display lum XA, lum XB, display lum XB) as level_blend's LAST ERR instance left it
    const float4* half_a;         // A: the count word cA, PA
    const float4* half_b;         // B as half_subtract wrote it
    const int32_t* object;        // RTPBR_BUF_FEAT_OBJECT
    float* error;                 // in: s per pixel; out: RTPBR_BUF_BLEND_ERROR
    NoiseStats* stats;            // out (zeroed before the launch)
    float threshold;
    float min_half;               // (float)min_half_samples
    int32_t width, height;
    int32_t radius;               // 1..3
    // (behind the others: the instances of rtpbr_blend_error keep their argument offsets)
    const float* slope;           // nullptr, or (rtpbr_blend_error_display) s per pixel in a plane of its own: `error` is then out only
};

void launch_half_update(const HalfArgs& A, hipStream_t st);
// form: LEVEL_FIRST, LEVEL_LAST (rt_features.hpp) and BLEND_LIN: the last level is the LIN instance (A.out stays linear).  A.xa !=
// nullptr: the ERR instances; fill != nullptr: the last level is the FILL instance (live: with BLEND_LIN, the plane it writes).
// false: the form has no instance (level_blend_form_ok, rt_dispatch.hpp), nothing was launched
enum : unsigned { BLEND_LIN = 4u };
bool launch_level_blend(const LevelsArgs& A, unsigned form, hipStream_t st, uint32_t* fill, uint8_t* live);
void launch_blend_error(const BlendErrorArgs& A, hipStream_t st);
void launch_half_blend(const BlendArgs& A, hipStream_t st);
void launch_half_subtract(const HalfArgs& A, hipStream_t st);
void launch_half_error(const ErrorArgs& A, hipStream_t st);

}  // namespace rt
