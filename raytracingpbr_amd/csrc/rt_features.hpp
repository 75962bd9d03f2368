// rt_features.hpp — first-hit feature buffers and the edge-aware a-trous filter (rtpbr_render_features, rtpbr_denoise and the
// filter levels of rtpbr_denoise_guided: the plain and the variance-guided filter are instances of one kernel).
//
// The reference's post_process() (src/postprocessor.py:24-43) tone-maps the raw Monte Carlo average and leaves a
// "# ToDo: Post Denoise" where a filter would go.  These kernels fill that gap without touching the sample path:
//   feature_rays<KIND>   one lane per pixel: the primary ray through the pixel centre (gen_ray with both jitters 0.5, no
//                        lens offset), marched with the configured march kind; writes albedo / shading normal / depth /
//                        object index of the first hit (RTPBR_BUF_FEAT_*) and the packed (normal, depth) record the filter reads;
//   atrous_level<F,L,G>  one a-trous level (Dammertz et al. 2010, "Edge-avoiding A-Trous wavelet transform for fast global
//                        illumination filtering"): 5x5 B3-spline taps at stride 2^k, weighted by colour, normal, depth and
//                        albedo distance (the last is 0 on every tap taken: see atrous_level), skipping other objects and empty
//                        pixels.  A level's output record is (colour, object index).  The average / demodulation is fused into
//                        the first level, remodulation and the tone map into the last.  GUIDED (rtpbr_denoise_guided): the
//                        colour term is scaled by the 3x3-filtered variance of the centre instead of a uniform sigma, and the
//                        variance (rt_noise.hip's estimate at level 0) is filtered along with the squared weights; it travels
//                        in a record of its own, 4 bytes, loaded only on taps that pass the object test.
//   atrous_none          iterations = 0 of either call: the average, tone-mapped.
//   COVER (rtpbr_denoise_coverage): the plain filter with every tap but the centre's weighted by the tap's coverage (rt_coverage.hpp).
//   FILL (rtpbr_denoise with option denoise_fill = 1): the plain filter in which a pixel without a colour takes the feature-weighted
//   mean of the live taps on its object, at the first level that reaches one.
//   COVER and FILL together (rtpbr_denoise_coverage with option coverage_fill = 1): the empty centre's taps carry the coverage weight
//   too, and the last level, LINEAR, writes who has a colour into a (W,H) byte plane for the resolve (rt_coverage.hip).
//   The last level and atrous_none have a LINEAR form (rtpbr_denoise_blend): the colour before the tone map goes to `out`.
//   rtpbr_denoise_blend_levels reads the non-last levels' records themselves: level k's (colour, object index) is the filter with
//   iterations = k before remodulation (level_blend, rt_half.hip).
// The arithmetic is fixed operation by operation (include/rtpbr.h, rtpbr_denoise / rtpbr_denoise_guided) so that the CPU
// restatements match bit for bit (tests/feature_ref, tests/noise_ref).
#pragma once
#include "rt_types.hpp"

namespace rt {

// feature_rays arguments (beside a copy of the context's Params, which stays the first kernel argument: the march table is
// read from the kernarg segment at offsetof(Params, objm))
struct FeatArgs {
    float* albedo;        // (W,H,3)
    float* normal;        // (W,H,3)
    float* depth;         // (W,H)
    int32_t* object;      // (W,H)
    float4* guide_nz;     // (W,H): (normal.xyz, depth)
};

// The counts of the FILL form: a wave adds to shard (its index in the grid) % FILL_SHARDS — (filled, empty, deepest level) in the first
// three words of a 64-byte line of its own, so that the waves of a lattice frame, which all report, do not queue on one address.
constexpr int FILL_SHARDS = 64, FILL_SHARD_WORDS = 16;

// object word of a level's output record for a pixel without a colour: matches no object index (>= -1).  level_blend's FILL instances
// (rt_half.hip) ask the last level's record of image_buffer's chain whether the ladder gave the pixel one.
constexpr int NO_SAMPLES = -2;

// atrous_level arguments: one level
struct DenoiseArgs {
    rtpbr_config cfg;             // tone map
    const float4* image_buffer;   // T7: read by the first level (average) and by the last (empty pixels, as post_process)
    const float4* guide_nz;
    const float* albedo;          // (W,H,3): the centre's, for (de)modulation
    const int32_t* object;        // (W,H): level 0's taps
    const float4* src;            // levels > 0: the previous level's (colour, object index as bits; -2 = pixel without samples)
    float4* dst;                  // every level but the last
    float* out;                   // the last level: denoised display colour (W,H,3); the linear form: the colour before the tone map
    float ic, in, iz;             // 1/sigma^2 of colour (already x 4^k; plain only), normal, depth (the albedo term is 0 on every tap taken)
    int32_t step;                 // 2^k
    int32_t demodulate;
    int32_t width, height;
    // the guided instances only (the coverage-weighted ones are plain: their plane shares var0's word, the layout stays as it was)
    union {
        const float* var0;        // level 0: v of noise_estimate (-1: no samples)
        const float* cover_k;     // COVER (rtpbr_denoise_coverage, rt_coverage.hpp): (W,H) k = (n_own / S)^power, the weight of the pixel as somebody's tap
    };
    union {
        const float* vsrc;        // levels > 0: the previous level's variance
        uint32_t* fill;           // FILL (rtpbr_denoise with option denoise_fill = 1; plain): the call's counts, FILL_SHARDS x FILL_SHARD_WORDS words
    };
    union {
        float* vdst;              // every level but the last
        uint8_t* live;            // COVER and FILL, the last level (LINEAR): (W,H) 1 = the pixel has a colour, 0 = still empty (out takes +0)
    };
    float sc2;                    // sigma_color * sigma_color
    float floor;                  // variance_floor
};

// r(c) = c / (1 + c): the compression the filter measures colour distances in and rt_noise.hip estimates the noise of
RT_D vec3 tonemap_r(vec3 c) { return mk(c.x / (1.0f + c.x), c.y / (1.0f + c.y), c.z / (1.0f + c.z)); }

// The form word of a filter launch: where the level stands in its chain, and the chain's kind.  LEVEL_* are level_blend's too.
enum : unsigned {
    LEVEL_FIRST = 1u,       // reads the (sum, count) buffer, not a record
    LEVEL_LAST = 2u,        // writes `out`, not a record
    LEVEL_ONLY = LEVEL_FIRST | LEVEL_LAST,
    ATROUS_GUIDED = 4u,     // rtpbr_denoise_guided
    ATROUS_LINEAR = 8u,     // the chain's last level (or its pass without a level) stops before the tone map; the levels before it are as without
    ATROUS_COVER = 16u,     // A.cover_k weights the taps; a last level of it only with ATROUS_LINEAR
    ATROUS_FILL = 32u,      // A.fill counts the pixels filled; with ATROUS_COVER the last level writes A.live
};

void launch_features(const Params& P, const FeatArgs& A, int kind, hipStream_t st);
// A.step = 0 (no level, LEVEL_ONLY) is the tone-map-only pass of every chain without ATROUS_COVER and ATROUS_FILL.  false: the form
// has no instance (atrous_form_ok, rt_dispatch.hpp), nothing was launched
bool launch_atrous_level(const DenoiseArgs& A, unsigned form, hipStream_t st);

}  // namespace rt
