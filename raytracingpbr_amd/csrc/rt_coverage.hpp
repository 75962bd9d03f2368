// rt_coverage.hpp — sub-pixel object coverage and the edge resolve (rtpbr_render_coverage, rtpbr_denoise_coverage).
//
// The features (rt_features.hpp) describe the ray through a pixel's CENTRE, while the pixel's samples are jittered over the whole
// pixel: on a silhouette the average in image_buffer mixes two objects and the filter takes it for a pure member of the centre's.
// These kernels count, for the pixels next to a silhouette only, how much of the pixel each object covers:
//   cover_mark        one lane per pixel: a pixel is a CANDIDATE when its 3x3 neighbourhood of the object plane holds another index.
//                     Every other pixel gets its record (S, -2, 0, S) here; the candidates go into a list built as the selection's
//                     is (rt_select.hip): a wave ballot, the lane's rank by mbcnt, one atomic per wave (the list's order is not
//                     defined and nothing depends on it).
//   cover_rays<K,G>   one lane per SUB-RAY of a candidate, S = G x G lanes per pixel (G = 4: one DPP row a pixel, four pixels a
//                     wave; G = 2: sixteen pixels a wave): sub-ray (a, b) is the feature ray of pixel (G px + a, G py + b) of the
//                     G-fold frame — same camera frame, march and wave loop as feature_rays.  The counts are reduced inside the
//                     lane group with shuffles (no memory pass); the group's first lane writes the record.
//   cover_weights     one lane per pixel: k = (n_own / S)^power into the plane an a-trous tap reads (atrous_level's COVER form,
//                     rt_features.hip), and the largest 1 - n_own / S of the frame.
//   cover_resolve     one lane per pixel, 16 x 16 tiles with a one-pixel halo of (F, object word, k) in LDS: the edge resolve on
//                     the filter's LINEAR result F and the tone map of every pixel (include/rtpbr.h, rtpbr_denoise_coverage).
//                     Its FILL form (option coverage_fill = 1) takes who has a colour from the plane the filling last level wrote.
// The arithmetic is fixed operation by operation in include/rtpbr.h; tests/coverage_ref restates it on the CPU.
#pragma once
#include "rt_types.hpp"

namespace rt {

constexpr int COVER_HEAD = 4;      // words in front of the candidate list: its length, the resolved pixels, the bits of max (1 - a), 0

struct CoverageArgs {
    const int32_t* object;        // (W,H) RTPBR_BUF_FEAT_OBJECT
    int4* coverage;               // (W,H) the coverage plane: (n_own, second_object, n_second, n_sub)
    uint32_t* list;               // COVER_HEAD words, then room for W * H candidates (buffer indices x * H + y)
    float* k;                     // (W,H): cover_weights
    int32_t width, height;        // of the frame (the Params of cover_rays carry the G-fold size)
    int32_t grid;                 // G
    int32_t power;
};

struct ResolveArgs {
    rtpbr_config cfg;             // tone map
    const float4* image_buffer;   // a pixel has samples when its count > 0; without, it shows what post_process shows
    const float* linear;          // (W,H,3): F, the filter's linear result (+0 without samples)
    const int32_t* object;
    const int4* coverage;
    const float* k;
    uint32_t* head;               // the list's head: [1] += resolved pixels
    float* out;                   // (W,H,3) denoised display colour
    int32_t width, height;
    int32_t resolve;
    const uint8_t* live;          // option coverage_fill = 1: (W,H) 1 = the pixel has a colour after the last level (then that, not the count, says who is shown, tapped and resolved); else null
};

void launch_cover_mark(const CoverageArgs& A, hipStream_t st);                              // the caller has zeroed the head
void launch_cover_rays(const Params& Pg, const CoverageArgs& A, int kind, int n_cu, int blocks, hipStream_t st);   // Pg: the G-fold configuration; blocks: 0 = automatic
void launch_cover_weights(const CoverageArgs& A, hipStream_t st);                           // the caller has zeroed head[1], head[2]
void launch_cover_resolve(const ResolveArgs& A, hipStream_t st);

}  // namespace rt
