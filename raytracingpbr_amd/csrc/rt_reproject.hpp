// rt_reproject.hpp — the gather kernels of rtpbr_reproject and rtpbr_reproject_scene: temporal reuse of the accumulated samples
// across a camera move and across rigid moves of objects.
//
//   reproject_gather   one lane per pixel (the buffers' contiguous index i = x * H + y, 256-lane blocks, as feature_rays): the
//                      new pixel's first hit (or, on a miss, its direction) is projected into the old camera; the history
//                      (image_buffer before the move) is gathered bilinearly from the 2x2 old pixels around it, keeping only
//                      taps on the same object with a matching depth and normal; the sum is renormalised and capped.
//                      The same lane resets what rtpbr_refresh resets except image_buffer (ray_buffer.depth, the diff buffers).
//                      reproject_gather<true, *> also warps the noise estimate's moments (rtpbr_noise_update) with the same taps,
//                      reproject_gather<*, true> half A of the two-half error estimate (rtpbr_set_half_mode, warp).
//   reproject_gather_scene   the same gather for rtpbr_reproject_scene: a first hit on an object that moved is carried through
//                      the object's frame into the old world (and its world-space normal turned back) before it is projected;
//                      the per-object table (old and new position and matrix) is staged in LDS by every block.
// The arithmetic is fixed operation by operation (include/rtpbr.h, rtpbr_reproject and rtpbr_reproject_scene) so that the CPU
// restatements match bit for bit (tests/post_ref/gather.h).
#pragma once
#include "rt_types.hpp"

namespace rt {

struct ReprojArgs {
    CamFrame cam0, cam1;            // old and new camera frames (rtpbr_set_camera; inv_w / inv_h of the new one filled in)
    const float4* hist_image;       // (W,H): image_buffer before the move
    const float4* hist_nz;          // (W,H): the old features' (normal, depth) records
    const int32_t* hist_object;     // (W,H): the old features' object indices
    const float4* new_nz;           // (W,H): the new features' (normal, depth) records
    const int32_t* new_object;      // (W,H)
    float4* image_buffer;           // out
    float2* motion;                 // out (RTPBR_BUF_MOTION)
    rtpbr_ray* ray_buffer;          // out: depth = 0
    float2* diff_buffer;            // out when adaptive: (1, 1)
    float* diff_pixels;             // out when adaptive: 1e32
    float max_history, depth_tol, normal_cos;
    int32_t width, height;
    int32_t pinhole;                // cfg.camera_kind == RTPBR_CAMERA_PINHOLE (how the new centre ray's u, v are formed)
    int32_t adaptive;
    int32_t normal_local;           // cfg.normal_space == RTPBR_NORMAL_LOCAL (reproject_gather_scene: stored normals do not turn with the object)
    // the noise estimate's moments (rt_noise.hpp), when the context tracks them: nullptr otherwise
    const float4* hist_moments;     // (W,H): the moments before the move
    float4* moments;                // out: warped with the image's taps and weights, capped with it
    float4* snapshot;               // out: the warped image_buffer
    // half A of the two-half error estimate (rt_half.hpp), when the context carries it (rtpbr_set_half_mode, warp): nullptr otherwise
    const float4* hist_half;        // (W,H): half A before the move
    float4* half_a;                 // out: warped with the image's taps and weights, scaled with it where the cap applies
};

// rtpbr_reproject_scene's per-object record: the moved flag (0.0f / 1.0f), p0, p1, R0, R1 (0 = old, 1 = new; R row major)
constexpr int SCENE_MOTION_WORDS = 25;

void launch_reproject(const ReprojArgs& A, hipStream_t st);
// table: device memory, n_obj * SCENE_MOTION_WORDS floats (n_obj <= MAX_OBJ)
void launch_reproject_scene(const ReprojArgs& A, const float* table, int n_obj, hipStream_t st);

}  // namespace rt
