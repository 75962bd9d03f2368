/*
 * half_mode_ref.c — CPU restatement of rtpbr_set_half_mode's two rules (TEST INFRASTRUCTURE ONLY).
 *
 *   hm_fold     what a dealing rtpbr_sample(n) / rtpbr_sample_selected(n) (per_sample = 1) leaves in RTPBR_BUF_HALF_BUFFER, the
 *               halves' snapshot and image_buffer, from the per-sample colours.  The HIP kernels are accumulate_*_dealt in
 *               raytracingpbr_amd/csrc/rt_kernels.hip.
 *   hm_gather   what rtpbr_reproject / rtpbr_reproject_scene (warp = 1) leave in image_buffer, RTPBR_BUF_MOTION and half A.  The
 *               HIP kernels are reproject_gather<*, true> / reproject_gather_scene<*, true> in rt_reproject.hip.
 *
 * include/rtpbr.h operation by operation, f32, nothing fused (tests/half_mode_ref_lib.py builds it with the oracle's flags,
 * -ffp-contract=off).  The gather is built from the unchanged restatement of rtpbr_reproject_scene by including its source (with
 * no object moved it is rtpbr_reproject's gather, expression for expression): half A rides through its second slot with the cap
 * switched off — max_history = +inf, so S / Wt and SA / Wt come back as they are —, and the cap is applied here by A's own rule,
 * which scales all four components by the image's quotient (the rule of that slot's fourth word is the moments', not A's).
 * Only hm_* is exported (half_mode_ref.map).
 */
#include "../reproject_scene_ref/reproject_scene_ref.c"

#define HM_API __attribute__((visibility("default")))

/* colours (n,W,H,3): sample k of pixel i at colours[(k * W * H + i) * 3]; mask (W,H) bytes, NULL = every pixel;
 * half_a, half_sh, image (W,H,4) are updated in place.  Pixels whose mask byte is 0 are not touched. */
HM_API int hm_fold(int n, int W, int H, const float* colours, const uint8_t* mask, float* half_a, float* half_sh, float* image) {
    if (n < 0 || W < 1 || H < 1 || !half_a || !half_sh || !image || (n > 0 && !colours)) return -1;
    const size_t np = (size_t)W * H;
    if (n == 0) return 0;
    for (size_t i = 0; i < np; i++) {
        if (mask && !mask[i]) continue;
        float* A = half_a + i * 4;
        float* b = image + i * 4;
        for (int k = 0; k < n; k++) {
            const float* c = colours + ((size_t)k * np + i) * 3;
            const float cB = b[3] - A[3];
            if (A[3] <= cB) {
                A[0] = A[0] + c[0];
                A[1] = A[1] + c[1];
                A[2] = A[2] + c[2];
                A[3] = A[3] + 1.0f;
            }
            b[0] += c[0];
            b[1] += c[1];
            b[2] += c[2];
            b[3] += 1.0f;
        }
        for (int j = 0; j < 4; j++) half_sh[i * 4 + j] = b[j];
    }
    return 0;
}

/* The arguments of rs_reproject_scene with old_half (W,H,4) in place of the moments; writes image (W,H,4), motion (W,H,2) and
 * half (W,H,4).  The counts of old_image must be finite. */
HM_API int hm_gather(const rtpbr_config* cfg, const rtpbr_camera* old_cam, const rtpbr_camera* new_cam, const rtpbr_object* old_objs,
                     int old_scale10, const rtpbr_object* new_objs, int new_scale10, int n_obj, const float* old_image, const float* old_half,
                     const float* old_normal, const float* old_depth, const int32_t* old_object, const float* new_normal,
                     const float* new_depth, const int32_t* new_object, float max_history, float depth_tol, float normal_cos, float* image,
                     float* motion, float* half) {
    if (!old_half || !half) return RTPBR_EINVAL;
    const int r = rs_reproject_scene(cfg, old_cam, new_cam, old_objs, old_scale10, new_objs, new_scale10, n_obj, old_image, old_half, old_normal,
                                     old_depth, old_object, new_normal, new_depth, new_object, INFINITY, depth_tol, normal_cos, image, motion, half);
    if (r) return r;
    const size_t np = (size_t)cfg->width * cfg->height;
    for (size_t i = 0; i < np; i++) {
        float* b = image + i * 4;
        float* A = half + i * 4;
        if (b[3] > max_history) {
            const float k = max_history / b[3];
            for (int j = 0; j < 4; j++) b[j] = b[j] * k;
            for (int j = 0; j < 4; j++) A[j] = A[j] * k;
        }
    }
    return RTPBR_OK;
}
