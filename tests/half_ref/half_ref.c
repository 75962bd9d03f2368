/*
 * half_ref.c — CPU restatement of rtpbr_half_update, the subtract pass, the window estimate of rtpbr_denoise_error and the rule
 * of rtpbr_select_error (TEST INFRASTRUCTURE ONLY).
 *
 * Plain C, built by tests/half_ref_lib.py with the oracle's floating-point flags (-ffp-contract=off, no fast math): only hr_*
 * is exported.  The two filter runs of rtpbr_denoise_error are not here: they go through tests/feature_ref_lib.py.  The
 * arithmetic follows include/rtpbr.h operation by operation; the HIP kernels are in raytracingpbr_amd/csrc/rt_half.hip and
 * rt_select.hip.
 */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#define HR_API __attribute__((visibility("default")))

static inline float lum(const float* c) { return (0.299f * c[0] + 0.587f * c[1]) + 0.114f * c[2]; }

/* image (W,H,4); snapshot and half_a (W,H,4) are updated in place */
HR_API int hr_update(int W, int H, const float* image, float* snapshot, float* half_a) {
    const size_t n = (size_t)W * H;
    for (size_t i = 0; i < n; i++) {
        const float* b = image + i * 4;
        float* s = snapshot + i * 4;
        float* a = half_a + i * 4;
        float d[4];
        for (int k = 0; k < 4; k++) d[k] = b[k] - s[k];
        if (d[3] > 0.0f) {
            const float cB = s[3] - a[3];
            if (a[3] <= cB)
                for (int k = 0; k < 4; k++) a[k] = a[k] + d[k];
        }
        for (int k = 0; k < 4; k++) s[k] = b[k];
    }
    return 0;
}

/* half_b = image - half_a per component */
HR_API int hr_subtract(int W, int H, const float* image, const float* half_a, float* half_b) {
    const size_t n = (size_t)W * H * 4;
    for (size_t i = 0; i < n; i++) half_b[i] = image[i] - half_a[i];
    return 0;
}

/* da, db (W,H,3): the filter's display colour of the halves; half_a, half_b (W,H,4): their count words are cA and cB;
 * error (W,H); e_map (W,H): e_q, -1 where q is not valid; stats = {pixels_estimated, pixels_above, bits of the maximum} */
HR_API int hr_error(int W, int H, const float* da, const float* db, const float* half_a, const float* half_b, const int32_t* object,
                    int radius, float threshold, float* error, float* e_map, uint32_t* stats) {
    if (radius < 1 || radius > 3) return -1;
    const size_t n = (size_t)W * H;
    float* e = e_map;
    for (size_t q = 0; q < n; q++) {
        const float cA = half_a[q * 4 + 3], cB = half_b[q * 4 + 3];
        if (cA > 0.0f && cB > 0.0f) {
            const float dl = lum(da + q * 3) - lum(db + q * 3);
            e[q] = fmaxf((dl * dl) * ((cA * cB) / ((cA + cB) * (cA + cB))), 0.0f);
        } else {
            e[q] = -1.0f;
        }
    }
    uint32_t est = 0, above = 0, mx = 0;
    for (int x = 0; x < W; x++)
        for (int y = 0; y < H; y++) {
            const size_t p = (size_t)x * H + y;
            if (!(e[p] >= 0.0f)) {
                error[p] = 0.0f;
                continue;
            }
            float S = 0.0f, cn = 0.0f;
            for (int dy = -radius; dy <= radius; dy++) {
                const int yq = y + dy;
                if (yq < 0 || yq >= H) continue;
                for (int dx = -radius; dx <= radius; dx++) {
                    const int xq = x + dx;
                    if (xq < 0 || xq >= W) continue;
                    const size_t q = (size_t)xq * H + yq;
                    if (object[q] != object[p] || !(e[q] >= 0.0f)) continue;
                    S = S + e[q];
                    cn = cn + 1.0f;
                }
            }
            const float sd = sqrtf(S / cn);
            error[p] = sd;
            est++;
            if (sd > threshold) above++;
            uint32_t bits;
            memcpy(&bits, &sd, 4);
            if (bits > mx) mx = bits;
        }
    stats[0] = est;
    stats[1] = above;
    stats[2] = mx;
    return 0;
}

/* mask (W,H) u8: the rule of rtpbr_select_error; returns how many are selected */
HR_API int hr_select(int W, int H, const float* image, const float* half_a, const float* error, float threshold, int dilate,
                     float min_samples, uint8_t* mask) {
    int count = 0;
    for (int x = 0; x < W; x++)
        for (int y = 0; y < H; y++) {
            const size_t p = (size_t)x * H + y;
            const float cnt = image[p * 4 + 3], ca = half_a[p * 4 + 3];
            int sel = !(cnt > 0.0f) || !(ca > 0.0f) || !(cnt - ca > 0.0f) || cnt < min_samples;
            for (int dx = -dilate; dx <= dilate && !sel; dx++)
                for (int dy = -dilate; dy <= dilate && !sel; dy++) {
                    const int xq = x + dx, yq = y + dy;
                    if (xq < 0 || xq >= W || yq < 0 || yq >= H) continue;
                    if (error[(size_t)xq * H + yq] > threshold) sel = 1;
                }
            mask[p] = (uint8_t)sel;
            count += sel;
        }
    return count;
}
