/*
 * blend_fill_ref.c — the CPU restatement of rtpbr_denoise_blend_levels, rtpbr_blend_error and rtpbr_blend_error_display with
 * option blend_fill = 1, without and with option blend_coverage (TEST INFRASTRUCTURE ONLY): the level blend on ladders that fill
 * their pixels without samples.  include/rtpbr.h operation by operation; the HIP kernels are atrous_level's FILL and COVER + FILL
 * forms (raytracingpbr_amd/csrc/rt_features.hip), level_blend<R, FIRST, LAST, ERR, LIN, FILL> and blend_error<R, DISPLAY>
 * (rt_half.hip), cover_weights and cover_resolve's FILL form (rt_coverage.hip).
 *
 * Three steps.  (1) bf_fill_levels: F_0 .. F_K of one buffer and, per level, who holds a colour; one tap loop for the plain and
 * the coverage-weighted filter (the weight k_q is applied only where a plane of them is given).  (2) blend.h's rule, unchanged,
 * on those ladders: a pixel with samples keeps its windows, statistics and error.  (3) the pixels whose image_buffer count is 0,
 * which blend.h shows as post_process does: the ones that level K of the whole buffer's ladder coloured are shown with F_K
 * (weight 1, depth K), the others keep post_process's colour (weight 1, depth 0); with blend_coverage the resolve runs over "has
 * a colour" = has samples or was filled.  Built by tests/ref_build.py with the oracle's flags, as post_ref.
 */
#include "../../oracle/rt_oracle.c"

#include "../post_ref/common.h"
#include "../post_ref/filter.h"      /* filter_args, filter_finish */
#include "../post_ref/blend.h"       /* blend_ladder, lr_blend_levels, ber_blend_error */

/* k = a * a * ... (power factors, left to right), a = (float)n_own / (float)n_sub */
static void share_weights(const int32_t* coverage, size_t n, int power, float* k) {
    for (size_t i = 0; i < n; i++) {
        const float av = (float)coverage[i * 4 + 0] / (float)coverage[i * 4 + 3];
        float kk = 1.0f;
        for (int j = 0; j < power; j++) kk = kk * av;
        k[i] = kk;
    }
}

/* One buffer's filling ladder.  levels (iterations + 1, W, H, 3): F_0 .. F_K, each finished FINISH_LINEAR (+0 where the level
 * holds no colour); live (iterations + 1, W, H) bytes: 1 = the level holds a colour of the pixel; counts (may be NULL): [0] the
 * pixels that were empty and hold a colour after level K, [1] those still empty, [2] the highest level (0-based, as the library
 * counts) at which one was filled, 0 when none was.  coverage (W,H,4) int32 or NULL: NULL is the plain filter (option
 * denoise_fill's rule), a plane the coverage-weighted one at `power` (option coverage_fill's rule). */
POST_API int bf_fill_levels(const rtpbr_config* cfg, const float* image_buffer, const float* albedo, const float* normal,
                            const float* depth, const int32_t* object, const int32_t* coverage, int iterations, int demodulate,
                            float sigma_color, float sigma_normal, float sigma_depth, float sigma_albedo, int power, float* levels,
                            unsigned char* live, uint32_t* counts) {
    const int W = cfg->width, H = cfg->height;
    const size_t n = (size_t)W * H;
    const filter_args a = {albedo, normal, depth, object, iterations, demodulate, sigma_color, sigma_normal, sigma_depth, sigma_albedo};
    float* cur = (float*)malloc(n * 4 * sizeof(float));
    float* nxt = (float*)malloc(n * 4 * sizeof(float));
    float* k = coverage ? (float*)malloc(n * sizeof(float)) : NULL;
    if (!cur || !nxt || (coverage && !k)) { free(cur); free(nxt); free(k); return RTPBR_ENOMEM; }
    if (coverage) share_weights(coverage, n, power, k);
    /* level 0: the average, demodulated by the pixel's own albedo; word 3: 1 = holds a colour */
    for (size_t i = 0; i < n; i++) {
        const float* b = image_buffer + i * 4;
        v3 c = v3_make(b[0] / b[3], b[1] / b[3], b[2] / b[3]);
        if (demodulate) c = demodulated(c, albedo + i * 3);
        store3(cur + i * 4, c);
        cur[i * 4 + 3] = b[3] > 0.0f ? 1.0f : 0.0f;
        live[i] = b[3] > 0.0f;
    }
    filter_finish(cfg, cur, 4, image_buffer, &a, FINISH_LINEAR, levels);
    const float ic0 = 1.0f / (sigma_color * sigma_color), in = 1.0f / (sigma_normal * sigma_normal);
    const float iz = 1.0f / (sigma_depth * sigma_depth), ia = 1.0f / (sigma_albedo * sigma_albedo);
    const float HK[3] = {0.375f, 0.25f, 0.0625f};
    uint32_t filled = 0, deepest = 0;
    for (int lv = 0; lv < iterations; lv++) {
        const int s = 1 << lv;
        const float ic = ic0 * (float)(1u << (2 * lv));
        uint32_t here = 0;
        for (int x = 0; x < W; x++)
            for (int y = 0; y < H; y++) {
                const size_t i = (size_t)x * H + y;
                const int has = cur[i * 4 + 3] != 0.0f;
                const v3 rp = range_map(load3(cur + i * 4));      /* (read for a centre that has a colour only) */
                const v3 np = load3(normal + i * 3), ap = load3(albedo + i * 3);
                const float zp = depth[i], izp = fmaxf(zp, 1e-6f);
                float sw = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f;
                FOR_WINDOW(q, 2, s, x, y, W, H) {
                    if (object[q] != object[i] || cur[q * 4 + 3] == 0.0f) continue;
                    const v3 cq = load3(cur + q * 4);
                    const float h = HK[dx < 0 ? -dx : dx] * HK[dy < 0 ? -dy : dy];
                    const float dz = (zp - depth[q]) / izp;
                    float e = 0.0f;      /* an empty centre has no colour to compare: the colour term is +0 */
                    if (has) e = sq3(v3_sub(rp, range_map(cq))) * ic;
                    e = e + sq3(v3_sub(np, load3(normal + q * 3))) * in;
                    e = e + (dz * dz) * iz;
                    if (has) e = e + sq3(v3_sub(ap, load3(albedo + q * 3))) * ia;      /* (+0 on every tap taken: one object, one albedo) */
                    float w = h * rto_expf(-fminf(e, 80.0f));
                    if (k && (dx != 0 || dy != 0)) w = w * k[q];
                    sw = sw + w;
                    sx = sx + w * cq.x;
                    sy = sy + w * cq.y;
                    sz = sz + w * cq.z;
                }
                if (has || sw > 0.0f) {      /* (a centre with a colour is its own tap, at 9/64: its sum is above 0) */
                    nxt[i * 4 + 0] = sx / sw; nxt[i * 4 + 1] = sy / sw; nxt[i * 4 + 2] = sz / sw;
                    nxt[i * 4 + 3] = 1.0f;
                    if (!has) here++;
                } else {
                    memset(nxt + i * 4, 0, 4 * sizeof(float));
                }
            }
        if (here) { filled += here; deepest = (uint32_t)lv; }
        float* t = cur; cur = nxt; nxt = t;
        filter_finish(cfg, cur, 4, image_buffer, &a, FINISH_LINEAR, levels + (size_t)(lv + 1) * n * 3);
        for (size_t i = 0; i < n; i++) live[(size_t)(lv + 1) * n + i] = cur[i * 4 + 3] != 0.0f;
    }
    if (counts) {
        uint32_t empty = 0;
        for (size_t i = 0; i < n; i++) empty += cur[i * 4 + 3] == 0.0f;
        counts[0] = filled; counts[1] = empty; counts[2] = deepest;
    }
    free(cur); free(nxt); free(k);
    return RTPBR_OK;
}

/* The three calls with option blend_fill = 1 and K > 0, on the ladders fd, fa, fb (K + 1, W, H, 3) of bf_fill_levels and liveK
 * (W,H), level K's bytes of fd's ladder.  image, half_a, half_b (W,H,4); radius, z2 = z * z as the host computes it and
 * m = (float)min_half_samples are the blend's.  coverage NULL: option blend_coverage off, and out is the ladder's frame; a plane:
 * on, at `power` and `resolve`, and out is the frame after the resolve.
 * mode 0: rtpbr_denoise_blend_levels (stats = the blend's; error, parts may be NULL); 1: rtpbr_blend_error; 2:
 * rtpbr_blend_error_display (stats = the error plane's; window, threshold as ber_blend_error's).
 * out (W,H,3): RTPBR_BUF_DENOISED_PIXELS; before (W,H,3): the display frame before the resolve (= out without coverage); weight,
 * depth (W,H); error (W,H), parts (3,W,H) as ber_blend_error's; *resolved: the pixels the resolve changed (0 without coverage). */
POST_API int bf_blend_fill(const rtpbr_config* cfg, const float* image, const float* half_a, const float* half_b, const float* fd,
                           const float* fa, const float* fb, const unsigned char* liveK, const int32_t* object, const int32_t* coverage,
                           int K, int radius, float z2, float m, int power, int resolve, int mode, int window, float threshold,
                           float* out, float* before, float* weight, float* depth, float* error, float* parts, uint32_t* stats,
                           uint32_t* resolved) {
    if (radius < 1 || radius > 3 || K < 1 || mode < 0 || mode > 2) return -1;
    const int W = cfg->width, H = cfg->height;
    const size_t n = (size_t)W * H;
    const float* fdK = fd + (size_t)K * n * 3;
    /* 1. the pixels with samples: blend.h's rule on these ladders (a pixel whose count is 0 is usable in nobody's window: its
     * halves' counts sum to 0 and m >= 1), and the error plane, which is 0 where a half is empty */
    int rc = mode == 0 ? lr_blend_levels(cfg, image, half_a, half_b, fd, fa, fb, object, K, radius, z2, m, weight, depth, before, stats)
                       : ber_blend_error(cfg, image, half_a, half_b, fd, fa, fb, object, K, radius, z2, m, window, threshold, mode == 2,
                                         before, weight, depth, error, parts, stats);
    if (rc) return rc;
    /* 2. the pixels without samples: F_K where the whole buffer's ladder reached them, every t_k = 1 */
    for (size_t p = 0; p < n; p++) {
        if (image[p * 4 + 3] > 0.0f) continue;
        weight[p] = 1.0f;
        if (liveK[p]) {
            store3(before + p * 3, tone_map3(cfg, fdK + p * 3));
            depth[p] = (float)K;
        } else {
            store3(before + p * 3, tone_map(cfg, image + p * 4));
            depth[p] = 0.0f;
        }
    }
    *resolved = 0;
    if (!coverage) {
        memcpy(out, before, n * 3 * sizeof(float));
        return RTPBR_OK;
    }
    /* 3. blend_coverage: the blended linear plane (the running colour, F_K itself where T_K == 1 and for a filled pixel, +0 for a
     * pixel still empty), then cover_resolve's filling form over the pixels that have a colour */
    float* buf = (float*)malloc(n * 12 * sizeof(float));
    unsigned char* usable = (unsigned char*)malloc(n);
    unsigned char* has = (unsigned char*)malloc(n);
    if (!buf || !usable || !has) { free(buf); free(usable); free(has); return RTPBR_ENOMEM; }
    float *run = buf + 3 * n, *T = buf + 6 * n, *D = buf + 7 * n, *k = buf + 8 * n, *lin = buf + 9 * n;
    blend_ladder(W, H, half_a, half_b, fd, fa, fb, object, K, radius, z2, m, buf, usable, T, D, run, NULL, NULL);
    for (size_t p = 0; p < n; p++) {
        const int sampled = image[p * 4 + 3] > 0.0f;
        has[p] = sampled || liveK[p];
        const float* c3 = (!sampled || T[p] == 1.0f) ? fdK + p * 3 : run + p * 3;
        for (int c = 0; c < 3; c++) lin[p * 3 + c] = has[p] ? c3[c] : 0.0f;
    }
    share_weights(coverage, n, power, k);
    uint32_t count = 0;
    for (int x = 0; x < W; x++)
        for (int y = 0; y < H; y++) {
            const size_t i = (size_t)x * H + y;
            if (!has[i]) {      /* no samples and no level reached it: what post_process shows */
                store3(out + i * 3, tone_map(cfg, image + i * 4));
                continue;
            }
            v3 f = load3(lin + i * 3);
            const int32_t* cv = coverage + i * 4;
            if (resolve && cv[2] > 0) {
                float sw = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f;
                FOR_WINDOW(q, 1, 1, x, y, W, H) {
                    if ((dx == 0 && dy == 0) || object[q] != cv[1] || !has[q]) continue;
                    const float w = k[q] * ((dx == 0 || dy == 0) ? 0.5f : 1.0f / 3.0f);
                    sw = sw + w;
                    sx = sx + w * lin[q * 3 + 0];
                    sy = sy + w * lin[q * 3 + 1];
                    sz = sz + w * lin[q * 3 + 2];
                }
                if (sw > 0.0f) {
                    const float no = (float)cv[0], ns = (float)cv[2], nt = (float)(cv[0] + cv[2]);
                    f = v3_make((no * f.x + ns * (sx / sw)) / nt, (no * f.y + ns * (sy / sw)) / nt, (no * f.z + ns * (sz / sw)) / nt);
                    count++;
                }
            }
            const float c3[3] = {f.x, f.y, f.z};
            store3(out + i * 3, tone_map3(cfg, c3));
        }
    *resolved = count;
    free(buf); free(usable); free(has);
    return RTPBR_OK;
}
