/*
 * levels_ref.c — CPU restatement of rtpbr_denoise_blend_levels (TEST INFRASTRUCTURE ONLY).
 *
 * Built on demand by tests/levels_ref_lib.py the way tests/blend_ref_lib.py builds the blend's restatement: the oracle's source is
 * included for its tone map and exp (hidden visibility, -Bsymbolic: only lr_* is exported).  lr_filter_levels restates
 * rtpbr_denoise's filter once and hands out every level on the way, F_0 .. F_K, each remodulated as a last level would be;
 * tests/test_levels_ref.py holds F_k equal to blend_ref's filter with iterations = k.  The subtract pass goes through
 * tests/half_ref_lib.py.  The arithmetic follows include/rtpbr.h operation by operation; the HIP kernels are
 * level_blend<R, FIRST, LAST> (raytracingpbr_amd/csrc/rt_half.hip) and the non-last atrous_level instances (rt_features.hip).
 */
#include "../../oracle/rt_oracle.c"

#define LR_API __attribute__((visibility("default")))

static inline float lr_sq3(v3 v) { return (v.x * v.x + v.y * v.y) + v.z * v.z; }
static inline v3 lr_r(v3 c) { return v3_make(c.x / (1.0f + c.x), c.y / (1.0f + c.y), c.z / (1.0f + c.z)); }
static inline float lr_lum(const float* c) { return (0.299f * c[0] + 0.587f * c[1]) + 0.114f * c[2]; }

/* F_k of the level held in cur (colour, 1 = has samples): the linear colour after remodulation, +0 without samples */
static void lr_emit(const float* cur, const float* albedo, int demodulate, size_t n, float* out) {
    for (size_t i = 0; i < n; i++) {
        v3 c = v3_make(0.0f, 0.0f, 0.0f);
        if (cur[i * 4 + 3] != 0.0f) {
            const float* a = albedo + i * 3;
            c = v3_make(cur[i * 4], cur[i * 4 + 1], cur[i * 4 + 2]);
            if (demodulate) c = v3_make(c.x * fmaxf(a[0], 1e-3f), c.y * fmaxf(a[1], 1e-3f), c.z * fmaxf(a[2], 1e-3f));
        }
        out[i * 3 + 0] = c.x; out[i * 3 + 1] = c.y; out[i * 3 + 2] = c.z;
    }
}

/* out (iterations + 1, W, H, 3): F_0 .. F_K of this buffer */
LR_API int lr_filter_levels(const rtpbr_config* cfg, const float* image_buffer, const float* albedo, const float* normal,
                            const float* depth, const int32_t* object, int iterations, int demodulate, float sigma_color,
                            float sigma_normal, float sigma_depth, float sigma_albedo, float* out) {
    const int W = cfg->width, H = cfg->height;
    const size_t n = (size_t)W * H;
    float* cur = (float*)malloc(n * 4 * sizeof(float));      /* (colour, 1 = has samples) */
    float* nxt = (float*)malloc(n * 4 * sizeof(float));
    if (!cur || !nxt) { free(cur); free(nxt); return RTPBR_ENOMEM; }
    for (size_t i = 0; i < n; i++) {
        const float* b = image_buffer + i * 4;
        const float* a = albedo + i * 3;
        v3 c = v3_make(b[0] / b[3], b[1] / b[3], b[2] / b[3]);
        if (demodulate) c = v3_make(c.x / fmaxf(a[0], 1e-3f), c.y / fmaxf(a[1], 1e-3f), c.z / fmaxf(a[2], 1e-3f));
        cur[i * 4 + 0] = c.x; cur[i * 4 + 1] = c.y; cur[i * 4 + 2] = c.z;
        cur[i * 4 + 3] = b[3] > 0.0f ? 1.0f : 0.0f;
    }
    lr_emit(cur, albedo, demodulate, n, out);
    const float ic0 = 1.0f / (sigma_color * sigma_color), in = 1.0f / (sigma_normal * sigma_normal);
    const float iz = 1.0f / (sigma_depth * sigma_depth), ia = 1.0f / (sigma_albedo * sigma_albedo);
    const float HK[3] = {0.375f, 0.25f, 0.0625f};
    for (int k = 0; k < iterations; k++) {
        const int s = 1 << k;
        const float ic = ic0 * (float)(1u << (2 * k));
#ifdef _OPENMP
#pragma omp parallel for schedule(static)
#endif
        for (int x = 0; x < W; x++)
            for (int y = 0; y < H; y++) {
                const size_t i = (size_t)x * H + y;
                if (cur[i * 4 + 3] == 0.0f) {
                    memset(nxt + i * 4, 0, 4 * sizeof(float));
                    continue;
                }
                const v3 cp = v3_make(cur[i * 4], cur[i * 4 + 1], cur[i * 4 + 2]);
                const v3 rp = lr_r(cp);
                const v3 np = v3_make(normal[i * 3], normal[i * 3 + 1], normal[i * 3 + 2]);
                const v3 ap = v3_make(albedo[i * 3], albedo[i * 3 + 1], albedo[i * 3 + 2]);
                const float zp = depth[i], izp = fmaxf(zp, 1e-6f);
                float sw = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f;
                for (int dy = -2; dy <= 2; dy++) {
                    const int yq = y + s * dy;
                    if (yq < 0 || yq >= H) continue;
                    for (int dx = -2; dx <= 2; dx++) {
                        const int xq = x + s * dx;
                        if (xq < 0 || xq >= W) continue;
                        const size_t q = (size_t)xq * H + yq;
                        if (object[q] != object[i] || cur[q * 4 + 3] == 0.0f) continue;
                        const v3 cq = v3_make(cur[q * 4], cur[q * 4 + 1], cur[q * 4 + 2]);
                        const float h = HK[dx < 0 ? -dx : dx] * HK[dy < 0 ? -dy : dy];
                        const float dz = (zp - depth[q]) / izp;
                        float e = lr_sq3(v3_sub(rp, lr_r(cq))) * ic;
                        e = e + lr_sq3(v3_sub(np, v3_make(normal[q * 3], normal[q * 3 + 1], normal[q * 3 + 2]))) * in;
                        e = e + (dz * dz) * iz;
                        e = e + lr_sq3(v3_sub(ap, v3_make(albedo[q * 3], albedo[q * 3 + 1], albedo[q * 3 + 2]))) * ia;
                        const float w = h * rto_expf(-fminf(e, 80.0f));
                        sw = sw + w;
                        sx = sx + w * cq.x;
                        sy = sy + w * cq.y;
                        sz = sz + w * cq.z;
                    }
                }
                nxt[i * 4 + 0] = sx / sw; nxt[i * 4 + 1] = sy / sw; nxt[i * 4 + 2] = sz / sw;
                nxt[i * 4 + 3] = 1.0f;
            }
        float* t = cur; cur = nxt; nxt = t;
        lr_emit(cur, albedo, demodulate, n, out + (size_t)(k + 1) * n * 3);
    }
    free(cur);
    free(nxt);
    return RTPBR_OK;
}

/* image, half_a, half_b (W,H,4); fd, fa, fb (K + 1, W, H, 3): F_0 .. F_K of the three; m = (float)min_half_samples, z2 = z * z as
 * the host computes it.  weight, depth (W,H), out (W,H,3); stats = {pixels_estimated, pixels_above, bits of the largest 1 - T_K} */
LR_API int lr_blend_levels(const rtpbr_config* cfg, const float* image, const float* half_a, const float* half_b, const float* fd,
                           const float* fa, const float* fb, const int32_t* object, int K, int radius, float z2, float m,
                           float* weight, float* depth, float* out, uint32_t* stats) {
    if (radius < 1 || radius > 3 || K < 0) return -1;
    const int W = cfg->width, H = cfg->height;
    const size_t n = (size_t)W * H;
    float* aq = (float*)malloc(n * 3 * sizeof(float));
    float* run = (float*)malloc(n * 3 * sizeof(float));      /* the running linear colour */
    unsigned char* usable = (unsigned char*)malloc(n);
    if (!aq || !run || !usable) { free(aq); free(run); free(usable); return RTPBR_ENOMEM; }
    float *qq = aq + n, *xq = aq + 2 * n;
    for (size_t q = 0; q < n; q++) {
        usable[q] = half_a[q * 4 + 3] >= m && half_b[q * 4 + 3] >= m;
        weight[q] = 1.0f;      /* T_0 */
        depth[q] = 0.0f;
        for (int ch = 0; ch < 3; ch++) run[q * 3 + ch] = fd[q * 3 + ch];      /* c = FD_0 */
    }
    for (int k = 1; k <= K; k++) {
        const float *fdk = fd + (size_t)k * n * 3, *fak = fa + (size_t)k * n * 3, *fbk = fb + (size_t)k * n * 3;
        const float *fd0 = fdk - n * 3, *fa0 = fak - n * 3, *fb0 = fbk - n * 3;      /* the finer level */
        for (size_t q = 0; q < n; q++) {
            aq[q] = qq[q] = xq[q] = 0.0f;
            if (!usable[q]) continue;
            const float cA = half_a[q * 4 + 3], cB = half_b[q * 4 + 3];
            const float f = (cA * cB) / ((cA + cB) * (cA + cB));
            const float lA0 = lr_lum(fa0 + q * 3), lB0 = lr_lum(fb0 + q * 3), lD0 = lr_lum(fd0 + q * 3);
            const float dA = lr_lum(fak + q * 3) - lA0;
            const float dB = lr_lum(fbk + q * 3) - lB0;
            const float dp = lA0 - lB0;
            const float dd = dA - dB;
            const float dl = lr_lum(fdk + q * 3) - lD0;
            aq[q] = (f * dp) * dd;
            qq[q] = dl * dl;
            xq[q] = dA * dB;
        }
        for (int x = 0; x < W; x++)
            for (int y = 0; y < H; y++) {
                const size_t p = (size_t)x * H + y;
                float t = 1.0f;
                if (usable[p]) {
                    float cn = 0.0f, SC = 0.0f, SQ = 0.0f, SX = 0.0f, SXX = 0.0f;
                    for (int dy = -radius; dy <= radius; dy++) {
                        const int yq = y + dy;
                        if (yq < 0 || yq >= H) continue;
                        for (int dx = -radius; dx <= radius; dx++) {
                            const int xx = x + dx;
                            if (xx < 0 || xx >= W) continue;
                            const size_t q = (size_t)xx * H + yq;
                            if (object[q] != object[p] || !usable[q]) continue;
                            cn = cn + 1.0f;
                            SC = SC + aq[q];
                            SQ = SQ + qq[q];
                            SX = SX + xq[q];
                            SXX = SXX + xq[q] * xq[q];
                        }
                    }
                    const float m1 = SX / cn;
                    const float v = fmaxf(SXX / cn - m1 * m1, 0.0f);
                    if (m1 > 0.0f && (m1 * m1) * cn > z2 * v) {
                        t = -SC / SQ;
                        if (!(t < 1.0f)) t = 1.0f;
                        if (t < 0.0f) t = 0.0f;
                    }
                }
                const float T = weight[p] * t;
                weight[p] = T;
                depth[p] = depth[p] + T;
                for (int ch = 0; ch < 3; ch++) run[p * 3 + ch] = run[p * 3 + ch] + T * (fdk[p * 3 + ch] - fd0[p * 3 + ch]);
            }
    }
    uint32_t est = 0, above = 0, mx = 0;
    const float* fdK = fd + (size_t)K * n * 3;
    for (size_t p = 0; p < n; p++) {
        const float* b = image + p * 4;
        const float T = weight[p];
        if (usable[p]) {
            const float one_minus = 1.0f - T;
            uint32_t bits;
            memcpy(&bits, &one_minus, 4);
            est++;
            if (T < 1.0f) above++;
            if (bits > mx) mx = bits;
        }
        v3 d;
        if (b[3] > 0.0f) {
            const float* c3 = T == 1.0f ? fdK + p * 3 : run + p * 3;
            const float c[4] = {c3[0], c3[1], c3[2], 1.0f};
            d = tone_map(cfg, c);
        } else {      /* no samples: what post_process shows; weight 1, depth K */
            d = tone_map(cfg, b);
            weight[p] = 1.0f;
            depth[p] = (float)K;
        }
        out[p * 3 + 0] = d.x; out[p * 3 + 1] = d.y; out[p * 3 + 2] = d.z;
    }
    stats[0] = est;
    stats[1] = above;
    stats[2] = mx;
    free(aq);
    free(run);
    free(usable);
    return 0;
}
