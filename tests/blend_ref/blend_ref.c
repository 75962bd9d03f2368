/*
 * blend_ref.c — CPU restatement of rtpbr_denoise_blend (TEST INFRASTRUCTURE ONLY).
 *
 * Built on demand by tests/blend_ref_lib.py the way tests/feature_ref_lib.py builds the feature reference: the oracle's source is
 * included for its tone map and exp (hidden visibility, -Bsymbolic: only br_* is exported).  br_filter restates rtpbr_denoise's
 * filter with the switch the blend needs — linear = 1 stops before the tone map —; with linear = 0 it is fr_denoise
 * (tests/feature_ref/feature_ref.c), and tests/test_blend_ref.py holds the two equal.  The subtract pass goes through
 * tests/half_ref_lib.py.  The arithmetic follows include/rtpbr.h operation by operation; the HIP kernels are half_blend<R>
 * (raytracingpbr_amd/csrc/rt_half.hip) and the LINEAR form of atrous_level / atrous_none (rt_features.hip).
 */
#include "../../oracle/rt_oracle.c"

#define BR_API __attribute__((visibility("default")))

static inline float br_sq3(v3 v) { return (v.x * v.x + v.y * v.y) + v.z * v.z; }
static inline v3 br_r(v3 c) { return v3_make(c.x / (1.0f + c.x), c.y / (1.0f + c.y), c.z / (1.0f + c.z)); }
static inline float br_lum(const float* c) { return (0.299f * c[0] + 0.587f * c[1]) + 0.114f * c[2]; }

/* out (W,H,3): linear = 0 the denoised display colour, linear = 1 the linear colour after remodulation (+0 without samples) */
BR_API int br_filter(const rtpbr_config* cfg, const float* image_buffer, const float* albedo, const float* normal, const float* depth,
                     const int32_t* object, int iterations, int demodulate, float sigma_color, float sigma_normal, float sigma_depth,
                     float sigma_albedo, int linear, float* out) {
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
                const v3 rp = br_r(cp);
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
                        float e = br_sq3(v3_sub(rp, br_r(cq))) * ic;
                        e = e + br_sq3(v3_sub(np, v3_make(normal[q * 3], normal[q * 3 + 1], normal[q * 3 + 2]))) * in;
                        e = e + (dz * dz) * iz;
                        e = e + br_sq3(v3_sub(ap, v3_make(albedo[q * 3], albedo[q * 3 + 1], albedo[q * 3 + 2]))) * ia;
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
    }
    for (size_t i = 0; i < n; i++) {
        v3 t = v3_make(0.0f, 0.0f, 0.0f);
        if (cur[i * 4 + 3] != 0.0f) {
            const float* a = albedo + i * 3;
            v3 c = v3_make(cur[i * 4], cur[i * 4 + 1], cur[i * 4 + 2]);
            if (demodulate) c = v3_make(c.x * fmaxf(a[0], 1e-3f), c.y * fmaxf(a[1], 1e-3f), c.z * fmaxf(a[2], 1e-3f));
            if (linear) {
                t = c;
            } else {
                const float b[4] = {c.x, c.y, c.z, 1.0f};
                t = tone_map(cfg, b);
            }
        } else if (!linear) {
            t = tone_map(cfg, image_buffer + i * 4);      /* no samples: what post_process shows */
        }
        out[i * 3 + 0] = t.x; out[i * 3 + 1] = t.y; out[i * 3 + 2] = t.z;
    }
    free(cur);
    free(nxt);
    return RTPBR_OK;
}

/* image, half_a, half_b (W,H,4); fd, fa, fb (W,H,3): the linear filter results of the three; m = (float)min_half_samples,
 * z2 = z * z as the host computes it.  weight (W,H), out (W,H,3); stats = {pixels_estimated, pixels_above, bits of the largest 1 - t} */
BR_API int br_blend(const rtpbr_config* cfg, const float* image, const float* half_a, const float* half_b, const float* fd,
                    const float* fa, const float* fb, const int32_t* object, int radius, float z2, float m, float* weight, float* out,
                    uint32_t* stats) {
    if (radius < 1 || radius > 3) return -1;
    const int W = cfg->width, H = cfg->height;
    const size_t n = (size_t)W * H;
    float* aq = (float*)malloc(n * 3 * sizeof(float));
    unsigned char* usable = (unsigned char*)malloc(n);
    if (!aq || !usable) { free(aq); free(usable); return RTPBR_ENOMEM; }
    float *qq = aq + n, *xq = aq + 2 * n;
    for (size_t q = 0; q < n; q++) {
        const float *b = image + q * 4, *A = half_a + q * 4, *B = half_b + q * 4;
        const float cA = A[3], cB = B[3];
        usable[q] = cA >= m && cB >= m;
        aq[q] = qq[q] = xq[q] = 0.0f;
        if (!usable[q]) continue;
        const float f = (cA * cB) / ((cA + cB) * (cA + cB));
        const float PA[3] = {A[0] / A[3], A[1] / A[3], A[2] / A[3]};
        const float PB[3] = {B[0] / B[3], B[1] / B[3], B[2] / B[3]};
        const float Pb[3] = {b[0] / b[3], b[1] / b[3], b[2] / b[3]};
        const float lPA = br_lum(PA), lPB = br_lum(PB), lPb = br_lum(Pb);
        const float dA = br_lum(fa + q * 3) - lPA;
        const float dB = br_lum(fb + q * 3) - lPB;
        const float dp = lPA - lPB;
        const float dd = dA - dB;
        const float dl = br_lum(fd + q * 3) - lPb;
        aq[q] = (f * dp) * dd;
        qq[q] = dl * dl;
        xq[q] = dA * dB;
    }
    uint32_t est = 0, above = 0, mx = 0;
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
                const float one_minus = 1.0f - t;
                uint32_t bits;
                memcpy(&bits, &one_minus, 4);
                est++;
                if (t < 1.0f) above++;
                if (bits > mx) mx = bits;
            }
            weight[p] = t;
            const float* b = image + p * 4;
            v3 d;
            if (b[3] > 0.0f) {
                float c[4] = {fd[p * 3], fd[p * 3 + 1], fd[p * 3 + 2], 1.0f};
                if (t != 1.0f) {
                    const float u = 1.0f - t;
                    for (int k = 0; k < 3; k++) c[k] = c[k] + u * (b[k] / b[3] - c[k]);
                }
                d = tone_map(cfg, c);
            } else {
                d = tone_map(cfg, b);
            }
            out[p * 3 + 0] = d.x; out[p * 3 + 1] = d.y; out[p * 3 + 2] = d.z;
        }
    stats[0] = est;
    stats[1] = above;
    stats[2] = mx;
    free(aq);
    free(usable);
    return 0;
}
