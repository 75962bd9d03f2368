/*
 * noise_ref.c — CPU restatement of rtpbr_noise_update / rtpbr_noise_estimate / rtpbr_denoise_guided and of the moment warp of
 * rtpbr_reproject (TEST INFRASTRUCTURE ONLY).
 *
 * Reuses the oracle's tone map, camera frame and math by including its source, as tests/feature_ref/feature_ref.c does, and is
 * built the same way (tests/noise_ref_lib.py: the oracle's flags, -ffp-contract=off, hidden visibility, -Bsymbolic): only nr_*
 * is exported.  The arithmetic follows include/rtpbr.h operation by operation; the HIP kernels are in
 * raytracingpbr_amd/csrc/rt_noise.hip and rt_reproject.hip.
 */
#include "../../oracle/rt_oracle.c"

#define NR_API __attribute__((visibility("default")))

static inline float sq3(v3 v) { return (v.x * v.x + v.y * v.y) + v.z * v.z; }
static inline v3 tonemap_r(v3 c) { return v3_make(c.x / (1.0f + c.x), c.y / (1.0f + c.y), c.z / (1.0f + c.z)); }
static inline float lum(v3 c) { return (0.299f * c.x + 0.587f * c.y) + 0.114f * c.z; }
static inline float lum_of_mean(float x, float y, float z, float cnt) { return lum(tonemap_r(v3_make(x / cnt, y / cnt, z / cnt))); }

/* image (W,H,4); snapshot and moments (W,H,4) are updated in place */
NR_API int nr_update(int W, int H, const float* image, float* snapshot, float* moments) {
    const size_t n = (size_t)W * H;
    for (size_t i = 0; i < n; i++) {
        const float* b = image + i * 4;
        float* s = snapshot + i * 4;
        float* M = moments + i * 4;
        const float cnt = b[3] - s[3];
        if (cnt > 0.0f) {
            const float L = lum(v3_make((b[0] - s[0]) / cnt, (b[1] - s[1]) / cnt, (b[2] - s[2]) / cnt));
            const float cL = cnt * L;
            M[0] = M[0] + cL;
            M[1] = M[1] + cL * L;
            M[2] = M[2] + cnt;
            M[3] = M[3] + 1.0f;
        }
        for (int k = 0; k < 4; k++) s[k] = b[k];
    }
    return RTPBR_OK;
}

/* noise (W,H) = sqrt(v); var0 (W,H) = v, -1 for a pixel without samples; stats = {pixels_estimated, pixels_above, bits of max_noise} */
NR_API int nr_estimate(int W, int H, const float* image, const float* moments, const int32_t* object, float threshold, float* noise,
                       float* var0, uint32_t* stats) {
    uint32_t est = 0, above = 0, mx = 0;
    for (int x = 0; x < W; x++)
        for (int y = 0; y < H; y++) {
            const size_t i = (size_t)x * H + y;
            const float* b = image + i * 4;
            const float* M = moments + i * 4;
            if (!(b[3] > 0.0f)) {
                noise[i] = 0.0f;
                var0[i] = -1.0f;
                continue;
            }
            float v = 0.0f;
            if (M[3] >= 2.0f) {
                const float mu = M[0] / M[2];
                const float sd = sqrtf(fmaxf((M[1] - (M[0] * M[0]) / M[2]) / ((M[3] - 1.0f) * M[2]), 0.0f));
                const float hi = mu + sd, lo = fmaxf(mu - sd, 0.0f);
                const float hw = 0.5f * (hi / (1.0f + hi) - lo / (1.0f + lo));
                v = fmaxf(hw * hw, 0.0f);
            } else {
                float cn = 0.0f, s1 = 0.0f, s2 = 0.0f;
                for (int dy = -3; dy <= 3; dy++) {
                    const int yq = y + dy;
                    if (yq < 0 || yq >= H) continue;
                    for (int dx = -3; dx <= 3; dx++) {
                        const int xq = x + dx;
                        if (xq < 0 || xq >= W) continue;
                        const size_t q = (size_t)xq * H + yq;
                        if (object[q] != object[i]) continue;
                        const float* bq = image + q * 4;
                        if (!(bq[3] > 0.0f)) continue;
                        const float L = lum_of_mean(bq[0], bq[1], bq[2], bq[3]);
                        cn = cn + 1.0f;
                        s1 = s1 + L;
                        s2 = s2 + L * L;
                    }
                }
                if (cn >= 2.0f) v = fmaxf((s2 - (s1 * s1) / cn) / (cn - 1.0f), 0.0f);
            }
            const float sd = sqrtf(v);
            noise[i] = sd;
            var0[i] = v;
            est++;
            if (sd > threshold) above++;
            uint32_t bits;
            memcpy(&bits, &sd, 4);
            if (bits > mx) mx = bits;
        }
    stats[0] = est;
    stats[1] = above;
    stats[2] = mx;
    return RTPBR_OK;
}

static inline v3 demod_div(v3 c, const float* a) {
    return v3_make(c.x / fmaxf(a[0], 1e-3f), c.y / fmaxf(a[1], 1e-3f), c.z / fmaxf(a[2], 1e-3f));
}
static inline v3 remod(v3 c, const float* a) {
    return v3_make(c.x * fmaxf(a[0], 1e-3f), c.y * fmaxf(a[1], 1e-3f), c.z * fmaxf(a[2], 1e-3f));
}

/* The guided display image (W,H,3) from image_buffer, the features and the level-0 variance var0 (as nr_estimate writes it). */
NR_API int nr_guided(const rtpbr_config* cfg, const float* image_buffer, const float* albedo, const float* normal, const float* depth,
                     const int32_t* object, const float* var0, int iterations, int demodulate, float sigma_color, float sigma_normal,
                     float sigma_depth, float variance_floor, float* out) {
    const int W = cfg->width, H = cfg->height;
    const size_t n = (size_t)W * H;
    float* cur = (float*)malloc(n * 5 * sizeof(float));      /* (colour, 1 = has samples, variance) */
    float* nxt = (float*)malloc(n * 5 * sizeof(float));
    if (!cur || !nxt) { free(cur); free(nxt); return RTPBR_ENOMEM; }
    for (size_t i = 0; i < n; i++) {
        const float* b = image_buffer + i * 4;
        v3 c = v3_make(b[0] / b[3], b[1] / b[3], b[2] / b[3]);
        if (demodulate) c = demod_div(c, albedo + i * 3);
        cur[i * 5 + 0] = c.x; cur[i * 5 + 1] = c.y; cur[i * 5 + 2] = c.z;
        cur[i * 5 + 3] = b[3] > 0.0f ? 1.0f : 0.0f;
        cur[i * 5 + 4] = iterations > 0 ? var0[i] : 0.0f;
    }
    const float sc2 = sigma_color * sigma_color, in = 1.0f / (sigma_normal * sigma_normal), iz = 1.0f / (sigma_depth * sigma_depth);
    const float HK[3] = {0.375f, 0.25f, 0.0625f};
    for (int k = 0; k < iterations; k++) {
        const int s = 1 << k;
#ifdef _OPENMP
#pragma omp parallel for schedule(static)
#endif
        for (int x = 0; x < W; x++)
            for (int y = 0; y < H; y++) {
                const size_t i = (size_t)x * H + y;
                if (cur[i * 5 + 3] == 0.0f) {
                    memset(nxt + i * 5, 0, 5 * sizeof(float));
                    continue;
                }
                float gs = 0.0f, gk = 0.0f;
                for (int dy = -1; dy <= 1; dy++) {
                    const int yq = y + dy;
                    if (yq < 0 || yq >= H) continue;
                    for (int dx = -1; dx <= 1; dx++) {
                        const int xq = x + dx;
                        if (xq < 0 || xq >= W) continue;
                        const size_t q = (size_t)xq * H + yq;
                        if (object[q] != object[i] || cur[q * 5 + 3] == 0.0f) continue;
                        const float kk = (dx == 0 ? 2.0f : 1.0f) * (dy == 0 ? 2.0f : 1.0f);
                        gs = gs + kk * cur[q * 5 + 4];
                        gk = gk + kk;
                    }
                }
                const float icp = 1.0f / (sc2 * fmaxf(gs / gk, variance_floor));
                const v3 cp = v3_make(cur[i * 5], cur[i * 5 + 1], cur[i * 5 + 2]);
                const v3 rp = tonemap_r(cp);
                const v3 np = v3_make(normal[i * 3], normal[i * 3 + 1], normal[i * 3 + 2]);
                const float zp = depth[i], izp = fmaxf(zp, 1e-6f);
                float sw = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f, sv = 0.0f;
                for (int dy = -2; dy <= 2; dy++) {
                    const int yq = y + s * dy;
                    if (yq < 0 || yq >= H) continue;
                    for (int dx = -2; dx <= 2; dx++) {
                        const int xq = x + s * dx;
                        if (xq < 0 || xq >= W) continue;
                        const size_t q = (size_t)xq * H + yq;
                        if (object[q] != object[i] || cur[q * 5 + 3] == 0.0f) continue;
                        const v3 cq = v3_make(cur[q * 5], cur[q * 5 + 1], cur[q * 5 + 2]);
                        const float h = HK[dx < 0 ? -dx : dx] * HK[dy < 0 ? -dy : dy];
                        const float dz = (zp - depth[q]) / izp;
                        float e = sq3(v3_sub(rp, tonemap_r(cq))) * icp;
                        e = e + sq3(v3_sub(np, v3_make(normal[q * 3], normal[q * 3 + 1], normal[q * 3 + 2]))) * in;
                        e = e + (dz * dz) * iz;
                        const float w = h * rto_expf(-fminf(e, 80.0f));
                        sw = sw + w;
                        sx = sx + w * cq.x;
                        sy = sy + w * cq.y;
                        sz = sz + w * cq.z;
                        sv = sv + (w * w) * cur[q * 5 + 4];
                    }
                }
                nxt[i * 5 + 0] = sx / sw; nxt[i * 5 + 1] = sy / sw; nxt[i * 5 + 2] = sz / sw;
                nxt[i * 5 + 3] = 1.0f;
                nxt[i * 5 + 4] = sv / (sw * sw);
            }
        float* t = cur; cur = nxt; nxt = t;
    }
    for (size_t i = 0; i < n; i++) {
        v3 t;
        if (cur[i * 5 + 3] != 0.0f) {
            v3 c = v3_make(cur[i * 5], cur[i * 5 + 1], cur[i * 5 + 2]);
            if (demodulate) c = remod(c, albedo + i * 3);
            const float b[4] = {c.x, c.y, c.z, 1.0f};
            t = tone_map(cfg, b);
        } else {
            t = tone_map(cfg, image_buffer + i * 4);      /* no samples: what post_process shows */
        }
        out[i * 3 + 0] = t.x; out[i * 3 + 1] = t.y; out[i * 3 + 2] = t.z;
    }
    free(cur);
    free(nxt);
    return RTPBR_OK;
}

/* ---- the moment warp of rtpbr_reproject: the gather of tests/reproject_ref/reproject_ref.c with the moments riding along */
static int frame_of(const rtpbr_config* cfg, const rtpbr_camera* cam, cam_frame* f) {
    struct rto_ctx* c;
    int r = rto_create(0, &c);
    if (r) return r;
    if ((r = rto_set_config(c, cfg)) || (r = rto_set_camera(c, cam))) {
        rto_destroy(c);
        return r;
    }
    camera_frame(c, f);
    rto_destroy(c);
    return RTPBR_OK;
}

static void snap_axis(float p, int* x0, float* fx) {
    const float fl = floorf(p);
    *x0 = (int)fl;
    *fx = p - fl;
    if (*fx < 0.0009765625f) {
        *fx = 0.0f;
    } else if (*fx > 0.9990234375f) {
        *x0 = *x0 + 1;
        *fx = 0.0f;
    }
}

/* Writes image (W,H,4) and moments (W,H,4) of the new view. */
NR_API int nr_reproject(const rtpbr_config* cfg, const rtpbr_camera* old_cam, const rtpbr_camera* new_cam, const float* old_image,
                        const float* old_moments, const float* old_normal, const float* old_depth, const int32_t* old_object,
                        const float* new_normal, const float* new_depth, const int32_t* new_object, float max_history, float depth_tol,
                        float normal_cos, float* image, float* moments) {
    cam_frame f0, f1;
    int r;
    if ((r = frame_of(cfg, old_cam, &f0)) || (r = frame_of(cfg, new_cam, &f1))) return r;
    const int W = cfg->width, H = cfg->height;
    for (int x = 0; x < W; x++)
        for (int y = 0; y < H; y++) {
            const size_t i = (size_t)x * H + y;
            float u, v;
            if (cfg->camera_kind == RTPBR_CAMERA_PINHOLE) {
                u = ((float)x + 0.5f) / (float)W;
                v = ((float)y + 0.5f) / (float)H;
            } else {
                u = ((float)x + 0.5f) * (1.0f / (float)W);
                v = ((float)y + 0.5f) * (1.0f / (float)H);
            }
            const v3 d = v3_normalize(v3_sub(v3_fma(v, f1.vertical, v3_fma(u, f1.horizontal, f1.llc)), f1.lookfrom));
            const int obj = new_object[i];
            const int hit = obj >= 0;
            v3 D = d, nn = v3_make(0.0f, 0.0f, 0.0f);
            if (hit) {
                D = v3_sub(v3_fma(new_depth[i], d, f1.lookfrom), f0.lookfrom);
                nn = v3_make(new_normal[i * 3], new_normal[i * 3 + 1], new_normal[i * 3 + 2]);
            }
            const v3 q = v3_sub(f0.llc, f0.lookfrom);
            const v3 N = v3_cross(f0.horizontal, f0.vertical);
            const float s = v3_dot(q, N) / v3_dot(D, N);
            float S[4] = {0.0f, 0.0f, 0.0f, 0.0f}, SM[4] = {0.0f, 0.0f, 0.0f, 0.0f}, Wt = 0.0f;
            if (s > 0.0f) {
                const v3 P = v3_sub(v3_scale(D, s), q);
                const float u0 = v3_dot(P, f0.horizontal) / v3_dot(f0.horizontal, f0.horizontal);
                const float v0 = v3_dot(P, f0.vertical) / v3_dot(f0.vertical, f0.vertical);
                const float px = u0 * (float)W - 0.5f, py = v0 * (float)H - 0.5f;
                if (px > -1.0f && px < (float)W && py > -1.0f && py < (float)H) {
                    int x0, y0;
                    float fx, fy;
                    snap_axis(px, &x0, &fx);
                    snap_axis(py, &y0, &fy);
                    const float L = hit ? v3_length(D) : 0.0f;
                    const float tolL = depth_tol * L;
                    const float wx[2] = {1.0f - fx, fx}, wy[2] = {1.0f - fy, fy};
                    for (int tj = 0; tj < 2; tj++)
                        for (int ti = 0; ti < 2; ti++) {
                            const float w = wx[ti] * wy[tj];
                            const int xq = x0 + ti, yq = y0 + tj;
                            if (w == 0.0f || xq < 0 || xq >= W || yq < 0 || yq >= H) continue;
                            const size_t qi = (size_t)xq * H + yq;
                            if (old_object[qi] != obj) continue;
                            const float* b = old_image + qi * 4;
                            if (!(b[3] > 0.0f)) continue;
                            if (hit) {
                                if (!(fabsf(old_depth[qi] - L) <= tolL)) continue;
                                const v3 no = v3_make(old_normal[qi * 3], old_normal[qi * 3 + 1], old_normal[qi * 3 + 2]);
                                if (!(normal_cos <= -1.0f || v3_dot(no, nn) >= normal_cos)) continue;
                            }
                            for (int k = 0; k < 4; k++) S[k] = S[k] + w * b[k];
                            Wt = Wt + w;
                            for (int k = 0; k < 4; k++) SM[k] = SM[k] + w * old_moments[qi * 4 + k];
                        }
                }
            }
            float* o = image + i * 4;
            float* M = moments + i * 4;
            if (Wt > 0.0f) {
                for (int k = 0; k < 4; k++) o[k] = S[k] / Wt;
                for (int k = 0; k < 4; k++) M[k] = SM[k] / Wt;
                if (o[3] > max_history) {
                    const float kk = max_history / o[3];
                    for (int k = 0; k < 4; k++) o[k] = o[k] * kk;
                    for (int k = 0; k < 3; k++) M[k] = M[k] * kk;
                    M[3] = M[3] > 1.0f ? 1.0f + (M[3] - 1.0f) * kk : M[3];
                }
            } else {
                o[0] = o[1] = o[2] = o[3] = 0.0f;
                M[0] = M[1] = M[2] = M[3] = 0.0f;
            }
        }
    return RTPBR_OK;
}
