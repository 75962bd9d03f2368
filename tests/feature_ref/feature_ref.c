/*
 * feature_ref.c — CPU reference of rtpbr_render_features / rtpbr_denoise (TEST INFRASTRUCTURE ONLY).
 *
 * Reuses the oracle's own camera frame, raycasts, normals and math by including its source; the oracle itself is not
 * changed.  Built on demand by the tests (tests/feature_ref_build.py) with the oracle's flags plus -fvisibility=hidden
 * -Wl,-Bsymbolic: this library carries its own copy of every rto_* symbol and of the bunny weights, which must not
 * interpose with librt_oracle.so, loaded RTLD_GLOBAL in the same process.  Only the fr_* functions are exported.
 *
 * The arithmetic follows include/rtpbr.h (rtpbr_denoise) operation by operation; the HIP kernels are in
 * raytracingpbr_amd/csrc/rt_features.hip.
 */
#include "../../oracle/rt_oracle.c"

#define FR_API __attribute__((visibility("default")))

/* Features of the first hit through every pixel centre.  The scene / configuration / camera / bunny weights (625 floats
 * or NULL) are set on a context of this library's own oracle copy. */
FR_API int fr_features(const rtpbr_config* cfg, const rtpbr_object* objs, int n, int scale10, const rtpbr_camera* cam,
                       const float* bunny_weights, float* albedo, float* normal, float* depth, int32_t* object) {
    struct rto_ctx* c;
    int r = rto_create(0, &c);
    if (r) return r;
    if ((r = rto_set_config(c, cfg)) || (r = rto_set_scene(c, objs, n, scale10)) || (r = rto_set_camera(c, cam))) {
        rto_destroy(c);
        return r;
    }
    if (bunny_weights) rto_set_bunny_weights(bunny_weights, 625);
    const int W = cfg->width, H = cfg->height;
    cam_frame f;
    camera_frame(c, &f);
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic, 1)
#endif
    for (int x = 0; x < W; x++) {
        rtpbr_counters ctr;
        memset(&ctr, 0, sizeof ctr);
        for (int y = 0; y < H; y++) {
            float u, v;
            if (cfg->camera_kind == RTPBR_CAMERA_PINHOLE) {
                u = ((float)x + 0.5f) / (float)W;
                v = ((float)y + 0.5f) / (float)H;
            } else {
                u = ((float)x + 0.5f) * (1.0f / (float)W);
                v = ((float)y + 0.5f) * (1.0f / (float)H);
            }
            ray_t ray;
            ray.origin = f.lookfrom;
            v3 po = v3_fma(v, f.vertical, v3_fma(u, f.horizontal, f.llc));
            ray.direction = v3_normalize(v3_sub(po, ray.origin));
            ray.color = v3_make(1, 1, 1);
            ray.depth = 0;
            v3 pos;
            int hit, idx;
            if (cfg->march_kind == RTPBR_MARCH_SRC) {
                ray_t m = ray;
                idx = raycast_src(c, &m, &hit, &ctr);
                pos = m.origin;
            } else if (cfg->march_kind == RTPBR_MARCH_PLAIN) {
                idx = raycast_plain(c, &ray, &pos, &hit, &ctr);
            } else {
                idx = raycast_relaxed(c, &ray, &pos, &hit, &ctr);
            }
            const size_t i = (size_t)x * H + y;
            if (hit) {
                const rtpbr_object* o = &c->obj[idx];
                v3 nn = calc_normal(c, o, pos);
                albedo[i * 3 + 0] = o->material.albedo[0];
                albedo[i * 3 + 1] = o->material.albedo[1];
                albedo[i * 3 + 2] = o->material.albedo[2];
                normal[i * 3 + 0] = nn.x;
                normal[i * 3 + 1] = nn.y;
                normal[i * 3 + 2] = nn.z;
                depth[i] = v3_length(v3_sub(pos, f.lookfrom));
                object[i] = idx;
            } else {
                albedo[i * 3 + 0] = albedo[i * 3 + 1] = albedo[i * 3 + 2] = 0.0f;
                normal[i * 3 + 0] = normal[i * 3 + 1] = normal[i * 3 + 2] = 0.0f;
                depth[i] = cfg->max_dis;
                object[i] = -1;
            }
        }
    }
    rto_destroy(c);
    return RTPBR_OK;
}

static inline float sq3(v3 v) { return (v.x * v.x + v.y * v.y) + v.z * v.z; }
static inline v3 tonemap_r(v3 c) { return v3_make(c.x / (1.0f + c.x), c.y / (1.0f + c.y), c.z / (1.0f + c.z)); }
static inline v3 demod_div(v3 c, const float* a) {
    return v3_make(c.x / fmaxf(a[0], 1e-3f), c.y / fmaxf(a[1], 1e-3f), c.z / fmaxf(a[2], 1e-3f));
}
static inline v3 remod(v3 c, const float* a) {
    return v3_make(c.x * fmaxf(a[0], 1e-3f), c.y * fmaxf(a[1], 1e-3f), c.z * fmaxf(a[2], 1e-3f));
}

/* The denoised display image (W,H,3) from image_buffer (W,H,4) and the features. */
FR_API int fr_denoise(const rtpbr_config* cfg, const float* image_buffer, const float* albedo, const float* normal, const float* depth,
                      const int32_t* object, int iterations, int demodulate, float sigma_color, float sigma_normal, float sigma_depth,
                      float sigma_albedo, float* out) {
    const int W = cfg->width, H = cfg->height;
    const size_t n = (size_t)W * H;
    float* cur = (float*)malloc(n * 4 * sizeof(float));      /* (colour, 1 = has samples) */
    float* nxt = (float*)malloc(n * 4 * sizeof(float));
    if (!cur || !nxt) { free(cur); free(nxt); return RTPBR_ENOMEM; }
    for (size_t i = 0; i < n; i++) {
        const float* b = image_buffer + i * 4;
        v3 c = v3_make(b[0] / b[3], b[1] / b[3], b[2] / b[3]);
        if (demodulate) c = demod_div(c, albedo + i * 3);
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
                const v3 rp = tonemap_r(cp);
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
                        float e = sq3(v3_sub(rp, tonemap_r(cq))) * ic;
                        e = e + sq3(v3_sub(np, v3_make(normal[q * 3], normal[q * 3 + 1], normal[q * 3 + 2]))) * in;
                        e = e + (dz * dz) * iz;
                        e = e + sq3(v3_sub(ap, v3_make(albedo[q * 3], albedo[q * 3 + 1], albedo[q * 3 + 2]))) * ia;
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
        v3 t;
        if (cur[i * 4 + 3] != 0.0f) {
            v3 c = v3_make(cur[i * 4], cur[i * 4 + 1], cur[i * 4 + 2]);
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
