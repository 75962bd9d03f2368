// rt_noise.hip — kernels of rtpbr_noise_update / rtpbr_noise_estimate / rtpbr_denoise_guided (see rt_noise.hpp).
#include <hip/hip_runtime.h>

#include "rt_noise.hpp"
#include "rt_device.hpp"

namespace rt {

RT_D vec3 nz_xyz(float4 v) { return mk(v.x, v.y, v.z); }
RT_D float nz_sq3(vec3 v) { return (v.x * v.x + v.y * v.y) + v.z * v.z; }      // |v|^2 in this order, no fma
RT_D vec3 nz_r(vec3 c) { return mk(c.x / (1.0f + c.x), c.y / (1.0f + c.y), c.z / (1.0f + c.z)); }
RT_D float nz_lum(vec3 c) { return (0.299f * c.x + 0.587f * c.y) + 0.114f * c.z; }
// compressed luminance of the mean of a texel (sum r, sum g, sum b, count), count > 0
RT_D float nz_lum_of_mean(float x, float y, float z, float cnt) { return nz_lum(nz_r(mk(x / cnt, y / cnt, z / cnt))); }

// One lane per pixel, i = x * H + y: all three buffers are read and written along the contiguous index.
__global__ void __launch_bounds__(256) noise_update(const NoiseArgs A) {
    const uint32_t n = (uint32_t)A.width * (uint32_t)A.height;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 b = A.image_buffer[i];
    const float4 s = A.snapshot[i];
    const float cnt = b.w - s.w;
    if (cnt > 0.0f) {
        const float L = nz_lum(mk((b.x - s.x) / cnt, (b.y - s.y) / cnt, (b.z - s.z) / cnt));      // linear: see rt_noise.hpp
        const float cL = cnt * L;
        float4 M = A.moments[i];
        M.x = M.x + cL;
        M.y = M.y + cL * L;
        M.z = M.z + cnt;
        M.w = M.w + 1.0f;
        A.moments[i] = M;
    }
    A.snapshot[i] = b;
}

// One lane per pixel.  Pixels with two batches or more take the temporal estimate (16 bytes of moments); the others walk their
// 7x7 neighbourhood: per tap the 4-byte object index, then — on the centre's object only — the 16-byte texel.
__global__ void __launch_bounds__(256) noise_estimate(const NoiseArgs A) {
    __shared__ uint32_t blk[3];
    if (threadIdx.x < 3) blk[threadIdx.x] = 0u;
    __syncthreads();
    const int H = A.height, W = A.width;
    const uint32_t n = (uint32_t)W * (uint32_t)H;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool estimated = false;
    float noise = 0.0f;
    if (i < n) {
        const float4 b = A.image_buffer[i];
        float v = 0.0f;
        if (b.w > 0.0f) {
            estimated = true;
            const float4 M = A.moments[i];
            if (M.w >= 2.0f) {
                // the variance of the mean linear luminance, carried through r by its two sigma points
                const float mu = M.x / M.z;
                const float sd = sqrt_ieee_(fmax_((M.y - (M.x * M.x) / M.z) / ((M.w - 1.0f) * M.z), 0.0f));
                const float hi = mu + sd, lo = fmax_(mu - sd, 0.0f);
                const float hw = 0.5f * (hi / (1.0f + hi) - lo / (1.0f + lo));
                v = fmax_(hw * hw, 0.0f);
            } else {
                const int x = (int)(i / (uint32_t)H), y = (int)(i - (uint32_t)x * (uint32_t)H);
                const int op = A.object[i];
                float cn = 0.0f, s1 = 0.0f, s2 = 0.0f;
                for (int dy = -3; dy <= 3; dy++) {
                    const int yq = y + dy;
                    if (yq < 0 || yq >= H) continue;
                    for (int dx = -3; dx <= 3; dx++) {
                        const int xq = x + dx;
                        if (xq < 0 || xq >= W) continue;
                        const size_t q = (size_t)xq * (size_t)H + (size_t)yq;
                        if (A.object[q] != op) continue;
                        const float4 bq = A.image_buffer[q];
                        if (!(bq.w > 0.0f)) continue;
                        const float L = nz_lum_of_mean(bq.x, bq.y, bq.z, bq.w);
                        cn = cn + 1.0f;
                        s1 = s1 + L;
                        s2 = s2 + L * L;
                    }
                }
                if (cn >= 2.0f) v = fmax_((s2 - (s1 * s1) / cn) / (cn - 1.0f), 0.0f);
            }
            noise = sqrt_ieee_(v);
        }
        A.noise[i] = noise;
        A.var0[i] = estimated ? v : -1.0f;
    }
    // the statistics: per wave a ballot and a butterfly maximum, per block three LDS atomics per wave, then three global ones
    const bool above = estimated && noise > A.threshold;
    const unsigned long long m_est = __ballot(estimated), m_abv = __ballot(above);
    uint32_t mx = __float_as_uint(noise);       // >= +0: the bit patterns order like the values
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)mx, o, 64);
        mx = other > mx ? other : mx;
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&blk[0], (uint32_t)__popcll(m_est));
        atomicAdd(&blk[1], (uint32_t)__popcll(m_abv));
        atomicMax(&blk[2], mx);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        NoiseStats* s = A.stats + (blockIdx.x % NOISE_SHARDS);
        if (blk[0]) atomicAdd(&s->estimated, blk[0]);
        if (blk[1]) atomicAdd(&s->above, blk[1]);
        if (blk[2]) atomicMax(&s->max_bits, blk[2]);
    }
}

// ---- the pooled estimate (rtpbr_set_noise_estimator with pool_batches > 0): noise_estimate with the young temporal pixels
// (2 <= M.w < pool_batches) taking max(own, pooled), pooled from the within-pixel sums of squares of the neighbours on the
// pixel's object.  A block owns a tile of POOL_TX x POOL_TY pixels (x by y, y contiguous; thread t: ly = t % POOL_TY, so a wave
// runs along y) and stages (ss_q, df_q, object_q) of the tile and an R-pixel halo into LDS once: 12 bytes per entry in three
// planes of one pitch.  Entries that are ineligible or outside the frame hold ss = +0 and df = 0: adding +0 to a non-negative
// sum is the identity, so the tap loop has one fixed trip count per radius and only the object compare in it.
// Traffic per staged entry: 16 bytes of moments, the count word of the 16-byte texel, 4 bytes of object; entries per pixel:
// (TX + 2R)(TY + 2R) / (TX TY).  Tile shapes measured at 1080p: DESIGN.md section 6f.
#ifndef RT_NOISE_POOL_TX
#define RT_NOISE_POOL_TX 16
#endif
#ifndef RT_NOISE_POOL_TY
#define RT_NOISE_POOL_TY 16
#endif
constexpr int POOL_TX = RT_NOISE_POOL_TX, POOL_TY = RT_NOISE_POOL_TY;
static_assert(POOL_TX * POOL_TY == 256 && (POOL_TY == 16 || POOL_TY == 32 || POOL_TY == 64), "a block of 256 lanes; a wave covers whole runs along y");
// the planes' pitch in words: the 64 / POOL_TY column runs a wave reads at once start 64 / (64 / POOL_TY) banks apart (of 64)
constexpr int pool_pitch(int hy) {
    if (POOL_TY == 64) return hy;
    int p = hy;
    while (p % 64 != POOL_TY && p % 64 != 64 - POOL_TY) p++;
    return p;
}

template <int R>
__global__ void __launch_bounds__(256) noise_estimate_pooled(const NoiseArgs A) {
    constexpr int HX = POOL_TX + 2 * R, HY = POOL_TY + 2 * R, PITCH = pool_pitch(HY);
    __shared__ float t_ss[HX * PITCH];
    __shared__ float t_df[HX * PITCH];
    __shared__ int t_obj[HX * PITCH];
    __shared__ uint32_t blk[3];
    if (threadIdx.x < 3) blk[threadIdx.x] = 0u;
    const int H = A.height, W = A.width;
    const int x0 = (int)blockIdx.x * POOL_TX, y0 = (int)blockIdx.y * POOL_TY;
    const int lx = (int)threadIdx.x / POOL_TY, ly = (int)threadIdx.x % POOL_TY;
    const int x = x0 + lx, y = y0 + ly;
    const bool inside = x < W && y < H;
    const uint32_t i = (uint32_t)x * (uint32_t)H + (uint32_t)y;      // used only when inside
    float4 b = make_float4(0.0f, 0.0f, 0.0f, 0.0f), M = b;
    int op = 0;
    {   // the lane's own entry: its texel and moments are loaded once, for the staging and for the estimate
        float ss = 0.0f, df = 0.0f;
        if (inside) {
            b = A.image_buffer[i];
            op = A.object[i];
            if (b.w > 0.0f) {
                M = A.moments[i];
                if (M.w >= 2.0f) {
                    ss = fmax_(M.y - (M.x * M.x) / M.z, 0.0f);
                    df = M.w - 1.0f;
                }
            }
        }
        const int e = (lx + R) * PITCH + (ly + R);
        t_ss[e] = ss;
        t_df[e] = df;
        t_obj[e] = op;
    }
    // the halo: HX x HY entries less the tile, hy fastest (contiguous in memory)
    for (int e = (int)threadIdx.x; e < HX * HY; e += 256) {
        const int hx = e / HY, hy = e - hx * HY;
        if (hx >= R && hx < R + POOL_TX && hy >= R && hy < R + POOL_TY) continue;
        const int xq = x0 - R + hx, yq = y0 - R + hy;
        float ss = 0.0f, df = 0.0f;
        int oq = 0;
        if (xq >= 0 && xq < W && yq >= 0 && yq < H) {
            const size_t q = (size_t)xq * (size_t)H + (size_t)yq;
            oq = A.object[q];
            if (A.image_buffer[q].w > 0.0f) {
                const float4 Mq = A.moments[q];
                if (Mq.w >= 2.0f) {
                    ss = fmax_(Mq.y - (Mq.x * Mq.x) / Mq.z, 0.0f);
                    df = Mq.w - 1.0f;
                }
            }
        }
        t_ss[hx * PITCH + hy] = ss;
        t_df[hx * PITCH + hy] = df;
        t_obj[hx * PITCH + hy] = oq;
    }
    __syncthreads();
    bool estimated = false;
    float noise = 0.0f;
    if (inside) {
        float v = 0.0f;
        if (b.w > 0.0f) {
            estimated = true;
            if (M.w >= 2.0f) {
                float var = fmax_((M.y - (M.x * M.x) / M.z) / ((M.w - 1.0f) * M.z), 0.0f);
                if (M.w < (float)A.pool_batches) {
                    float SS = 0.0f, DF = 0.0f;
#pragma unroll
                    for (int dy = -R; dy <= R; dy++) {
#pragma unroll
                        for (int dx = -R; dx <= R; dx++) {
                            const int e = (lx + R + dx) * PITCH + (ly + R + dy);
                            const bool same = t_obj[e] == op;
                            SS = SS + (same ? t_ss[e] : 0.0f);
                            DF = DF + (same ? t_df[e] : 0.0f);
                        }
                    }
                    var = fmax_(var, SS / (DF * M.z));
                }
                const float mu = M.x / M.z;
                const float sd = sqrt_ieee_(var);
                const float hi = mu + sd, lo = fmax_(mu - sd, 0.0f);
                const float hw = 0.5f * (hi / (1.0f + hi) - lo / (1.0f + lo));
                v = fmax_(hw * hw, 0.0f);
            } else {      // as noise_estimate
                float cn = 0.0f, s1 = 0.0f, s2 = 0.0f;
                for (int dy = -3; dy <= 3; dy++) {
                    const int yq = y + dy;
                    if (yq < 0 || yq >= H) continue;
                    for (int dx = -3; dx <= 3; dx++) {
                        const int xq = x + dx;
                        if (xq < 0 || xq >= W) continue;
                        const size_t q = (size_t)xq * (size_t)H + (size_t)yq;
                        if (A.object[q] != op) continue;
                        const float4 bq = A.image_buffer[q];
                        if (!(bq.w > 0.0f)) continue;
                        const float L = nz_lum_of_mean(bq.x, bq.y, bq.z, bq.w);
                        cn = cn + 1.0f;
                        s1 = s1 + L;
                        s2 = s2 + L * L;
                    }
                }
                if (cn >= 2.0f) v = fmax_((s2 - (s1 * s1) / cn) / (cn - 1.0f), 0.0f);
            }
            noise = sqrt_ieee_(v);
        }
        A.noise[i] = noise;
        A.var0[i] = estimated ? v : -1.0f;
    }
    // the statistics, as noise_estimate
    const bool above = estimated && noise > A.threshold;
    const unsigned long long m_est = __ballot(estimated), m_abv = __ballot(above);
    uint32_t mx = __float_as_uint(noise);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)mx, o, 64);
        mx = other > mx ? other : mx;
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&blk[0], (uint32_t)__popcll(m_est));
        atomicAdd(&blk[1], (uint32_t)__popcll(m_abv));
        atomicMax(&blk[2], mx);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        NoiseStats* s = A.stats + ((blockIdx.y * gridDim.x + blockIdx.x) % NOISE_SHARDS);
        if (blk[0]) atomicAdd(&s->estimated, blk[0]);
        if (blk[1]) atomicAdd(&s->above, blk[1]);
        if (blk[2]) atomicMax(&s->max_bits, blk[2]);
    }
}

RT_D vec3 g_albedo_clamped(const GuidedArgs& A, uint32_t i) {
    return mk(fmax_(A.albedo[(size_t)i * 3 + 0], 1e-3f), fmax_(A.albedo[(size_t)i * 3 + 1], 1e-3f), fmax_(A.albedo[(size_t)i * 3 + 2], 1e-3f));
}
RT_D vec3 g_start_colour(float4 b, vec3 ac, int demod) {
    vec3 c = mk(b.x / b.w, b.y / b.w, b.z / b.w);
    return demod ? mk(c.x / ac.x, c.y / ac.y, c.z / ac.z) : c;
}
constexpr int G_NO_SAMPLES = -2;      // as atrous_level's NO_SAMPLES

// One guided level: atrous_level's structure (rt_features.hip) with the variance beside it.  Tap loads: the object word (4 bytes
// at level 0, inside the 16-byte colour record later), then on the centre's object the texel (level 0), the (normal, depth)
// record and the 4-byte variance: 40 bytes per tap at level 0, 36 later (atrous_level: 36 / 32).  The 3x3 prefilter adds nine
// taps of object word + variance (8 bytes each).
template <bool FIRST, bool LAST>
__global__ void __launch_bounds__(256) guided_level(const GuidedArgs A) {
    const int H = A.height, W = A.width;
    const uint32_t n = (uint32_t)W * (uint32_t)H;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int x = (int)(i / (uint32_t)H), y = (int)(i - (uint32_t)x * (uint32_t)H);
    int op;
    float4 cp4;
    bool valid;
    if constexpr (FIRST) {
        cp4 = A.image_buffer[i];
        op = A.object[i];
        valid = cp4.w > 0.0f;
    } else {
        cp4 = A.src[i];
        op = __float_as_int(cp4.w);
        valid = op != G_NO_SAMPLES;
    }
    if (!valid) {
        if constexpr (LAST) {
            const vec3 t = tone_map(A.cfg, A.image_buffer[i]);
            A.out[(size_t)i * 3 + 0] = t.x;
            A.out[(size_t)i * 3 + 1] = t.y;
            A.out[(size_t)i * 3 + 2] = t.z;
        } else {
            A.dst[i] = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(G_NO_SAMPLES));
            A.vdst[i] = 0.0f;
        }
        return;
    }
    // g: the 3x3 Gaussian of the level's variance over the neighbours with samples on the centre's object (stride 1)
    float gs = 0.0f, gk = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; dy++) {
        const int yq = y + dy;
        if (yq < 0 || yq >= H) continue;
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
            const int xq = x + dx;
            if (xq < 0 || xq >= W) continue;
            const size_t q = (size_t)xq * (size_t)H + (size_t)yq;
            float vq;
            if constexpr (FIRST) {
                if (A.object[q] != op) continue;
                vq = A.var0[q];
                if (!(vq >= 0.0f)) continue;
            } else {
                if (__float_as_int(A.src[q].w) != op) continue;
                vq = A.vsrc[q];
            }
            const float k = (dx == 0 ? 2.0f : 1.0f) * (dy == 0 ? 2.0f : 1.0f);
            gs = gs + k * vq;
            gk = gk + k;
        }
    }
    const float icp = 1.0f / (A.sc2 * fmax_(gs / gk, A.floor));
    const bool need_albedo = (FIRST || LAST) && A.demodulate;
    const vec3 ac = need_albedo ? g_albedo_clamped(A, i) : mk(1.0f, 1.0f, 1.0f);
    const vec3 cp = FIRST ? g_start_colour(cp4, ac, A.demodulate) : nz_xyz(cp4);
    const float4 gp_nz = A.guide_nz[i];
    const vec3 np = nz_xyz(gp_nz);
    const float zp = gp_nz.w;
    const float izp = fmax_(zp, 1e-6f);
    const vec3 rp = nz_r(cp);
    const int s = A.step;
    float sw = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f, sv = 0.0f;
    constexpr float HK[3] = {0.375f, 0.25f, 0.0625f};
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const int yq = y + s * dy;
        if (yq < 0 || yq >= H) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int xq = x + s * dx;
            if (xq < 0 || xq >= W) continue;
            const size_t q = (size_t)xq * (size_t)H + (size_t)yq;
            vec3 cq;
            float vq;
            if constexpr (FIRST) {
                if (A.object[q] != op) continue;
                const float4 b = A.image_buffer[q];
                if (!(b.w > 0.0f)) continue;
                cq = g_start_colour(b, ac, A.demodulate);
                vq = A.var0[q];
            } else {
                const float4 c4 = A.src[q];
                if (__float_as_int(c4.w) != op) continue;
                cq = nz_xyz(c4);
                vq = A.vsrc[q];
            }
            const float4 gq_nz = A.guide_nz[q];
            const float h = HK[dx < 0 ? -dx : dx] * HK[dy < 0 ? -dy : dy];
            const float dz = (zp - gq_nz.w) / izp;
            float e = nz_sq3(rp - nz_r(cq)) * icp;
            e = e + nz_sq3(np - nz_xyz(gq_nz)) * A.in;
            e = e + (dz * dz) * A.iz;
            const float w = h * exp_(-fmin_(e, 80.0f));
            sw = sw + w;
            sx = sx + w * cq.x;
            sy = sy + w * cq.y;
            sz = sz + w * cq.z;
            sv = sv + (w * w) * vq;
        }
    }
    vec3 c = mk(sx / sw, sy / sw, sz / sw);
    if constexpr (LAST) {
        if (A.demodulate) c = mk(c.x * ac.x, c.y * ac.y, c.z * ac.z);
        const vec3 t = tone_map(A.cfg, make_float4(c.x, c.y, c.z, 1.0f));
        A.out[(size_t)i * 3 + 0] = t.x;
        A.out[(size_t)i * 3 + 1] = t.y;
        A.out[(size_t)i * 3 + 2] = t.z;
    } else {
        A.dst[i] = make_float4(c.x, c.y, c.z, __int_as_float(op));
        A.vdst[i] = sv / (sw * sw);
    }
}

static unsigned grid_of(int w, int h) { return (unsigned)(((size_t)w * h + 255) / 256); }

void launch_noise_update(const NoiseArgs& A, hipStream_t st) {
    hipLaunchKernelGGL(noise_update, dim3(grid_of(A.width, A.height)), dim3(256), 0, st, A);
}

void launch_noise_estimate(const NoiseArgs& A, hipStream_t st) {
    if (A.pool_batches > 0) {      // (rt_capi.hip admits radius 1..3 only)
        const dim3 grid((unsigned)((A.width + POOL_TX - 1) / POOL_TX), (unsigned)((A.height + POOL_TY - 1) / POOL_TY));
        if (A.pool_radius == 1) hipLaunchKernelGGL(noise_estimate_pooled<1>, grid, dim3(256), 0, st, A);
        else if (A.pool_radius == 2) hipLaunchKernelGGL(noise_estimate_pooled<2>, grid, dim3(256), 0, st, A);
        else hipLaunchKernelGGL(noise_estimate_pooled<3>, grid, dim3(256), 0, st, A);
        return;
    }
    hipLaunchKernelGGL(noise_estimate, dim3(grid_of(A.width, A.height)), dim3(256), 0, st, A);
}

void launch_guided_level(const GuidedArgs& A, bool first, bool last, hipStream_t st) {
    const unsigned grid = grid_of(A.width, A.height);
    if (first && last) hipLaunchKernelGGL((guided_level<true, true>), dim3(grid), dim3(256), 0, st, A);
    else if (first) hipLaunchKernelGGL((guided_level<true, false>), dim3(grid), dim3(256), 0, st, A);
    else if (last) hipLaunchKernelGGL((guided_level<false, true>), dim3(grid), dim3(256), 0, st, A);
    else hipLaunchKernelGGL((guided_level<false, false>), dim3(grid), dim3(256), 0, st, A);
}

}  // namespace rt
