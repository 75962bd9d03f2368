// rt_noise.hip — kernels of rtpbr_noise_update / rtpbr_noise_estimate (see rt_noise.hpp).
#include <hip/hip_runtime.h>

#include "rt_noise.hpp"
#include "rt_features.hpp"
#include "rt_device.hpp"

namespace rt {

// compressed luminance of the mean of a texel (sum r, sum g, sum b, count), count > 0
RT_D float nz_lum_of_mean(float x, float y, float z, float cnt) { return nz_lum(tonemap_r(mk(x / cnt, y / cnt, z / cnt))); }

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

// ---- the pieces noise_estimate and noise_estimate_pooled<R> share
// the variance of the mean linear luminance from a pixel's moments (K = M.w >= 2)
RT_D float nz_var_of_mean(float4 M) { return fmax_((M.y - (M.x * M.x) / M.z) / ((M.w - 1.0f) * M.z), 0.0f); }

// (mu, var) of the mean linear luminance -> the variance of r(mean), carried through r by its two sigma points
RT_D float nz_sigma_points(float mu, float var) {
    const float sd = sqrt_ieee_(var);
    const float hi = mu + sd, lo = fmax_(mu - sd, 0.0f);
    const float hw = 0.5f * (hi / (1.0f + hi) - lo / (1.0f + lo));
    return fmax_(hw * hw, 0.0f);
}

// what a pixel's moments give to a pooled sum: the within-pixel sum of squares and its degrees of freedom; under two batches
// nothing (ss and df stay as they are: 0)
RT_D void nz_ss_df(float4 M, float& ss, float& df) {
    if (M.w >= 2.0f) {
        ss = fmax_(M.y - (M.x * M.x) / M.z, 0.0f);
        df = M.w - 1.0f;
    }
}

// the spatial fallback of a pixel under two batches: the variance of the compressed luminance over the 7x7 neighbourhood on the
// pixel's object.  Per tap the 4-byte object index, then — on the centre's object only — the 16-byte texel.
RT_D float nz_spatial(const NoiseArgs& A, int x, int y, int op) {
    const int H = A.height, W = A.width;
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
    return cn >= 2.0f ? fmax_((s2 - (s1 * s1) / cn) / (cn - 1.0f), 0.0f) : 0.0f;
}

// One lane per pixel.  Pixels with two batches or more take the temporal estimate (16 bytes of moments); the others walk their
// 7x7 neighbourhood (nz_spatial).
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
                v = nz_sigma_points(M.x / M.z, nz_var_of_mean(M));
            } else {
                const int x = (int)(i / (uint32_t)H), y = (int)(i - (uint32_t)x * (uint32_t)H);
                v = nz_spatial(A, x, y, A.object[i]);
            }
            noise = sqrt_ieee_(v);
        }
        A.noise[i] = noise;
        A.var0[i] = estimated ? v : -1.0f;
    }
    nz_stats(A.stats, A.threshold, blk, estimated, noise, blockIdx.x);
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
                nz_ss_df(M, ss, df);
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
            if (A.image_buffer[q].w > 0.0f) nz_ss_df(A.moments[q], ss, df);
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
                float var = nz_var_of_mean(M);
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
                v = nz_sigma_points(M.x / M.z, var);
            } else {
                v = nz_spatial(A, x, y, op);
            }
            noise = sqrt_ieee_(v);
        }
        A.noise[i] = noise;
        A.var0[i] = estimated ? v : -1.0f;
    }
    nz_stats(A.stats, A.threshold, blk, estimated, noise, blockIdx.y * gridDim.x + blockIdx.x);
}

static unsigned grid_of(int w, int h) { return (unsigned)(((size_t)w * h + 255) / 256); }

void launch_noise_update(const NoiseArgs& A, hipStream_t st) {
    hipLaunchKernelGGL(noise_update, dim3(grid_of(A.width, A.height)), dim3(256), 0, st, A);
}

void launch_noise_estimate(const NoiseArgs& A, hipStream_t st) {
    if (A.pool_batches > 0) {      // (rt_capi.hip admits radius 1..3 only)
        const dim3 grid((unsigned)((A.width + POOL_TX - 1) / POOL_TX), (unsigned)((A.height + POOL_TY - 1) / POOL_TY));
        with_radius(A.pool_radius, [&](auto R) { hipLaunchKernelGGL(noise_estimate_pooled<R()>, grid, dim3(256), 0, st, A); });
        return;
    }
    hipLaunchKernelGGL(noise_estimate, dim3(grid_of(A.width, A.height)), dim3(256), 0, st, A);
}

}  // namespace rt
