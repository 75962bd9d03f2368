// rt_half.hip — kernels of rtpbr_half_update / rtpbr_denoise_error (see rt_half.hpp).
#include <hip/hip_runtime.h>

#include "rt_half.hpp"
#include "rt_device.hpp"

namespace rt {

// One lane per pixel, i = x * H + y: all three buffers are read and written along the contiguous index.
__global__ void __launch_bounds__(256) half_update(const HalfArgs A) {
    const uint32_t n = (uint32_t)A.width * (uint32_t)A.height;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 b = A.image_buffer[i];
    const float4 s = A.snapshot[i];
    const float4 d = make_float4(b.x - s.x, b.y - s.y, b.z - s.z, b.w - s.w);
    if (d.w > 0.0f) {
        float4 a = A.half_a[i];
        const float cB = s.w - a.w;
        if (a.w <= cB) {      // the half with fewer samples takes the batch; otherwise it stays in B = image_buffer - A
            a.x = a.x + d.x;
            a.y = a.y + d.y;
            a.z = a.z + d.z;
            a.w = a.w + d.w;
            A.half_a[i] = a;
        }
    }
    A.snapshot[i] = b;
}

__global__ void __launch_bounds__(256) half_subtract(const HalfArgs A) {
    const uint32_t n = (uint32_t)A.width * (uint32_t)A.height;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 b = A.image_buffer[i];
    const float4 a = A.half_a[i];
    A.half_b[i] = make_float4(b.x - a.x, b.y - a.y, b.z - a.z, b.w - a.w);
}

// ---- the window kernel.  A block owns a tile of ERR_TX x ERR_TY pixels (x by y, y contiguous; thread t: ly = t % ERR_TY, so a
// wave runs along y) and stages (e_q, object_q) of the tile and an R-pixel halo into LDS once: 8 bytes per entry in two planes of
// one pitch.  An entry that is not valid (a half without samples) or lies outside the frame holds e = +0 and an object word no
// pixel has (ERR_NOBODY; first hits are >= -1): the object compare of the tap loop is then the whole test, the loop has one fixed
// trip count per radius, and adding +0 to a non-negative sum is the identity.  The tile is noise_estimate_pooled<R>'s (16 x 16:
// the shape measured best there) and so is the planes' pitch.
// Traffic per staged entry: 24 bytes of the two filtered colours, the two count words of 16-byte texels, 4 bytes of object;
// entries per pixel: (TX + 2R)(TY + 2R) / (TX TY) = 1.27 / 1.56 / 1.89.
constexpr int ERR_TX = 16, ERR_TY = 16;
constexpr int ERR_NOBODY = (int)0x80000000;
// the pitch in words: the four column runs a wave reads at once start 16 banks apart (ds_read_b32 serves two runs per group of 32 lanes over 32 banks)
constexpr int err_pitch(int hy) {
    int p = hy;
    while (p % 32 != 16) p++;
    return p;
}

template <int R>
__global__ void __launch_bounds__(256) half_error(const ErrorArgs A) {
    constexpr int HX = ERR_TX + 2 * R, HY = ERR_TY + 2 * R, PITCH = err_pitch(HY);
    __shared__ float t_e[HX * PITCH];
    __shared__ int t_obj[HX * PITCH];
    __shared__ uint32_t blk[3];
    if (threadIdx.x < 3) blk[threadIdx.x] = 0u;
    const int H = A.height, W = A.width;
    const int x0 = (int)blockIdx.x * ERR_TX, y0 = (int)blockIdx.y * ERR_TY;
    // the tile and its halo, hy fastest (contiguous in memory)
    for (int t = (int)threadIdx.x; t < HX * HY; t += 256) {
        const int hx = t / HY, hy = t - hx * HY;
        const int xq = x0 - R + hx, yq = y0 - R + hy;
        float e = 0.0f;
        int oq = ERR_NOBODY;
        if (xq >= 0 && xq < W && yq >= 0 && yq < H) {
            const size_t q = (size_t)xq * (size_t)H + (size_t)yq;
            const float cA = A.half_a[q].w, cB = A.half_b[q].w;
            if (cA > 0.0f && cB > 0.0f) {
                const float dl = nz_lum(mk(A.da[q * 3 + 0], A.da[q * 3 + 1], A.da[q * 3 + 2])) -
                                 nz_lum(mk(A.db[q * 3 + 0], A.db[q * 3 + 1], A.db[q * 3 + 2]));
                e = fmax_((dl * dl) * ((cA * cB) / ((cA + cB) * (cA + cB))), 0.0f);      // (a NaN gives 0)
                oq = A.object[q];
            }
        }
        t_e[hx * PITCH + hy] = e;
        t_obj[hx * PITCH + hy] = oq;
    }
    __syncthreads();
    const int lx = (int)threadIdx.x / ERR_TY, ly = (int)threadIdx.x % ERR_TY;
    const int x = x0 + lx, y = y0 + ly;
    bool estimated = false;
    float err = 0.0f;
    if (x < W && y < H) {
        const int op = t_obj[(lx + R) * PITCH + (ly + R)];
        if (op != ERR_NOBODY) {
            estimated = true;
            float S = 0.0f, cn = 0.0f;
#pragma unroll
            for (int dy = -R; dy <= R; dy++) {
#pragma unroll
                for (int dx = -R; dx <= R; dx++) {
                    const int q = (lx + R + dx) * PITCH + (ly + R + dy);
                    const bool same = t_obj[q] == op;
                    S = S + (same ? t_e[q] : 0.0f);
                    cn = cn + (same ? 1.0f : 0.0f);
                }
            }
            err = sqrt_ieee_(S / cn);
        }
        A.error[(size_t)x * (size_t)H + (size_t)y] = err;
    }
    nz_stats(A.stats, A.threshold, blk, estimated, err, blockIdx.y * gridDim.x + blockIdx.x);
}

static unsigned grid_of(int w, int h) { return (unsigned)(((size_t)w * h + 255) / 256); }

void launch_half_update(const HalfArgs& A, hipStream_t st) {
    hipLaunchKernelGGL(half_update, dim3(grid_of(A.width, A.height)), dim3(256), 0, st, A);
}

void launch_half_subtract(const HalfArgs& A, hipStream_t st) {
    hipLaunchKernelGGL(half_subtract, dim3(grid_of(A.width, A.height)), dim3(256), 0, st, A);
}

void launch_half_error(const ErrorArgs& A, hipStream_t st) {      // (rt_capi.hip admits radius 1..3 only)
    const dim3 grid((unsigned)((A.width + ERR_TX - 1) / ERR_TX), (unsigned)((A.height + ERR_TY - 1) / ERR_TY));
    if (A.radius == 1) hipLaunchKernelGGL(half_error<1>, grid, dim3(256), 0, st, A);
    else if (A.radius == 2) hipLaunchKernelGGL(half_error<2>, grid, dim3(256), 0, st, A);
    else hipLaunchKernelGGL(half_error<3>, grid, dim3(256), 0, st, A);
}

}  // namespace rt
