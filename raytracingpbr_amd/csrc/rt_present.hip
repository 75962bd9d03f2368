// rt_present.hip — the kernel of rtpbr_present (see rt_present.hpp for the layout, include/rtpbr.h for the arithmetic).
#include <hip/hip_runtime.h>

#include "rt_present.hpp"
#include "rt_device.hpp"

namespace rt {

// the 8 x 8 Bayer matrix of include/rtpbr.h, [top-down row & 7][column & 7]
__device__ const uint8_t PRESENT_BAYER[64] = {
    0,  32, 8,  40, 2,  34, 10, 42,  48, 16, 56, 24, 50, 18, 58, 26,  12, 44, 4,  36, 14, 46, 6,  38,  60, 28, 52, 20, 62, 30, 54, 22,
    3,  35, 11, 43, 1,  33, 9,  41,  51, 19, 59, 27, 49, 17, 57, 25,  15, 47, 7,  39, 13, 45, 5,  37,  63, 31, 55, 23, 61, 29, 53, 21};

// v -> 0..255: NaN is 0, clamp, one rounded multiply, one rounded add (the intrinsics are never contracted), truncation
RT_D uint32_t present_quant(float v, float t) {
    v = (v != v) ? 0.0f : v;
    v = fminf(fmaxf(v, 0.0f), 1.0f);
    return (uint32_t)__fadd_rn(__fmul_rn(v, 255.0f), t);
}

template <bool ACCUM, bool RGBA, bool DITHER>
__global__ void __launch_bounds__(256) present_kernel(const PresentArgs A) {
    constexpr int T = PRESENT_TILE, PITCH = T + 1;
    __shared__ uint32_t tile[T * PITCH];      // [x][y], one dword per pixel: r | g << 8 | b << 16 (the top byte is not used)
    __shared__ float thr[64];                 // DITHER: t per cell of the matrix
    const int W = A.width, H = A.height;
    const int x0 = (int)blockIdx.x * T, y0 = (int)blockIdx.y * T;
    const int nx = min(T, W - x0), ny = min(T, H - y0);
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    if constexpr (DITHER) {
        if (threadIdx.x < 64u) thr[threadIdx.x] = ((float)PRESENT_BAYER[threadIdx.x] + 0.5f) * 0.015625f;
        __syncthreads();
    }
    // ---- in: columns of the tile, contiguous along y
#pragma unroll 4
    for (int xl = wave; xl < nx; xl += 4) {
        const int x = x0 + xl;
        const size_t first = (size_t)x * (size_t)H + (size_t)y0;
        if constexpr (ACCUM) {
            if (lane < ny) {
                const vec3 c = tone_map(A.cfg, A.src4[first + (size_t)lane]);
                float t = 0.5f;
                if constexpr (DITHER) t = thr[((H - 1 - (y0 + lane)) & 7) * 8 + (x & 7)];
                tile[xl * PITCH + lane] = present_quant(c.x, t) | (present_quant(c.y, t) << 8) | (present_quant(c.z, t) << 16);
            }
        } else {
            const float* s = A.src3 + first * 3;
            uint8_t* tb = reinterpret_cast<uint8_t*>(tile);
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const int d = lane + 64 * k;      // dword of the stretch: pixel d / 3, channel d % 3
                if (d < 3 * ny) {
                    const float v = s[d];
                    const int yl = d / 3, c = d - 3 * yl;
                    float t = 0.5f;
                    if constexpr (DITHER) t = thr[((H - 1 - (y0 + yl)) & 7) * 8 + (x & 7)];
                    tb[(xl * PITCH + yl) * 4 + c] = (uint8_t)present_quant(v, t);
                }
            }
        }
    }
    __syncthreads();
    // ---- out: rows of the tile, contiguous along x; field row y is picture row H - 1 - y
    for (int yl = wave; yl < ny; yl += 4) {
        const size_t r = (size_t)(H - 1 - (y0 + yl));
        if constexpr (RGBA) {
            if (lane < nx)
                reinterpret_cast<uint32_t*>(A.out)[r * (size_t)W + (size_t)(x0 + lane)] = (tile[lane * PITCH + yl] & 0xFFFFFFu) | 0xFF000000u;
        } else {
            // the stretch is bytes a .. a + nb - 1 of the frame (whose base is dword-aligned): head bytes up to the next dword
            // boundary, nd aligned dwords, tail bytes
            const size_t a = (r * (size_t)W + (size_t)x0) * 3;
            const int nb = 3 * nx;
            const int head = min((int)((4u - (unsigned)(a & 3u)) & 3u), nb);
            const int nd = (nb - head) >> 2;
            const int tail_at = head + 4 * nd, tail = nb - tail_at;
            if (lane < nd) {
                // bytes o .. o + 3 of the stretch lie in pixels p0 = o / 3 and p0 + 1 = (o + 3) / 3 <= nx - 1
                const int o = head + 4 * lane, p0 = o / 3, sh = 8 * (o - 3 * p0);
                const uint32_t lo = tile[p0 * PITCH + yl] & 0xFFFFFFu, hi = tile[(p0 + 1) * PITCH + yl];
                *reinterpret_cast<uint32_t*>(A.out + a + (size_t)o) = (lo >> sh) | (hi << (24 - sh));      // hi's unused top byte leaves at the top
            }
            if (lane < head + tail) {
                const int o = lane < head ? lane : tail_at + (lane - head), p = o / 3, c = o - 3 * p;
                A.out[a + (size_t)o] = (uint8_t)(tile[p * PITCH + yl] >> (8 * c));
            }
        }
    }
}

void launch_present(const PresentArgs& A, bool accum, bool rgba, bool dither, hipStream_t st) {
    const dim3 grid((unsigned)((A.width + PRESENT_TILE - 1) / PRESENT_TILE), (unsigned)((A.height + PRESENT_TILE - 1) / PRESENT_TILE));
    with_bools([&](auto AC, auto RG, auto DI) { hipLaunchKernelGGL((present_kernel<AC(), RG(), DI()>), grid, dim3(256), 0, st, A); }, accum, rgba, dither);
}

}  // namespace rt
