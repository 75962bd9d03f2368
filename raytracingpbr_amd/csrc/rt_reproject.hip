// rt_reproject.hip — the gather kernels of rtpbr_reproject and rtpbr_reproject_scene (see rt_reproject.hpp; the arithmetic is fixed in include/rtpbr.h).
#include <hip/hip_runtime.h>

#include "rt_dispatch.hpp"
#include "rt_reproject.hpp"

namespace rt {

RT_D vec3 v3f(const float (&a)[3]) { return mk(a[0], a[1], a[2]); }

// Snap of one axis (include/rtpbr.h): a fractional offset within 2^-10 of 0 or 1 moves onto that pixel
RT_D void snap_axis(float p, int& x0, float& fx) {
    const float fl = floorf(p);
    x0 = (int)fl;
    fx = p - fl;
    if (fx < 0.0009765625f) {
        fx = 0.0f;
    } else if (fx > 0.9990234375f) {
        x0 = x0 + 1;
        fx = 0.0f;
    }
}

// The new pixel's centre ray, as feature_rays forms it
RT_D vec3 centre_ray(const ReprojArgs& A, int x, int y) {
    const int H = A.height, W = A.width;
    const CamFrame& f1 = A.cam1;
    float u, v;
    if (A.pinhole) {
        u = ((float)x + 0.5f) / (float)W;
        v = ((float)y + 0.5f) / (float)H;
    } else {
        u = ((float)x + 0.5f) * f1.inv_w;
        v = ((float)y + 0.5f) * f1.inv_h;
    }
    return normalize(fma3(v, v3f(f1.ver), fma3(u, v3f(f1.hor), v3f(f1.llc))) - v3f(f1.lf));
}

// The gather of pixel i from D (the first hit as the old eye sees it; on a miss the direction) and nn (the normal the old
// normals are compared with), and everything the pixel's lane writes: shared by reproject_gather and reproject_gather_scene.
// A tap loads the 4-byte old object first, then the 16-byte history texel, then (hits only) the 16-byte (normal, depth) record.
// HALVES: half A (rt_half.hpp) rides along like the moments: one more 16-byte load per accepted tap, one more 16-byte store per
// pixel.  Where the cap applies A is scaled by the image's own quotient k, so 0 <= A.w <= image_buffer.w stays exact (a_q.w <=
// b_q.w per tap, w >= 0, and every operation is monotone).
template <bool MOMENTS, bool HALVES>
RT_D void gather_taps(const ReprojArgs& A, uint32_t i, int obj, vec3 D, vec3 nn) {
    const int H = A.height, W = A.width;
    const CamFrame& f0 = A.cam0;
    const bool hit = obj >= 0;
    const vec3 lf0 = v3f(f0.lf);
    // into the old image plane: the ray lf0 + s D meets the plane of llc0 / hor0 / ver0
    const vec3 hor0 = v3f(f0.hor), ver0 = v3f(f0.ver);
    const vec3 q = v3f(f0.llc) - lf0;
    const vec3 N = cross(hor0, ver0);
    const float s = dot(q, N) / dot(D, N);
    float4 S = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float4 SM = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float4 SA = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float Wt = 0.0f;
    float2 mv = make_float2(-1.0f, -1.0f);
    if (s > 0.0f) {
        const vec3 P = D * s - q;
        const float u0 = dot(P, hor0) / dot(hor0, hor0);
        const float v0 = dot(P, ver0) / dot(ver0, ver0);
        const float px = u0 * (float)W - 0.5f, py = v0 * (float)H - 0.5f;
        if (px > -1.0f && px < (float)W && py > -1.0f && py < (float)H) {      // (also false on NaN): floorf below fits an int
            int x0, y0;
            float fx, fy;
            snap_axis(px, x0, fx);
            snap_axis(py, y0, fy);
            const float L = hit ? length(D) : 0.0f;
            const float tolL = A.depth_tol * L;
            const float wx[2] = {1.0f - fx, fx}, wy[2] = {1.0f - fy, fy};
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const int ti = t & 1, tj = t >> 1;
                const float w = wx[ti] * wy[tj];
                const int xq = x0 + ti, yq = y0 + tj;
                if (w == 0.0f || xq < 0 || xq >= W || yq < 0 || yq >= H) continue;
                const size_t qi = (size_t)xq * (size_t)H + (size_t)yq;
                if (A.hist_object[qi] != obj) continue;
                const float4 b = A.hist_image[qi];
                if (!(b.w > 0.0f)) continue;
                if (hit) {
                    const float4 g = A.hist_nz[qi];
                    if (!(fabsf(g.w - L) <= tolL)) continue;
                    if (!(A.normal_cos <= -1.0f || dot(mk(g.x, g.y, g.z), nn) >= A.normal_cos)) continue;
                }
                S.x = S.x + w * b.x;
                S.y = S.y + w * b.y;
                S.z = S.z + w * b.z;
                S.w = S.w + w * b.w;
                Wt = Wt + w;
                if constexpr (MOMENTS) {
                    const float4 m = A.hist_moments[qi];
                    SM.x = SM.x + w * m.x;
                    SM.y = SM.y + w * m.y;
                    SM.z = SM.z + w * m.z;
                    SM.w = SM.w + w * m.w;
                }
                if constexpr (HALVES) {
                    const float4 a = A.hist_half[qi];
                    SA.x = SA.x + w * a.x;
                    SA.y = SA.y + w * a.y;
                    SA.z = SA.z + w * a.z;
                    SA.w = SA.w + w * a.w;
                }
            }
            if (Wt > 0.0f) mv = make_float2((float)x0 + fx, (float)y0 + fy);
        }
    }
    float4 b = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float4 M = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float4 HA = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (Wt > 0.0f) {
        b = make_float4(S.x / Wt, S.y / Wt, S.z / Wt, S.w / Wt);
        if constexpr (MOMENTS) M = make_float4(SM.x / Wt, SM.y / Wt, SM.z / Wt, SM.w / Wt);
        if constexpr (HALVES) HA = make_float4(SA.x / Wt, SA.y / Wt, SA.z / Wt, SA.w / Wt);
        if (b.w > A.max_history) {
            const float k = A.max_history / b.w;
            b = make_float4(b.x * k, b.y * k, b.z * k, b.w * k);
            // the history weighs max_history samples in the estimate as in the image; the per-sample variance stays
            if constexpr (MOMENTS) M = make_float4(M.x * k, M.y * k, M.z * k, M.w > 1.0f ? 1.0f + (M.w - 1.0f) * k : M.w);
            if constexpr (HALVES) HA = make_float4(HA.x * k, HA.y * k, HA.z * k, HA.w * k);
        }
    }
    A.image_buffer[i] = b;
    if constexpr (MOMENTS) {
        A.moments[i] = M;
        A.snapshot[i] = b;      // what is in image_buffer now is no batch
    }
    if constexpr (HALVES) A.half_a[i] = HA;
    A.motion[i] = mv;
    // what rtpbr_refresh resets besides image_buffer (refresh_kernel, rt_kernels.hip)
    A.ray_buffer[i].depth = 0;
    if (A.adaptive) {
        A.diff_buffer[i] = make_float2(1.0f, 1.0f);
        A.diff_pixels[i] = 1e32f;
    }
}

// One lane per pixel, i = x * H + y: lanes of a wave walk down a column, so the new features are read and the outputs written
// contiguously; the four taps of neighbouring lanes share old pixels (the history is read where the motion takes it, through
// the caches: for a small move a wave's taps cover about two columns' worth of old pixels).
// MOMENTS: the luminance moments of the noise estimate (rt_noise.hpp) ride along — the same accepted taps and weights, 16 more
// bytes per accepted tap; the image's arithmetic is untouched.
// HALVES: so does half A of the two-half error estimate (rtpbr_set_half_mode, warp).
template <bool MOMENTS, bool HALVES>
__global__ void __launch_bounds__(256) reproject_gather(const ReprojArgs A) {
    const int H = A.height, W = A.width;
    const uint32_t n = (uint32_t)W * (uint32_t)H;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int x = (int)(i / (uint32_t)H), y = (int)(i - (uint32_t)x * (uint32_t)H);
    const vec3 d = centre_ray(A, x, y);
    const int obj = A.new_object[i];
    vec3 D = d;                                   // a miss: the direction, a point at infinity
    vec3 nn = mk(0.0f, 0.0f, 0.0f);
    if (obj >= 0) {
        const float4 nz = A.new_nz[i];
        D = fma3(nz.w, d, v3f(A.cam1.lf)) - v3f(A.cam0.lf);             // the first hit as the old eye sees it
        nn = mk(nz.x, nz.y, nz.z);
    }
    gather_taps<MOMENTS, HALVES>(A, i, obj, D, nn);
}

// reproject_gather with objects that moved rigidly between the old and the new frame (rtpbr_reproject_scene).  `table`: per
// object SCENE_MOTION_WORDS words — the moved flag (as a float: 0 or 1), p0, p1, R0, R1 (positions and row-major world-to-local
// matrices, 0 = old, 1 = new) — staged into LDS by the whole block: the lanes of a wave hit different objects, and a divergent
// LDS read costs a few cycles where a divergent global read costs a cache line per object.  Every thread of the block takes
// part in the staging and reaches the barrier, whether it owns a pixel or not (the last block of a frame, or a frame with
// fewer pixels than table words).  A hit on an object that did not move, and a miss, take reproject_gather's expressions.
template <bool MOMENTS, bool HALVES>
__global__ void __launch_bounds__(256) reproject_gather_scene(const ReprojArgs A, const float* __restrict__ table, const int n_obj) {
    __shared__ float T[MAX_OBJ * SCENE_MOTION_WORDS];
    const int words = (n_obj < MAX_OBJ ? n_obj : MAX_OBJ) * SCENE_MOTION_WORDS;
    for (int k = (int)threadIdx.x; k < words; k += (int)blockDim.x) T[k] = table[k];
    __syncthreads();
    const int H = A.height, W = A.width;
    const uint32_t n = (uint32_t)W * (uint32_t)H;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int x = (int)(i / (uint32_t)H), y = (int)(i - (uint32_t)x * (uint32_t)H);
    const vec3 d = centre_ray(A, x, y);
    const int obj = A.new_object[i];
    vec3 D = d;
    vec3 nn = mk(0.0f, 0.0f, 0.0f);
    if (obj >= 0) {
        const float4 nz = A.new_nz[i];
        const vec3 X1 = fma3(nz.w, d, v3f(A.cam1.lf));
        nn = mk(nz.x, nz.y, nz.z);
        const float* t = T + (obj < n_obj ? obj : 0) * SCENE_MOTION_WORDS;      // (the features never name an object past the table)
        if (obj < n_obj && t[0] != 0.0f) {
            const vec3 p0 = mk(t[1], t[2], t[3]), p1 = mk(t[4], t[5], t[6]);
            const float* R0 = t + 7;
            const float* R1 = t + 16;
            // world (new) -> the object's frame -> world (old): X0 = R0^T (R1 (X1 - p1)) + p0
            const vec3 a = X1 - p1;
            const vec3 l = mk(dot(mk(R1[0], R1[1], R1[2]), a), dot(mk(R1[3], R1[4], R1[5]), a), dot(mk(R1[6], R1[7], R1[8]), a));
            const vec3 X0 = mk(dot(mk(R0[0], R0[3], R0[6]), l) + p0.x, dot(mk(R0[1], R0[4], R0[7]), l) + p0.y, dot(mk(R0[2], R0[5], R0[8]), l) + p0.z);
            D = X0 - v3f(A.cam0.lf);
            if (!A.normal_local) {      // world-space normals turn with the object; local-frame normals are the object's own
                const vec3 m = mk(dot(mk(R1[0], R1[1], R1[2]), nn), dot(mk(R1[3], R1[4], R1[5]), nn), dot(mk(R1[6], R1[7], R1[8]), nn));
                nn = mk(dot(mk(R0[0], R0[3], R0[6]), m), dot(mk(R0[1], R0[4], R0[7]), m), dot(mk(R0[2], R0[5], R0[8]), m));
            }
        } else {
            D = X1 - v3f(A.cam0.lf);
        }
    }
    gather_taps<MOMENTS, HALVES>(A, i, obj, D, nn);
}

void launch_reproject(const ReprojArgs& A, hipStream_t st) {
    const unsigned grid = (unsigned)(((size_t)A.width * A.height + 255) / 256);
    with_bools([&](auto M, auto HV) { hipLaunchKernelGGL((reproject_gather<M(), HV()>), dim3(grid), dim3(256), 0, st, A); },
               A.hist_moments != nullptr, A.hist_half != nullptr);
}

void launch_reproject_scene(const ReprojArgs& A, const float* table, int n_obj, hipStream_t st) {
    const unsigned grid = (unsigned)(((size_t)A.width * A.height + 255) / 256);
    with_bools([&](auto M, auto HV) { hipLaunchKernelGGL((reproject_gather_scene<M(), HV()>), dim3(grid), dim3(256), 0, st, A, table, n_obj); },
               A.hist_moments != nullptr, A.hist_half != nullptr);
}

}  // namespace rt
