// rt_coverage.hip — kernels of rtpbr_render_coverage and the resolve of rtpbr_denoise_coverage (see rt_coverage.hpp).
#include <hip/hip_runtime.h>

#include "rt_coverage.hpp"
#include "rt_trace.hpp"

namespace rt {

RT_D uint32_t cover_rank(unsigned long long m) {      // set bits below this lane
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
}

// One lane per pixel, i = x * H + y.  Candidate: some pixel of the 3x3 neighbourhood inside the frame holds another object index.
__global__ void __launch_bounds__(256) cover_mark(const CoverageArgs A) {
    const int H = A.height, W = A.width;
    const uint32_t n = (uint32_t)W * (uint32_t)H;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool cand = false;
    if (i < n) {
        const int x = (int)(i / (uint32_t)H), y = (int)(i - (uint32_t)x * (uint32_t)H);
        const int op = A.object[i];
        for (int dx = -1; dx <= 1; dx++) {
            const int xq = x + dx;
            if (xq < 0 || xq >= W) continue;
            for (int dy = -1; dy <= 1; dy++) {
                const int yq = y + dy;
                if (yq < 0 || yq >= H) continue;
                cand = cand || A.object[(size_t)xq * (size_t)H + (size_t)yq] != op;
            }
        }
        const int S = A.grid * A.grid;
        if (!cand) A.coverage[i] = make_int4(S, -2, 0, S);
    }
    // (no lane has left: the ballot and the broadcast see the whole wave)
    const unsigned long long m = __ballot(cand);
    if (m == 0) return;
    uint32_t at = 0;
    if ((threadIdx.x & 63) == 0) at = atomicAdd(A.list, (uint32_t)__popcll(m));
    at = (uint32_t)__builtin_amdgcn_readfirstlane((int)at);
    if (cand) A.list[COVER_HEAD + at + cover_rank(m)] = i;      // at + rank < the total <= n: the list has n entries of room
}

// S = G * G lanes per candidate, 256 / S candidates per block, blocks stride over the list.  Pg carries the G-fold configuration
// (width, height, inv_w, inv_h): sub-ray (a, b) of pixel (px, py) is feature_rays' ray of pixel (G px + a, G py + b) there.
template <int KIND, int G>
__global__ void __launch_bounds__(256) cover_rays(const Params P, const CoverageArgs A) {
    constexpr int S = G * G, PER_BLOCK = 256 / S;
    const uint32_t count = A.list[0];
    const int H = A.height;
    const CamFrame& f = P.cam;
    const vec3 lf = mk(f.lf[0], f.lf[1], f.lf[2]);
    const bool src = P.cfg.march_kind == RTPBR_MARCH_SRC;
    const int sub = (int)(threadIdx.x % S);
    for (uint32_t base = blockIdx.x * PER_BLOCK; base < count; base += gridDim.x * PER_BLOCK) {      // (uniform in the block)
        const uint32_t slot = base + threadIdx.x / S;
        const bool live = slot < count;
        const uint32_t i = live ? A.list[COVER_HEAD + slot] : 0u;
        const int px = (int)(i / (uint32_t)H), py = (int)(i - (uint32_t)px * (uint32_t)H);
        const int sx = G * px + sub / G, sy = G * py + sub % G;
        Lane L;
        L.state = ST_IDLE;
        L.n_steps = L.n_raycasts = L.n_hits = L.n_sky = 0;
        L.o = L.d = mk(0, 0, 0);
        L.t = L.w = L.s = L.dist = L.t_eval = 0.0f;
        L.idx = 0;
        L.steps_left = 0;
        if (live) {      // as feature_rays
            float u, v;
            if (P.cfg.camera_kind == RTPBR_CAMERA_PINHOLE) {
                u = ((float)sx + 0.5f) / (float)P.cfg.width;
                v = ((float)sy + 0.5f) / (float)P.cfg.height;
            } else {
                u = ((float)sx + 0.5f) * f.inv_w;
                v = ((float)sy + 0.5f) * f.inv_h;
            }
            vec3 po = fma3(v, mk(f.ver[0], f.ver[1], f.ver[2]), fma3(u, mk(f.hor[0], f.hor[1], f.hor[2]), mk(f.llc[0], f.llc[1], f.llc[2])));
            L.o = lf;
            L.d = normalize(po - lf);
            if (src) {
                L.w = P.cfg.omega0;
                L.dist = P.cfg.max_dis;
                L.steps_left = P.cfg.max_raymarch;
                L.state = ST_MARCH;
            } else {
                march_init(P, L);
            }
        }
        if (src) {
            while (__any(L.state == ST_MARCH))
                if (L.state == ST_MARCH) march_step_src<KIND>(P, L);
        } else {
            while (__any(L.state == ST_MARCH))
                if (L.state == ST_MARCH) march_step<KIND, 0>(P, L);
        }
        // the whole wave is here again.  obj: this sub-ray's object (-1 = miss); own: the pixel's
        const int obj = L.state == ST_HIT ? L.idx : -1;
        const int own = live ? A.object[i] : -1;
        const int group = (int)(threadIdx.x & 63u) & ~(S - 1);      // first lane of this pixel's group in the wave
        int same = 0;                                               // sub-rays of the pixel on this lane's object
#pragma unroll
        for (int j = 0; j < S; j++) same += __shfl(obj, group + j, 64) == obj ? 1 : 0;
        // the most frequent other object, ties to the smaller index: the largest (count, -index) over the group, the index in 8 bits
        static_assert(MAX_OBJ <= 254, "the key holds object index + 1 in its low byte");
        int key = obj != own ? (same << 8) | (255 - (obj + 1)) : 0;
#pragma unroll
        for (int off = 1; off < S; off <<= 1) {
            const int other = __shfl_xor(key, off, 64);
            key = other > key ? other : key;
        }
        const unsigned long long mine = __ballot(obj == own) >> group;
        const int n_own = __popcll(mine & ((1ull << S) - 1ull));
        if (live && sub == 0) A.coverage[i] = key ? make_int4(n_own, 254 - (key & 255), key >> 8, S) : make_int4(n_own, -2, 0, S);
    }
}

// k = a * a * ... (power factors, left to right), a = (float)n_own / (float)S; head[2] = bits of the largest 1 - a (one atomic per wave)
__global__ void __launch_bounds__(256) cover_weights(const CoverageArgs A) {
    const uint32_t n = (uint32_t)A.width * (uint32_t)A.height;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    float lack = 0.0f;
    if (i < n) {
        const int4 c = A.coverage[i];
        const float a = (float)c.x / (float)c.w;
        float k = 1.0f;
        for (int j = 0; j < A.power; j++) k = k * a;
        A.k[i] = k;
        lack = 1.0f - a;
    }
    uint32_t bits = __float_as_uint(lack);      // lack >= +0: the bit patterns order as the values do
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)bits, off, 64);
        bits = other > bits ? other : bits;
    }
    if ((threadIdx.x & 63) == 0 && bits != 0) atomicMax(A.list + 2, bits);
}

// The resolve and the tone map of rtpbr_denoise_coverage.  Block (16, 16): thread (tx, ty) has pixel (16 bx + tx, 16 by + ty), ty along
// y, the buffers' contiguous index.  The tile and its halo, 18 x 18 cells of (F, object word, k): object word -3 = outside the frame
// or without samples (matches no second object: those are >= -1).
// FILL (option coverage_fill = 1): "with samples" is "has a colour after the last level", the byte the filling last level wrote
// into A.live (atrous_level's COVER and FILL form, rt_features.hip) — for the centre and for its eight neighbours alike.
constexpr int RES_T = 16, RES_P = RES_T + 2;
constexpr int RES_NONE = -3;
template <bool FILL>
__global__ void __launch_bounds__(256) cover_resolve(const ResolveArgs A) {
    __shared__ float tf[RES_P * RES_P][3];
    __shared__ int to[RES_P * RES_P];
    __shared__ float tk[RES_P * RES_P];
    const int H = A.height, W = A.width;
    const int x0 = (int)blockIdx.x * RES_T - 1, y0 = (int)blockIdx.y * RES_T - 1;
    for (int c = (int)threadIdx.x; c < RES_P * RES_P; c += 256) {
        const int cx = c / RES_P, cy = c - cx * RES_P;
        const int xq = x0 + cx, yq = y0 + cy;
        int o = RES_NONE;
        float fx = 0.0f, fy = 0.0f, fz = 0.0f, k = 0.0f;
        if (xq >= 0 && xq < W && yq >= 0 && yq < H) {
            const size_t q = (size_t)xq * (size_t)H + (size_t)yq;
            if (FILL ? A.live[q] != 0 : A.image_buffer[q].w > 0.0f) {
                o = A.object[q];
                fx = A.linear[q * 3 + 0];
                fy = A.linear[q * 3 + 1];
                fz = A.linear[q * 3 + 2];
                k = A.k[q];
            }
        }
        tf[c][0] = fx;
        tf[c][1] = fy;
        tf[c][2] = fz;
        to[c] = o;
        tk[c] = k;
    }
    __syncthreads();
    const int tx = (int)threadIdx.x / RES_T, ty = (int)threadIdx.x % RES_T;
    const int x = x0 + 1 + tx, y = y0 + 1 + ty;
    const bool in_frame = x < W && y < H;
    bool resolved = false;
    if (in_frame) {
        const size_t i = (size_t)x * (size_t)H + (size_t)y;
        const int cc = (tx + 1) * RES_P + (ty + 1);
        vec3 t;
        if (to[cc] == RES_NONE) {      // no samples (FILL: and no level reached it): exactly what post_process shows
            t = tone_map(A.cfg, A.image_buffer[i]);
        } else {
            vec3 F = mk(tf[cc][0], tf[cc][1], tf[cc][2]);
            const int4 cov = A.coverage[i];
            if (A.resolve && cov.z > 0) {
                float sw = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f;
#pragma unroll
                for (int dy = -1; dy <= 1; dy++) {
#pragma unroll
                    for (int dx = -1; dx <= 1; dx++) {
                        if (dx == 0 && dy == 0) continue;
                        const int cq = cc + dx * RES_P + dy;
                        if (to[cq] != cov.y) continue;
                        const float w = tk[cq] * ((dx == 0 || dy == 0) ? 0.5f : 1.0f / 3.0f);
                        sw = sw + w;
                        sx = sx + w * tf[cq][0];
                        sy = sy + w * tf[cq][1];
                        sz = sz + w * tf[cq][2];
                    }
                }
                if (sw > 0.0f) {
                    const float no = (float)cov.x, ns = (float)cov.z, nt = (float)(cov.x + cov.z);
                    F = mk((no * F.x + ns * (sx / sw)) / nt, (no * F.y + ns * (sy / sw)) / nt, (no * F.z + ns * (sz / sw)) / nt);
                    resolved = true;
                }
            }
            t = tone_map(A.cfg, make_float4(F.x, F.y, F.z, 1.0f));
        }
        A.out[i * 3 + 0] = t.x;
        A.out[i * 3 + 1] = t.y;
        A.out[i * 3 + 2] = t.z;
    }
    const unsigned long long m = __ballot(resolved);
    if ((threadIdx.x & 63) == 0 && m != 0) atomicAdd(A.head + 1, (uint32_t)__popcll(m));
}

void launch_cover_mark(const CoverageArgs& A, hipStream_t st) {
    const unsigned grid = (unsigned)(((size_t)A.width * A.height + 255) / 256);
    hipLaunchKernelGGL(cover_mark, dim3(grid), dim3(256), 0, st, A);
}

// The list's length stays on the device: the grid is what the whole frame would need, capped at eight blocks per CU (blocks > 0:
// at that many, option cover_blocks), and the blocks stride over the list (a block past its end reads the length and leaves).
void launch_cover_rays(const Params& P, const CoverageArgs& A, int kind, int n_cu, int blocks, hipStream_t st) {
    const size_t per_block = 256 / (size_t)(A.grid * A.grid);
    const size_t need = ((size_t)A.width * A.height + per_block - 1) / per_block;
    const size_t cap = blocks > 0 ? (size_t)blocks : (size_t)(n_cu > 0 ? n_cu : 256) * 8;
    const unsigned grid = (unsigned)(need < cap ? need : cap);
    with_kind(kind, [&](auto K) {      // (rt_capi.hip admits grid 2 and 4 only)
        constexpr int KIND = K();
        with_bools([&](auto two) { hipLaunchKernelGGL((cover_rays<KIND, two() ? 2 : 4>), dim3(grid), dim3(256), 0, st, P, A); }, A.grid == 2);
    });
}

void launch_cover_weights(const CoverageArgs& A, hipStream_t st) {
    const unsigned grid = (unsigned)(((size_t)A.width * A.height + 255) / 256);
    hipLaunchKernelGGL(cover_weights, dim3(grid), dim3(256), 0, st, A);
}

void launch_cover_resolve(const ResolveArgs& A, hipStream_t st) {
    const dim3 grid((unsigned)((A.width + RES_T - 1) / RES_T), (unsigned)((A.height + RES_T - 1) / RES_T));
    with_bools([&](auto FILL) { hipLaunchKernelGGL(cover_resolve<FILL()>, grid, dim3(256), 0, st, A); }, A.live != nullptr);
}

}  // namespace rt
