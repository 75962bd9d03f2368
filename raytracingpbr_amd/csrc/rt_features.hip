// rt_features.hip — kernels of rtpbr_render_features / rtpbr_denoise and the filter of rtpbr_denoise_guided (see rt_features.hpp).
#include <hip/hip_runtime.h>

#include "rt_features.hpp"
#include "rt_trace.hpp"

namespace rt {

// Primary ray through the centre of pixel i = x * H + y (lanes along y: the buffers' contiguous index).  Modelled on
// primary_rays_impl (rt_trace.hpp) without its claim counter: one lane per pixel, P.counters untouched.
template <int KIND>
__global__ void __launch_bounds__(256) feature_rays(const Params P, const FeatArgs A) {
    __shared__ ObjFull lds_obj[MAX_OBJ];
    stage_objects(P, lds_obj);
    const int H = P.cfg.height;
    const uint32_t n = (uint32_t)P.cfg.width * (uint32_t)H;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool in_frame = i < n;
    const int px = (int)(i / (uint32_t)H), py = (int)(i - (uint32_t)px * (uint32_t)H);
    const CamFrame& f = P.cam;
    const vec3 lf = mk(f.lf[0], f.lf[1], f.lf[2]);
    const bool src = P.cfg.march_kind == RTPBR_MARCH_SRC;
    Lane L;
    L.state = ST_IDLE;
    L.n_steps = L.n_raycasts = L.n_hits = L.n_sky = 0;
    L.o = L.d = mk(0, 0, 0);
    L.t = L.w = L.s = L.dist = L.t_eval = 0.0f;
    L.idx = 0;
    L.steps_left = 0;
    if (in_frame) {
        // gen_ray (rt_device.hpp) with j1 = j2 = 0.5 and no lens draws: the origin is lookfrom for both camera kinds
        float u, v;
        if (P.cfg.camera_kind == RTPBR_CAMERA_PINHOLE) {
            u = ((float)px + 0.5f) / (float)P.cfg.width;
            v = ((float)py + 0.5f) / (float)P.cfg.height;
        } else {
            u = ((float)px + 0.5f) * f.inv_w;
            v = ((float)py + 0.5f) * f.inv_h;
        }
        vec3 po = fma3(v, mk(f.ver[0], f.ver[1], f.ver[2]), fma3(u, mk(f.hor[0], f.hor[1], f.hor[2]), mk(f.llc[0], f.llc[1], f.llc[2])));
        L.o = lf;
        L.d = normalize(po - lf);
        if (src) {      // raycast() src/scene.py:59-84: t = 0, d = MAX_DIS
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
    if (!in_frame) return;
    vec3 alb = mk(0, 0, 0), nrm = mk(0, 0, 0);
    float depth = P.cfg.max_dis;
    int obj = -1;
    if (L.state == ST_HIT) {
        // the hit position the sample path shades at: src moves the origin, the examples evaluate at o + t_eval d
        const vec3 hp = src ? L.o : fma3(L.t_eval, L.d, L.o);
        const ObjFull& o = lds_obj[L.idx];
        alb = mk(o.albedo[0], o.albedo[1], o.albedo[2]);
        nrm = calc_normal<KIND>(P, o, hp);
        depth = length(hp - lf);
        obj = L.idx;
    }
    A.albedo[(size_t)i * 3 + 0] = alb.x;
    A.albedo[(size_t)i * 3 + 1] = alb.y;
    A.albedo[(size_t)i * 3 + 2] = alb.z;
    A.normal[(size_t)i * 3 + 0] = nrm.x;
    A.normal[(size_t)i * 3 + 1] = nrm.y;
    A.normal[(size_t)i * 3 + 2] = nrm.z;
    A.depth[i] = depth;
    A.object[i] = obj;
    A.guide_nz[i] = make_float4(nrm.x, nrm.y, nrm.z, depth);
}

RT_D vec3 xyz(float4 v) { return mk(v.x, v.y, v.z); }
RT_D float sq3(vec3 v) { return (v.x * v.x + v.y * v.y) + v.z * v.z; }      // |v|^2 in this order, no fma
RT_D vec3 albedo_clamped(const DenoiseArgs& A, uint32_t i) {
    return mk(fmax_(A.albedo[(size_t)i * 3 + 0], 1e-3f), fmax_(A.albedo[(size_t)i * 3 + 1], 1e-3f), fmax_(A.albedo[(size_t)i * 3 + 2], 1e-3f));
}
// The filter's start colour of a pixel from T7 (level 0): the average, divided by max(albedo, 1e-3) when demodulating
RT_D vec3 start_colour(float4 b, vec3 ac, int demod) {
    vec3 c = mk(b.x / b.w, b.y / b.w, b.z / b.w);
    return demod ? mk(c.x / ac.x, c.y / ac.y, c.z / ac.z) : c;
}

// One a-trous level.  Taps: dy outer, dx inner, -2..2, at p + step (dx, dy); h = H[|dx|] H[|dy|], H = {3/8, 1/4, 1/16};
// e = |r(c_p) - r(c_q)|^2 ic + |n_p - n_q|^2 in + ((z_p - z_q) / max(z_p, 1e-6))^2 iz + |a_p - a_q|^2 ia (left to right),
// r(c) = c / (1 + c); w = h exp_(-min(e, 80)).  Taps outside the frame, without samples or on another object are skipped.
// A tap is only taken on the centre's own object index and the albedo is a per-object constant (0 on a miss), so a_q = a_p on
// every tap taken: the albedo term is exactly +0 (e + 0 = e) and the neighbour's demodulation divides by the centre's albedo.
// Neither is loaded per tap: a tap reads the 4-byte object index (level 0) or the object word carried in the previous level's
// record (colour, object), then — on the centre's object only — the 16-byte (normal, depth) record: 36 bytes per tap at level 0,
// 32 later.
// GUIDED: the colour term's ic is per pixel, 1 / (sigma_c^2 max(g, floor)), g the 3x3 Gaussian of the level's variance (nine
// more taps of object word + variance, 8 bytes each), and the variance is filtered beside the colour with the squared weights:
// 4 more bytes per tap taken (40 / 36), one more 4-byte record written.
// LINEAR (last level only; rtpbr_denoise_blend): out takes the linear colour after remodulation — exactly the value the other
// form hands to tone_map — and +0 for a pixel without samples.
// COVER (rtpbr_denoise_coverage; plain, its last level LINEAR): every tap but the centre's is weighted by k_q of the coverage plane
// (rt_coverage.hpp), w = (h exp_(-min(e, 80))) k_q: 4 more bytes per tap taken.
// FILL (rtpbr_denoise with option denoise_fill = 1; plain, never LINEAR): a centre without a colour (no samples, or not reached by
// an earlier level) runs the same tap loop with the colour term of e taken as +0 — it has no colour to compare — and, when any
// tap was taken (sw > 0), leaves as any other pixel does: its record carries its object index, so it is live from the next level
// on; the last level remodulates it by its own albedo.  Its taps are the live pixels of its own object (A.object[p]; a level's
// record of an empty pixel carries NO_SAMPLES and matches nobody).  One loop serves both kinds of centre: on a lattice they
// alternate within a wave.  A.fill: FILL_SHARDS shards of (filled, empty, deepest level), summed / maximised by the reader.
// COVER and FILL (rtpbr_denoise_coverage with option coverage_fill = 1; LINEAR at the last level as COVER is): every tap an empty
// centre takes is weighted by k_q as well (its own position is not live and never a tap), so whether it is filled is the computed
// sw > 0, not reach alone: k_q may be 0, and k_q times a weight near h exp_(-80) may underflow.  The linear plane has no object word:
// the last level writes A.live, 1 for a pixel that leaves with a colour and 0 beside the +0 of a pixel still empty.
template <bool FIRST, bool LAST, bool GUIDED, bool LINEAR = false, bool COVER = false, bool FILL = false>
__global__ void __launch_bounds__(256) atrous_level(const DenoiseArgs A) {
    static_assert(atrous_form_ok(FIRST, LAST, GUIDED, LINEAR, COVER, FILL), "no such form (rt_dispatch.hpp)");
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
        valid = op != NO_SAMPLES;
        if constexpr (FILL)
            if (!valid) op = A.object[i];
    }
    if (!FILL && !valid) {       // no samples: exactly what post_process shows, and nobody's neighbour
        if constexpr (LAST) {
            const vec3 t = LINEAR ? mk(0.0f, 0.0f, 0.0f) : tone_map(A.cfg, A.image_buffer[i]);
            A.out[(size_t)i * 3 + 0] = t.x;
            A.out[(size_t)i * 3 + 1] = t.y;
            A.out[(size_t)i * 3 + 2] = t.z;
        } else {
            A.dst[i] = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(NO_SAMPLES));
            if constexpr (GUIDED) A.vdst[i] = 0.0f;
        }
        return;
    }
    float icp = A.ic;
    if constexpr (GUIDED) {
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
        icp = 1.0f / (A.sc2 * fmax_(gs / gk, A.floor));
    }
    const bool need_albedo = (FIRST || LAST) && A.demodulate;
    const vec3 ac = need_albedo ? albedo_clamped(A, i) : mk(1.0f, 1.0f, 1.0f);
    const vec3 cp = FIRST ? start_colour(cp4, ac, A.demodulate) : xyz(cp4);
    const float4 gp_nz = A.guide_nz[i];
    const vec3 np = xyz(gp_nz);
    const float zp = gp_nz.w;
    const float izp = fmax_(zp, 1e-6f);
    const vec3 rp = tonemap_r(cp);
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
            float vq = 0.0f;
            if constexpr (FIRST) {
                if (A.object[q] != op) continue;
                const float4 b = A.image_buffer[q];
                if (!(b.w > 0.0f)) continue;
                cq = start_colour(b, ac, A.demodulate);
                if constexpr (GUIDED) vq = A.var0[q];
            } else {
                const float4 c4 = A.src[q];
                if (__float_as_int(c4.w) != op) continue;
                cq = xyz(c4);
                if constexpr (GUIDED) vq = A.vsrc[q];
            }
            const float4 gq_nz = A.guide_nz[q];
            const float h = HK[dx < 0 ? -dx : dx] * HK[dy < 0 ? -dy : dy];
            const float dz = (zp - gq_nz.w) / izp;
            float e;
            if constexpr (FILL) {      // (0 + x = x: the features' terms alone; a wave of empty centres skips the divides)
                e = 0.0f;
                if (valid) e = sq3(rp - tonemap_r(cq)) * icp;
            } else {
                e = sq3(rp - tonemap_r(cq)) * icp;
            }
            e = e + sq3(np - xyz(gq_nz)) * A.in;
            e = e + (dz * dz) * A.iz;
            // (+ |a_p - a_q|^2 ia = + 0: see above)
            // (e is clamped where exp no longer matters: a weight under 2e-35 against the centre's 9/64; far past it the Cephes
            // reduction of exp_ loses its argument and could overflow)
            float w = h * exp_(-fmin_(e, 80.0f));
            if constexpr (COVER)
                if (dx != 0 || dy != 0) w = w * A.cover_k[q];
            sw = sw + w;
            sx = sx + w * cq.x;
            sy = sy + w * cq.y;
            sz = sz + w * cq.z;
            if constexpr (GUIDED) sv = sv + (w * w) * vq;
        }
    }
    if constexpr (FILL) {
        const bool empty = !valid && !(sw > 0.0f);
        // the counts: a wave that has something to report adds to its shard (lane 0 is in the frame whenever a lane of its wave is).
        // On a lattice every wave fills pixels at level 0: the pixels filled are counted once, at the last level (empty at the
        // start, a colour at the end); a level above 0 that fills raises the deepest level (level 0 leaves the zero it finds).
        uint32_t* const shard = A.fill + (((blockIdx.x * 4u + (threadIdx.x >> 6)) % (uint32_t)FILL_SHARDS) * (uint32_t)FILL_SHARD_WORDS);
        if constexpr (!FIRST) {
            const unsigned long long mf = __ballot(!valid && !empty);
            if ((threadIdx.x & 63) == 0 && mf != 0) atomicMax(shard + 2, (uint32_t)(31 - __clz(A.step)));
        }
        if constexpr (LAST) {
            const bool was_empty = FIRST ? !valid : !(A.image_buffer[i].w > 0.0f);
            const unsigned long long mf = __ballot(was_empty && !empty), me = __ballot(empty);
            if ((threadIdx.x & 63) == 0 && mf != 0) atomicAdd(shard, (uint32_t)__popcll(mf));
            if ((threadIdx.x & 63) == 0 && me != 0) atomicAdd(shard + 1, (uint32_t)__popcll(me));
        }
        if (empty) {      // no tap of this level was live on its object: as a pixel without samples leaves the other forms
            if constexpr (LAST) {
                const vec3 t = LINEAR ? mk(0.0f, 0.0f, 0.0f) : tone_map(A.cfg, A.image_buffer[i]);
                A.out[(size_t)i * 3 + 0] = t.x;
                A.out[(size_t)i * 3 + 1] = t.y;
                A.out[(size_t)i * 3 + 2] = t.z;
                if constexpr (LINEAR) A.live[i] = 0;
            } else {
                A.dst[i] = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(NO_SAMPLES));
            }
            return;
        }
        if constexpr (LINEAR) A.live[i] = 1;
    }
    vec3 c = mk(sx / sw, sy / sw, sz / sw);
    if constexpr (LAST) {
        if (A.demodulate) c = mk(c.x * ac.x, c.y * ac.y, c.z * ac.z);
        const vec3 t = LINEAR ? c : tone_map(A.cfg, make_float4(c.x, c.y, c.z, 1.0f));
        A.out[(size_t)i * 3 + 0] = t.x;
        A.out[(size_t)i * 3 + 1] = t.y;
        A.out[(size_t)i * 3 + 2] = t.z;
    } else {
        A.dst[i] = make_float4(c.x, c.y, c.z, __int_as_float(op));
        if constexpr (GUIDED) A.vdst[i] = sv / (sw * sw);
    }
}

// iterations = 0: the average, demodulated and remodulated, tone-mapped (with demodulate = 0 bit for bit post_process's image_pixels)
// LINEAR: as atrous_level's
template <bool LINEAR>
__global__ void __launch_bounds__(256) atrous_none(const DenoiseArgs A) {
    const uint32_t n = (uint32_t)A.width * (uint32_t)A.height;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 b = A.image_buffer[i];
    vec3 t;
    if (b.w > 0.0f) {
        const vec3 ac = A.demodulate ? albedo_clamped(A, i) : mk(1.0f, 1.0f, 1.0f);
        vec3 c = start_colour(b, ac, A.demodulate);
        if (A.demodulate) c = mk(c.x * ac.x, c.y * ac.y, c.z * ac.z);
        t = LINEAR ? c : tone_map(A.cfg, make_float4(c.x, c.y, c.z, 1.0f));
    } else {
        t = LINEAR ? mk(0.0f, 0.0f, 0.0f) : tone_map(A.cfg, b);
    }
    A.out[(size_t)i * 3 + 0] = t.x;
    A.out[(size_t)i * 3 + 1] = t.y;
    A.out[(size_t)i * 3 + 2] = t.z;
}

void launch_features(const Params& P, const FeatArgs& A, int kind, hipStream_t st) {
    const unsigned grid = (unsigned)(((size_t)P.cfg.width * P.cfg.height + 255) / 256);
    with_kind(kind, [&](auto K) { hipLaunchKernelGGL((feature_rays<K()>), dim3(grid), dim3(256), 0, st, P, A); });
}

bool launch_atrous_level(const DenoiseArgs& A, unsigned form, hipStream_t st) {
    const unsigned grid = (unsigned)(((size_t)A.width * A.height + 255) / 256);
    const bool first = (form & LEVEL_FIRST) != 0, last = (form & LEVEL_LAST) != 0;
    const bool linear = (form & ATROUS_LINEAR) != 0 && last;
    if (A.step == 0) {      // no level: the iterations = 0 pass
        if ((form & (ATROUS_COVER | ATROUS_FILL)) != 0) return false;
        with_bools([&](auto LN) { hipLaunchKernelGGL(atrous_none<LN()>, dim3(grid), dim3(256), 0, st, A); }, linear);
        return true;
    }
    return with_bools(
        [&](auto F, auto L, auto G, auto LN, auto C, auto FL) {
            constexpr bool ok = atrous_form_ok(F(), L(), G(), LN(), C(), FL());
            if constexpr (ok) hipLaunchKernelGGL((atrous_level<F(), L(), G(), LN(), C(), FL()>), dim3(grid), dim3(256), 0, st, A);
            return ok;
        },
        first, last, (form & ATROUS_GUIDED) != 0, linear, (form & ATROUS_COVER) != 0, (form & ATROUS_FILL) != 0);
}

}  // namespace rt
