// rt_half.hip — kernels of rtpbr_half_update / rtpbr_denoise_error / rtpbr_denoise_blend / rtpbr_denoise_blend_levels / rtpbr_blend_error / rtpbr_blend_error_display (see rt_half.hpp).
#include <hip/hip_runtime.h>

#include <type_traits>

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

// ---- the window kernels' shared pieces.  A block owns a tile of ERR_TX x ERR_TY pixels (x by y, y contiguous; thread t: ly = t %
// ERR_TY, so a wave runs along y) and stages what it sums of the tile and an R-pixel halo into LDS once: 4-byte planes of one pitch,
// the last of them the entry's object word.  An entry that is not valid (what "valid" asks is the kernel's) or lies outside the
// frame holds +0 in every value plane and an object word no pixel has (ERR_NOBODY; first hits are >= -1): the object compare of
// the tap loop is then the whole test, the loop has one fixed trip count per radius, and adding +0 for a skipped tap is the
// identity: to a non-negative sum, and to a signed one as well, since a sum that starts at +0 never becomes -0 (x + (-x) = +0 in
// round-to-nearest, +0 + -0 = +0).  The tile is noise_estimate_pooled<R>'s (16 x 16: the shape measured best there, DESIGN.md
// section 6f) and so is the planes' pitch.  Entries per pixel: (TX + 2R)(TY + 2R) / (TX TY) = 1.27 / 1.56 / 1.89.
constexpr int ERR_TX = 16, ERR_TY = 16;
constexpr int ERR_NOBODY = (int)0x80000000;
// the pitch in words: the four column runs a wave reads at once start 16 banks apart (ds_read_b32 serves two runs per group of 32 lanes over 32 banks)
constexpr int err_pitch(int hy) {
    int p = hy;
    while (p % 32 != 16) p++;
    return p;
}
template <int R>
struct Win {
    static constexpr int HX = ERR_TX + 2 * R, HY = ERR_TY + 2 * R, PITCH = err_pitch(HY), WORDS = HX * PITCH;      // (WORDS: one plane)
};

// staging: entry(slot, at) for every entry of the block's tile and halo, hy fastest (contiguous in memory); slot is the entry's
// word in a plane, at() its pixel index where at.inside() says that it lies in the frame (computed there, not per entry)
struct WinPixel {
    int xq, yq, W, H;
    RT_D bool inside() const { return xq >= 0 && xq < W && yq >= 0 && yq < H; }
    RT_D size_t operator()() const { return (size_t)xq * (size_t)H + (size_t)yq; }
};
template <int R, class F>
RT_D void win_for_each_entry(int x0, int y0, int W, int H, F entry) {
    constexpr int HY = Win<R>::HY;
    for (int t = (int)threadIdx.x; t < Win<R>::HX * HY; t += 256) {
        const int hx = t / HY, hy = t - hx * HY;
        const int xq = x0 - R + hx, yq = y0 - R + hy;
        entry(hx * Win<R>::PITCH + hy, WinPixel{xq, yq, W, H});
    }
}

// the lane's own entry, and tap(q, same) over its (2R+1)^2 window: same = the tap lies on the centre's object op.  ROWS_UNROLLED is
// the kernel's choice: with the rows a loop only one row's LDS reads are in flight
template <int R>
RT_D int win_centre(int lx, int ly) { return (lx + R) * Win<R>::PITCH + (ly + R); }
template <int R, bool ROWS_UNROLLED, class F>
RT_D void win_for_each_tap(int lx, int ly, const int* t_obj, int op, F tap) {
    constexpr int ROWS = ROWS_UNROLLED ? 2 * R + 1 : 1;
#pragma unroll ROWS
    for (int dy = -R; dy <= R; dy++) {
#pragma unroll
        for (int dx = -R; dx <= R; dx++) {
            const int q = (lx + R + dx) * Win<R>::PITCH + (ly + R + dy);
            tap(q, t_obj[q] == op);
        }
    }
}

// f of include/rtpbr.h, and e_q of half_error<R> and blend_error<R> from the two halves' luminance difference dl
RT_D float win_f(float cA, float cB) { return (cA * cB) / ((cA + cB) * (cA + cB)); }
RT_D float win_e(float dl, float cA, float cB) { return fmax_((dl * dl) * win_f(cA, cB), 0.0f); }      // (a NaN gives 0)

// The blend rule of half_blend<R> and level_blend.  An entry's three values from the luminances of the finer (l.0: the raw
// average, or level k - 1) and the coarser (l.k: the filter result, or level k) frame of either half and of the full frame: the
// regression's cross term a_q, q_q = (coarser - finer)^2 and x_q, the product of the halves' (coarser - finer), whose expectation
// is bias^2.
RT_D void blend_stage(float f, float lA0, float lB0, float lD0, float lAk, float lBk, float lDk, float& aq, float& qq, float& xx) {
    const float dA = lAk - lA0;
    const float dB = lBk - lB0;
    const float dp = lA0 - lB0;
    const float dd = dA - dB;
    const float dl = lDk - lD0;
    aq = (f * dp) * dd;
    qq = dl * dl;
    xx = dA * dB;
}
// ... and the weight t of the lane whose object is op, from the sums over its window.  (Rows stay a loop: with all (2R+1)^2 x 4
// LDS reads hoisted half_blend takes 103 / 199 VGPRs at R = 2 / 3 and runs at four / two waves per SIMD; a row at a time it takes
// 48 at every radius.)
template <int R>
RT_D float blend_weight(int lx, int ly, const float* t_a, const float* t_q, const float* t_x, const int* t_obj, int op, float z2) {
    float n = 0.0f, SC = 0.0f, SQ = 0.0f, SX = 0.0f, SXX = 0.0f;
    win_for_each_tap<R, false>(lx, ly, t_obj, op, [&](int q, bool same) {
        const float xq = same ? t_x[q] : 0.0f;
        n = n + (same ? 1.0f : 0.0f);
        SC = SC + (same ? t_a[q] : 0.0f);
        SQ = SQ + (same ? t_q[q] : 0.0f);
        SX = SX + xq;
        SXX = SXX + xq * xq;
    });
    float t = 1.0f;
    const float m1 = SX / n;
    const float v = fmax_(SXX / n - m1 * m1, 0.0f);
    if (m1 > 0.0f && (m1 * m1) * n > z2 * v) {
        t = -SC / SQ;
        if (!(t < 1.0f)) t = 1.0f;      // (a NaN gives 1)
        if (t < 0.0f) t = 0.0f;
    }
    return t;
}

// ---- the error kernel: two planes (e_q, object_q), 8 bytes per entry; valid = both halves have samples.  Both tap loops are
// unrolled (102 VGPRs and four waves per SIMD at R = 3).
// Traffic per staged entry: 24 bytes of the two filtered colours, the two count words of 16-byte texels, 4 bytes of object.
template <int R>
__global__ void __launch_bounds__(256) half_error(const ErrorArgs A) {
    __shared__ float t_e[Win<R>::WORDS];
    __shared__ int t_obj[Win<R>::WORDS];
    __shared__ uint32_t blk[3];
    if (threadIdx.x < 3) blk[threadIdx.x] = 0u;
    const int H = A.height, W = A.width;
    const int x0 = (int)blockIdx.x * ERR_TX, y0 = (int)blockIdx.y * ERR_TY;
    win_for_each_entry<R>(x0, y0, W, H, [&](int slot, WinPixel at) {
        float e = 0.0f;
        int oq = ERR_NOBODY;
        if (at.inside()) {
            const size_t q = at();
            const float cA = A.half_a[q].w, cB = A.half_b[q].w;
            if (cA > 0.0f && cB > 0.0f) {
                const float dl = nz_lum(mk(A.da[q * 3 + 0], A.da[q * 3 + 1], A.da[q * 3 + 2])) -
                                 nz_lum(mk(A.db[q * 3 + 0], A.db[q * 3 + 1], A.db[q * 3 + 2]));
                e = win_e(dl, cA, cB);
                oq = A.object[q];
            }
        }
        t_e[slot] = e;
        t_obj[slot] = oq;
    });
    __syncthreads();
    const int lx = (int)threadIdx.x / ERR_TY, ly = (int)threadIdx.x % ERR_TY;
    const int x = x0 + lx, y = y0 + ly;
    bool estimated = false;
    float err = 0.0f;
    if (x < W && y < H) {
        const int op = t_obj[win_centre<R>(lx, ly)];
        if (op != ERR_NOBODY) {
            estimated = true;
            float S = 0.0f, cn = 0.0f;
            win_for_each_tap<R, true>(lx, ly, t_obj, op, [&](int q, bool same) {
                S = S + (same ? t_e[q] : 0.0f);
                cn = cn + (same ? 1.0f : 0.0f);
            });
            err = sqrt_ieee_(S / cn);
        }
        A.error[(size_t)x * (size_t)H + (size_t)y] = err;
    }
    nz_stats(A.stats, A.threshold, blk, estimated, err, blockIdx.y * gridDim.x + blockIdx.x);
}

// ---- the blend kernel: four planes (a_q, q_q, x_q, object_q), 16 bytes per entry; valid = usable, both halves have min_half
// samples.  The lane that summed the window makes t, the blend and the tone map.
// Traffic per staged entry: the three 16-byte texels, 36 bytes of the three linear filtered colours, 4 bytes of object: 88 bytes
// against half_error's 36 (the count words there cost a whole texel each on the bus); per pixel 28 more (b and FD of the centre
// again, 16 written).
template <int R>
__global__ void __launch_bounds__(256) half_blend(const BlendArgs A) {
    __shared__ float t_a[Win<R>::WORDS];
    __shared__ float t_q[Win<R>::WORDS];
    __shared__ float t_x[Win<R>::WORDS];
    __shared__ int t_obj[Win<R>::WORDS];
    __shared__ uint32_t blk[3];
    if (threadIdx.x < 3) blk[threadIdx.x] = 0u;
    const int H = A.height, W = A.width;
    const int x0 = (int)blockIdx.x * ERR_TX, y0 = (int)blockIdx.y * ERR_TY;
    win_for_each_entry<R>(x0, y0, W, H, [&](int slot, WinPixel at) {
        float aq = 0.0f, qq = 0.0f, xx = 0.0f;
        int oq = ERR_NOBODY;
        if (at.inside()) {
            const size_t q = at();
            const float4 ha = A.half_a[q], hb = A.half_b[q];
            const float cA = ha.w, cB = hb.w;
            if (cA >= A.min_half && cB >= A.min_half) {
                const float4 b = A.image_buffer[q];
                const float f = win_f(cA, cB);
                const float lPA = nz_lum(mk(ha.x / ha.w, ha.y / ha.w, ha.z / ha.w));
                const float lPB = nz_lum(mk(hb.x / hb.w, hb.y / hb.w, hb.z / hb.w));
                const float lPb = nz_lum(mk(b.x / b.w, b.y / b.w, b.z / b.w));
                blend_stage(f, lPA, lPB, lPb, nz_lum(mk(A.fa[q * 3 + 0], A.fa[q * 3 + 1], A.fa[q * 3 + 2])),
                            nz_lum(mk(A.fb[q * 3 + 0], A.fb[q * 3 + 1], A.fb[q * 3 + 2])),
                            nz_lum(mk(A.fd[q * 3 + 0], A.fd[q * 3 + 1], A.fd[q * 3 + 2])), aq, qq, xx);
                oq = A.object[q];
            }
        }
        t_a[slot] = aq;
        t_q[slot] = qq;
        t_x[slot] = xx;
        t_obj[slot] = oq;
    });
    __syncthreads();
    const int lx = (int)threadIdx.x / ERR_TY, ly = (int)threadIdx.x % ERR_TY;
    const int x = x0 + lx, y = y0 + ly;
    bool usable = false;
    float t = 1.0f;
    if (x < W && y < H) {
        const int op = t_obj[win_centre<R>(lx, ly)];
        if (op != ERR_NOBODY) {
            usable = true;
            t = blend_weight<R>(lx, ly, t_a, t_q, t_x, t_obj, op, A.z2);
        }
        const size_t p = (size_t)x * (size_t)H + (size_t)y;
        const float4 b = A.image_buffer[p];
        vec3 d;
        if (b.w > 0.0f) {
            vec3 c = mk(A.fd[p * 3 + 0], A.fd[p * 3 + 1], A.fd[p * 3 + 2]);
            if (t != 1.0f) {
                const float u = 1.0f - t;
                c = mk(c.x + u * (b.x / b.w - c.x), c.y + u * (b.y / b.w - c.y), c.z + u * (b.z / b.w - c.z));
            }
            d = tone_map(A.cfg, make_float4(c.x, c.y, c.z, 1.0f));
        } else {      // no samples: what post_process shows
            d = tone_map(A.cfg, b);
        }
        A.weight[p] = t;
        A.out[p * 3 + 0] = d.x;
        A.out[p * 3 + 1] = d.y;
        A.out[p * 3 + 2] = d.z;
    }
    // pixels_above = usable pixels with t < 1 (1 - t > 0 exactly then), max_noise = the largest 1 - t
    nz_stats(A.stats, 0.0f, blk, usable, 1.0f - t, blockIdx.y * gridDim.x + blockIdx.x);
}

// ---- the level kernel of rtpbr_denoise_blend_levels: half_blend<R>'s four planes and rule, once per a-trous level k = 1..K, with
// the finer level k - 1 in the place of the raw average.  A level's record (colour, object word) is the filter with
// iterations = k before remodulation; level 0 (FIRST) is made from the (sum, count) buffers with atrous_none<LINEAR>'s operations.
// A usable entry has samples in all three buffers (cA >= m >= 1, cB >= m, b.w = cA + cB), so its six records are colours and not
// the NO_SAMPLES record.  After the window the lane updates its own pixel's running T (in `weight`), depth and linear colour (in
// `out`) in place: no other lane reads or writes them.  LAST tone-maps and makes the statistics.
// Traffic per staged entry: six 16-byte records (FIRST: three and the three 16-byte texels), the two count words, 4 bytes of
// object, 12 of albedo when demodulating: 108 to 120 bytes against half_blend's 88; per pixel two records and 20 bytes of running
// state both ways.
// ERR (rtpbr_blend_error): the lane also carries XA and XB, its T_k applied to either half's own ladder, in two float4 planes: the
// centre pixel's four half records are the only new loads (64 bytes, 32 of running state both ways; FIRST takes level 0 from the
// two texels).  LAST hands blend_error<R> what it stages — (lum XA, display lum XA, lum XB, display lum XB) in the first plane —
// and the slope s of the display luminance at the blended colour in the error plane, so the tone map runs per pixel and never per
// staged entry.  The instances without ERR keep their code.
// LIN (LAST only; option blend_coverage = 1): the last level stores the blended linear colour, +0 for a pixel without samples, in
// the place of the display colour — A.out is a private plane in these calls, and cover_resolve tone-maps from it.  With ERR the
// display colour is still computed, for the slope alone.  12 bytes written per pixel either way.
// FILL (LAST only; option blend_fill = 1, the chains ran atrous_level's filling form): a pixel without samples in image_buffer is
// never usable and its running state is nobody's; the last level shows it from level K's record of image_buffer's chain alone.  A
// colour there: the remodulated F_K, as every t_k = 1 would give (T = 1, depth K: the sums above).  NO_SAMPLES: what post_process
// shows, T = 1, depth 0.  A wave with such pixels adds their counts to its shard of A.fill, as atrous_level's last level does;
// LIN writes A.live beside the colour (1: samples or filled).  ERR: the slope of such a pixel stays 0 and its luminances are never
// read (blend_error<R> stages a pixel with samples in both halves).  No new load: the record and the texel are the centre's.
RT_D vec3 lv_albedo(const LevelsArgs& A, size_t i) {
    if (!A.demodulate) return mk(1.0f, 1.0f, 1.0f);
    return mk(fmax_(A.albedo[i * 3 + 0], 1e-3f), fmax_(A.albedo[i * 3 + 1], 1e-3f), fmax_(A.albedo[i * 3 + 2], 1e-3f));
}
// F_k of a record: remodulated as the last level does
RT_D vec3 lv_record(float4 r, vec3 ac, int demod) { return demod ? mk(r.x * ac.x, r.y * ac.y, r.z * ac.z) : mk(r.x, r.y, r.z); }
// F_0 of a (sum, count) texel: the average, demodulated and remodulated
RT_D vec3 lv_average(float4 b, vec3 ac, int demod) {
    vec3 c = mk(b.x / b.w, b.y / b.w, b.z / b.w);
    if (demod) {
        c = mk(c.x / ac.x, c.y / ac.y, c.z / ac.z);
        c = mk(c.x * ac.x, c.y * ac.y, c.z * ac.z);
    }
    return c;
}

// s of include/rtpbr.h: the slope of the display luminance at the linear colour c, whose display colour is d
RT_D float lv_slope(const rtpbr_config& cfg, vec3 c, vec3 d) {
    const float Y = nz_lum(c);
    if (!(Y > 0.0f)) return 0.0f;
    const vec3 d1 = tone_map(cfg, make_float4(1.0625f * c.x, 1.0625f * c.y, 1.0625f * c.z, 1.0f));
    return (nz_lum(d1) - nz_lum(d)) / (0.0625f * Y);
}
// what LAST leaves of XA and XB: (lum XA, display lum XA, lum XB, display lum XB)
RT_D float4 lv_lums(const rtpbr_config& cfg, vec3 xa, vec3 xb) {
    return make_float4(nz_lum(xa), nz_lum(tone_map(cfg, make_float4(xa.x, xa.y, xa.z, 1.0f))), nz_lum(xb),
                       nz_lum(tone_map(cfg, make_float4(xb.x, xb.y, xb.z, 1.0f))));
}

template <int R, bool FIRST, bool LAST, bool ERR = false, bool LIN = false, bool FILL = false>
__global__ void __launch_bounds__(256) level_blend(const std::conditional_t<FILL, LevelsFillArgs, LevelsArgs> A) {
    static_assert(level_blend_form_ok(FIRST, LAST, LIN, FILL), "no such form (rt_dispatch.hpp)");
    __shared__ float t_a[Win<R>::WORDS];
    __shared__ float t_q[Win<R>::WORDS];
    __shared__ float t_x[Win<R>::WORDS];
    __shared__ int t_obj[Win<R>::WORDS];
    __shared__ uint32_t blk[3];
    if constexpr (LAST)
        if (threadIdx.x < 3) blk[threadIdx.x] = 0u;
    const int H = A.height, W = A.width;
    const int x0 = (int)blockIdx.x * ERR_TX, y0 = (int)blockIdx.y * ERR_TY;
    win_for_each_entry<R>(x0, y0, W, H, [&](int slot, WinPixel at) {
        float aq = 0.0f, qq = 0.0f, xx = 0.0f;
        int oq = ERR_NOBODY;
        if (at.inside()) {
            const size_t q = at();
            const float cA = A.half_a[q].w, cB = A.half_b[q].w;
            if (cA >= A.min_half && cB >= A.min_half) {
                const vec3 ac = lv_albedo(A, q);
                const float f = win_f(cA, cB);
                float lA0, lB0, lD0;      // the finer level
                if constexpr (FIRST) {
                    lA0 = nz_lum(lv_average(A.half_a[q], ac, A.demodulate));
                    lB0 = nz_lum(lv_average(A.half_b[q], ac, A.demodulate));
                    lD0 = nz_lum(lv_average(A.image_buffer[q], ac, A.demodulate));
                } else {
                    lA0 = nz_lum(lv_record(A.pa[q], ac, A.demodulate));
                    lB0 = nz_lum(lv_record(A.pb[q], ac, A.demodulate));
                    lD0 = nz_lum(lv_record(A.pd[q], ac, A.demodulate));
                }
                blend_stage(f, lA0, lB0, lD0, nz_lum(lv_record(A.ka[q], ac, A.demodulate)), nz_lum(lv_record(A.kb[q], ac, A.demodulate)),
                            nz_lum(lv_record(A.kd[q], ac, A.demodulate)), aq, qq, xx);
                oq = A.object[q];
            }
        }
        t_a[slot] = aq;
        t_q[slot] = qq;
        t_x[slot] = xx;
        t_obj[slot] = oq;
    });
    __syncthreads();
    const int lx = (int)threadIdx.x / ERR_TY, ly = (int)threadIdx.x % ERR_TY;
    const int x = x0 + lx, y = y0 + ly;
    bool usable = false;
    bool filled = false, empty = false;      // FILL: a pixel without samples that level K's record gives a colour / does not
    float T = 1.0f;
    if (x < W && y < H) {
        float t = 1.0f;
        const int op = t_obj[win_centre<R>(lx, ly)];
        if (op != ERR_NOBODY) {
            usable = true;
            t = blend_weight<R>(lx, ly, t_a, t_q, t_x, t_obj, op, A.z2);
        }
        const size_t p = (size_t)x * (size_t)H + (size_t)y;
        const vec3 ac = lv_albedo(A, p);
        const float4 rk = A.kd[p];
        const vec3 fk = lv_record(rk, ac, A.demodulate);
        float4 b = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if constexpr (FIRST || LAST) b = A.image_buffer[p];
        vec3 f0, c;
        float depth;
        if constexpr (FIRST) {      // T_0 = 1, depth = 0, c = FD_0
            f0 = lv_average(b, ac, A.demodulate);
            c = f0;
            depth = 0.0f;
        } else {
            f0 = lv_record(A.pd[p], ac, A.demodulate);
            c = mk(A.out[p * 3 + 0], A.out[p * 3 + 1], A.out[p * 3 + 2]);
            depth = A.depth[p];
            T = A.weight[p];
        }
        T = T * t;
        depth = depth + T;
        c = mk(c.x + T * (fk.x - f0.x), c.y + T * (fk.y - f0.y), c.z + T * (fk.z - f0.z));
        vec3 xa, xb;
        if constexpr (ERR) {      // the same T_k on either half's own ladder (a half without samples: its values are never read)
            const vec3 ak = lv_record(A.ka[p], ac, A.demodulate), bk = lv_record(A.kb[p], ac, A.demodulate);
            vec3 a0, b0;
            if constexpr (FIRST) {
                a0 = lv_average(A.half_a[p], ac, A.demodulate);
                b0 = lv_average(A.half_b[p], ac, A.demodulate);
                xa = a0;
                xb = b0;
            } else {
                a0 = lv_record(A.pa[p], ac, A.demodulate);
                b0 = lv_record(A.pb[p], ac, A.demodulate);
                const float4 va = A.xa[p], vb = A.xb[p];
                xa = mk(va.x, va.y, va.z);
                xb = mk(vb.x, vb.y, vb.z);
            }
            xa = mk(xa.x + T * (ak.x - a0.x), xa.y + T * (ak.y - a0.y), xa.z + T * (ak.z - a0.z));
            xb = mk(xb.x + T * (bk.x - b0.x), xb.y + T * (bk.y - b0.y), xb.z + T * (bk.z - b0.z));
            if constexpr (LAST) {
                if (T == 1.0f) {
                    xa = ak;
                    xb = bk;
                }
            } else {
                A.xa[p] = make_float4(xa.x, xa.y, xa.z, 0.0f);
                A.xb[p] = make_float4(xb.x, xb.y, xb.z, 0.0f);
            }
        }
        if constexpr (LAST) {
            if (T == 1.0f) c = fk;      // every t_k was 1: rtpbr_denoise's bytes
            // (no samples: what post_process shows; T = 1 and depth = K by the sums above)
            bool coloured = b.w > 0.0f;
            if constexpr (FILL) {
                if (!coloured) {
                    filled = __float_as_int(rk.w) != NO_SAMPLES;
                    empty = !filled;
                    coloured = filled;
                    T = 1.0f;
                    c = fk;
                    if (empty) depth = 0.0f;
                }
            }
            const vec3 lin = c;
            if constexpr (!LIN || ERR) c = coloured ? tone_map(A.cfg, make_float4(c.x, c.y, c.z, 1.0f)) : tone_map(A.cfg, b);
            if constexpr (ERR) {
                A.xa[p] = lv_lums(A.cfg, xa, xb);
                A.slope[p] = b.w > 0.0f ? lv_slope(A.cfg, lin, c) : 0.0f;
            }
            if constexpr (LIN) c = coloured ? lin : mk(0.0f, 0.0f, 0.0f);
            if constexpr (LIN && FILL) A.live[p] = coloured ? 1 : 0;
        }
        A.weight[p] = T;
        A.depth[p] = depth;
        A.out[p * 3 + 0] = c.x;
        A.out[p * 3 + 1] = c.y;
        A.out[p * 3 + 2] = c.z;
    }
    // pixels_above = usable pixels with T_K < 1 (1 - T_K > 0 exactly then), max_noise = the largest 1 - T_K
    if constexpr (LAST) nz_stats(A.stats, 0.0f, blk, usable, 1.0f - T, blockIdx.y * gridDim.x + blockIdx.x);
    if constexpr (FILL) {      // (every lane of the block arrives here; a lane outside the frame reports nothing)
        const uint32_t wave = (blockIdx.y * gridDim.x + blockIdx.x) * 4u + (threadIdx.x >> 6);
        uint32_t* const shard = A.fill + (wave % (uint32_t)FILL_SHARDS) * (uint32_t)FILL_SHARD_WORDS;
        const unsigned long long mf = __ballot(filled), me = __ballot(empty);
        if ((threadIdx.x & 63) == 0 && mf != 0) atomicAdd(shard, (uint32_t)__popcll(mf));
        if ((threadIdx.x & 63) == 0 && me != 0) atomicAdd(shard + 1, (uint32_t)__popcll(me));
    }
}

// K = 0 of rtpbr_denoise_blend_levels (the frame is atrous_none's): weight 1, depth 0, and the count of usable pixels.  ERR: XA,
// XB and the blended colour are level 0 of the three buffers.
template <bool ERR = false>
__global__ void __launch_bounds__(256) level_blend_none(const LevelsArgs A) {
    __shared__ uint32_t blk[3];
    if (threadIdx.x < 3) blk[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t n = (uint32_t)A.width * (uint32_t)A.height;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool usable = false;
    if (i < n) {
        usable = A.half_a[i].w >= A.min_half && A.half_b[i].w >= A.min_half;
        A.weight[i] = 1.0f;
        A.depth[i] = 0.0f;
        if constexpr (ERR) {
            const vec3 ac = lv_albedo(A, i);
            const float4 b = A.image_buffer[i];
            A.xa[i] = lv_lums(A.cfg, lv_average(A.half_a[i], ac, A.demodulate), lv_average(A.half_b[i], ac, A.demodulate));
            float s = 0.0f;
            if (b.w > 0.0f) {
                const vec3 c = lv_average(b, ac, A.demodulate);
                s = lv_slope(A.cfg, c, tone_map(A.cfg, make_float4(c.x, c.y, c.z, 1.0f)));
            }
            A.slope[i] = s;
        }
    }
    nz_stats(A.stats, 0.0f, blk, usable, 0.0f, blockIdx.x);
}

// ---- the window kernel of rtpbr_blend_error: four planes (e_q, x_q, usable_q, object_q), 16 bytes per entry; valid as in
// half_error<R>, and a valid entry that is not usable (half_blend<R>'s test) holds x = +0 and usable = 0, so adding +0 covers an
// unusable tap too.  The centre lane reads its slope s from the error plane (level_blend's LAST ERR instance wrote it) and
// overwrites it with the error: no other lane reads or writes that word.
// LDS: 4 planes = 13.8 / 15.4 / 16.9 KB at R = 1 / 2 / 3 (the pitch is 48 words at every radius; half_blend<R>'s footprint: eight
// blocks of four waves still fit a CU's 160 KB), rows a loop as there.
// Traffic per staged entry: the 16-byte texel of luminances, the two 16-byte texels of the halves (count words and, where usable,
// the raw averages), 4 bytes of object: 52 bytes against half_error's 36 + its two filtered colours; per pixel 4 read, 4 written.
// DISPLAY (rtpbr_blend_error_display): the bias in display space per tap.  A usable entry stages xd_q = (s_q * s_q) * x_q with its
// own slope — s * s once per staged entry, never per tap — and the centre adds the window's mean as it is.  A halo entry's s_q is
// the slope of a pixel that another block owns and may already have overwritten with its error, so for this call level_blend's
// LAST ERR instance (the same code, another pointer) leaves s in a plane of its own that no window kernel writes.  Traffic: +4
// bytes per usable staged entry (56 against 52), and the centre's 4-byte read goes.  LDS, the tap loop and the rows are the same.
template <int R, bool DISPLAY = false>
__global__ void __launch_bounds__(256) blend_error(const BlendErrorArgs A) {
    __shared__ float t_e[Win<R>::WORDS];
    __shared__ float t_x[Win<R>::WORDS];
    __shared__ float t_u[Win<R>::WORDS];
    __shared__ int t_obj[Win<R>::WORDS];
    __shared__ uint32_t blk[3];
    if (threadIdx.x < 3) blk[threadIdx.x] = 0u;
    const int H = A.height, W = A.width;
    const int x0 = (int)blockIdx.x * ERR_TX, y0 = (int)blockIdx.y * ERR_TY;
    win_for_each_entry<R>(x0, y0, W, H, [&](int slot, WinPixel at) {
        float e = 0.0f, xx = 0.0f, u = 0.0f;
        int oq = ERR_NOBODY;
        if (at.inside()) {
            const size_t q = at();
            const float4 ha = A.half_a[q], hb = A.half_b[q];
            const float cA = ha.w, cB = hb.w;
            if (cA > 0.0f && cB > 0.0f) {
                const float4 l = A.lx[q];
                e = win_e(l.y - l.w, cA, cB);
                if (cA >= A.min_half && cB >= A.min_half) {
                    const float lPA = nz_lum(mk(ha.x / ha.w, ha.y / ha.w, ha.z / ha.w));
                    const float lPB = nz_lum(mk(hb.x / hb.w, hb.y / hb.w, hb.z / hb.w));
                    xx = (l.x - lPA) * (l.z - lPB);
                    if constexpr (DISPLAY) {
                        const float s = A.slope[q];
                        xx = (s * s) * xx;
                    }
                    u = 1.0f;
                }
                oq = A.object[q];
            }
        }
        t_e[slot] = e;
        t_x[slot] = xx;
        t_u[slot] = u;
        t_obj[slot] = oq;
    });
    __syncthreads();
    const int lx = (int)threadIdx.x / ERR_TY, ly = (int)threadIdx.x % ERR_TY;
    const int x = x0 + lx, y = y0 + ly;
    bool estimated = false;
    float err = 0.0f;
    if (x < W && y < H) {
        const int op = t_obj[win_centre<R>(lx, ly)];
        const size_t p = (size_t)x * (size_t)H + (size_t)y;
        if (op != ERR_NOBODY) {
            estimated = true;
            float S = 0.0f, cn = 0.0f, SX = 0.0f, nb = 0.0f;
            win_for_each_tap<R, false>(lx, ly, t_obj, op, [&](int q, bool same) {
                S = S + (same ? t_e[q] : 0.0f);
                cn = cn + (same ? 1.0f : 0.0f);
                SX = SX + (same ? t_x[q] : 0.0f);
                nb = nb + (same ? t_u[q] : 0.0f);
            });
            const float bias2 = nb > 0.0f ? fmax_(SX / nb, 0.0f) : 0.0f;      // (a NaN gives 0)
            if constexpr (DISPLAY) {
                err = sqrt_ieee_(S / cn + bias2);
            } else {
                const float s = A.error[p];
                err = sqrt_ieee_(S / cn + (s * s) * bias2);
            }
        }
        A.error[p] = err;
    }
    nz_stats(A.stats, A.threshold, blk, estimated, err, blockIdx.y * gridDim.x + blockIdx.x);
}

static unsigned grid_of(int w, int h) { return (unsigned)(((size_t)w * h + 255) / 256); }
static dim3 tile_grid(int w, int h) { return dim3((unsigned)((w + ERR_TX - 1) / ERR_TX), (unsigned)((h + ERR_TY - 1) / ERR_TY)); }

void launch_half_update(const HalfArgs& A, hipStream_t st) {
    hipLaunchKernelGGL(half_update, dim3(grid_of(A.width, A.height)), dim3(256), 0, st, A);
}

void launch_half_subtract(const HalfArgs& A, hipStream_t st) {
    hipLaunchKernelGGL(half_subtract, dim3(grid_of(A.width, A.height)), dim3(256), 0, st, A);
}

void launch_half_error(const ErrorArgs& A, hipStream_t st) {
    with_radius(A.radius, [&](auto R) { hipLaunchKernelGGL(half_error<R()>, tile_grid(A.width, A.height), dim3(256), 0, st, A); });
}

void launch_half_blend(const BlendArgs& A, hipStream_t st) {
    with_radius(A.radius, [&](auto R) { hipLaunchKernelGGL(half_blend<R()>, tile_grid(A.width, A.height), dim3(256), 0, st, A); });
}

// no level (no records): the K = 0 pass.  A.xa (rtpbr_blend_error): the ERR instances.  BLEND_LIN (with a last level only): the LIN
// instances.  fill (with a last level only): the FILL instances, which take LevelsFillArgs
bool launch_level_blend(const LevelsArgs& A, unsigned form, hipStream_t st, uint32_t* fill, uint8_t* live) {
    const bool err = A.xa != nullptr;
    if (!A.kd) {
        with_bools([&](auto E) { hipLaunchKernelGGL(level_blend_none<E()>, dim3(grid_of(A.width, A.height)), dim3(256), 0, st, A); }, err);
        return true;
    }
    const bool first = (form & LEVEL_FIRST) != 0, last = (form & LEVEL_LAST) != 0;
    LevelsFillArgs B{};
    static_cast<LevelsArgs&>(B) = A;
    B.fill = fill;
    B.live = live;
    return with_radius(A.radius, [&](auto radius) {
        constexpr int R = radius();
        return with_bools(
            [&](auto F, auto L, auto E, auto LN, auto FL) {
                constexpr bool ok = level_blend_form_ok(F(), L(), LN(), FL());
                if constexpr (ok && FL()) hipLaunchKernelGGL((level_blend<R, F(), L(), E(), LN(), true>), tile_grid(A.width, A.height), dim3(256), 0, st, B);
                else if constexpr (ok) hipLaunchKernelGGL((level_blend<R, F(), L(), E(), LN(), false>), tile_grid(A.width, A.height), dim3(256), 0, st, A);
                return ok;
            },
            first, last, err, (form & BLEND_LIN) != 0 && last, fill != nullptr && last);
    });
}

// A.slope != nullptr (rtpbr_blend_error_display): the DISPLAY instances
void launch_blend_error(const BlendErrorArgs& A, hipStream_t st) {
    with_radius(A.radius, [&](auto radius) {
        constexpr int R = radius();
        with_bools([&](auto D) { hipLaunchKernelGGL((blend_error<R, D()>), tile_grid(A.width, A.height), dim3(256), 0, st, A); }, A.slope != nullptr);
    });
}

}  // namespace rt
