// rt_select.hpp — the pixel selection of rtpbr_select_mask / rtpbr_select_noisy / rtpbr_select_error: RTPBR_BUF_SELECTION and the compacted,
// ordered list rtpbr_sample_selected traces.
//
//   select_mark_*       one lane per pixel along the contiguous index i = x * H + y: decide "selected" (the host mask's byte, or the
//                       rule of rtpbr_select_noisy or rtpbr_select_error: comparisons only), write the byte of RTPBR_BUF_SELECTION, and count per block of
//                       256 pixels — a wave64 ballot + popcount per wave, four LDS words, ONE plain store per block: no global atomics.
//   select_scan         one block: the exclusive prefix sum of the block counts in place (tiles of 256 with a carry: 8100 counts at
//                       1080p are 32 tiles), the total behind them.
//   select_scatter      one lane per pixel again: rank inside the wave from the ballot (mbcnt), the earlier waves' counts from LDS,
//                       the block's start from the scan: list[start + rank] = i.  Ascending i by construction, whatever the schedule.
// Only the total comes back to the host (4 bytes).
#pragma once
#include "rt_lattice.hpp"
#include "rt_types.hpp"

namespace rt {

enum { SELECT_MASK = 0, SELECT_NOISY = 1, SELECT_ERROR = 2 };      // the rule of select_mark

struct SelectArgs {
    const float4* image_buffer;   // noisy, error: pixels without samples are selected
    const float* noise;           // noisy: RTPBR_BUF_NOISE of the estimate just made; error: RTPBR_BUF_DENOISED_ERROR as it is
    const float4* half_a;         // error: RTPBR_BUF_HALF_BUFFER — pixels with an empty half are selected
    const uint8_t* host_mask;     // mask: the caller's bytes, uploaded (nonzero = selected); may be `mask` itself
    uint8_t* mask;                // out: RTPBR_BUF_SELECTION, 0 / 1
    uint32_t* blocks;             // n_blocks counts -> starts, then the total
    uint32_t* list;               // out: the selected buffer indices, ascending
    float threshold;
    int32_t dilate;               // 0..3: Chebyshev radius
    float min_samples;            // noisy, error: pixels with fewer samples are selected too (0 = off: no count is below it)
    int32_t width, height;
};

void launch_select(const SelectArgs& A, int rule, hipStream_t st);      // the three passes; A.blocks[n_blocks] = the list's length afterwards
inline uint32_t select_blocks(int w, int h) { return (uint32_t)(((size_t)w * (size_t)h + 255) / 256); }

// The tiered selection (option select_tiers = T > 1): every selected pixel carries a tier 0 .. T - 1 (include/rtpbr.h has the rule),
// RTPBR_BUF_SELECTION holds 1 + tier, and the list is ordered by tier, then by buffer index, so that "the pixels of tiers 0 .. t" is
// a prefix of it.
//   select_mark_tiered_*   select_mark's membership; the tier from the window MAXIMUM of the plane (the walk cannot stop at the
//                          first hit: from dilate 2 on the block stages its window in LDS, 2 d + 1 contiguous runs of the plane);
//                          a ballot + popcount per tier and wave, the block's T counts into blocks[t * nb + block]
//   select_scan            the same kernel over T * nb entries: tier-major starts, blocks[(t + 1) * nb] = L_t, the pixels of tiers
//                          0 .. t, blocks[T * nb] = the total
//   select_scatter_tiered  the rank among the wave's lanes of the SAME tier, earlier waves' counts of that tier from LDS
//   select_tier_counts     L_0 .. L_{T-1} gathered into blocks[T * nb + 1 ..]: one copy of 4 T bytes to the host
constexpr int SELECT_MAX_TIERS = 8;

struct SelectTierArgs {
    SelectArgs A;                          // blocks: room for select_tier_words() words
    int32_t tiers;                         // T, 2 .. SELECT_MAX_TIERS
    float bound[SELECT_MAX_TIERS - 1];     // noisy, error: bound[k - 1] = (float)max(1, select_batch >> k), k = 1 .. T - 1
};

void launch_select_tiered(const SelectTierArgs& S, int rule, hipStream_t st);      // the four passes; blocks[T * n_blocks + 1 + t] = L_t afterwards
inline size_t select_tier_words(int w, int h) { return (size_t)select_blocks(w, h) * SELECT_MAX_TIERS + 1 + SELECT_MAX_TIERS; }

// The lattice selection (option "select_lattice"): which pixels, how many and each one's list position are known in closed form
// (rt_lattice.hpp), so ONE kernel writes the plane and the list, nothing is counted or scanned, and nothing comes back to the host.
//   select_lattice_build   one lane per four pixels along i = x * H + y (one word of the plane); a lattice pixel also writes
//                          list[rank] = i, rank in the order RT_LATTICE_ORDER (rt_select.hip) names: ascending unless built otherwise
struct LatticeArgs {
    uint8_t* mask;      // out: RTPBR_BUF_SELECTION, 0 / 1
    uint32_t* list;     // out: the nx * ny lattice pixels' buffer indices
    Lattice l;
    int32_t width, height;
};

void launch_select_lattice(const LatticeArgs& A, hipStream_t st);

}  // namespace rt
