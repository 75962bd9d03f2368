// rt_present.hpp — the present stage (rtpbr_present): a display buffer in the field layout ((W,H,C) f32, y fastest, bottom-up)
// becomes a packed 8-bit frame ((H,W,3|4) u8, x fastest, top-down) in one kernel.
//
// The pass is a transpose: the source is contiguous along y, the destination along x.  One workgroup of 256 lanes (four waves)
// moves a tile of 64 x 64 pixels through LDS:
//   in    a wave takes every fourth column of the tile.  A column's stretch of 64 pixels is contiguous in the source: the
//         float3 fields are read as flat dwords (lane l takes dwords l, l + 64, l + 128 of the 192: three fully coalesced loads),
//         image_buffer as one float4 per lane (1 KiB per wave) that goes through tone_map.  Each value is quantised at once and
//         lands in LDS as a byte (float3) or a packed pixel (float4) of tile[x][y], one dword per pixel;
//   out   a wave takes every fourth row.  It reads tile[0..63][y] — stride PITCH = 65 dwords, so the 32 lanes of a ds_read_b32 group
//         hit 32 different banks — and stores the row's stretch of the frame: RGBA8 one dword per lane (256 B per wave and row),
//         RGB8 the 24-bit pixels funnelled into dwords (lane j builds bytes 4j .. 4j + 3 from two neighbouring pixels; 192 B per
//         wave and row).  An RGB8 row starts at byte 3 (r W + x0), which is dword-aligned for every row only when W % 4 == 0:
//         the stretch is stored as up to 3 head bytes, aligned dwords, up to 3 tail bytes, whatever W is.
// Partial tiles on either axis are predicated per lane (dwords of the stretch in, pixels / bytes of the row out).
// The arithmetic is fixed in include/rtpbr.h (rtpbr_present); tests/present_ref_lib.py restates it in numpy.
#pragma once
#include "rt_types.hpp"

namespace rt {

struct PresentArgs {
    rtpbr_config cfg;             // ACCUM: the tone map
    const float* src3;            // PIXELS / DENOISED: (W,H,3)
    const float4* src4;           // ACCUM: image_buffer
    uint8_t* out;                 // (H,W,C), row 0 = top
    int32_t width, height;
};

constexpr int PRESENT_TILE = 64;      // pixels per tile edge (both axes)

void launch_present(const PresentArgs& A, bool accum, bool rgba, bool dither, hipStream_t st);

}  // namespace rt
