// rt_lattice.hpp — a lattice selection in closed form (option "select_lattice", include/rtpbr.h): the pixels with x % px == phx and
// y % py == phy, how many there are, and where each one stands in the list rtpbr_sample_selected traces.  Plain C++ without a HIP
// include, so that a host compiler takes it as it is (tests/lattice_rank): RT_LATTICE_HD is all that differs on the device.
//
// Lattice coordinates: the pixel (phx + a * px, phy + b * py) is (a, b), 0 <= a < nx, 0 <= b < ny.  Two orders of the list:
//   ascending   rank = a * ny + b: ascending buffer index x * H + y, what mark / scan / scatter make of the same mask.
//   tiled       lattice coordinates in tiles of 8 x 8: tile columns along x, within a column the tiles along y, within a tile
//               la * hb + lb.  A tile on the far edge has its true width wa = min(8, nx - 8 ta) and height hb = min(8, ny - 8 tb),
//               so rank = ta * 8 * ny + tb * 8 * wa + la * hb + lb: the wa * ny entries of a column are a run of their own, as are
//               the wa * hb of a tile in it, and the map is a bijection onto [0, nx * ny) whatever the frame size.  Every aligned
//               run of 64 entries inside full tiles is one 8 x 8 block of lattice pixels: a wave of a selected launch then traces
//               a square patch of the frame instead of a strip one pixel wide.
// The selected kernels read the list entry by entry and nothing else about its order, and a pixel's k-th sample is the same ray
// wherever the pixel stands in it: both orders give the same image, bit for bit.
#pragma once
#include <stdint.h>

#ifndef RT_LATTICE_HD
#ifdef __HIP__
#define RT_LATTICE_HD __attribute__((host)) __attribute__((device)) inline
#else
#define RT_LATTICE_HD inline
#endif
#endif

namespace rt {

enum { LATTICE_ASCENDING = 0, LATTICE_TILED = 1 };
constexpr int LATTICE_MAX_PERIOD = 8;

struct Lattice {
    int32_t px, py, phx, phy;      // 1 <= px, py <= 8, 0 <= phx < px, 0 <= phy < py
    uint32_t nx, ny;               // lattice pixels per axis in the frame it was counted for
};

// the value of option "select_lattice": px + 16 py + 256 phx + 4096 phy, no other bits.  false: not an encoding of a lattice.
RT_LATTICE_HD bool lattice_decode(long long value, Lattice* l) {
    if (value < 0 || value > 0xffff) return false;
    const int px = (int)(value & 15), py = (int)((value >> 4) & 15), phx = (int)((value >> 8) & 15), phy = (int)((value >> 12) & 15);
    if (px < 1 || px > LATTICE_MAX_PERIOD || py < 1 || py > LATTICE_MAX_PERIOD || phx >= px || phy >= py) return false;
    l->px = px;
    l->py = py;
    l->phx = phx;
    l->phy = phy;
    l->nx = l->ny = 0;
    return true;
}

// lattice pixels along one axis of `extent` pixels
RT_LATTICE_HD uint32_t lattice_axis_count(int extent, int period, int phase) {
    return phase < extent ? (uint32_t)((extent - phase + period - 1) / period) : 0u;
}

RT_LATTICE_HD void lattice_count(Lattice* l, int width, int height) {
    l->nx = lattice_axis_count(width, l->px, l->phx);
    l->ny = lattice_axis_count(height, l->py, l->phy);
}

// the list position of lattice pixel (a, b), a < nx, b < ny
RT_LATTICE_HD uint32_t lattice_rank(int order, uint32_t a, uint32_t b, uint32_t nx, uint32_t ny) {
    if (order == LATTICE_ASCENDING) return a * ny + b;
    const uint32_t ta = a >> 3, tb = b >> 3, la = a & 7u, lb = b & 7u;
    const uint32_t ra = nx - 8u * ta, rb = ny - 8u * tb;      // what is left of the lattice from this tile on: >= 1
    const uint32_t wa = ra < 8u ? ra : 8u, hb = rb < 8u ? rb : 8u;
    return ta * 8u * ny + tb * 8u * wa + la * hb + lb;
}

}  // namespace rt
