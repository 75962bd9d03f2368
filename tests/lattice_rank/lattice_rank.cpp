// Test shim of raytracingpbr_amd/csrc/rt_lattice.hpp (test infrastructure): the header as the host compiler takes it, behind one C
// function.  tests/test_lattice_rank.py loads it; san_main.cpp includes it.
#include "../../raytracingpbr_amd/csrc/rt_lattice.hpp"

#define LATTICE_NONE 0xffffffffu

// Walks the frame as the kernel does, one buffer index i = x * H + y after the other: ranks[i] = the list position of pixel i in
// `order` (0 ascending, 1 tiled), LATTICE_NONE for a pixel that is not on the lattice `value` encodes (option select_lattice).
// Returns the closed-form count nx * ny, -1 for a value that is no lattice.
extern "C" __attribute__((visibility("default"))) long long lattice_ranks(int order, int width, int height, long long value, uint32_t* ranks) {
    rt::Lattice l;
    if (!rt::lattice_decode(value, &l)) return -1;
    rt::lattice_count(&l, width, height);
    for (uint32_t x = 0; x < (uint32_t)width; x++)
        for (uint32_t y = 0; y < (uint32_t)height; y++) {
            const bool on = x % (uint32_t)l.px == (uint32_t)l.phx && y % (uint32_t)l.py == (uint32_t)l.phy;
            ranks[x * (uint32_t)height + y] = on ? rt::lattice_rank(order, x / (uint32_t)l.px, y / (uint32_t)l.py, l.nx, l.ny) : LATTICE_NONE;
        }
    return (long long)l.nx * (long long)l.ny;
}
