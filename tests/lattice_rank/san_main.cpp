// Sanitizer driver of the lattice ranks (test infrastructure; nothing is loaded into Python for this):
//     g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all tests/lattice_rank/san_main.cpp -o lattice_san && ./lattice_san
// The enumeration of tests/test_lattice_rank.py: every frame of 1..20 x 1..20 pixels, every period 1..8 x 1..8, every phase, both
// orders.  The ranks go into an array of exactly nx * ny flags, so a rank outside [0, n) is an out-of-bounds write the sanitizer
// reports; a rank taken twice, a lattice pixel missed, a pixel off the lattice with a rank, and an ascending order that is not
// the order of the buffer indices are counted.  Exit 0 = none.
#include "lattice_rank.cpp"

#include <stdio.h>
#include <stdlib.h>

int main() {
    long long failures = 0, frames = 0;
    for (int W = 1; W <= 20; W++)
        for (int H = 1; H <= 20; H++) {
            uint32_t* ranks = (uint32_t*)malloc((size_t)W * H * sizeof(uint32_t));
            for (int px = 1; px <= 8; px++)
                for (int py = 1; py <= 8; py++)
                    for (int phx = 0; phx < px; phx++)
                        for (int phy = 0; phy < py; phy++)
                            for (int order = 0; order <= 1; order++) {
                                const long long n = lattice_ranks(order, W, H, px + 16 * py + 256 * phx + 4096 * phy, ranks);
                                long long want = 0;
                                for (int x = phx; x < W; x += px)
                                    for (int y = phy; y < H; y += py) want++;
                                if (n != want) {
                                    fprintf(stderr, "%dx%d (%d,%d)@(%d,%d): count %lld, walked %lld\n", W, H, px, py, phx, phy, n, want);
                                    failures++;
                                    continue;
                                }
                                unsigned char* seen = (unsigned char*)calloc((size_t)n, 1);
                                long long next = 0;
                                for (int i = 0; i < W * H; i++) {
                                    const bool on = (i / H) % px == phx && (i % H) % py == phy;
                                    if (on != (ranks[i] != LATTICE_NONE)) failures++;
                                    if (ranks[i] == LATTICE_NONE) continue;
                                    const unsigned char before = seen[ranks[i]];
                                    seen[ranks[i]] = 1;
                                    failures += before;
                                    if (order == 0 && ranks[i] != (uint32_t)next) failures++;
                                    next++;
                                }
                                if (next != n) failures++;
                                free(seen);
                                frames++;
                            }
            free(ranks);
        }
    // values that encode no lattice
    const long long bad[] = {-1, 0x10, 0x01, 0x91, 0x19, 0x222, 0x2022, 0x10022, 1LL << 40, -0x7fffffffffffffffLL - 1};
    uint32_t one = 0;
    for (long long v : bad)
        if (lattice_ranks(1, 1, 1, v, &one) != -1) failures++;
    printf("lattice ranks under the sanitizers: %lld selections, %lld failures\n", frames, failures);
    return failures != 0;
}
