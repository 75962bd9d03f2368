/* Sanitizer driver of the blend_fill restatement (test infrastructure; nothing is loaded into Python for this):
 *     gcc -O1 -g -std=gnu11 -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -fopenmp \
 *         tests/blend_fill_ref/san_main.c -o blend_fill_san -lm && ./blend_fill_san
 * The 24x16 two-object frame of tests/test_blend_fill_ref.py (flat features, power-of-two radiances, coverage set by hand) with
 * holes in the interior, on either side of the silhouette and a 5x5 block, and then with object 1 left without any sample, through
 * bf_fill_levels (plain and coverage-weighted) and the three modes of bf_blend_fill at 1 and 3 levels, radius 1..3, both resolve
 * settings; then a hostile 7x5 frame (special values in count and colour words) through the same calls.  Exit 0 = the calls returned 0
 * and the counts are the expected ones. */
#include "blend_fill_ref.c"

#include <float.h>
#include <stdio.h>

enum { W0 = 24, H0 = 16, N0 = W0 * H0 };

int main(void) {
    static const float L[2][3] = {{0.5f, 0.25f, 1.0f}, {2.0f, 1.0f, 0.5f}};
    rtpbr_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.width = W0;
    cfg.height = H0;
    cfg.tonemap_order = RTPBR_TONEMAP_GAMMA_ACES_CLAMP;
    cfg.exposure = 1.0f;
    cfg.gamma = 2.2f;
    float *albedo = malloc(N0 * 3 * 4), *normal = malloc(N0 * 3 * 4), *depth = malloc(N0 * 4), *ib = malloc(N0 * 16), *ha = malloc(N0 * 16),
          *hb = malloc(N0 * 16);
    int32_t *object = malloc(N0 * 4), *cov = malloc(N0 * 16);
    float *out = malloc(N0 * 12), *before = malloc(N0 * 12), *weight = malloc(N0 * 4), *dep = malloc(N0 * 4), *error = malloc(N0 * 4),
          *parts = malloc(N0 * 12);
    int failures = 0;
    for (int scene = 0; scene <= 1; scene++) {      /* 0: holes that can be filled; 1: object 1 has no sample at all */
        uint32_t holes = 0, gone = 0;
        for (int x = 0; x < W0; x++)
            for (int y = 0; y < H0; y++) {
                const int i = x * H0 + y, o = x >= W0 / 2;
                int hole = (x == W0 / 2 - 1 && y == 5) || (x == W0 / 2 && (y == 9 || y == 10)) || (x >= 2 && x < 7 && y >= 3 && y < 8);
                if (scene == 1 && o) { hole = 1; gone++; }
                else holes += hole;
                const int border = x == W0 / 2 - 1 || x == W0 / 2;
                object[i] = o;
                depth[i] = 3.0f;
                for (int c = 0; c < 3; c++) {
                    albedo[i * 3 + c] = 0.5f;
                    normal[i * 3 + c] = c == 2 ? 1.0f : 0.0f;
                    ib[i * 4 + c] = hole ? 0.0f : L[o][c] * 8.0f;
                }
                ib[i * 4 + 3] = hole ? 0.0f : 8.0f;
                cov[i * 4 + 0] = border ? 12 : 16;
                cov[i * 4 + 1] = border ? 1 - o : -2;
                cov[i * 4 + 2] = border ? 4 : 0;
                cov[i * 4 + 3] = 16;
            }
        for (int i = 0; i < N0 * 4; i++) {
            ha[i] = ib[i] * 0.5f;
            hb[i] = ib[i] - ha[i];
        }
        for (int K = 1; K <= 3; K += 2)
            for (int demodulate = 0; demodulate <= 1; demodulate++)
                for (int cover = 0; cover <= 1; cover++) {
                    float* f[3];
                    unsigned char* live[3];
                    const float* in[3] = {ib, ha, hb};
                    uint32_t counts[3] = {9, 9, 9};
                    for (int j = 0; j < 3; j++) {
                        f[j] = malloc((size_t)(K + 1) * N0 * 12);
                        live[j] = malloc((size_t)(K + 1) * N0);
                        if (bf_fill_levels(&cfg, in[j], albedo, normal, depth, object, cover ? cov : NULL, K, demodulate, 2.0f, 0.3f, 0.2f, 0.1f, 4,
                                           f[j], live[j], j == 0 ? counts : NULL))
                            failures++;
                    }
                    /* one level leaves the centre of the 5x5 block; object 1 stays empty whatever K is */
                    const uint32_t want_empty = gone + (K == 1 ? 1u : 0u);
                    if (counts[0] != holes - (K == 1 ? 1u : 0u) || counts[1] != want_empty || counts[2] != (K == 1 ? 0u : 1u)) {
                        fprintf(stderr, "scene %d K %d cover %d: counts %u %u %u\n", scene, K, cover, counts[0], counts[1], counts[2]);
                        failures++;
                    }
                    for (int mode = 0; mode <= 2; mode++)
                        for (int radius = 1; radius <= 3; radius++)
                            for (int resolve = 0; resolve <= 1; resolve++) {
                                uint32_t stats[3], resolved = 99999;
                                if (bf_blend_fill(&cfg, ib, ha, hb, f[0], f[1], f[2], live[0] + (size_t)K * N0, object, cover ? cov : NULL, K, radius,
                                                  radius == 2 ? 4.0f : 0.0f, 4.0f, 4, resolve, mode, 4 - radius, 0.01f, out, before, weight, dep,
                                                  error, parts, stats, &resolved))
                                    failures++;
                                /* every border pixel has a colour in scene 0 (filled ones included); in scene 1 object 0's border
                                 * column has no neighbour with a colour on object 1 */
                                const uint32_t want = cover && resolve && scene == 0 ? 2u * H0 : 0u;
                                if (resolved != want) {
                                    fprintf(stderr, "scene %d K %d cover %d mode %d radius %d resolve %d: resolved %u\n", scene, K, cover, mode, radius,
                                            resolve, resolved);
                                    failures++;
                                }
                            }
                    for (int j = 0; j < 3; j++) { free(f[j]); free(live[j]); }
                }
    }
    /* a hostile 7x5 frame (tests/hostile.py's words, by hand): NaN, +-inf, FLT_MAX, -0, -3, 2^-149, 2^24 and 1e30 in count words, NaN,
     * +-inf, the pole -1 and -100 in colour words; two objects, the border columns with coverage 12 of 16.  The arrays above are
     * larger than it needs.  Only the return codes are judged: the sanitizers judge the rest. */
    {
        enum { W1 = 7, H1 = 5, N1 = W1 * H1 };
        static const float counts_w[] = {4.0f, NAN, 4.0f, INFINITY, -0.0f, 4.0f, -3.0f, 1.401298464e-45f, 4.0f, 16777216.0f, 1e30f, 0.0f,
                                         -INFINITY, FLT_MAX};
        static const float colour_w[] = {2.0f, 1.0f, NAN, 0.5f, INFINITY, 4.0f, -4.0f, 8.0f, -INFINITY, -400.0f, FLT_MAX, 0.25f};
        cfg.width = W1;
        cfg.height = H1;
        for (int x = 0; x < W1; x++)
            for (int y = 0; y < H1; y++) {
                const int i = x * H1 + y, o = x >= 4, border = x == 3 || x == 4;
                object[i] = o;
                depth[i] = 3.0f;
                for (int c = 0; c < 3; c++) {
                    albedo[i * 3 + c] = 0.5f;
                    normal[i * 3 + c] = c == 2 ? 1.0f : 0.0f;
                    ib[i * 4 + c] = colour_w[(i * 3 + c) % (int)(sizeof colour_w / sizeof *colour_w)];
                }
                ib[i * 4 + 3] = counts_w[i % (int)(sizeof counts_w / sizeof *counts_w)];
                cov[i * 4 + 0] = border ? 12 : 16;
                cov[i * 4 + 1] = border ? 1 - o : -2;
                cov[i * 4 + 2] = border ? 4 : 0;
                cov[i * 4 + 3] = 16;
            }
        for (int i = 0; i < N1 * 4; i++) {
            ha[i] = ib[i] * 0.5f;
            hb[i] = ib[i] - ha[i];
        }
        for (int K = 1; K <= 4; K += 3)
            for (int demodulate = 0; demodulate <= 1; demodulate++)
                for (int cover = 0; cover <= 1; cover++) {
                    float* f[3];
                    unsigned char* live[3];
                    const float* in[3] = {ib, ha, hb};
                    uint32_t counts[3];
                    for (int j = 0; j < 3; j++) {
                        f[j] = malloc((size_t)(K + 1) * N1 * 12);
                        live[j] = malloc((size_t)(K + 1) * N1);
                        if (bf_fill_levels(&cfg, in[j], albedo, normal, depth, object, cover ? cov : NULL, K, demodulate, 0.5f, 0.3f, 0.05f, 0.1f, 4,
                                           f[j], live[j], j == 0 ? counts : NULL))
                            failures++;
                    }
                    for (int mode = 0; mode <= 2; mode++)
                        for (int radius = 1; radius <= 3; radius++) {
                            uint32_t stats[3], resolved;
                            if (bf_blend_fill(&cfg, ib, ha, hb, f[0], f[1], f[2], live[0] + (size_t)K * N1, object, cover ? cov : NULL, K, radius,
                                              radius == 2 ? 2.0f : 0.0f, 1.0f, 4, 1, mode, 4 - radius, 0.05f, out, before, weight, dep, error,
                                              parts, stats, &resolved))
                                failures++;
                        }
                    for (int j = 0; j < 3; j++) { free(f[j]); free(live[j]); }
                }
    }
    free(albedo); free(normal); free(depth); free(ib); free(ha); free(hb); free(object); free(cov);
    free(out); free(before); free(weight); free(dep); free(error); free(parts);
    printf("blend_fill_ref under the sanitizers: %d failures\n", failures);
    return failures != 0;
}
