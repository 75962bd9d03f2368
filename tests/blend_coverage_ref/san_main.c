/* Sanitizer driver of the blend_coverage restatement (test infrastructure; nothing is loaded into Python for this):
 *     gcc -O1 -g -std=gnu11 -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -fopenmp \
 *         tests/blend_coverage_ref/san_main.c -o blend_coverage_san -lm && ./blend_coverage_san
 * The 24x16 two-object frame of tests/test_blend_coverage_ref.py (flat features, power-of-two radiances, coverage set by hand) with
 * holes in the interior and on either side of the silhouette and one pixel of share 0, through bc_filter_levels and the three
 * modes of bc_blend_coverage at 1 and 3 levels, radius 1..3, both resolve settings; then a hostile 7x5 frame (special values in
 * count and colour words) through the same calls.  Exit 0 = the calls returned 0 and the resolved counts are the expected ones. */
#include "blend_coverage_ref.c"

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
    int failures = 0;
    for (int x = 0; x < W0; x++)
        for (int y = 0; y < H0; y++) {
            const int i = x * H0 + y, o = x >= W0 / 2;
            const int hole = (x == W0 / 2 - 1 && y == 5) || (x == W0 / 2 && (y == 9 || y == 10)) || (x >= 3 && x < 5 && y >= 3 && y < 6);
            const int border = x == W0 / 2 - 1 || x == W0 / 2;
            object[i] = o;
            depth[i] = 3.0f;
            for (int c = 0; c < 3; c++) {
                albedo[i * 3 + c] = 0.5f;
                normal[i * 3 + c] = c == 2 ? 1.0f : 0.0f;
                ib[i * 4 + c] = hole ? 0.0f : L[o][c] * 32.0f;
            }
            ib[i * 4 + 3] = hole ? 0.0f : 32.0f;
            cov[i * 4 + 0] = border ? 12 : 16;
            cov[i * 4 + 1] = border ? 1 - o : -2;
            cov[i * 4 + 2] = border ? 4 : 0;
            cov[i * 4 + 3] = 16;
        }
    {      /* a pixel of share 0 with another radiance */
        const int i = 8 * H0 + 12;
        cov[i * 4 + 0] = 0; cov[i * 4 + 1] = 1; cov[i * 4 + 2] = 16;
        for (int c = 0; c < 3; c++) ib[i * 4 + c] = 8.0f * 32.0f;
    }
    for (int i = 0; i < N0 * 4; i++) {
        ha[i] = ib[i] * 0.5f;
        hb[i] = ib[i] - ha[i];
    }
    float *out = malloc(N0 * 12), *before = malloc(N0 * 12), *weight = malloc(N0 * 4), *dep = malloc(N0 * 4), *error = malloc(N0 * 4),
          *parts = malloc(N0 * 12);
    for (int K = 1; K <= 3; K += 2)
        for (int demodulate = 0; demodulate <= 1; demodulate++)
            for (int power = 0; power <= 8; power += 4) {
                float* f[3];
                const float* in[3] = {ib, ha, hb};
                for (int j = 0; j < 3; j++) {
                    f[j] = malloc((size_t)(K + 1) * N0 * 12);
                    if (bc_filter_levels(&cfg, in[j], albedo, normal, depth, object, cov, K, demodulate, 2.0f, 0.3f, 0.2f, 0.1f, power, f[j])) failures++;
                }
                for (int mode = 0; mode <= 2; mode++)
                    for (int radius = 1; radius <= 3; radius++)
                        for (int resolve = 0; resolve <= 1; resolve++) {
                            uint32_t stats[3], resolved = 99999;
                            if (bc_blend_coverage(&cfg, ib, ha, hb, f[0], f[1], f[2], object, cov, K, radius, radius == 2 ? 4.0f : 0.0f, 16.0f, power,
                                                  resolve, mode, 4 - radius, 0.01f, out, before, weight, dep, error, parts, stats, &resolved))
                                failures++;
                            if (resolved != (resolve ? 2u * H0 - 3u : 0u)) {
                                fprintf(stderr, "K %d power %d mode %d radius %d resolve %d: resolved %u\n", K, power, mode, radius, resolve, resolved);
                                failures++;
                            }
                        }
                for (int j = 0; j < 3; j++) free(f[j]);
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
                for (int power = 0; power <= 4; power += 4) {
                    float* f[3];
                    const float* in[3] = {ib, ha, hb};
                    for (int j = 0; j < 3; j++) {
                        f[j] = malloc((size_t)(K + 1) * N1 * 12);
                        if (bc_filter_levels(&cfg, in[j], albedo, normal, depth, object, cov, K, demodulate, 0.5f, 0.3f, 0.05f, 0.1f, power, f[j]))
                            failures++;
                    }
                    for (int mode = 0; mode <= 2; mode++)
                        for (int radius = 1; radius <= 3; radius++) {
                            uint32_t stats[3], resolved;
                            if (bc_blend_coverage(&cfg, ib, ha, hb, f[0], f[1], f[2], object, cov, K, radius, radius == 2 ? 2.0f : 0.0f, 1.0f, power, 1,
                                                  mode, 4 - radius, 0.05f, out, before, weight, dep, error, parts, stats, &resolved))
                                failures++;
                        }
                    for (int j = 0; j < 3; j++) free(f[j]);
                }
    }
    free(albedo); free(normal); free(depth); free(ib); free(ha); free(hb); free(object); free(cov);
    free(out); free(before); free(weight); free(dep); free(error); free(parts);
    printf("blend_coverage_ref under the sanitizers: %d failures\n", failures);
    return failures != 0;
}
