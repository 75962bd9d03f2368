// Sanitizer driver of the launch plans (test infrastructure; nothing is loaded into Python for this):
//     g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all tests/launch_plan/san_main.cpp -o launch_plan_san && ./launch_plan_san
// The sweep of tests/test_launch_plan_host.py through the same shim: every frame, device, occupancy and option value of that test, so
// that a signed overflow, a shift out of range, a division by zero or a narrowing that loses bits on the way to a plan is reported.
// What the plans must hold whatever the inputs is counted: a grid of at least one block, 1 <= K <= left, items that fit 32 bits with
// the margin, a dense claim size that divides or is divided by K, a batch of whole units within the limit.  Exit 0 = none.
#include "launch_plan.cpp"

#include <stdio.h>

int main() {
    const long long NP[] = {1, 255, 256, 257, 384, 4096, 65536, 331776, 589824, 2073600, 2500000, 2500001, 3686400, 33177600};
    const int N_CU[] = {1, 8, 256, 304, 2048}, PER_CU[] = {-3, 0, 1, 2, 4, 5, 8}, SPP[] = {1, 2, 3, 12, 16, 27, 256, 4096};
    const int CHUNK[] = {0, 31, 32, 36, 96, 240, 256, 257, 777, 8192}, WAVES_PER_CU[] = {0, 1, 7, 32}, GRID_BLOCKS[] = {0, 1, 65535};
    const long long STAGING[] = {1LL << 20, 16LL << 30};
    const int CHAIN_WAVES[] = {0, 1, 1024, 2048}, SPLIT_HEAD[] = {-1, 0, 1}, SPARSE[] = {24, 8, 64};
    long long failures = 0, plans = 0, out[8];
    for (long long np : NP)
        for (int n_cu : N_CU) {
            for (int per_cu : PER_CU)
                for (int w : WAVES_PER_CU) {
                    for (int n : SPP) {
                        const long long total = np * n;
                        if (total + rt::work_margin(n_cu) > 0xFFFFFFFFLL) continue;
                        lp_scalars(per_cu, w, n_cu, total, out);
                        const long long grid = out[1];
                        if (out[0] < 1 || grid < 1 || grid > (total + 255) / 256 || out[3] < 1) failures++;
                        for (int opt : CHUNK) {
                            lp_claim(total, grid, opt, out);
                            const long long chunk = out[0];
                            if (chunk < 1 || (opt > 0 && chunk != opt)) failures++;
                            lp_dense(total, n, chunk, opt, out);
                            if (out[0] && (out[1] < 32 || out[1] > 256 || (out[1] % n && n % out[1]) || out[2] > 4096 || out[2] % out[1] || out[2] % n ||
                                           out[5] != total / out[1] + 1))
                                failures++;
                            plans += 2;
                        }
                    }
                    for (int gb : GRID_BLOCKS) {
                        for (int cw : CHAIN_WAVES)
                            for (int flags = 0; flags < 4; flags++) {
                                lp_pool(np, rt::blocks_per_cu(per_cu, w), n_cu, cw, flags & 1, flags >> 1, gb, out);
                                if (out[0] < 1 || (gb > 0 && out[0] != gb) || out[4] < 1) failures++;
                                plans++;
                            }
                        for (int head : SPLIT_HEAD)
                            for (int sparse : SPARSE)
                                for (int op = 0; op < 2; op++)
                                    for (int n_obj = 8; n_obj <= 9; n_obj++) {
                                        lp_march(np, per_cu, n_cu, w, gb, head, sparse, op, n_obj, out);
                                        if (out[0] < 1 || out[1] != (np + 255) / 256 || out[2] < 1 || out[2] > 1024 || out[2] > out[0] || out[3] < 0) failures++;
                                        plans++;
                                    }
                    }
                }
            for (int n : SPP)
                for (long long staging : STAGING)
                    for (int flags = 0; flags < 4; flags++)
                        for (int ps = 0; ps <= 2; ps++) {
                            lp_staging(np, n, staging, n_cu, flags & 1, flags >> 1, ps, out);
                            if (out[1] < 1 || out[1] > n || out[3] != np * out[1] || out[3] + rt::work_margin(n_cu) > 0xFFFFFFFFLL) failures++;
                            plans++;
                        }
        }
    for (int n = 1; n <= 70; n++)
        for (int T = 1; T <= 8; T++) {
            int covered = 0;
            for (int t = T - 1; t >= 0; t--) {
                lp_tier(n, t, T, out);
                if (out[0] != covered || out[1] < out[0]) failures++;      // the stages' index ranges follow each other from 0
                covered = (int)out[1];
                plans++;
            }
            if (covered != n) failures++;
        }
    printf("launch plans under the sanitizers: %lld plans, %lld failures\n", plans, failures);
    return failures != 0;
}
