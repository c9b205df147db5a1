// Host check of the group arithmetic of the grouped integer kernels (dfq_int_gemm_plan.h: igg_*).
// For every K:g argument it walks the kernel's loop -- K steps, passes, the 64 lanes and their 16
// elements -- and checks that every k < K is added in exactly one pass, by a lane of that pass,
// to group k / g; that a group closes once, in the pass that holds its last element, with the
// contract's length; and that groups close in ascending order.  Prints "ok" per argument.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dfq_int_gemm_plan.h"

using namespace dfq;

static bool check(int64_t K, int g) {
    if (igg_check(g, 0) != DFQ_OK || igg_check(g, DFQ_INT_B_PER_ROW) != DFQ_ERR_INVALID) return false;
    const int64_t G = igg_groups(K, g);
    const int steps = (int)ig_steps(K), passes = igg_passes(g);
    std::vector<int> added(K, 0), open_count(G, 0), closed(G, 0);
    int64_t next_close = 0;
    for (int s = 0; s < steps; ++s) {
        for (int pass = 0; pass < passes; ++pass) {
            const int grp = igg_group(s, pass, g), len = igg_group_len(grp, g, K);
            if (len <= 0) break;
            if (grp >= G || closed[grp]) return false;
            for (int lane = 0; lane < 64; lane += 16) {   // one lane per lane group: the others hold other rows
                if (!igg_lane_in_pass(lane, pass, g)) continue;
                const int64_t k0 = ig_lane_k0(s, lane);
                const int nv = ig_lane_valid(0, 1, k0, K);
                for (int e = 0; e < nv; ++e) {
                    if ((k0 + e) / g != grp) return false;
                    ++added[k0 + e];
                    ++open_count[grp];
                }
            }
            if (!igg_closes(s, steps, g)) continue;
            if (grp != next_close++ || open_count[grp] != len) return false;
            const int64_t want = K - (int64_t)grp * g < g ? K - (int64_t)grp * g : g;
            if (len != want) return false;
            closed[grp] = 1;
        }
    }
    for (int64_t k = 0; k < K; ++k)
        if (added[k] != 1) return false;
    if (next_close != G) return false;
    return igg_param_offset(3, G - 1, G) == 3 * G + G - 1;
}

int main(int argc, char** argv) {
    for (const int bad : {0, -1, 16, 48, 96, 63, 32768 + 64})
        if (igg_check(bad, 0) != (bad < 1 ? DFQ_ERR_INVALID : DFQ_ERR_UNSUPPORTED)) return 2;
    for (int i = 1; i < argc; ++i) {
        long long K = 0;
        int g = 0;
        if (std::sscanf(argv[i], "%lld:%d", &K, &g) != 2) return 2;
        if (!check(K, g)) {
            std::printf("FAIL %s\n", argv[i]);
            return 1;
        }
        std::printf("ok\n");
    }
    return 0;
}
