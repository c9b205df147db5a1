// The pair-statistics planner on its own: dfq_stats_plan.cpp linked with this main
// and nothing else, so it runs under AddressSanitizer / UBSan on a machine without
// a GPU (tests/test_pair_stats_host.py builds and runs it).
// Input: a text file of lists -- `n`, then n lines `rows row_len want_rows_out`.
// (Addresses are stand-ins: the planner never dereferences them.)
// Output per list:
//   list <i> rc <code> tasks <n> slots <n> buf_rows <n> o_tasks <B> o_slots <B> o_rows <B> total <B> ws <B>
//   pair <p> slot_base <s> row_base <r>          (one per pair)
//   task <pair> <nrows> <first>                  (one per task, in table order)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dfq_stats_plan.h"

int main(int argc, char** argv) {
    if (argc != 2) return fprintf(stderr, "usage: %s lists.txt\n", argv[0]), 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return perror(argv[1]), 2;
    long long n;
    for (int li = 0; fscanf(f, "%lld", &n) == 1; ++li) {
        std::vector<dfq_pair_desc> d((size_t)n);
        for (dfq_pair_desc& p : d) {
            long long rows, row_len, want;
            if (fscanf(f, "%lld %lld %lld", &rows, &row_len, &want) != 3)
                return fprintf(stderr, "list %d: truncated\n", li), 2;
            p.x = reinterpret_cast<const float*>((uintptr_t)0x1000);
            p.y = reinterpret_cast<const float*>((uintptr_t)0x2000);
            p.rows_out = want ? reinterpret_cast<double*>((uintptr_t)0x3000) : nullptr;
            p.total_out = reinterpret_cast<double*>((uintptr_t)0x4000);
            p.rows = rows;
            p.row_len = row_len;
        }
        dfq::PairLayout L;
        std::vector<dfq::PairTask> tasks;
        std::vector<int64_t> slot_base, row_base;
        const int rc = dfq::pair_stats_plan(d.data(), (int32_t)n, L, tasks, slot_base, row_base);
        printf("list %d rc %d tasks %lld slots %lld buf_rows %lld o_tasks %lld o_slots %lld o_rows %lld total %lld ws %lld\n",
               li, rc, (long long)L.n_tasks, (long long)L.n_slots, (long long)L.n_buf_rows, (long long)L.o_tasks,
               (long long)L.o_slots, (long long)L.o_rows, (long long)L.total,
               (long long)dfq_pair_stats_ws_bytes(d.data(), (int32_t)n));
        if (rc != DFQ_OK) continue;
        for (size_t p = 0; p < d.size(); ++p)
            printf("pair %zu slot_base %lld row_base %lld\n", p, (long long)slot_base[p], (long long)row_base[p]);
        for (const dfq::PairTask& t : tasks) printf("task %d %d %lld\n", t.pair, t.nrows, (long long)t.first);
    }
    fclose(f);
    return 0;
}
