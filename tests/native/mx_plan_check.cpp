// The MX planner on its own: dfq_mx_plan.cpp linked with this main and nothing else,
// so it runs under AddressSanitizer / UBSan on a machine without a GPU
// (tests/test_mx_host.py builds and runs it).
// Input: a text file of lists -- `n`, then n lines `rows row_len khw esum aligned`.
// (Addresses are stand-ins: the planner never dereferences them.)
// Output per list:
//   list <i> rc <code> tasks <n> lds_jobs <n> o_tasks <B> total <B> ws <B> job_bytes <B> task_bytes <B>
//   job <p> vec <0|1> cap <elements> piece <elements> rows_per_task <n>     (one per tensor)
//   task <job> <nrows> <row> <col>                                          (one per task, in table order)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dfq_mx_plan.h"

int main(int argc, char** argv) {
    if (argc != 2) return fprintf(stderr, "usage: %s lists.txt\n", argv[0]), 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return perror(argv[1]), 2;
    long long n;
    for (int li = 0; fscanf(f, "%lld", &n) == 1; ++li) {
        std::vector<dfq_mx_desc> d((size_t)n);
        for (dfq_mx_desc& p : d) {
            long long rows, row_len, khw, esum, aligned;
            if (fscanf(f, "%lld %lld %lld %lld %lld", &rows, &row_len, &khw, &esum, &aligned) != 5)
                return fprintf(stderr, "list %d: truncated\n", li), 2;
            p = dfq_mx_desc{};
            p.src = reinterpret_cast<const float*>((uintptr_t)(aligned ? 0x1000 : 0x1004));
            p.dst = reinterpret_cast<float*>((uintptr_t)(aligned ? 0x1000 : 0x1004));
            p.codes = reinterpret_cast<uint8_t*>((uintptr_t)0x2000);
            p.scales = reinterpret_cast<uint8_t*>((uintptr_t)0x3000);
            p.esum = esum ? reinterpret_cast<float*>((uintptr_t)0x4000) : nullptr;
            p.rows = rows;
            p.row_len = row_len;
            p.khw = (int32_t)khw;
            p.format = (int32_t)((rows + row_len) % 2);
        }
        dfq::MxLayout L;
        std::vector<dfq::MxTask> tasks;
        const int rc = dfq::mx_plan(d.data(), (int32_t)n, L, tasks);
        printf("list %d rc %d tasks %lld lds_jobs %lld o_tasks %lld total %lld ws %lld job_bytes %zu task_bytes %zu\n", li,
               rc, (long long)L.n_tasks, (long long)L.lds_jobs, (long long)L.o_tasks, (long long)L.total,
               (long long)dfq_mx_quantize_ws_bytes(d.data(), (int32_t)n), sizeof(dfq::MxJob), sizeof(dfq::MxTask));
        if (rc != DFQ_OK) continue;
        if ((long long)tasks.size() != L.n_tasks) return fprintf(stderr, "list %d: table size differs from the layout\n", li), 1;
        for (size_t p = 0; p < d.size(); ++p)
            printf("job %zu vec %d cap %lld piece %lld rows_per_task %lld\n", p, dfq::mx_vec(d[p]) ? 1 : 0,
                   (long long)dfq::mx_task_cap(d[p]), (long long)(dfq::mx_split(d[p]) ? dfq::mx_piece_len(d[p]) : 0),
                   (long long)(dfq::mx_split(d[p]) ? 0 : dfq::mx_rows_per_task(d[p])));
        for (const dfq::MxTask& t : tasks) printf("task %d %d %lld %lld\n", t.job, t.nrows, (long long)t.row, (long long)t.col);
    }
    fclose(f);
    return 0;
}
