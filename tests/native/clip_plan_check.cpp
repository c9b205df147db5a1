// The clip-search planner on its own: dfq_clip_plan.cpp linked with this main and
// nothing else, so it runs under AddressSanitizer / UBSan on a machine without a
// GPU (tests/test_clip_search_host.py builds and runs it).
// Input: a text file of lists -- `n`, then n lines `rows row_len mode candidates dry`.
// (Addresses are stand-ins: the planner never dereferences them.)
// Output per list:
//   list <i> rc <code> tasks <n> piece_tasks <n> split_units <n> slot_doubles <n> clamp_tasks <n>
//        o_tasks <B> o_fin <B> o_urec <B> o_slots <B> total <B> ws <B>
//        task_bytes <B> fin_bytes <B> urec_bytes <B>
//   job <p> urec_base <u> slot_base <s>           (one per weight)
//   task <job> <nunits> <first>                   (one per task, in table order)
//   fin <job> <unit>                              (one per split unit, in table order)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dfq_clip_plan.h"

int main(int argc, char** argv) {
    if (argc != 2) return fprintf(stderr, "usage: %s lists.txt\n", argv[0]), 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return perror(argv[1]), 2;
    long long n;
    for (int li = 0; fscanf(f, "%lld", &n) == 1; ++li) {
        std::vector<dfq_clip_search_desc> d((size_t)n);
        for (dfq_clip_search_desc& p : d) {
            long long rows, row_len, mode, cand, dry;
            if (fscanf(f, "%lld %lld %lld %lld %lld", &rows, &row_len, &mode, &cand, &dry) != 5)
                return fprintf(stderr, "list %d: truncated\n", li), 2;
            p = dfq_clip_search_desc{};
            p.w = reinterpret_cast<float*>((uintptr_t)0x1000);
            p.rows = rows;
            p.row_len = row_len;
            p.bits = 4;
            p.mode = (int32_t)mode;
            p.candidates = (int32_t)cand;
            p.flags = dry ? DFQ_CLIP_SEARCH_DRY : 0;
            p.min_frac = 0.5f;
            p.choice = reinterpret_cast<int32_t*>((uintptr_t)0x2000);
            p.noise = reinterpret_cast<double*>((uintptr_t)0x3000);
        }
        dfq::ClipLayout L;
        std::vector<dfq::ClipTask> tasks;
        std::vector<dfq::ClipFin> fin;
        std::vector<int64_t> urec_base, slot_base;
        const int rc = dfq::clip_search_plan(d.data(), (int32_t)n, L, tasks, fin, urec_base, slot_base);
        printf("list %d rc %d tasks %lld piece_tasks %lld split_units %lld slot_doubles %lld clamp_tasks %lld "
               "o_tasks %lld o_fin %lld o_urec %lld o_slots %lld total %lld ws %lld task_bytes %zu fin_bytes %zu "
               "urec_bytes %zu\n",
               li, rc, (long long)L.n_tasks, (long long)L.n_piece_tasks, (long long)L.n_split_units,
               (long long)L.n_slot_doubles, (long long)L.n_clamp_piece_tasks, (long long)L.o_tasks, (long long)L.o_fin,
               (long long)L.o_urec, (long long)L.o_slots, (long long)L.total,
               (long long)dfq_clip_search_ws_bytes(d.data(), (int32_t)n), sizeof(dfq::ClipTask), sizeof(dfq::ClipFin),
               sizeof(dfq::ClipUnit));
        if (rc != DFQ_OK) continue;
        if ((long long)tasks.size() != L.n_tasks || (long long)fin.size() != L.n_split_units)
            return fprintf(stderr, "list %d: table sizes differ from the layout\n", li), 1;
        for (size_t p = 0; p < d.size(); ++p)
            printf("job %zu urec_base %lld slot_base %lld\n", p, (long long)urec_base[p], (long long)slot_base[p]);
        for (const dfq::ClipTask& t : tasks) printf("task %d %d %lld\n", t.job, t.nunits, (long long)t.first);
        for (const dfq::ClipFin& x : fin) printf("fin %d %lld\n", x.job, (long long)x.unit);
    }
    fclose(f);
    return 0;
}
