// The CLE planner on its own: dfq_cle_plan.cpp linked with this main and nothing
// else, so it runs under AddressSanitizer / UBSan on a machine without a GPU
// (tests/test_cle_structure.py builds and runs it).
// Input: a text file of cases -- `n_rel n_targets threads`, the 13 integers of each
// dfq_cle_rel (w1 w2 b1 bn_w bn_b s_acc c1 len1 o2 i2 khw2 s_acc_init reserved;
// addresses are stand-ins, only compared), the target addresses, the target sizes.
// Every case runs through dfq_diag_cle_check_structure under each schedule switch;
// one line per run: `<case> <schedule> <return code> <message>` (the message of a
// structure that passed is `digest <16 hex digits>`).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dfq_diag.h"

struct Schedule {
    const char* tag;
    const char* name;    // the switch set for this schedule (null: none)
    const char* value;
};
static const Schedule kSchedules[] = {
    {"product", nullptr, nullptr},      {"no_lag", "DFQ_CLE_LAG", "0"},   {"unfused", "DFQ_CLE_FUSED", "0"},
    {"band0", "DFQ_CLE_BAND", "0"},     {"band1", "DFQ_CLE_BAND", "1"},   {"band2", "DFQ_CLE_BAND", "2"},
    {"stop_arrival", "DFQ_CLE_STOP", "arrival"},
};
static const char* const kSwitches[] = {"DFQ_CLE_LAG", "DFQ_CLE_FUSED", "DFQ_CLE_BAND", "DFQ_CLE_STOP"};

int main(int argc, char** argv) {
    if (argc != 2) return fprintf(stderr, "usage: %s cases.txt\n", argv[0]), 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return perror(argv[1]), 2;
    int bad = 0;
    long long n_rel, n_targets, threads;
    for (int ci = 0; fscanf(f, "%lld %lld %lld", &n_rel, &n_targets, &threads) == 3; ++ci) {
        auto next = [&] {
            long long v = 0;
            if (fscanf(f, "%lld", &v) != 1) exit((fprintf(stderr, "case %d: truncated\n", ci), 2));
            return v;
        };
        std::vector<dfq_cle_rel> rels((size_t)n_rel);
        for (dfq_cle_rel& r : rels) {
            float** p[6] = {&r.w1, &r.w2, &r.b1, &r.bn_w, &r.bn_b, &r.s_acc};
            for (float** q : p) *q = reinterpret_cast<float*>((uintptr_t)next());
            for (int64_t* q : {&r.c1, &r.len1, &r.o2, &r.i2, &r.khw2}) *q = next();
            r.s_acc_init = (int32_t)next();
            r.reserved = (int32_t)next();
        }
        std::vector<float*> targets((size_t)n_targets);
        std::vector<int64_t> sizes((size_t)n_targets);
        for (float*& t : targets) t = reinterpret_cast<float*>((uintptr_t)next());
        for (int64_t& n : sizes) n = next();
        for (const Schedule& s : kSchedules) {
            for (const char* k : kSwitches) unsetenv(k);
            if (s.name) setenv(s.name, s.value, 1);
            int64_t info[8] = {};
            char msg[512] = "";
            const int rc = dfq_diag_cle_check_structure(rels.data(), (int32_t)n_rel, targets.data(), sizes.data(),
                                                        (int32_t)n_targets, (int32_t)threads, info, msg, sizeof(msg));
            printf("%d %s %d %s\n", ci, s.tag, rc, msg);
            bad += rc != DFQ_OK;
        }
    }
    fclose(f);
    return bad ? 1 : 0;
}
