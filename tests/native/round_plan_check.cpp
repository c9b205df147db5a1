// The sum-rounding planner on its own: dfq_round_plan.cpp linked with this main and
// nothing else, so it runs under AddressSanitizer / UBSan on a machine without a
// GPU (tests/test_sum_round_host.py builds and runs it).
// Input: a text file of lists -- `n`, then n lines `rows row_len khw bits mode`.
// (Addresses are stand-ins: the planner never dereferences them.)
// Output: first `self <failures>` -- the shared inline functions and every LDS layout
// the limits allow, checked here -- then per list:
//   list <i> rc <code> total_rows <n> n_tensor <n> grid <n> lds <B> o_range <B> total <B> ws <B> job_bytes <B>
//   job <p> row0 <r> row_len <l> khw <k> sym <0|1> range <word offset from the range base, -1: none>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dfq_round_plan.h"

using namespace dfq;

static int self_check() {
    int bad = 0;
    // step 3 at its edges: an exact tie, a clamped element, the smallest differences
    bad += sr_perturb(2.f, 2.5f) != -kSrHalf || sr_perturb(4.f, 3.5f) != kSrHalf || sr_perturb(3.f, 3.f) != 0;
    bad += sr_perturb(0.f, 0x1p-30f) != 0 || sr_perturb(1.f, 1.f - 0x1p-24f) != 1 || sr_perturb(0.f, -0.25f) != 1 << 22;
    // steps 4 and 5: round half down, both signs, beyond int32
    bad += sr_flip_count(kSrHalf) != 0 || sr_flip_count(kSrHalf + 1) != 1 || sr_flip_count(-kSrHalf) != 0;
    bad += sr_flip_count(-(int64_t)kSrHalf - 1) != 1 || sr_flip_count(3 * (int64_t)kSrHalf) != 1;
    bad += sr_flip_count(3 * (int64_t)kSrHalf + 1) != 2 || sr_flip_count((int64_t)16384 * kSrHalf) != 8192;
    // the key keeps the candidates' order and puts everything else below them
    bad += !(sr_key(5, true) > sr_key(4, true) && sr_key(4, true) > sr_key(0, true)) || sr_key(-7, true) != 0;
    bad += !(sr_key(-5, false) > sr_key(-4, false)) || sr_key(7, false) != 0 || sr_key(kSrStep + kSrHalf, true) != 3u << 23;
    // a flipped word is apart from every unflipped one, exact ties included
    for (int32_t p : {-kSrHalf, -1, 0, 1, kSrHalf}) {
        bad += sr_code_offset(p) != 0 || sr_value(p) != p;
        if (p > 0) bad += sr_code_offset(p - kSrMark) != -1 || sr_value(p - kSrMark) != p - kSrStep;
        if (p < 0) bad += sr_code_offset(p + kSrMark) != 1 || sr_value(p + kSrMark) != p + kSrStep;
    }
    // every layout the limits allow: odd pitch, parts in order and apart, inside the LDS
    for (int khw = 1; khw <= DFQ_SR_MAX_KHW; ++khw)
        for (int64_t len = khw; len <= DFQ_SR_MAX_ROW; len += khw) {
            const SrLds L = sr_lds_layout(len, khw);
            const int64_t G = len / khw, pitch = sr_pitch(khw);
            bad += pitch < khw || (khw > 1 && pitch % 2 == 0);
            bad += L.o_s != 0 || L.o_q % 4 != 0 || L.o_q < 4 * G * pitch || L.total < L.o_q + len;
            bad += khw == 1 ? L.o_e != 0 : (L.o_e < 4 * G * pitch || L.o_e + 4 * G > L.o_q);
            bad += L.total + 4096 > kSrLdsLimit;   // the kernel's static words fit beside it
        }
    return bad;
}

int main(int argc, char** argv) {
    if (argc != 2) return fprintf(stderr, "usage: %s lists.txt\n", argv[0]), 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return perror(argv[1]), 2;
    printf("self %d\n", self_check());
    uint32_t* const range_base = reinterpret_cast<uint32_t*>((uintptr_t)0x100000);
    long long n;
    for (int li = 0; fscanf(f, "%lld", &n) == 1; ++li) {
        std::vector<dfq_sum_round_desc> d((size_t)n);
        for (dfq_sum_round_desc& p : d) {
            long long rows, row_len, khw, bits, mode;
            if (fscanf(f, "%lld %lld %lld %lld %lld", &rows, &row_len, &khw, &bits, &mode) != 5)
                return fprintf(stderr, "list %d: truncated\n", li), 2;
            p = dfq_sum_round_desc{};
            p.src = reinterpret_cast<const float*>((uintptr_t)0x1000);
            p.codes = reinterpret_cast<void*>((uintptr_t)0x2000);
            p.rows = rows;
            p.row_len = row_len;
            p.khw = (int32_t)khw;
            p.bits = (int32_t)bits;
            p.mode = (int32_t)mode;
        }
        SrLayout L;
        const int rc = sum_round_layout(d.data(), (int32_t)n, L);
        printf("list %d rc %d total_rows %lld n_tensor %d grid %d lds %d o_range %lld total %lld ws %lld job_bytes %zu\n",
               li, rc, (long long)L.total_rows, L.n_tensor, L.grid, L.lds_bytes, (long long)L.o_range,
               (long long)L.total, (long long)dfq_sum_round_ws_bytes(d.data(), (int32_t)n), sizeof(SrJob));
        if (rc != DFQ_OK) continue;
        std::vector<SrJob> jobs((size_t)n);
        sum_round_jobs(d.data(), (int32_t)n, range_base, jobs.data());
        for (size_t p = 0; p < jobs.size(); ++p)
            printf("job %zu row0 %lld row_len %d khw %d sym %d range %lld\n", p, (long long)jobs[p].row0, jobs[p].row_len,
                   jobs[p].khw, jobs[p].sym, jobs[p].range ? (long long)(jobs[p].range - range_base) : -1LL);
    }
    fclose(f);
    return 0;
}
