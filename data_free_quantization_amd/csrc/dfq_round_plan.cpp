// Host-only planner of dfq_sum_round_batch: argument checks, the job table, the LDS
// size and the grid (dfq_round_plan.h).  Plain C++: no HIP header, no device code.
#include "dfq_round_plan.h"

namespace dfq {

int sum_round_check(const dfq_sum_round_desc& p) {
    if (!p.src || reinterpret_cast<uintptr_t>(p.src) % 4) return DFQ_ERR_INVALID;
    if (!p.dst && !p.codes && !p.scale && !p.zero && !p.flips) return DFQ_ERR_INVALID;
    if (reinterpret_cast<uintptr_t>(p.dst) % 4 || reinterpret_cast<uintptr_t>(p.scale) % 4 ||
        reinterpret_cast<uintptr_t>(p.zero) % 4 || reinterpret_cast<uintptr_t>(p.flips) % 4)
        return DFQ_ERR_INVALID;
    if (p.rows < 1 || p.row_len < 1 || p.khw < 1 || p.reserved != 0) return DFQ_ERR_INVALID;
    if (p.bits < 2 || p.bits > 8) return DFQ_ERR_INVALID;
    if (p.mode < DFQ_TENSOR_ASYM || p.mode > DFQ_CHANNEL_SYM) return DFQ_ERR_INVALID;
    if (p.rows > (int64_t(1) << 40)) return DFQ_ERR_INVALID;   // element indices stay far inside int64
    if (p.row_len % p.khw != 0) return DFQ_ERR_SHAPE;
    if (p.row_len > DFQ_SR_MAX_ROW || p.khw > DFQ_SR_MAX_KHW) return DFQ_ERR_UNSUPPORTED;
    return DFQ_OK;
}

int sum_round_layout(const dfq_sum_round_desc* d, int32_t n, SrLayout& L) {
    L = SrLayout{};
    if (n < 0 || n > 65535 || (n > 0 && !d)) return DFQ_ERR_INVALID;
    for (int32_t p = 0; p < n; ++p) {
        const int rc = sum_round_check(d[p]);
        if (rc != DFQ_OK) return rc;
        L.total_rows += d[p].rows;
        L.n_tensor += d[p].mode < DFQ_CHANNEL_ASYM;
        const SrLds lds = sr_lds_layout(d[p].row_len, d[p].khw);
        if (lds.total > L.lds_bytes) L.lds_bytes = lds.total;
    }
    L.grid = (int32_t)(L.total_rows < kSrGridCap ? L.total_rows : kSrGridCap);
    L.o_jobs = 0;
    L.o_range = round256((int64_t)sizeof(SrJob) * n);
    L.total = L.o_range + round256((int64_t)8 * n);
    return DFQ_OK;
}

void sum_round_jobs(const dfq_sum_round_desc* d, int32_t n, uint32_t* range_base, SrJob* jobs) {
    int64_t row0 = 0;
    for (int32_t p = 0; p < n; ++p) {
        const bool tensor = d[p].mode < DFQ_CHANNEL_ASYM;
        jobs[p] = SrJob{d[p].src, d[p].dst, d[p].codes, d[p].scale, d[p].zero, d[p].flips,
                        tensor ? range_base + 2 * p : nullptr, d[p].rows, row0, (int32_t)d[p].row_len, d[p].khw,
                        d[p].bits, (d[p].mode == DFQ_TENSOR_SYM || d[p].mode == DFQ_CHANNEL_SYM) ? 1 : 0};
        row0 += d[p].rows;
    }
}

}  // namespace dfq

extern "C" int64_t dfq_sum_round_ws_bytes(const dfq_sum_round_desc* descs, int32_t n) {
    dfq::SrLayout L;
    if (dfq::sum_round_layout(descs, n, L) != DFQ_OK) return -1;
    return L.total > 256 ? L.total : 256;
}
