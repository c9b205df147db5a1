// Host-only planner of dfq_pair_stats_batch: argument checks, the task table and
// the workspace layout (dfq_stats_plan.h).  Plain C++: no HIP header, no device code.
#include "dfq_stats_plan.h"

namespace dfq {


static bool pair_ok(const dfq_pair_desc& p) {
    if (!p.x || !p.y || (!p.rows_out && !p.total_out)) return false;
    if (p.rows < 1 || p.row_len < 1) return false;
    if (reinterpret_cast<uintptr_t>(p.x) % 4 || reinterpret_cast<uintptr_t>(p.y) % 4) return false;
    if (reinterpret_cast<uintptr_t>(p.rows_out) % 8 || reinterpret_cast<uintptr_t>(p.total_out) % 8) return false;
    // element and slot indices stay far inside int64
    return p.rows <= (int64_t(1) << 40) && p.row_len <= (int64_t(1) << 40) &&
           p.rows <= (int64_t(1) << 56) / p.row_len;
}

static int64_t pair_tasks(const dfq_pair_desc& p) {
    return p.row_len > kPairPiece ? p.rows * pair_pieces(p.row_len) : ceil_div(p.rows, pair_rows_per_task(p.row_len));
}

int pair_stats_layout(const dfq_pair_desc* d, int32_t n, PairLayout& L) {
    L = PairLayout{};
    if (n < 0 || (n > 0 && !d)) return DFQ_ERR_INVALID;
    for (int32_t p = 0; p < n; ++p) {
        if (!pair_ok(d[p])) return DFQ_ERR_INVALID;
        L.n_tasks += pair_tasks(d[p]);
        if (d[p].row_len > kPairPiece) L.n_slots += d[p].rows * pair_pieces(d[p].row_len);
        if (!d[p].rows_out) L.n_buf_rows += d[p].rows;
    }
    const int64_t rec = (int64_t)sizeof(double) * kPairSlotDoubles;
    L.o_jobs = 0;
    L.o_tasks = L.o_jobs + round256((int64_t)sizeof(PairJob) * n);
    L.o_slots = L.o_tasks + round256((int64_t)sizeof(PairTask) * L.n_tasks);
    L.o_rows = L.o_slots + round256(rec * L.n_slots);
    L.total = L.o_rows + round256(rec * L.n_buf_rows);
    return DFQ_OK;
}

int pair_stats_plan(const dfq_pair_desc* d, int32_t n, PairLayout& L, std::vector<PairTask>& tasks,
                    std::vector<int64_t>& slot_base, std::vector<int64_t>& row_base) {
    const int rc = pair_stats_layout(d, n, L);
    if (rc != DFQ_OK) return rc;
    tasks.clear();
    tasks.reserve((size_t)L.n_tasks);
    slot_base.assign((size_t)n, -1);
    row_base.assign((size_t)n, -1);
    int64_t slots = 0, buf_rows = 0;
    for (int32_t p = 0; p < n; ++p) {
        const dfq_pair_desc& x = d[p];
        if (!x.rows_out) {
            row_base[p] = buf_rows;
            buf_rows += x.rows;
        }
        if (x.row_len > kPairPiece) {
            const int64_t np = x.rows * pair_pieces(x.row_len);
            slot_base[p] = slots;
            slots += np;
            for (int64_t s = 0; s < np; ++s) tasks.push_back(PairTask{p, 0, s});
        } else {
            const int64_t per = pair_rows_per_task(x.row_len);
            for (int64_t r = 0; r < x.rows; r += per)
                tasks.push_back(PairTask{p, (int32_t)(x.rows - r < per ? x.rows - r : per), r});
        }
    }
    return DFQ_OK;
}

}  // namespace dfq

extern "C" int64_t dfq_pair_stats_ws_bytes(const dfq_pair_desc* descs, int32_t n) {
    dfq::PairLayout L;
    if (dfq::pair_stats_layout(descs, n, L) != DFQ_OK) return -1;
    return L.total > 256 ? L.total : 256;
}
