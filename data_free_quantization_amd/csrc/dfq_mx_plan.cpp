// Host-only planner of dfq_mx_quantize_batch: argument checks, the task table and
// the workspace layout (dfq_mx_plan.h).  Plain C++: no HIP header, no device code.
#include "dfq_mx_plan.h"

namespace dfq {

static uintptr_t addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }

static int mx_check(const dfq_mx_desc& p) {
    if (!p.src || addr(p.src) % 4 || addr(p.dst) % 4 || addr(p.esum) % 4) return DFQ_ERR_INVALID;
    if (!p.dst && !p.codes && !p.scales && !p.esum) return DFQ_ERR_INVALID;
    if (p.rows < 1 || p.row_len < 1 || p.khw < 1) return DFQ_ERR_INVALID;
    if (p.format != DFQ_MX_FP4_E2M1 && p.format != DFQ_MX_FP8_E4M3 && p.format != DFQ_MX_FP6_E2M3 &&
        p.format != DFQ_MX_FP6_E3M2)
        return DFQ_ERR_INVALID;
    if (p.flags != 0) return DFQ_ERR_INVALID;
    // element, code and task indices stay far inside int64
    if (p.rows > (int64_t(1) << 40) || p.row_len > (int64_t(1) << 40) || p.rows > (int64_t(1) << 50) / p.row_len)
        return DFQ_ERR_INVALID;
    if (p.esum && p.row_len % p.khw != 0) return DFQ_ERR_SHAPE;
    if (mx_split(p) && mx_piece_len(p) == 0) return DFQ_ERR_UNSUPPORTED;
    return DFQ_OK;
}

bool mx_vec(const dfq_mx_desc& d) {
    return d.row_len % 4 == 0 && addr(d.src) % 16 == 0 && addr(d.dst) % 16 == 0 && addr(d.esum) % 16 == 0 &&
           addr(d.codes) % 4 == 0;
}

int mx_layout(const dfq_mx_desc* d, int32_t n, MxLayout& L) {
    L = MxLayout{};
    if (n < 0 || (n > 0 && !d)) return DFQ_ERR_INVALID;
    for (int32_t p = 0; p < n; ++p) {
        const int rc = mx_check(d[p]);
        if (rc != DFQ_OK) return rc;
        if (mx_split(d[p])) L.n_tasks += d[p].rows * ceil_div(d[p].row_len, mx_piece_len(d[p]));
        else L.n_tasks += ceil_div(d[p].rows, mx_rows_per_task(d[p]));
        L.lds_jobs += mx_lds_esum(d[p]) ? 1 : 0;
    }
    L.o_jobs = 0;
    L.o_tasks = L.o_jobs + round256((int64_t)sizeof(MxJob) * n);
    L.total = L.o_tasks + round256((int64_t)sizeof(MxTask) * L.n_tasks);
    return DFQ_OK;
}

int mx_plan(const dfq_mx_desc* d, int32_t n, MxLayout& L, std::vector<MxTask>& tasks) {
    const int rc = mx_layout(d, n, L);
    if (rc != DFQ_OK) return rc;
    tasks.clear();
    tasks.reserve((size_t)L.n_tasks);
    for (int32_t p = 0; p < n; ++p) {
        if (mx_split(d[p])) {
            const int64_t piece = mx_piece_len(d[p]);
            for (int64_t r = 0; r < d[p].rows; ++r)
                for (int64_t c = 0; c < d[p].row_len; c += piece) tasks.push_back(MxTask{p, 0, r, c});
        } else {
            const int64_t per = mx_rows_per_task(d[p]);
            for (int64_t r = 0; r < d[p].rows; r += per)
                tasks.push_back(MxTask{p, (int32_t)(d[p].rows - r < per ? d[p].rows - r : per), r, 0});
        }
    }
    return DFQ_OK;
}

}  // namespace dfq

extern "C" int64_t dfq_mx_quantize_ws_bytes(const dfq_mx_desc* descs, int32_t n) {
    dfq::MxLayout L;
    if (dfq::mx_layout(descs, n, L) != DFQ_OK) return -1;
    return L.total > 256 ? L.total : 256;
}
