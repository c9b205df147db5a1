// The MX planner (dfq_mx_plan.cpp): host-only code that cuts a list of weights into
// the wave tasks of dfq_mx_quantize_batch (dfq_mx.hip) and lays out its workspace.
// This header holds what the planner and the kernel share and includes no HIP header,
// so the planner builds as plain C++ (and on its own, under a sanitizer:
// tests/native/mx_plan_check.cpp).
//
// The partition of a tensor depends on (rows, row_len, khw, whether esum is wanted)
// alone -- never on the other tensors of the list, its position in it, or the grid.
// With cap = mx_task_cap() elements and Lp = 32 * ceil(row_len / 32), a row padded to
// whole MX blocks:
//   Lp <= cap: whole-row tasks of cap / Lp rows (the last one shorter);
//   Lp >  cap: every row is cut at multiples of mx_piece_len() elements (a multiple
//     of 32 and, where error sums wait in LDS, of khw) from its start; one task per
//     piece, row after row, a row's pieces in order.
// So an MX block and a khw group of error sums always lie inside one task, and a
// task's padded elements (<= cap) index its codes, scales and LDS copy.
#pragma once
#include <stdint.h>

#include <vector>

#include "dfq_cle_plan.h"   // DFQ_HOST_DEVICE, ceil_div
#include "dfq_hip.h"

namespace dfq {

constexpr int64_t kMxBlock = DFQ_MX_BLOCK;

// One wave's work.  nrows > 0: rows [row, row + nrows) of the job, whole (col == 0).
// nrows == 0: the piece of row `row` that starts at column `col`.
struct MxTask {
    int32_t job;
    int32_t nrows;
    int64_t row;
    int64_t col;
};

// A tensor as the kernel sees it.
struct MxJob {
    const float* src;
    float* dst;
    uint8_t* codes;
    uint8_t* scales;
    float* esum;
    int64_t row_len;
    int64_t nb;          // MX blocks per row
    int64_t piece;       // mx_piece_len (pieces only)
    int32_t khw;
    int32_t format;
    int32_t vec;         // every row start 16-B aligned: 16-B loads and stores
    int32_t lds_esum;    // esum with khw > 1: the errors go through the wave's LDS copy
};

DFQ_HOST_DEVICE inline bool mx_lds_esum(const dfq_mx_desc& d) { return d.esum != nullptr && d.khw > 1; }
DFQ_HOST_DEVICE inline int64_t mx_task_cap(const dfq_mx_desc& d) {
    return mx_lds_esum(d) ? DFQ_MX_ESUM_TASK_ELEMS : DFQ_MX_TASK_ELEMS;
}
DFQ_HOST_DEVICE inline int64_t mx_blocks(int64_t row_len) { return ceil_div(row_len, kMxBlock); }
// the unit a piece is a multiple of: 32, or lcm(32, khw) where khw groups must stay whole
DFQ_HOST_DEVICE inline int64_t mx_piece_unit(const dfq_mx_desc& d) {
    if (!mx_lds_esum(d)) return kMxBlock;
    int64_t a = kMxBlock, b = d.khw;
    while (b) {
        const int64_t t = a % b;
        a = b;
        b = t;
    }
    return kMxBlock / a * d.khw;
}
// elements of a piece of a split row (0: no piece fits the task)
DFQ_HOST_DEVICE inline int64_t mx_piece_len(const dfq_mx_desc& d) {
    const int64_t u = mx_piece_unit(d), cap = mx_task_cap(d);
    return cap / u * u;
}
DFQ_HOST_DEVICE inline bool mx_split(const dfq_mx_desc& d) { return mx_blocks(d.row_len) * kMxBlock > mx_task_cap(d); }
DFQ_HOST_DEVICE inline int64_t mx_rows_per_task(const dfq_mx_desc& d) {
    return mx_task_cap(d) / (mx_blocks(d.row_len) * kMxBlock);
}

// Workspace of one call: [jobs | tasks], each part 256-B aligned, all of it uploaded.
struct MxLayout {
    int64_t n_tasks = 0;
    int64_t lds_jobs = 0;   // jobs whose error sums go through LDS (0: the launch takes none)
    int64_t o_jobs = 0, o_tasks = 0, total = 0;
};

// Arguments as dfq_mx_quantize_ws_bytes checks them, and the layout (no table built).
int mx_layout(const dfq_mx_desc* d, int32_t n, MxLayout& L);
// The task table, in list order.
int mx_plan(const dfq_mx_desc* d, int32_t n, MxLayout& L, std::vector<MxTask>& tasks);
// 16-B path: every row of every given array starts 16-B aligned (codes: 4-B)
bool mx_vec(const dfq_mx_desc& d);

}  // namespace dfq
