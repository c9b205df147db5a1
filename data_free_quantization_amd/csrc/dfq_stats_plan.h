// The pair-statistics planner (dfq_stats_plan.cpp): host-only code that cuts a
// list of (reference, compared) tensor pairs into the wave tasks of
// dfq_pair_stats_batch (dfq_stats.hip) and lays out its workspace.  This header
// holds what the planner and the kernels share and includes no HIP header, so the
// planner builds as plain C++ (and on its own, under a sanitizer:
// tests/native/stats_plan_check.cpp).
//
// The partition of a pair depends on its shape alone -- never on the other pairs
// of the list, its position in it, or the grid -- so its result is the same bits
// wherever it is computed:
//   row_len <= DFQ_PAIR_PIECE_ELEMS: whole-row tasks of pair_rows_per_task() rows
//     (<= 64 rows and <= DFQ_PAIR_PIECE_ELEMS elements, at least one row);
//   row_len >  DFQ_PAIR_PIECE_ELEMS: every row is cut at multiples of
//     DFQ_PAIR_PIECE_ELEMS elements from its start; one task per piece, row after
//     row, a row's pieces in order.  Piece k of row r writes partial slot
//     r * pieces + k of the pair.
#pragma once
#include <stdint.h>

#include <vector>

#include "dfq_cle_plan.h"   // DFQ_HOST_DEVICE, ceil_div
#include "dfq_hip.h"

namespace dfq {

constexpr int64_t kPairPiece = DFQ_PAIR_PIECE_ELEMS;
constexpr int kPairTaskRows = 64;   // most rows of one whole-row task
constexpr int kPairSlotDoubles = 4; // {signal, noise, max_err, max_abs}: a row's record, a piece's partial

// One wave's work.  nrows > 0: rows [first, first + nrows) of the pair, whole.
// nrows == 0: piece `first % pieces` of row `first / pieces` (first = the slot index).
struct PairTask {
    int32_t pair;
    int32_t nrows;
    int64_t first;
};

// A pair as the kernels see it.
struct PairJob {
    const float* x;
    const float* y;
    double* rows_buf;    // [rows][4]: the caller's rows_out, or workspace when that is NULL
    double* total_out;   // [4] or NULL
    double* slots;       // [rows * pieces][4] partial slots in the workspace (NULL: no row is split)
    int64_t rows;
    int64_t row_len;
};

DFQ_HOST_DEVICE inline int64_t pair_pieces(int64_t row_len) {
    return row_len > kPairPiece ? ceil_div(row_len, kPairPiece) : 1;
}
// rows of one whole-row task (row_len <= kPairPiece)
DFQ_HOST_DEVICE inline int64_t pair_rows_per_task(int64_t row_len) {
    const int64_t r = kPairPiece / row_len;
    return r > kPairTaskRows ? kPairTaskRows : (r < 1 ? 1 : r);
}
// Lanes that share one row of a whole-row task (a power of two; 64 / lanes rows are
// in flight per wave): up to four 16-B loads of x per lane, so short rows (depthwise
// filters, narrow 1x1 convs) still fill the wave and take one round trip to memory.
// A piece takes the whole wave.
DFQ_HOST_DEVICE inline int pair_group_lanes(int64_t row_len) {
    int g = 1;
    while (g < 64 && (int64_t)g * 16 < row_len) g <<= 1;
    return g;
}

// Workspace of one call: [jobs | tasks | partial slots | row records of the pairs
// without rows_out], each part 256-B aligned.
struct PairLayout {
    int64_t n_tasks = 0;
    int64_t n_slots = 0;      // partial slots of every split pair
    int64_t n_buf_rows = 0;   // rows of the pairs whose rows_out is NULL
    int64_t o_jobs = 0, o_tasks = 0, o_slots = 0, o_rows = 0, total = 0;
};

// Arguments as dfq_pair_stats_ws_bytes checks them, and the layout (no table built).
int pair_stats_layout(const dfq_pair_desc* d, int32_t n, PairLayout& L);
// The tables: tasks in list order; slot_base[p] / row_base[p] = pair p's first
// partial slot / workspace row record (-1: it has none).
int pair_stats_plan(const dfq_pair_desc* d, int32_t n, PairLayout& L, std::vector<PairTask>& tasks,
                    std::vector<int64_t>& slot_base, std::vector<int64_t>& row_base);

}  // namespace dfq
