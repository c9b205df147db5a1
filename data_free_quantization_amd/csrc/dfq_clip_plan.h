// The clip-search planner (dfq_clip_plan.cpp): host-only code that cuts a list of
// weights into the wave tasks of dfq_clip_search_batch (dfq_clip.hip) and lays out
// its workspace.  This header holds what the planner and the kernels share and
// includes no HIP header, so the planner builds as plain C++ (and on its own, under
// a sanitizer: tests/native/clip_plan_check.cpp).
//
// A unit is a row (CHANNEL modes) or the whole tensor (TENSOR modes): `units` of
// `unit_len` elements each, contiguous.  The partition of a weight depends on
// (units, unit_len) alone -- never on the other weights of the list, its position
// in it, or the grid -- so its result is the same bits wherever it is computed:
//   unit_len <= DFQ_CLIP_PIECE_ELEMS: whole-unit tasks of clip_units_per_task()
//     units (<= 64 units and <= DFQ_CLIP_PIECE_ELEMS elements, at least one unit);
//   unit_len >  DFQ_CLIP_PIECE_ELEMS: every unit is cut at multiples of
//     DFQ_CLIP_PIECE_ELEMS elements from its start; one task per piece, unit after
//     unit, a unit's pieces in order.  Piece k of unit u writes the K partial sums
//     of slot u * pieces + k of the weight.
// The table holds every piece task first (the range and clamp launches walk only
// those), then the whole-unit tasks, each group in list order.
#pragma once
#include <stdint.h>

#include <vector>

#include "dfq_cle_plan.h"   // DFQ_HOST_DEVICE, ceil_div
#include "dfq_hip.h"

namespace dfq {

constexpr int64_t kClipPiece = DFQ_CLIP_PIECE_ELEMS;
constexpr int kClipTaskUnits = 64;   // most units of one whole-unit task
constexpr int kClipMaxCand = DFQ_CLIP_MAX_CANDIDATES;

// One wave's work.  nunits > 0: units [first, first + nunits) of the job, whole.
// nunits == 0: piece `first % pieces` of unit `first / pieces` (first = the slot index).
struct ClipTask {
    int32_t job;
    int32_t nunits;
    int64_t first;
};

// A split unit's record in the workspace: its range while the pieces are evaluated
// (zeroed by the call, then exact integer atomic maxima of the ordered encoding),
// and the chosen clamp for the clamp launch.
struct ClipUnit {
    uint32_t enc[2];   // {~enc(min), enc(max)}
    float lo, hi;      // the chosen (lo_k, hi_k)
    int32_t k;         // the choice
    int32_t pad;
};

// A weight as the kernels see it.
struct ClipJob {
    float* w;
    int32_t* choice;       // [units] or NULL
    float* range;          // [units][2] or NULL
    double* noise;         // [units][2] or NULL
    uint32_t* range_enc;   // [2] or NULL (TENSOR modes only)
    ClipUnit* urec;        // [units] records of the split units (NULL: no unit is split)
    double* slots;         // [units * pieces][K] partial sums (NULL: no unit is split)
    int64_t units;
    int64_t unit_len;
    int32_t bits;
    int32_t sym;
    int32_t K;
    int32_t dry;
    float min_frac;
    int32_t pad;
};

// One split unit for the finish launch (one wave each).
struct ClipFin {
    int32_t job;
    int32_t pad;
    int64_t unit;
};

DFQ_HOST_DEVICE inline int64_t clip_units(const dfq_clip_search_desc& d) {
    return d.mode >= DFQ_CHANNEL_ASYM ? d.rows : 1;
}
DFQ_HOST_DEVICE inline int64_t clip_unit_len(const dfq_clip_search_desc& d) {
    return d.mode >= DFQ_CHANNEL_ASYM ? d.row_len : d.rows * d.row_len;
}
DFQ_HOST_DEVICE inline int64_t clip_pieces(int64_t unit_len) {
    return unit_len > kClipPiece ? ceil_div(unit_len, kClipPiece) : 1;
}
// units of one whole-unit task (unit_len <= kClipPiece)
DFQ_HOST_DEVICE inline int64_t clip_units_per_task(int64_t unit_len) {
    const int64_t r = kClipPiece / unit_len;
    return r > kClipTaskUnits ? kClipTaskUnits : (r < 1 ? 1 : r);
}
// Lanes that share one unit of a whole-unit task (a power of two; 64 / lanes units
// are in flight per wave): up to 16 elements per lane until the whole wave takes
// one unit, so short rows (depthwise filters, narrow 1x1 convs) still fill the
// wave, and the units in flight never exceed 1024 elements of the wave's LDS copy.
// A piece takes the whole wave.
DFQ_HOST_DEVICE inline int clip_group_lanes(int64_t unit_len) {
    int g = 1;
    while (g < 64 && (int64_t)g * 16 < unit_len) g <<= 1;
    return g;
}

// Workspace of one call: [jobs | tasks | finish list | split units' records |
// partial slots], each part 256-B aligned.  The first three are uploaded
// (o_urec bytes), the records are zeroed, the slots are written before they are read.
struct ClipLayout {
    int64_t n_tasks = 0;
    int64_t n_piece_tasks = 0;   // the first n_piece_tasks tasks are pieces
    int64_t n_split_units = 0;   // = finish list entries = unit records
    int64_t n_slot_doubles = 0;  // sum over split weights of units * pieces * K
    int64_t n_clamp_piece_tasks = 0;   // piece tasks of the weights that are not dry (0: no clamp launch)
    int64_t o_jobs = 0, o_tasks = 0, o_fin = 0, o_urec = 0, o_slots = 0, total = 0;
};

// Arguments as dfq_clip_search_ws_bytes checks them, and the layout (no table built).
int clip_search_layout(const dfq_clip_search_desc* d, int32_t n, ClipLayout& L);
// The tables: tasks (pieces first), the finish list, and per weight urec_base[p] /
// slot_base[p] = its first unit record / first partial-sum double (-1: not split).
int clip_search_plan(const dfq_clip_search_desc* d, int32_t n, ClipLayout& L, std::vector<ClipTask>& tasks,
                     std::vector<ClipFin>& fin, std::vector<int64_t>& urec_base, std::vector<int64_t>& slot_base);

}  // namespace dfq
