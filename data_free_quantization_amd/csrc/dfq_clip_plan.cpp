// Host-only planner of dfq_clip_search_batch: argument checks, the task table, the
// finish list and the workspace layout (dfq_clip_plan.h).  Plain C++: no HIP
// header, no device code.
#include "dfq_clip_plan.h"

namespace dfq {


static bool clip_ok(const dfq_clip_search_desc& p) {
    if (!p.w || reinterpret_cast<uintptr_t>(p.w) % 4) return false;
    if (p.rows < 1 || p.row_len < 1) return false;
    if (p.bits < 2 || p.bits > 16) return false;
    if (p.mode < DFQ_TENSOR_ASYM || p.mode > DFQ_CHANNEL_SYM) return false;
    if (p.candidates < 1 || p.candidates > kClipMaxCand) return false;
    if (p.flags & ~DFQ_CLIP_SEARCH_DRY) return false;
    if (!(p.min_frac >= 0.f && p.min_frac <= 1.f)) return false;   // NaN fails both
    if (reinterpret_cast<uintptr_t>(p.choice) % 4 || reinterpret_cast<uintptr_t>(p.range) % 4 ||
        reinterpret_cast<uintptr_t>(p.noise) % 8 || reinterpret_cast<uintptr_t>(p.range_enc) % 4)
        return false;
    // element and slot indices stay far inside int64
    return p.rows <= (int64_t(1) << 40) && p.row_len <= (int64_t(1) << 40) &&
           p.rows <= (int64_t(1) << 50) / p.row_len;
}

int clip_search_layout(const dfq_clip_search_desc* d, int32_t n, ClipLayout& L) {
    L = ClipLayout{};
    if (n < 0 || (n > 0 && !d)) return DFQ_ERR_INVALID;
    for (int32_t p = 0; p < n; ++p) {
        if (!clip_ok(d[p])) return DFQ_ERR_INVALID;
        const int64_t units = clip_units(d[p]), len = clip_unit_len(d[p]);
        if (len > kClipPiece) {
            const int64_t np = units * clip_pieces(len);
            L.n_tasks += np;
            L.n_piece_tasks += np;
            L.n_split_units += units;
            L.n_slot_doubles += np * d[p].candidates;
            if (!(d[p].flags & DFQ_CLIP_SEARCH_DRY)) L.n_clamp_piece_tasks += np;
        } else {
            L.n_tasks += ceil_div(units, clip_units_per_task(len));
        }
    }
    L.o_jobs = 0;
    L.o_tasks = L.o_jobs + round256((int64_t)sizeof(ClipJob) * n);
    L.o_fin = L.o_tasks + round256((int64_t)sizeof(ClipTask) * L.n_tasks);
    L.o_urec = L.o_fin + round256((int64_t)sizeof(ClipFin) * L.n_split_units);
    L.o_slots = L.o_urec + round256((int64_t)sizeof(ClipUnit) * L.n_split_units);
    L.total = L.o_slots + round256((int64_t)sizeof(double) * L.n_slot_doubles);
    return DFQ_OK;
}

int clip_search_plan(const dfq_clip_search_desc* d, int32_t n, ClipLayout& L, std::vector<ClipTask>& tasks,
                     std::vector<ClipFin>& fin, std::vector<int64_t>& urec_base, std::vector<int64_t>& slot_base) {
    const int rc = clip_search_layout(d, n, L);
    if (rc != DFQ_OK) return rc;
    tasks.clear();
    tasks.reserve((size_t)L.n_tasks);
    fin.clear();
    fin.reserve((size_t)L.n_split_units);
    urec_base.assign((size_t)n, -1);
    slot_base.assign((size_t)n, -1);
    int64_t urecs = 0, slots = 0;
    for (int32_t p = 0; p < n; ++p) {   // the pieces of every split weight first
        const int64_t units = clip_units(d[p]), len = clip_unit_len(d[p]);
        if (len <= kClipPiece) continue;
        const int64_t np = units * clip_pieces(len);
        urec_base[p] = urecs;
        slot_base[p] = slots;
        urecs += units;
        slots += np * d[p].candidates;
        for (int64_t s = 0; s < np; ++s) tasks.push_back(ClipTask{p, 0, s});
        for (int64_t u = 0; u < units; ++u) fin.push_back(ClipFin{p, 0, u});
    }
    for (int32_t p = 0; p < n; ++p) {
        const int64_t units = clip_units(d[p]), len = clip_unit_len(d[p]);
        if (len > kClipPiece) continue;
        const int64_t per = clip_units_per_task(len);
        for (int64_t u = 0; u < units; u += per)
            tasks.push_back(ClipTask{p, (int32_t)(units - u < per ? units - u : per), u});
    }
    return DFQ_OK;
}

}  // namespace dfq

extern "C" int64_t dfq_clip_search_ws_bytes(const dfq_clip_search_desc* descs, int32_t n) {
    dfq::ClipLayout L;
    if (dfq::clip_search_layout(descs, n, L) != DFQ_OK) return -1;
    return L.total > 256 ? L.total : 256;
}
