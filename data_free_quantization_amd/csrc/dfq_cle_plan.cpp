// The CLE loop's planner: from the relations' and targets' shapes and tensor
// identities to the tables of the device-resident loop (dfq_cle.hip) -- chains and
// steps, rescale / range tasks, metric chunks and units, the lagged placement, and
// the facts the launches derive from them (which step kernel, how many tiled chunks) --
// in phases that each take and return a small struct.  Plain C++: no device
// memory, no HIP call (the addresses are only compared), so it also builds and
// runs on its own (tests/native/cle_plan_check.cpp).
#include "dfq_cle_plan.h"

#include <algorithm>
#include <atomic>
#include <climits>
#include <cstdio>
#include <cstring>
#include <list>
#include <mutex>
#include <numeric>
#include <utility>

namespace dfq {

CleSwitches CleSwitches::from_env() {
    CleSwitches sw;
    auto rows = [](const char* name, int64_t dflt) {
        const char* e = ab_env(name);
        return e && *e ? std::max<int64_t>(1, atoll(e)) : dflt;
    };
    if (const char* e = ab_env("DFQ_CLE_FUSED")) sw.fused = e[0] != '0';
    sw.w1_mult = rows("DFQ_CLE_W1_ROWS", 0);
    sw.dw_mult = rows("DFQ_CLE_DW_ROWS", kCleDwRowsMult);
    if (const char* e = ab_env("DFQ_CLE_LAG")) sw.lag = e[0] != '0';
    if (const char* e = ab_env("DFQ_CLE_STOP")) sw.stop_arrival = e[0] == 'a';
    if (const char* e = ab_env("DFQ_CLE_BAND")) sw.band = atoi(e);
    return sw;
}
void CleSwitches::append_to(std::vector<int64_t>& key) const {
    key.insert(key.end(), {(int64_t)fused, w1_mult, dw_mult, (int64_t)lag, (int64_t)stop_arrival, (int64_t)band});
}

int cle_rels_from_desc(const dfq_cle_rel* rels, int32_t n_rel, std::vector<CleRel>& R, int64_t& M) {
    R.assign(n_rel, CleRel{});
    M = 0;
    for (int32_t r = 0; r < n_rel; ++r) {
        const dfq_cle_rel& d = rels[r];
        if (!d.w1 || !d.w2 || !d.b1 || d.c1 <= 0 || d.len1 <= 0 || d.o2 <= 0 || d.i2 <= 0 || d.khw2 <= 0)
            return DFQ_ERR_INVALID;
        int64_t groups = 1;
        if (d.c1 != d.i2) {
            groups = d.c1 / d.i2;
            if (groups <= 0 || groups * d.i2 != d.c1) return DFQ_ERR_SHAPE;
        }
        if (d.o2 % groups != 0) return DFQ_ERR_SHAPE;
        CleRel c{};
        c.w1 = d.w1; c.w2 = d.w2; c.b1 = d.b1; c.bnw = d.bn_w; c.bnb = d.bn_b; c.sacc = d.s_acc;
        c.c1 = d.c1; c.len1 = d.len1; c.o2 = d.o2; c.i2 = d.i2; c.khw2 = d.khw2; c.o2g = d.o2 / groups;
        c.moff = M;
        c.sacc_init = d.s_acc_init;
        c.vec1 = (d.len1 % 4 == 0 && reinterpret_cast<uintptr_t>(d.w1) % 16 == 0) ? 1 : 0;
        c.vec2 = (d.i2 == 1 && (c.o2g * d.khw2) % 4 == 0 && reinterpret_cast<uintptr_t>(d.w2) % 16 == 0) ? 1 : 0;
        c.fuse_next = -1;
        c.dw_prev = -1;
        c.w1_self = 0;
        c.w2_self = 0;
        M += 2 * d.c1;
        R[r] = c;
    }
    return DFQ_OK;
}

// Weight elements a rescale task reads and writes (per-channel vector tasks: none)
// and a range task reads (resets: none); the callers put the bytes per element.
static int64_t cle_apply_elems(const CleTask& tk, const CleRel& q) {
    const int64_t n = tk.b - tk.a;
    switch (tk.kind) {
        case kApplyW1: return n * q.len1;
        case kApplyW2Tile: return n * (tk.c1 - tk.c0) * q.khw2;
        case kApplyChannels: return 0;
        default: return n * q.o2g * q.khw2;   // kApplyW2Contig, kApplyDwBoth
    }
}
static int64_t cle_range_elems(const CleTask& tk, const CleRel& q) {
    const int64_t n = tk.b - tk.a;
    switch (tk.kind) {
        case kRangeW1: return n * q.len1;
        case kRangeW2Contig: return n * q.o2g * q.khw2;
        case kRangeW2Tile: return n * (tk.c1 - tk.c0) * q.khw2;
        default: return 0;
    }
}

// ---- phase 1: chains and steps, the fused / depthwise pairing ---------------------
struct CleChains {
    int32_t chains = 0, steps = 0;
    bool fused = true;
    std::vector<int32_t> step_of;   // per relation: its rescale launch
    std::vector<int32_t> w1_src;    // >= 0: the relation whose W2 rescale produces this W1's row ranges
    std::vector<int32_t> dw_next;   // >= 0: the relation paired with this one's depthwise W2
};

// Sets fuse_next / dw_prev of R.
static CleChains cle_chains(std::vector<CleRel>& R, const CleSwitches& sw) {
    const int32_t n_rel = (int32_t)R.size();
    CleChains C;
    // chains: connected components over the tensors a relation touches
    std::vector<int32_t> parent(n_rel);
    std::iota(parent.begin(), parent.end(), 0);
    auto find = [&](int32_t x) {
        while (parent[x] != x) x = parent[x] = parent[parent[x]];
        return x;
    };
    for (int32_t a = 0; a < n_rel; ++a) {
        const void* pa[5] = {R[a].w1, R[a].w2, R[a].b1, R[a].bnw, R[a].bnb};
        for (int32_t b = 0; b < a; ++b) {
            const void* pb[5] = {R[b].w1, R[b].w2, R[b].b1, R[b].bnw, R[b].bnb};
            bool share = false;
            for (int i = 0; i < 5 && !share; ++i)
                for (int j = 0; j < 5 && !share; ++j) share = pa[i] && pa[i] == pb[j];
            if (share) parent[find(a)] = find(b);
        }
    }
    std::vector<int32_t> comp_len(n_rel, 0);
    C.step_of.resize(n_rel);
    for (int32_t r = 0; r < n_rel; ++r) {
        const int32_t c = find(r);
        if (comp_len[c] == 0) ++C.chains;
        C.step_of[r] = comp_len[c]++;
        C.steps = std::max(C.steps, C.step_of[r] + 1);
    }
    // Fused schedule: a relation's W2 must be untouched by the earlier relations of
    // its chain (its column range can be taken at the start of the iteration), and
    // its W1 untouched too, or the W2 of the immediately preceding relation -- whose
    // rescale then produces the W1 row ranges.  Otherwise: per-step range launches.
    C.w1_src.assign(n_rel, -1);
    C.fused = sw.fused;
    std::vector<std::vector<int32_t>> chain_of(n_rel);
    for (int32_t r = 0; r < n_rel; ++r) chain_of[find(r)].push_back(r);
    for (const auto& L : chain_of) {
        for (size_t j = 0; j < L.size() && C.fused; ++j) {
            const CleRel& cr = R[L[j]];
            for (size_t i = 0; i < j && C.fused; ++i) {
                const CleRel& cq = R[L[i]];
                if (cq.w1 == cr.w2 || cq.w2 == cr.w2) C.fused = false;
                if (cq.w1 == cr.w1 || cq.w2 == cr.w1) {
                    const bool ok = i + 1 == j && cq.w2 == cr.w1 && cq.w1 != cr.w1 && C.w1_src[L[j]] < 0 &&
                                    (cq.i2 > 1 || cq.o2g == 1) && cr.c1 == cq.o2 && cr.len1 == cq.i2 * cq.khw2;
                    if (ok) C.w1_src[L[j]] = L[i];
                    else C.fused = false;
                }
            }
        }
    }
    if (C.fused)
        for (int32_t r = 0; r < n_rel; ++r)
            if (C.w1_src[r] >= 0) R[C.w1_src[r]].fuse_next = r;
    // Depthwise pairs (fused schedule): relation r whose W1 is the depthwise W2 of
    // the relation q right before it in its chain runs in q's launch: its W1 row
    // ranges are derived from q's W2 range words (cle_rel_scale), q's filter
    // rescale and r's W1 rescale become ONE task (kApplyDwBoth), and r no longer
    // needs W1 range words.  MobileNetV2: 5 rescale launches per iteration -> 3.
    C.dw_next.assign(n_rel, -1);
    if (C.fused) {
        for (int32_t r = 0; r < n_rel; ++r) {
            const int32_t q = C.w1_src[r];
            if (q < 0 || R[q].dw_prev >= 0 || C.dw_next[q] >= 0) continue;
            const CleRel& cq = R[q];
            const CleRel& cr = R[r];
            const bool dw = cq.i2 == 1 && cq.o2g == 1 && cq.o2 == cq.c1 && cr.c1 == cq.o2 && cr.len1 == cq.khw2;
            if (!dw) continue;
            R[r].dw_prev = q;
            R[q].fuse_next = -1;   // no range words to produce for r's W1
            C.dw_next[q] = r;
        }
        // steps again: a depthwise-paired relation shares its predecessor's step
        std::vector<int32_t> cur(n_rel, 0);
        C.steps = 0;
        for (int32_t r = 0; r < n_rel; ++r) {
            const int32_t c = find(r);
            C.step_of[r] = R[r].dw_prev >= 0 ? C.step_of[R[r].dw_prev] : cur[c]++;
            C.steps = std::max(C.steps, C.step_of[r] + 1);
        }
    }
    return C;
}

// ---- phase 2: range and rescale tasks ----------------------------------------------
struct CleTaskTables {
    std::vector<CleTask> rt, at;
    std::vector<int64_t> rstep{0}, astep{0};   // task offsets per step
    int64_t ri0 = 0, ri1 = 0;                  // fused: each iteration's range tasks
};

static void cle_w2_range_tasks(const CleRel& c, int32_t r, std::vector<CleTask>& out) {
    if (c.i2 == 1) {
        const int64_t k = rows_per_task(c.o2g * c.khw2);
        for (int64_t a = 0; a < c.c1; a += k) out.push_back({r, kRangeW2Contig, a, std::min<int64_t>(a + k, c.c1), 0, 0});
    } else {
        for (int64_t a = 0; a < c.o2; a += kColTileRows)
            for (int64_t i0 = 0; i0 < c.i2; i0 += kThreads)
                out.push_back({r, kRangeW2Tile, a, std::min<int64_t>(a + kColTileRows, c.o2), i0,
                               std::min<int64_t>(i0 + kThreads, c.i2)});
        for (int64_t a = 0; a < c.c1; a += kCleChansPerTask)
            out.push_back({r, kRangeReset, a, std::min<int64_t>(a + kCleChansPerTask, c.c1), 0, 0});
    }
}
// produced: the previous relation's rescale writes this W1's row ranges (reset the next parity)
static void cle_w1_range_tasks(const CleRel& c, int32_t r, bool produced, std::vector<CleTask>& out) {
    if (c.dw_prev >= 0) return;   // derived from the depthwise predecessor's W2 words
    const int32_t kind = produced ? kRangeResetW1 : kRangeW1;
    const int64_t k = produced ? kCleChansPerTask : rows_per_task(c.len1);
    for (int64_t a = 0; a < c.c1; a += k) out.push_back({r, kind, a, std::min<int64_t>(a + k, c.c1), 0, 0});
}
static void cle_apply_tasks(const CleRel& c, int32_t r, int32_t dw_next, const CleSwitches& sw,
                            std::vector<CleTask>& out) {
    // rows per W1 / depthwise-pair rescale task: rows_per_task (one row per wave)
    // times a factor: twice the rows for tasks of short rows, or the switches'
    if (c.dw_prev < 0) {   // else the predecessor's kApplyDwBoth rescales this W1
        int64_t k = rows_per_task(c.len1);
        k = sw.w1_mult > 0 ? sw.w1_mult * k : (k * c.len1 < kCleW1SmallElems ? 2 * k : k);
        for (int64_t a = 0; a < c.c1; a += k) out.push_back({r, kApplyW1, a, std::min<int64_t>(a + k, c.c1), 0, 0});
    }
    if (dw_next >= 0) {
        for (int64_t a = 0, k = sw.dw_mult * rows_per_task(c.o2g * c.khw2); a < c.c1; a += k)
            out.push_back({r, kApplyDwBoth, a, std::min<int64_t>(a + k, c.c1), dw_next, 0});
    } else if (c.i2 == 1) {
        for (int64_t a = 0, k = rows_per_task(c.o2g * c.khw2); a < c.c1; a += k)
            out.push_back({r, kApplyW2Contig, a, std::min<int64_t>(a + k, c.c1), 0, 0});
    } else {
        // KH*KW > 1 tiles go position-parallel, a row at a time: fewer rows per
        // task, more tasks in flight (ResNet-50's 3x3 W2 tiles: 16 rows took
        // ~70 us, DFQ_CLE_TL); 1x1 tiles keep kColTileRows (loads issued together)
        const int64_t rows = (c.khw2 > 1 && c.khw2 <= kTileMaxKhw) ? kPosTileMaxRows : kColTileRows;
        for (int64_t a = 0; a < c.o2; a += rows)
            for (int64_t i0 = 0; i0 < c.i2; i0 += kThreads)
                out.push_back({r, kApplyW2Tile, a, std::min<int64_t>(a + rows, c.o2), i0,
                               std::min<int64_t>(i0 + kThreads, c.i2)});
    }
    // one channel per thread: each channel's scale is a chain of dependent loads
    // and fp32 divides, and 1,024-channel tasks (4 channels a thread, one after
    // the other) were the slowest of their steps (6-9 us, DFQ_CLE_TL)
    for (int64_t a = 0; a < c.c1; a += kThreads)
        out.push_back({r, kApplyChannels, a, std::min<int64_t>(a + kThreads, c.c1), 0, 0});
}

// Per-step range + rescale launches, or (fused) one range launch for every
// relation's W2 (and untouched W1) followed by the rescale launches.  Sets
// w1_self / w2_self of R.
static CleTaskTables cle_tasks(std::vector<CleRel>& R, const CleChains& C, const CleSwitches& sw) {
    const int32_t n_rel = (int32_t)R.size();
    CleTaskTables T;
    auto range_tasks = [&](int32_t r) {
        cle_w1_range_tasks(R[r], r, C.fused && C.w1_src[r] >= 0, T.rt);
        cle_w2_range_tasks(R[r], r, T.rt);
    };
    if (C.fused) {
        for (int32_t r = 0; r < n_rel; ++r) range_tasks(r);
        T.rstep.push_back((int64_t)T.rt.size());
        // Self ranges: a W1 that no earlier relation of its chain touches is final
        // once its own row rescale ran, so that task writes the row's next range
        // (no kRangeW1 task); likewise a depthwise W2 after kApplyDwBoth.  The
        // first iteration's ranges still come from the full list [rstep0, rstep1);
        // each iteration's tiles launch runs the rest, [ri0, ri1).
        for (int32_t r = 0; r < n_rel; ++r) {
            if (C.w1_src[r] < 0 && R[r].dw_prev < 0) R[r].w1_self = 1;
            if (C.dw_next[r] >= 0) R[r].w2_self = 1;
        }
        T.ri0 = (int64_t)T.rt.size();
        for (int64_t t = T.rstep[0]; t < T.rstep[1]; ++t) {
            const CleTask tk = T.rt[t];
            if (tk.kind == kRangeW1 && R[tk.rel].w1_self) continue;
            if (tk.kind == kRangeW2Contig && R[tk.rel].w2_self) continue;
            T.rt.push_back(tk);
        }
        T.ri1 = (int64_t)T.rt.size();
    }
    for (int32_t k = 0; k < C.steps; ++k) {
        for (int32_t r = 0; r < n_rel; ++r) {
            if (C.step_of[r] != k) continue;
            if (!C.fused) range_tasks(r);
            cle_apply_tasks(R[r], r, C.dw_next[r], sw, T.at);
        }
        // The step's slowest tasks first (its span is the last task's end): W2 row
        // tiles (strided columns, their loads and stores a row at a time), the
        // per-channel vectors (each a chain of dependent loads), then the depthwise
        // pairs, W1 rows and contiguous W2 channels (profiles/r03/cle_tl_*.log: tile
        // tasks started up to 10 us into a step and ran ~10 us)
        auto prio = [](int32_t kind) {
            switch (kind) {
                case kApplyW2Tile: return 0;
                case kApplyChannels: return 1;
                case kApplyDwBoth: return 2;
                case kApplyW1: return 3;
                default: return 4;
            }
        };
        std::stable_sort(T.at.begin() + T.astep.back(), T.at.end(),
                         [&](const CleTask& x, const CleTask& y) { return prio(x.kind) < prio(y.kind); });
        if (!C.fused) T.rstep.push_back((int64_t)T.rt.size());
        T.astep.push_back((int64_t)T.at.size());
    }
    return T;
}

// ---- phase 3: metric chunks and units -----------------------------------------------
struct CleMetric {
    std::vector<CleLayer> layers;
    std::vector<CleChunk> chunks;
    std::vector<CleUnit> units;
    std::vector<int64_t> b1off;
    int64_t nb1_total = 0;
};

// torch.mean = sum / n; the sum is two_pass_reduction over
// min(threads, ceil(n / 32768)) equal chunks when n >= 32768 (serial below)
static int cle_metric(float* const* targets, const int64_t* target_n, int32_t n_targets, int32_t ref_threads,
                      CleMetric& X) {
    X.layers.resize(n_targets);
    for (int32_t l = 0; l < n_targets; ++l) {
        const int64_t n = target_n[l];
        if (!targets[l] || n <= 0) return DFQ_ERR_INVALID;
        X.layers[l] = CleLayer{nullptr, nullptr, n, 1};   // the tensor and its snapshot: bound per plan
        int64_t nt = 1;
        if (n >= 32768 && ref_threads > 1) nt = std::min<int64_t>(ref_threads, ceil_div(n, (int64_t)32768));
        X.layers[l].nt = nt;
        const int64_t chunk = ceil_div(n, nt);
        for (int64_t t = 0; t < nt; ++t) {
            const int64_t b = t * chunk;
            if (b >= n) break;
            const int64_t len = std::min<int64_t>(n, b + chunk) - b;
            const int64_t sz = len / 32;
            if (aten_ceil_log2(sz) / 4 > 4) return DFQ_ERR_UNSUPPORTED;   // > 16M / chunk
            const int32_t ci = (int32_t)X.chunks.size();
            X.chunks.push_back(CleChunk{l, (int32_t)t, b, len});
            const int64_t nb1 = sz / 256;
            X.b1off.push_back(32 * X.nb1_total);   // float offset of this chunk's [nb1][32] level-1 sums
            X.nb1_total += nb1;
            if (len >= 8)
                for (int64_t g = 0; g <= nb1; ++g) X.units.push_back(CleUnit{ci, (int32_t)g});
        }
    }
    return DFQ_OK;
}

// ---- phase 4: placement of the metric tiles and the next iteration's range tasks ----
// An iteration group has nlaunch launches: the steps' rescale launches (and, in the
// round-4 schedule, one tiles-only launch after them).  Every tile unit and
// range task gets an OFFSET in [0, 2 nlaunch): offset k < nlaunch runs in
// launch k of its own iteration's group, offset nlaunch + k in launch k of the
// next group.  A tensor's tiles and ranges must run after its last rescale of
// iteration i and before its first rescale of iteration i + 1: offsets
// [last + 1, nlaunch + first - 1].  Resets of a relation's range words go after
// that relation's own step and before the next accumulation.
// Lagged schedule (nlaunch = steps: no tiles-only launch): the tiles of one
// iteration sit in a band of nlaunch - 1 offsets and the stop rule runs as a
// block of its own one offset after the band (it reads the chunk sums the
// tiles' last arrivals left, after a launch boundary): iteration i's stop rule
// runs beside the rescale tasks of iteration i + 1 instead of after a serial
// tile -> chunk-combine -> stop-rule chain in a launch of its own, and every
// tile of iteration i + 1 starts after it (cle_loop_step_kernel).
// MobileNetV2: 4 -> 3 launches per iteration.  Needs the fused range schedule
// and no tiny chunks (the stop rule takes their sums from the live weights);
// where no band fits (ResNet-50: a tensor rescaled at both steps) or without
// lag (DFQ_CLE_LAG=0, diagnostics): the round-4 schedule, everything in the
// tiles-only launch and the stop rule at the last tile arrival.
struct ClePlacement {
    std::vector<int32_t> layer_off;   // per target layer: its tiles' offset
    std::vector<int32_t> rt_off;      // per range task of [ri0, ri1)
    int32_t nlaunch = 0;
    int32_t stop_off = -1;   // lagged: the stop rule's own block at this offset (else: the last tile arrival)
    bool lagged = false;
};

// (first, last) step of every tensor the relations rescale: a linear table (a few
// hundred tensors at most), looked up once per relation and target layer
struct CleSpans {
    std::vector<const float*> w;
    std::vector<std::pair<int32_t, int32_t>> v;
    std::vector<int32_t> rel_t1, rel_t2;   // per relation: its W1's / W2's entry
    std::vector<int32_t> lay_t;            // per target layer: its entry, or -1 (untouched)
    int32_t find(const float* p) const {
        for (size_t i = 0; i < w.size(); ++i)
            if (w[i] == p) return (int32_t)i;
        return -1;
    }
};
static CleSpans cle_spans(const std::vector<CleRel>& R, const CleChains& C, float* const* targets, int32_t n_targets) {
    const int32_t n_rel = (int32_t)R.size();
    CleSpans P;
    P.rel_t1.resize(n_rel);
    P.rel_t2.resize(n_rel);
    for (int32_t r = 0; r < n_rel; ++r)
        for (int side = 0; side < 2; ++side) {
            const float* w = side ? R[r].w2 : R[r].w1;
            int32_t i = P.find(w);
            if (i < 0) {
                i = (int32_t)P.w.size();
                P.w.push_back(w);
                P.v.push_back({C.step_of[r], C.step_of[r]});
            } else {
                P.v[i] = {std::min(P.v[i].first, C.step_of[r]), std::max(P.v[i].second, C.step_of[r])};
            }
            (side ? P.rel_t2 : P.rel_t1)[r] = i;
        }
    P.lay_t.resize(n_targets);
    for (int32_t l = 0; l < n_targets; ++l) P.lay_t[l] = P.find(targets[l]);
    return P;
}

// The lagged placement for groups of nl launches: loads in bytes per launch
// position of a group -- the steps' rescale traffic, then greedy by size: each
// range task and each layer's tiles to the least-loaded admissible offset.
// False: no band fits.  lag_max: the placement's largest tile offset.
static bool cle_place_lagged(int32_t nl, const std::vector<CleRel>& R, const CleChains& C, const CleTaskTables& T,
                             const CleSpans& P, const int64_t* target_n, int32_t n_targets, const CleSwitches& sw,
                             ClePlacement& out, int32_t& lag_max) {
    auto window = [&](int32_t ti) -> std::pair<int32_t, int32_t> {   // [lo, hi] offsets (untouched: anywhere)
        if (ti < 0) return {0, 2 * nl - 1};
        return {P.v[ti].second + 1, std::min(2 * nl - 1, nl + P.v[ti].first - 1)};
    };
    std::vector<double> base_load(nl, 0.0);
    for (int32_t k = 0; k < C.steps && k < nl; ++k)
        for (int64_t t = T.astep[k]; t < T.astep[k + 1]; ++t)
            base_load[k] += 8.0 * (double)cle_apply_elems(T.at[t], R[T.at[t].rel]);
    // range tasks: their own windows and bytes
    const int64_t nr = T.ri1 - T.ri0;
    std::vector<std::pair<int32_t, int32_t>> rwin((size_t)nr);
    std::vector<double> rbytes((size_t)nr);
    for (int64_t x = 0; x < nr; ++x) {
        const CleTask& tk = T.rt[T.ri0 + x];
        std::pair<int32_t, int32_t> w;
        switch (tk.kind) {
            case kRangeW1: w = window(P.rel_t1[tk.rel]); break;
            case kRangeW2Contig:
            case kRangeW2Tile: w = window(P.rel_t2[tk.rel]); break;
            case kRangeReset:   // after the consumer step, before the next accumulation (>= nl + last + 1)
                w = {C.step_of[tk.rel] + 1, std::min(2 * nl - 1, nl + P.v[P.rel_t2[tk.rel]].second)};
                break;
            default:            // kRangeResetW1: after the consumer step, before the producer's step two groups on
                w = {C.step_of[tk.rel] + 1, 2 * nl - 1};
        }
        if (w.first > w.second) return false;
        rwin[x] = w;
        rbytes[x] = tk.kind >= kRangeReset ? 64.0 : 4.0 * (double)cle_range_elems(tk, R[tk.rel]);
    }
    // tiles: a band [B0, B0 + nl - 2] meeting every layer's window; the stop
    // rule one offset after the band's last used offset
    int32_t maxlo = 0, minhi = 2 * nl - 1;
    std::vector<std::pair<int32_t, int32_t>> lwin(n_targets);
    for (int32_t l = 0; l < n_targets; ++l) {
        lwin[l] = window(P.lay_t[l]);
        if (lwin[l].first > lwin[l].second) return false;
        maxlo = std::max(maxlo, lwin[l].first);
        minhi = std::min(minhi, lwin[l].second);
    }
    const int32_t bw = sw.stop_arrival ? nl : nl - 1;   // band width
    if (bw < 1) return false;
    const int32_t b_lo = std::max(0, maxlo - bw + 1), b_hi = std::min(minhi, 2 * nl - 1 - bw);
    if (b_lo > b_hi) return false;
    std::vector<int32_t> lord(n_targets);
    std::iota(lord.begin(), lord.end(), 0);
    std::sort(lord.begin(), lord.end(),
              [&](int32_t x, int32_t y) { return target_n[x] != target_n[y] ? target_n[x] > target_n[y] : x < y; });
    std::vector<int64_t> rord((size_t)nr);
    std::iota(rord.begin(), rord.end(), 0);
    std::sort(rord.begin(), rord.end(),
              [&](int64_t x, int64_t y) { return rbytes[x] != rbytes[y] ? rbytes[x] > rbytes[y] : x < y; });
    double best = 1e300;
    std::vector<int32_t> roff((size_t)nr), loff(n_targets);
    for (int32_t B0 = b_lo; B0 <= b_hi; ++B0) {
        if (sw.band >= 0 && B0 != sw.band && sw.band >= b_lo && sw.band <= b_hi) continue;
        std::vector<double> load = base_load;
        auto pick = [&](int32_t lo, int32_t hi, double bytes) {
            int32_t bo = lo;
            for (int32_t o = lo; o <= hi; ++o)
                if (load[o % nl] < load[bo % nl]) bo = o;
            load[bo % nl] += bytes;
            return bo;
        };
        for (int64_t x : rord) roff[x] = pick(rwin[x].first, rwin[x].second, rbytes[x]);
        int32_t maxoff = 0;
        for (int32_t l : lord) {
            loff[l] = pick(std::max(lwin[l].first, B0), std::min(lwin[l].second, B0 + bw - 1), 12.0 * target_n[l]);
            maxoff = std::max(maxoff, loff[l]);
        }
        if (!sw.stop_arrival && maxoff + 1 > 2 * nl - 1) continue;
        double cost = *std::max_element(load.begin(), load.end());
        if (cost < best) {
            best = cost;
            out.layer_off = loff;
            out.rt_off = roff;
            out.stop_off = sw.stop_arrival ? -1 : maxoff + 1;
            lag_max = maxoff;
        }
    }
    return best < 1e300;
}

static ClePlacement cle_place(const std::vector<CleRel>& R, const CleChains& C, const CleTaskTables& T,
                              const CleMetric& X, float* const* targets, const int64_t* target_n, int32_t n_targets,
                              const CleSwitches& sw) {
    const bool tiny = std::any_of(X.chunks.begin(), X.chunks.end(), [](const CleChunk& c) { return c.len < 8; });
    const bool have_tiles = std::any_of(X.chunks.begin(), X.chunks.end(), [](const CleChunk& c) { return c.len >= 8; });
    const bool lag_ok = C.fused && !tiny && have_tiles && C.steps > 0 && sw.lag;
    ClePlacement P;
    int32_t lag_max = -1;
    if (lag_ok &&
        cle_place_lagged(C.steps, R, C, T, cle_spans(R, C, targets, n_targets), target_n, n_targets, sw, P, lag_max) &&
        (sw.stop_arrival ? lag_max >= C.steps : P.stop_off >= C.steps)) {
        P.nlaunch = C.steps;
        P.lagged = true;
    } else {   // everything in the tiles-only launch after the steps (offset steps), the stop rule at the last arrival
        P.nlaunch = C.steps + 1;
        P.stop_off = -1;
        P.layer_off.assign(n_targets, C.steps);
        P.rt_off.assign((size_t)(T.ri1 - T.ri0), C.steps);
    }
    return P;
}

// ---- phase 5: units and range tasks in offset order: uoffs / roffs -------------------
static void cle_bucket(const ClePlacement& P, bool fused, CleTaskTables& T, CleMetric& X, std::vector<int64_t>& uoffs,
                       std::vector<int64_t>& roffs) {
    const int32_t nb = 2 * P.nlaunch;
    uoffs.assign(nb + 1, 0);
    roffs.assign(nb + 1, 0);
    std::vector<std::vector<CleUnit>> ub(nb);
    for (const CleUnit& u : X.units) ub[P.layer_off[X.chunks[u.chunk].layer]].push_back(u);
    X.units.clear();
    for (int32_t k = 0; k < nb; ++k) {
        uoffs[k] = (int64_t)X.units.size();
        X.units.insert(X.units.end(), ub[k].begin(), ub[k].end());
    }
    uoffs[nb] = (int64_t)X.units.size();
    if (!fused) return;   // (the unfused schedule's range tasks are per step: rstep; roffs stay empty)
    std::vector<std::vector<CleTask>> rb(nb);
    for (int64_t t = T.ri0; t < T.ri1; ++t) rb[P.rt_off[t - T.ri0]].push_back(T.rt[t]);
    T.rt.resize(T.ri0);
    for (int32_t k = 0; k < nb; ++k) {
        roffs[k] = (int64_t)T.rt.size();
        T.rt.insert(T.rt.end(), rb[k].begin(), rb[k].end());
    }
    roffs[nb] = T.ri1 = (int64_t)T.rt.size();
}

// ---- phase 6: algorithmic bytes of one iteration (CleStructure::bytes_*) -------------
static void cle_bytes(CleStructure& S) {
    for (const CleTask& tk : S.at) {
        const CleRel& q = S.R[tk.rel];
        if (tk.kind == kApplyChannels)
            S.bytes_rescale += 8 * (tk.b - tk.a) * ((q.b1 ? 1 : 0) + (q.bnw ? 1 : 0) + (q.bnb ? 1 : 0) + (q.sacc ? 1 : 0));
        else
            S.bytes_rescale += 8 * cle_apply_elems(tk, q);
    }
    for (const CleLayer& l : S.layers) S.bytes_metric += 12 * l.n;
    const int64_t r0 = S.fused ? S.ri0 : 0, r1 = S.fused ? S.ri1 : (int64_t)S.rt.size();
    for (int64_t t = r0; t < r1; ++t) S.bytes_range += 4 * cle_range_elems(S.rt[t], S.R[S.rt[t].rel]);
}

static std::atomic<uint64_t> g_struct_ids{0};

int cle_build_structure(std::vector<CleRel> R, int64_t M, float* const* targets, const int64_t* target_n,
                        int32_t n_targets, int32_t ref_threads, const CleSwitches& sw, CleStructure& S) {
    const double tp1 = now_us();
    const CleChains C = cle_chains(R, sw);
    const double tp2 = now_us();
    CleTaskTables T = cle_tasks(R, C, sw);
    const double tp3 = now_us();
    CleMetric X;
    if (const int rc = cle_metric(targets, target_n, n_targets, ref_threads, X); rc != DFQ_OK) return rc;
    const double tp4 = now_us();
    const ClePlacement P = cle_place(R, C, T, X, targets, target_n, n_targets, sw);
    cle_bucket(P, C.fused, T, X, S.uoffs, S.roffs);
    S.R = std::move(R);
    S.M = M;
    S.chains = C.chains;
    S.steps = C.steps;
    S.fused = C.fused;
    S.rt = std::move(T.rt);
    S.at = std::move(T.at);
    S.rstep = std::move(T.rstep);
    S.astep = std::move(T.astep);
    S.ri0 = T.ri0;
    S.ri1 = T.ri1;
    S.layers = std::move(X.layers);
    S.chunks = std::move(X.chunks);
    S.units = std::move(X.units);
    S.b1off = std::move(X.b1off);
    S.nb1_total = X.nb1_total;
    S.nlaunch = P.nlaunch;
    S.stop_off = P.stop_off;
    S.lagged = P.lagged;
    S.step_pos.assign(std::max<int32_t>(S.steps, 1), 0);
    for (int32_t k = 0; k < S.steps; ++k)
        for (int64_t t = S.astep[k]; t < S.astep[k + 1]; ++t)
            if (S.at[t].kind == kApplyW2Tile && S.R[S.at[t].rel].khw2 > 1) S.step_pos[k] = 1;
    for (const CleChunk& c : S.chunks) S.nbig += c.len >= 8 ? 1 : 0;
    S.id = ++g_struct_ids;
    cle_bytes(S);
    const double tp5 = now_us();
    S.t_chains = tp2 - tp1;
    S.t_tasks = tp3 - tp2;
    S.t_chunks = tp4 - tp3;
    S.t_place = tp5 - tp4;
    return DFQ_OK;
}

// The structure key: shapes, flags and the identity pattern of every tensor
// address (which relation / target slots share a tensor), the metric's thread
// count and the diagnostics library's schedule switches.  Two calls with equal
// keys get equal structures.
static std::vector<int64_t> cle_structure_key(const std::vector<CleRel>& R, int64_t M, float* const* targets,
                                              const int64_t* target_n, int32_t n_targets, int32_t ref_threads,
                                              const CleSwitches& sw) {
    std::vector<std::pair<uintptr_t, int32_t>> ps;
    ps.reserve(5 * R.size() + n_targets);
    for (const CleRel& c : R)
        for (const void* q : {(const void*)c.w1, (const void*)c.w2, (const void*)c.b1, (const void*)c.bnw,
                              (const void*)c.bnb})
            ps.push_back({reinterpret_cast<uintptr_t>(q), (int32_t)ps.size()});
    for (int32_t l = 0; l < n_targets; ++l) ps.push_back({reinterpret_cast<uintptr_t>(targets[l]), (int32_t)ps.size()});
    std::vector<int32_t> id(ps.size());
    std::vector<std::pair<uintptr_t, int32_t>> srt = ps;
    std::sort(srt.begin(), srt.end());
    for (size_t i = 0; i < srt.size();) {   // every slot -> the first slot holding the same address
        size_t j = i;
        while (j < srt.size() && srt[j].first == srt[i].first) ++j;
        for (size_t k = i; k < j; ++k) id[srt[k].second] = srt[i].first ? srt[i].second : -1;
        i = j;
    }
    std::vector<int64_t> key;
    key.reserve(16 * R.size() + 2 * n_targets + 16);
    key.push_back((int64_t)R.size());
    key.push_back(M);
    key.push_back(n_targets);
    key.push_back(ref_threads);
    sw.append_to(key);
    size_t q = 0;
    for (const CleRel& c : R) {
        key.insert(key.end(), {c.c1, c.len1, c.o2, c.i2, c.khw2, (int64_t)c.sacc_init, (int64_t)c.vec1, (int64_t)c.vec2,
                               (int64_t)(c.sacc != nullptr)});
        for (int k = 0; k < 5; ++k) key.push_back(id[q++]);
    }
    for (int32_t l = 0; l < n_targets; ++l) {
        key.push_back(target_n[l]);
        key.push_back(id[q++]);
    }
    return key;
}

std::shared_ptr<const CleStructure> cle_structure_cached(const std::vector<CleRel>& R, int64_t M,
                                                         float* const* targets, const int64_t* target_n,
                                                         int32_t n_targets, int32_t ref_threads, int& rc, bool& cached) {
    static std::mutex mu;
    static std::list<std::pair<std::vector<int64_t>, std::shared_ptr<const CleStructure>>> cache;   // most recent first
    constexpr size_t kCap = 8;
    rc = DFQ_OK;
    cached = false;
    const CleSwitches sw = CleSwitches::from_env();
    const std::vector<int64_t> key = cle_structure_key(R, M, targets, target_n, n_targets, ref_threads, sw);
    {
        std::lock_guard<std::mutex> lock(mu);
        for (auto it = cache.begin(); it != cache.end(); ++it)
            if (it->first == key) {
                cache.splice(cache.begin(), cache, it);
                cached = true;
                return it->second;
            }
    }
    auto built = std::make_shared<CleStructure>();
    rc = cle_build_structure(R, M, targets, target_n, n_targets, ref_threads, sw, *built);
    if (rc != DFQ_OK) return nullptr;
    std::lock_guard<std::mutex> lock(mu);
    cache.emplace_front(key, built);
    if (cache.size() > kCap) cache.pop_back();
    return built;
}

}  // namespace dfq

#ifdef DFQ_DIAGNOSTICS
#include "dfq_diag.h"   // default visibility for the entry point below
using namespace dfq;

// 64-bit FNV-1a over every address-free field of the structure (each as eight
// little-endian bytes of an int64): what tests/golden/cle_structure_digests.json
// pins.  No pointer, no id, no timing field.
static uint64_t cle_structure_digest(const CleStructure& S) {
    uint64_t h = 0xcbf29ce484222325ull;
    auto put = [&](int64_t v) {
        for (int i = 0; i < 8; ++i) h = (h ^ (((uint64_t)v >> (8 * i)) & 0xff)) * 0x100000001b3ull;
    };
    auto put_all = [&](const std::vector<int64_t>& v) {
        put((int64_t)v.size());
        for (int64_t x : v) put(x);
    };
    auto put_tasks = [&](const std::vector<CleTask>& v) {
        put((int64_t)v.size());
        for (const CleTask& t : v)
            for (int64_t x : {(int64_t)t.rel, (int64_t)t.kind, t.a, t.b, t.c0, t.c1}) put(x);
    };
    for (int64_t x : {S.M, (int64_t)S.chains, (int64_t)S.steps, (int64_t)S.fused, (int64_t)S.lagged, (int64_t)S.nlaunch,
                      (int64_t)S.stop_off, S.ri0, S.ri1, S.nb1_total})
        put(x);
    put((int64_t)S.R.size());
    for (const CleRel& c : S.R)
        for (int64_t x : {c.moff, (int64_t)c.vec1, (int64_t)c.vec2, (int64_t)c.fuse_next, (int64_t)c.dw_prev,
                          (int64_t)c.w1_self, (int64_t)c.w2_self, c.o2g})
            put(x);
    put_tasks(S.at);
    put_tasks(S.rt);
    put_all(S.rstep);
    put_all(S.astep);
    put((int64_t)S.layers.size());
    for (const CleLayer& l : S.layers) put(l.n), put(l.nt);
    put((int64_t)S.chunks.size());
    for (const CleChunk& c : S.chunks) put(c.layer), put(c.t), put(c.c0), put(c.len);
    put((int64_t)S.units.size());
    for (const CleUnit& u : S.units) put(u.chunk), put(u.tile);
    put_all(S.b1off);
    put_all(S.uoffs);
    put_all(S.roffs);
    put(S.bytes_rescale), put(S.bytes_metric), put(S.bytes_range);
    return h;
}

// ---- diagnostics: the plan structure's index invariants, on the host -----------
// Builds the structure dfq_cle_plan_create would (chains, tasks, metric chunks and
// units, the lagged placement) -- host code only, no device memory, so it runs on
// a machine without a GPU and with stand-in addresses -- and checks every index
// the step, range, tile, stop-rule and rollback blocks derive from it:
//  * task tables: step offsets monotone and inside the tables; every task's
//    relation, rows / channels / columns inside that relation's shapes;
//  * range words and rollback saves: moff + 2 c1 <= M (both parities' words) and
//    2 moff + 4 c1 <= 2 M (vsave: b1 | bn_w | bn_b | S per channel);
//  * the facts the launches read: step_pos (which cle_loop_step_kernel a step
//    launches) recomputed from the step's tasks, nbig from the chunks;
//  * metric chunks and units: layer, element span, level-1 slots inside the tables;
//  * placement: per launch offset the unit / range slices partition the tables;
//    a tensor's tiles and ranges sit after its last rescale of iteration i and
//    before its first rescale of iteration i + 1 (its window), range resets after
//    their relation's step; lagged plans: the stop rule one offset after every tile
//    of its iteration and before the next iteration's first tile.
// The round-5 fault of a development tree was in this code's
// domain; tests/test_cle_structure.py runs it on every zoo model and schedule
// switch and on fuzzed relation graphs.
// info[0..7] = steps, nlaunch, lagged, stop_off, rescale tasks, range tasks, units,
// chunks (eight slots, as every caller's buffer has held).  Returns DFQ_OK with
// "digest <16 hex digits>" (cle_structure_digest) in msg, or DFQ_ERR_INVALID with
// the first violation in msg.
extern "C" int dfq_diag_cle_check_structure(const dfq_cle_rel* rels, int32_t n_rel, float* const* targets,
                                            const int64_t* target_n, int32_t n_targets, int32_t ref_threads,
                                            int64_t* info, char* msg, int32_t msg_cap) {
    auto fail = [&](const char* fmt, long long a, long long b, long long c) {
        if (msg && msg_cap > 0) snprintf(msg, (size_t)msg_cap, fmt, a, b, c);
        return DFQ_ERR_INVALID;
    };
    if (n_rel < 0 || n_targets < 0 || (n_rel > 0 && !rels) || (n_targets > 0 && (!targets || !target_n)))
        return fail("bad arguments %lld %lld %lld", n_rel, n_targets, 0);
    std::vector<CleRel> R0;
    int64_t M = 0;
    if (const int rc = cle_rels_from_desc(rels, n_rel, R0, M); rc != DFQ_OK) return rc;
    CleStructure S;
    if (const int rc = cle_build_structure(R0, M, targets, target_n, n_targets, ref_threads, CleSwitches::from_env(), S);
        rc != DFQ_OK)
        return rc;
    const std::vector<CleRel>& R = S.R;
    const int32_t steps = S.steps, NL = S.nlaunch;
    if (const char* e = getenv("DFQ_CLE_PLACE_DUMP"); e && *e) {
        // per launch offset: blocks and bytes of rescale tasks, metric tiles and range tasks
        fprintf(stderr, "DFQ_CLE_PLACE steps %d nlaunch %d lagged %d stop_off %d\n", steps, NL, (int)S.lagged,
                S.stop_off);
        for (int32_t k = 0; k < 2 * NL; ++k) {
            int64_t na = 0;
            double ba = 0;
            if (k < steps)
                for (int64_t t = S.astep[k]; t < S.astep[k + 1]; ++t, ++na)
                    ba += 8.0 * (double)cle_apply_elems(S.at[t], R[S.at[t].rel]);
            double bu = 0;
            for (int64_t u = S.uoffs[k]; u < S.uoffs[k + 1]; ++u) {
                const CleChunk& ch = S.chunks[S.units[u].chunk];
                const int64_t nb1 = ch.len / kCleTile;
                bu += 12.0 * (S.units[u].tile < nb1 ? kCleTile : ch.len - nb1 * kCleTile);
            }
            double br = 0;
            for (int64_t t = S.roffs[k]; t < S.roffs[k + 1]; ++t)
                br += 4.0 * (double)cle_range_elems(S.rt[t], R[S.rt[t].rel]);
            fprintf(stderr, "DFQ_CLE_PLACE offset %d: rescale %lld blocks %.2f MB, tiles %lld blocks %.2f MB, ranges %lld blocks %.2f MB\n",
                    k, (long long)na, ba / 1e6, (long long)(S.uoffs[k + 1] - S.uoffs[k]), bu / 1e6,
                    (long long)(S.roffs[k + 1] - S.roffs[k]), br / 1e6);
        }
    }
    if (info) {
        const int64_t v[8] = {steps, NL, S.lagged ? 1 : 0, S.stop_off, (int64_t)S.at.size(), (int64_t)S.rt.size(),
                              (int64_t)S.units.size(), (int64_t)S.chunks.size()};
        std::memcpy(info, v, sizeof(v));
    }
    // relations: range words and rollback saves inside their tables, links valid
    for (int32_t r = 0; r < n_rel; ++r) {
        const CleRel& c = R[r];
        if (c.moff < 0 || c.moff + 2 * c.c1 > S.M) return fail("rel %lld: range words [%lld, +2 c1) past M %lld", r, c.moff, S.M);
        if (2 * c.moff + 4 * c.c1 > 2 * S.M) return fail("rel %lld: rollback saves past 2 M (moff %lld, c1 %lld)", r, c.moff, c.c1);
        if (c.fuse_next >= n_rel || c.dw_prev >= n_rel || c.fuse_next < -1 || c.dw_prev < -1)
            return fail("rel %lld: link out of range (fuse_next %lld, dw_prev %lld)", r, c.fuse_next, c.dw_prev);
        if (c.fuse_next >= 0 && R[c.fuse_next].moff + R[c.fuse_next].c1 > S.M)
            return fail("rel %lld: fused W1 words of rel %lld past M %lld", r, c.fuse_next, S.M);
    }
    // rescale tasks per step
    if ((int32_t)S.astep.size() != steps + 1 || S.astep[0] != 0 || S.astep.back() != (int64_t)S.at.size())
        return fail("astep: %lld entries for %lld steps, last %lld", (long long)S.astep.size(), steps,
                    S.astep.empty() ? -1 : S.astep.back());
    std::vector<int32_t> rel_step(n_rel, -1);
    std::vector<std::pair<const float*, int32_t>> touch;   // (tensor, step) of every weight rescale
    // which step kernel a step launches (cle_loop_step_kernel<POS>): recomputed from its tasks
    if ((int32_t)S.step_pos.size() != std::max<int32_t>(steps, 1) || (steps == 0 && S.step_pos[0] != 0))
        return fail("step_pos: %lld entries for %lld steps (first %lld)", (long long)S.step_pos.size(), steps,
                    S.step_pos.empty() ? -1 : S.step_pos[0]);
    for (int32_t k = 0; k < steps; ++k) {
        if (S.astep[k + 1] < S.astep[k]) return fail("astep not monotone at step %lld: %lld > %lld", k, S.astep[k], S.astep[k + 1]);
        bool pos = false;   // a W2 row tile with KH*KW > 1 in this step
        for (int64_t t = S.astep[k]; t < S.astep[k + 1]; ++t) {
            const CleTask& tk = S.at[t];
            if (tk.rel < 0 || tk.rel >= n_rel) return fail("rescale task %lld: relation %lld of %lld", t, tk.rel, n_rel);
            const CleRel& c = R[tk.rel];
            if (tk.a < 0 || tk.a >= tk.b) return fail("rescale task %lld: empty or negative span [%lld, %lld)", t, tk.a, tk.b);
            switch (tk.kind) {
                case kApplyW1:
                    if (tk.b > c.c1) return fail("W1 task %lld: rows to %lld of %lld", t, tk.b, c.c1);
                    touch.push_back({c.w1, k});
                    break;
                case kApplyW2Contig:
                    if (tk.b > c.c1 || c.i2 != 1) return fail("W2 contig task %lld: channels to %lld of %lld", t, tk.b, c.c1);
                    touch.push_back({c.w2, k});
                    break;
                case kApplyDwBoth:
                    if (tk.b > c.c1 || tk.c0 < 0 || tk.c0 >= n_rel || R[tk.c0].w1 != c.w2 || R[tk.c0].dw_prev != tk.rel)
                        return fail("depthwise pair task %lld: partner %lld, channels to %lld", t, tk.c0, tk.b);
                    touch.push_back({c.w2, k});
                    break;
                case kApplyW2Tile:
                    if (tk.b > c.o2 || tk.c0 < 0 || tk.c0 >= tk.c1 || tk.c1 > c.i2)
                        return fail("W2 tile task %lld: rows to %lld, columns to %lld", t, tk.b, tk.c1);
                    touch.push_back({c.w2, k});
                    pos = pos || c.khw2 > 1;
                    break;
                case kApplyChannels:
                    if (tk.b > c.c1) return fail("channel task %lld: channels to %lld of %lld", t, tk.b, c.c1);
                    if (rel_step[tk.rel] >= 0 && rel_step[tk.rel] != k)
                        return fail("relation %lld: channel tasks in steps %lld and %lld", tk.rel, rel_step[tk.rel], k);
                    rel_step[tk.rel] = k;
                    break;
                default:
                    return fail("rescale task %lld: kind %lld", t, tk.kind, 0);
            }
        }
        if ((S.step_pos[k] != 0) != pos)
            return fail("step %lld: step_pos %lld, its tasks say %lld (the wrong step kernel)", k, S.step_pos[k], pos);
    }
    for (int32_t r = 0; r < n_rel; ++r)
        if (rel_step[r] < 0) return fail("relation %lld has no channel task", r, 0, 0);
    // range tasks
    const int64_t nrt = (int64_t)S.rt.size();
    if (S.ri0 < 0 || S.ri0 > S.ri1 || S.ri1 > nrt) return fail("range slice [%lld, %lld) of %lld tasks", S.ri0, S.ri1, nrt);
    for (int64_t t = 0; t < nrt; ++t) {
        const CleTask& tk = S.rt[t];
        if (tk.rel < 0 || tk.rel >= n_rel) return fail("range task %lld: relation %lld of %lld", t, tk.rel, n_rel);
        const CleRel& c = R[tk.rel];
        if (tk.a < 0 || tk.a >= tk.b) return fail("range task %lld: span [%lld, %lld)", t, tk.a, tk.b);
        const bool ok = tk.kind == kRangeW2Tile ? (tk.b <= c.o2 && tk.c0 >= 0 && tk.c0 < tk.c1 && tk.c1 <= c.i2)
                                                : (tk.kind >= kRangeW1 && tk.kind <= kRangeResetW1 && tk.b <= c.c1);
        if (!ok) return fail("range task %lld (kind %lld): span to %lld out of the relation's shape", t, tk.kind, tk.b);
    }
    // metric chunks and units
    int64_t nb1_seen = 0, nbig_seen = 0;   // level-1 slots; chunks with tiles (the stop rule's arrivals)
    for (size_t ci = 0; ci < S.chunks.size(); ++ci) {
        const CleChunk& ch = S.chunks[ci];
        if (ch.layer < 0 || ch.layer >= n_targets) return fail("chunk %lld: layer %lld of %lld", (long long)ci, ch.layer, n_targets);
        if (ch.c0 < 0 || ch.len <= 0 || ch.c0 + ch.len > target_n[ch.layer])
            return fail("chunk %lld: elements [%lld, +%lld) past its layer", (long long)ci, ch.c0, ch.len);
        const int64_t nb1 = ch.len / 32 / 256;
        if (S.b1off[ci] != 32 * nb1_seen) return fail("chunk %lld: level-1 offset %lld, expected %lld", (long long)ci, S.b1off[ci], 32 * nb1_seen);
        nb1_seen += nb1;
        nbig_seen += ch.len >= 8 ? 1 : 0;
    }
    if (nb1_seen != S.nb1_total) return fail("level-1 slots %lld, table %lld", nb1_seen, S.nb1_total, 0);
    if (nbig_seen != S.nbig) return fail("chunks with tiles %lld, nbig %lld", nbig_seen, S.nbig, 0);
    for (size_t u = 0; u < S.units.size(); ++u) {
        const CleUnit& un = S.units[u];
        if (un.chunk < 0 || un.chunk >= (int32_t)S.chunks.size()) return fail("unit %lld: chunk %lld", (long long)u, un.chunk, 0);
        const CleChunk& ch = S.chunks[un.chunk];
        if (ch.len < 8 || un.tile < 0 || un.tile > ch.len / 32 / 256)
            return fail("unit %lld: tile %lld of chunk %lld", (long long)u, un.tile, un.chunk);
        // cle_tiles_body's element ranges: a full tile is 8,192 elements inside the
        // chunk; a tail tile's [e0, len) (empty when 8,192 divides the chunk) fits the
        // LDS staging area below the b0 sums
        const int64_t nb1 = ch.len / 32 / 256, e0 = (int64_t)un.tile * kCleTile;
        if (un.tile < nb1 ? e0 + kCleTile > ch.len : (ch.len - e0 < 0 || ch.len - e0 > kCleTile + kCleTailWords))
            return fail("unit %lld: tile past chunk %lld (len %lld)", (long long)u, un.chunk, ch.len);
    }
    // placement tables
    if ((int32_t)S.uoffs.size() != 2 * NL + 1 || S.uoffs[0] != 0 || S.uoffs.back() != (int64_t)S.units.size())
        return fail("uoffs: %lld entries for %lld launches, last %lld", (long long)S.uoffs.size(), NL, S.uoffs.back());
    for (int32_t k = 0; k < 2 * NL; ++k)
        if (S.uoffs[k + 1] < S.uoffs[k]) return fail("uoffs not monotone at %lld", k, 0, 0);
    if (S.fused) {
        if ((int32_t)S.roffs.size() != 2 * NL + 1 || S.roffs[0] != S.ri0 || S.roffs.back() != S.ri1)
            return fail("roffs: %lld entries, [%lld, %lld)", (long long)S.roffs.size(), S.roffs.empty() ? -1 : S.roffs[0],
                        S.roffs.empty() ? -1 : S.roffs.back());
        for (int32_t k = 0; k < 2 * NL; ++k)
            if (S.roffs[k + 1] < S.roffs[k]) return fail("roffs not monotone at %lld", k, 0, 0);
    } else if ((int32_t)S.rstep.size() != steps + 1 || S.rstep.back() != nrt) {
        return fail("unfused rstep: %lld entries, last %lld of %lld", (long long)S.rstep.size(), S.rstep.back(), nrt);
    }
    if (NL != (S.lagged ? steps : steps + 1)) return fail("nlaunch %lld for %lld steps (lagged %lld)", NL, steps, S.lagged);
    // windows: a tensor's first / last rescale step
    auto span = [&](const float* w, int32_t& first, int32_t& last) {
        first = INT32_MAX;
        last = -1;
        for (const auto& x : touch)
            if (x.first == w) {
                first = std::min(first, x.second);
                last = std::max(last, x.second);
            }
        return last >= 0;
    };
    auto in_window = [&](const float* w, int32_t o) {
        int32_t f, l;
        if (!span(w, f, l)) return o >= 0 && o <= 2 * NL - 1;
        return o >= l + 1 && o <= std::min(2 * NL - 1, NL + f - 1);
    };
    int32_t umin = INT32_MAX, umax = -1;
    for (int32_t k = 0; k < 2 * NL; ++k)
        for (int64_t u = S.uoffs[k]; u < S.uoffs[k + 1]; ++u) {
            const int32_t l = S.chunks[S.units[u].chunk].layer;
            if (!S.lagged && k != steps) return fail("unit %lld of layer %lld at offset %lld outside the tiles-only launch", u, l, k);
            if (!in_window(targets[l], k)) return fail("unit %lld of layer %lld at offset %lld outside its tensor's window", u, l, k);
            umin = std::min(umin, k);
            umax = std::max(umax, k);
        }
    if (S.fused)
        for (int32_t k = 0; k < 2 * NL; ++k)
            for (int64_t t = S.roffs[k]; t < S.roffs[k + 1]; ++t) {
                const CleTask& tk = S.rt[t];
                const CleRel& c = R[tk.rel];
                bool ok = true;
                switch (tk.kind) {
                    case kRangeW1: ok = in_window(c.w1, k); break;
                    case kRangeW2Contig:
                    case kRangeW2Tile: ok = in_window(c.w2, k); break;
                    case kRangeReset: {
                        int32_t f, l;
                        span(c.w2, f, l);
                        ok = k >= rel_step[tk.rel] + 1 && k <= std::min(2 * NL - 1, NL + l);
                        break;
                    }
                    default: ok = k >= rel_step[tk.rel] + 1 && k <= 2 * NL - 1;   // kRangeResetW1
                }
                if (!S.lagged && k != steps) ok = false;
                if (!ok) return fail("range task %lld (kind %lld) at offset %lld outside its window", t, tk.kind, k);
            }
    if (S.lagged && S.stop_off >= 0) {
        if (S.stop_off < steps || S.stop_off > 2 * NL - 1) return fail("stop rule at offset %lld of [%lld, %lld]", S.stop_off, steps, 2 * NL - 1);
        if (umax >= 0 && S.stop_off <= umax) return fail("stop rule at offset %lld, not after the last tile offset %lld", S.stop_off, umax, 0);
        if (umax >= 0 && umin + NL <= S.stop_off)
            return fail("the next iteration's first tile (offset %lld + %lld) not after the stop rule at %lld", umin, NL, S.stop_off);
    } else if (!S.lagged && S.stop_off != -1) {
        return fail("unlagged plan with a stop-rule offset %lld", S.stop_off, 0, 0);
    }
    if (msg && msg_cap > 0) snprintf(msg, (size_t)msg_cap, "digest %016llx", (unsigned long long)cle_structure_digest(S));
    return DFQ_OK;
}
#endif
