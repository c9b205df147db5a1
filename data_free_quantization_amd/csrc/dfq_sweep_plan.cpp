// Host-only planner of the sweep (dfq_sweep_plan.h): descriptor checks, the task
// tables of the reduce and main launches, the plan's variant and the two workspace
// layouts.  Plain C++: no HIP header, no device code.
#include "dfq_sweep_plan.h"

#include <algorithm>
#include <numeric>

namespace dfq {

static bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }

static int validate(const dfq_tensor_desc& d) {
    if (d.rows < 0 || d.row_len < 0) return DFQ_ERR_INVALID;
    if (!d.src && d.rows * d.row_len > 0) return DFQ_ERR_INVALID;
    if (d.bits < 2 || d.bits > 16) return DFQ_ERR_INVALID;
    if (d.mode < DFQ_TENSOR_ASYM || d.mode > DFQ_CHANNEL_SYM) return DFQ_ERR_INVALID;
    if (d.khw < 1) return DFQ_ERR_INVALID;
    if (d.esum && (d.row_len % d.khw) != 0) return DFQ_ERR_SHAPE;
    if (d.rows > INT32_MAX) return DFQ_ERR_UNSUPPORTED;
    const bool channel = d.mode >= DFQ_CHANNEL_ASYM;
    if (channel && (d.flags & DFQ_GIVEN_RANGE)) return DFQ_ERR_INVALID;
    if (d.flags & DFQ_DEVICE_RANGE) {
        if (channel || (d.flags & DFQ_GIVEN_RANGE) || !d.range_enc) return DFQ_ERR_INVALID;
    }
    return DFQ_OK;
}

static DevTensor to_dev(const dfq_tensor_desc& d) {
    DevTensor t{};
    t.src = d.src; t.dst = d.dst; t.codes = d.codes; t.scale = d.scale; t.zero = d.zero; t.esum = d.esum;
    t.rows = d.rows; t.row_len = d.row_len; t.khw = d.khw; t.bits = d.bits; t.mode = d.mode;
    t.flags = d.flags; t.clip_lo = d.clip_lo; t.clip_hi = d.clip_hi;
    t.given_min = d.given_min; t.given_max = d.given_max;
    t.range_enc = (d.flags & DFQ_DEVICE_RANGE) ? d.range_enc : nullptr;
    t.inv_len = d.row_len > 0 ? 1.0f / (float)d.row_len : 0.f;
    t.len_magic = (d.row_len >= 2 && d.row_len < (int64_t(1) << 31))
                      ? (uint32_t)(((uint64_t(1) << 32) + (uint64_t)d.row_len - 1) / (uint64_t)d.row_len)
                      : 0u;
    t.code_bytes = (d.flags & DFQ_PACK_INT4) ? 0 : (d.bits <= 8 ? 1 : 2);   // 0: packed nibbles
    const int64_t n = d.rows * d.row_len;
    const bool channel = d.mode >= DFQ_CHANNEL_ASYM;
    bool v = (n % 4 == 0) && aligned(d.src, 16) && (!d.dst || aligned(d.dst, 16)) &&
             (!d.codes || aligned(d.codes, t.code_bytes ? 4 * t.code_bytes : 2)) &&
             (!d.esum || d.khw > 1 || aligned(d.esum, 16));
    if (channel) v = v && (d.row_len % 4 == 0);
    t.vec4 = v ? 1 : 0;
    return t;
}

// What every piece of a tensor is a multiple of: khw (E sums never straddle a
// piece), 4 (vec4) and 2 (packed nibbles: a byte never straddles two tasks).
static int64_t piece_unit(const DevTensor& T) {
    const bool packed = (T.flags & DFQ_PACK_INT4) != 0;
    return T.vec4 ? std::lcm<int64_t>(4, T.khw) : (packed ? std::lcm<int64_t>(2, T.khw) : T.khw);
}
// `blen` elements in `parts` balanced pieces of whole units
static int64_t balanced_piece(int64_t blen, int64_t unit, int64_t parts) {
    return ceil_div(ceil_div(blen, unit), parts) * unit;
}

static DevTask task(const DevTensor& T, int32_t ti, int64_t elem_start, int64_t n, int64_t row0, int32_t nrows,
                    int64_t slot, bool first) {
    return DevTask{T.src + elem_start, ti, (int32_t)n, (int32_t)row0, nrows, (int32_t)slot,
                   (first ? 1 : 0) | (T.vec4 ? 2 : 0)};
}

// A/B and diagnostics switches (DFQ_SWEEP_VARIANT / _REDUCE_SPAN /
// _SHUFFLE / _BLOCKS_PER_CU) are read only by the diagnostics library
// (libdfq_diag.so, -DDFQ_DIAGNOSTICS); the product library runs the measured
// defaults whatever the environment says.

// DFQ_SWEEP_GROUP_ROWS=1 (diagnostics): per-channel rows of kChunk/2 .. 4 kChunk
// elements as row groups instead of whole-row tasks / block-row pieces.  Bit-exact
// and neutral (-1.4 .. +1.4 % on the five replicated configs interleaved on one box,
// profiles/r02/ab_group_rows.json: task fill is not what limits the 3x3 families),
// so the product keeps the simpler tasks.
static bool group_rows_enabled() {
    const char* e = ab_env("DFQ_SWEEP_GROUP_ROWS");
    return e && e[0] == '1';
}

// DFQ_SWEEP_BLOCKROW=0 (diagnostics library): long rows through the reduce launch
// instead (an alternative schedule, parity-tested against the default).
static bool blockrow_enabled() {
    const char* e = ab_env("DFQ_SWEEP_BLOCKROW");
    return !(e && e[0] == '0');
}

// Two-pass ranges pipelined in slabs (the quantize pass of slab k re-reading its
// inputs while they are still in the 256 MB Infinity Cache, on two streams) were
// measured slower at every slab size (profiles/r02/ab_slab.json: 16-256 MB slabs
// 1.34-3.9 ms per step against 1.11 for the two passes back to back) and deleted
// in round 4.

// Reduce-launch tasks: consecutive pieces of one range merged up to `span`
// elements per wave task (fewer same-address atomics, longer read streams).
// DFQ_SWEEP_REDUCE_SPAN overrides (A/B).
static int64_t reduce_span() {
    const char* e = ab_env("DFQ_SWEEP_REDUCE_SPAN");
    return (e && *e) ? std::max<int64_t>(1, atoll(e)) : 16384;
}
static void push_reduce(std::vector<DevTask>& R, const DevTask& k, int64_t span) {
    if (!R.empty()) {
        DevTask& p = R.back();
        if (p.slot == k.slot && p.tensor == k.tensor && p.src + p.n == k.src && (int64_t)p.n + k.n <= span) {
            p.n += k.n;
            return;
        }
    }
    R.push_back(k);
}

// DFQ_SWEEP_SHUFFLE=<seed> (A/B): visit the main list's 4-task units (one
// workgroup's grid-stride step; block-row groups stay whole) in a seeded random
// order instead of list order.
static void shuffle_quads(std::vector<DevTask>& main) {
    const char* e = ab_env("DFQ_SWEEP_SHUFFLE");
    if (!e || !*e) return;
    const int64_t units = (int64_t)main.size() / kWavesPerBlock;
    if (units < 2) return;
    uint64_t x = (uint64_t)atoll(e) * 0x9E3779B97F4A7C15ull + 1;
    auto next = [&x]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    for (int64_t u = units - 1; u > 0; --u) {
        const int64_t v = (int64_t)(next() % (uint64_t)(u + 1));
        if (v != u)
            std::swap_ranges(main.begin() + u * kWavesPerBlock, main.begin() + (u + 1) * kWavesPerBlock,
                             main.begin() + v * kWavesPerBlock);
    }
}

// The tables of a list at variant V.  B.main: block-row (and row-group) quads, then
// the tasks needing no reduce, then the slot pieces in reduce order.
static int build(const dfq_tensor_desc* descs, int32_t n, SweepTables& B, const Variant& V) {
    const int64_t rspan = reduce_span();
    const bool use_blockrow = blockrow_enabled();
    const int kChunk = V.chunk, kMaxRows = V.max_rows;
    std::vector<DevTask> blockrow, slotted;   // groups of kWavesPerBlock; slot pieces
    for (int32_t ti = 0; ti < n; ++ti) {
        const dfq_tensor_desc& d = descs[ti];
        int rc = validate(d);
        if (rc) return rc;
        const DevTensor T = to_dev(d);
        const bool packed = (d.flags & DFQ_PACK_INT4) != 0;
        if (packed && d.bits > 4) return DFQ_ERR_INVALID;
        // packed codes need every task to start at an even element: per channel,
        // odd rows must come in pairs within one whole-row task (row_len <= chunk/2)
        if (packed && d.mode >= DFQ_CHANNEL_ASYM && (d.row_len & 1) && 2 * d.row_len > kChunk && d.rows > 1)
            return DFQ_ERR_UNSUPPORTED;
        const int64_t total = d.rows * d.row_len;
        B.elems += total;
        // algorithmic bytes: read x, write dq / codes / E / per-row params once
        int64_t bytes = 4 * total;
        if (d.dst) bytes += 4 * total;
        if (d.codes) bytes += T.code_bytes ? (int64_t)T.code_bytes * total : total / 2;
        if (d.esum) bytes += 4 * (total / d.khw);
        const bool channel = d.mode >= DFQ_CHANNEL_ASYM;
        const int64_t nparams = channel ? d.rows : 1;
        if (d.scale) bytes += 4 * nparams;
        if (d.zero) bytes += 4 * nparams;
        B.algo_bytes += bytes;
        B.tensors.push_back(T);
        if (total == 0) continue;
        const int64_t unit = piece_unit(T);
        const int64_t plen = (kChunk / unit) * unit;   // the longest piece
        if (plen <= 0) return DFQ_ERR_UNSUPPORTED;     // khw > kChunk
        // a given or device-resident range: single-pass tasks, no slot
        const bool given = (d.flags & (DFQ_GIVEN_RANGE | DFQ_DEVICE_RANGE)) != 0;
        const int64_t blen = channel ? d.row_len : total;   // the range's extent
        // Row groups (per-channel rows of kChunk/2 .. 4 kChunk elements): R whole rows
        // split into 4 balanced pieces, one per wave of a block, the rows' ranges
        // combined through LDS -- tasks hold ~R len / 4 elements instead of one row
        // (1,152-element 3x3 rows: 56 % of a task) or half a row.
        int64_t grp_rows = 0;
        if (channel && use_blockrow && !V.prefetch && !given && d.row_len > kChunk / 2 &&
            d.row_len <= (int64_t)kWavesPerBlock * kChunk && group_rows_enabled()) {
            for (int64_t R = std::min<int64_t>(kGroupMaxRows, (int64_t)kWavesPerBlock * kChunk / d.row_len); R >= 1;
                 --R) {
                if (balanced_piece(R * d.row_len, unit, kWavesPerBlock) <= kChunk) {
                    grp_rows = R;
                    break;
                }
            }
            // whole-row tasks already fill >= 85 % of a task: keep them
            if (grp_rows > 0 && d.row_len <= kChunk && (kChunk / d.row_len) * d.row_len * 100 >= 85 * kChunk)
                grp_rows = 0;
        }
        if (grp_rows > 0) {
            for (int64_t r0 = 0; r0 < d.rows; r0 += grp_rows) {
                const int64_t R = std::min<int64_t>(grp_rows, d.rows - r0);
                const int64_t tot = R * d.row_len;
                const int64_t piece = balanced_piece(tot, unit, kWavesPerBlock);
                for (int i = 0; i < kWavesPerBlock; ++i) {
                    const int64_t off = std::min<int64_t>((int64_t)i * piece, tot);
                    blockrow.push_back(task(T, ti, r0 * d.row_len + off, std::min<int64_t>(piece, tot - off), r0,
                                            kGroupTag - (int32_t)(R - 1), -1, false));
                }
            }
            continue;
        }
        const bool block_row = use_blockrow && !V.prefetch && !given && blen <= (int64_t)kWavesPerBlock * plen &&
                               (!channel || d.row_len > kChunk);
        if (block_row) {
            // A group of 4 list entries = 4 waves of one block: one row in 4 pieces,
            // or (rows <= 2 pieces) two rows in 2 pieces each.  Balanced pieces:
            // the group waits for its slowest wave.
            const int64_t nr = channel ? d.rows : 1;
            const int gs = blen <= 2 * plen ? 2 : kWavesPerBlock;
            const int64_t bpl = balanced_piece(blen, unit, gs);
            const int64_t rows_per_group = kWavesPerBlock / gs;
            for (int64_t r0 = 0; r0 < nr; r0 += rows_per_group) {
                for (int i = 0; i < kWavesPerBlock; ++i) {
                    const int64_t r = r0 + i / gs;
                    const int64_t off = (int64_t)(i % gs) * bpl;
                    if (r < nr) {
                        blockrow.push_back(task(T, ti, r * blen + std::min<int64_t>(off, blen),
                                                std::max<int64_t>(0, std::min<int64_t>(bpl, blen - off)), r, -gs, -1,
                                                i % gs == 0));
                    } else {   // padding half-group: no data, writes nothing
                        blockrow.push_back(task(T, ti, r0 * blen, 0, r0, -gs, -1, false));
                    }
                }
            }
        } else if (channel && d.row_len <= kChunk) {
            // short rows (depthwise 3x3: 9 elements) are reduced one lane per row and run
            // the scalar path: at most one row per lane keeps such a task's latency
            // near a vector task's (single-model sweeps are latency-bound)
            const int64_t row_cap = d.row_len < 32 ? kWave : kMaxRows;
            int64_t rpt = std::max<int64_t>(1, std::min<int64_t>(row_cap, kChunk / d.row_len));
            if (packed && (d.row_len & 1) && rpt > 1) rpt &= ~int64_t(1);   // even task starts
            for (int64_t r = 0; r < d.rows; r += rpt) {
                const int64_t nr = std::min<int64_t>(rpt, d.rows - r);
                B.main.push_back(task(T, ti, r * d.row_len, nr * d.row_len, r, (int32_t)nr, -1, false));
            }
        } else if (channel) {   // long rows: one slot per row
            for (int64_t r = 0; r < d.rows; ++r) {
                const int64_t slot = B.slots++;
                for (int64_t off = 0; off < d.row_len; off += plen) {
                    const DevTask k = task(T, ti, r * d.row_len + off, std::min<int64_t>(plen, d.row_len - off), r, 0,
                                           slot, off == 0);
                    push_reduce(B.reduce, k, rspan);
                    slotted.push_back(k);
                }
            }
        } else {                // tensor modes: one slot per tensor (none for a given range)
            const int64_t slot = given ? -1 : B.slots++;
            for (int64_t off = 0; off < total; off += plen) {
                const DevTask k = task(T, ti, off, std::min<int64_t>(plen, total - off), 0, 0, slot, off == 0);
                if (!given) {
                    push_reduce(B.reduce, k, rspan);
                    slotted.push_back(k);
                } else {
                    B.main.push_back(k);
                }
            }
        }
    }
    B.main.insert(B.main.begin(), blockrow.begin(), blockrow.end());
    B.main.insert(B.main.end(), slotted.begin(), slotted.end());   // slot pieces after the single-pass tasks
    shuffle_quads(B.main);
    return DFQ_OK;
}

static PlanLayout plan_layout(const SweepTables& B) {
    PlanLayout L;
    L.o_reduce = L.o_tensors + round256((int64_t)sizeof(DevTensor) * (int64_t)B.tensors.size());
    L.o_main = L.o_reduce + round256((int64_t)sizeof(DevTask) * (int64_t)B.reduce.size());
    L.o_slots = L.o_main + round256((int64_t)sizeof(DevTask) * (int64_t)B.main.size());
    L.total = L.o_slots + round256((int64_t)sizeof(uint32_t) * 2 * B.slots);
    return L;
}

static SingleLayout single_ws_layout(const SweepTables& B) {
    SingleLayout L;
    auto align64 = [](size_t o) { return (o + 63) & ~size_t(63); };
    L.o_tensor = align64(sizeof(uint32_t) * 2 * (size_t)B.slots);
    L.o_reduce = align64(L.o_tensor + sizeof(DevTensor) * B.tensors.size());
    L.o_main = align64(L.o_reduce + sizeof(DevTask) * B.reduce.size());
    L.total = L.o_main + sizeof(DevTask) * B.main.size();
    return L;
}

// The plan's kernel variant and task table.  A diagnostics DFQ_SWEEP_VARIANT wins.
// Otherwise the default variant's 2,048-element tasks, unless the list is small
// enough that 1,536-element tasks (variant 10) still fit in ONE round of resident
// blocks (4 per CU at 97 VGPRs): a one-round grid of range-dependent tasks is
// latency-bound, and 4/3 as many waves hide more of it (MobileNetV2 single model:
// 560 -> 747 blocks).  Lists past one round keep 2,048 (DeepLab's single model at
// 1,536 needs 1,123 blocks and measured 12.0 against 9.2 us; profiles/r06/chunk_rule_ab_r06o.jsonl).
// The rule was measured for variant 6 and holds only while that is the default.
int sweep_plan_tables(const dfq_tensor_desc* descs, int32_t n, SweepTables& T, PlanLayout& L) {
    const char* e = ab_env("DFQ_SWEEP_VARIANT");
    const bool forced = e && *e;
    T = SweepTables{};
    const int v = forced ? atoi(e) : kDefaultVariant;
    if (v >= 0 && v < kNumVariants) T.variant = v;
    if (int rc = build(descs, n, T, kVariants[T.variant])) return rc;
    const int64_t blocks = ceil_div((int64_t)T.main.size(), (int64_t)kWavesPerBlock);
    // 4/3 the tasks would not fit one round: no second table
    if (!forced && kDefaultVariant == 6 && !T.main.empty() && 4 * blocks <= 3 * kResidentBlocks) {
        SweepTables S;
        S.variant = kSmallVariant;
        if (build(descs, n, S, kVariants[kSmallVariant]) == DFQ_OK &&
            ceil_div((int64_t)S.main.size(), (int64_t)kWavesPerBlock) <= kResidentBlocks)
            T = std::move(S);
    }
    L = plan_layout(T);
    return DFQ_OK;
}

int sweep_single_tables(const dfq_tensor_desc& d, SweepTables& T, SingleLayout& L) {
    T = SweepTables{};
    if (int rc = build(&d, 1, T, kVariants[kDefaultVariant])) return rc;
    L = single_ws_layout(T);
    return DFQ_OK;
}

}  // namespace dfq

extern "C" int64_t dfq_sweep_plan_ws_bytes(const dfq_tensor_desc* descs, int32_t n) {
    if ((n > 0 && !descs) || n < 0) return -1;
    dfq::SweepTables T;
    dfq::PlanLayout L;
    if (dfq::sweep_plan_tables(descs, n, T, L)) return -1;
    return L.total;
}

extern "C" int dfq_quantize_ws_bytes(const dfq_tensor_desc* d, size_t* bytes) {
    if (!d || !bytes) return DFQ_ERR_INVALID;
    dfq::SweepTables T;
    dfq::SingleLayout L;
    if (int rc = dfq::sweep_single_tables(*d, T, L)) return rc;
    *bytes = L.total;
    return DFQ_OK;
}
