// The CLE loop's planner (dfq_cle_plan.cpp): host-only code that turns the
// relations' and targets' shapes and tensor identities into the tables the
// device-resident loop runs from (its host runtime: dfq_cle.hip; its kernels:
// dfq_cle_kernels.h).  This header holds what the planner, the runtime and the
// kernels share -- records, constants, index helpers, the structure a plan keeps --
// and includes no HIP header, so the planner builds as plain C++ (and on its own,
// under a sanitizer: tests/native/cle_plan_check.cpp).
#pragma once
#include <stdint.h>
#include <stdlib.h>

#include <chrono>
#include <memory>
#include <vector>

#include "dfq_hip.h"

#ifdef __HIPCC__
#define DFQ_HOST_DEVICE __host__ __device__
#else
#define DFQ_HOST_DEVICE
#endif

namespace dfq {

// Environment switches for A/B runs and diagnostics: read only by the diagnostics
// library (libdfq_diag.so, built with -DDFQ_DIAGNOSTICS); the product library
// runs its measured defaults whatever the environment says.
inline const char* ab_env(const char* name) {
#ifdef DFQ_DIAGNOSTICS
    return getenv(name);
#else
    (void)name;
    return nullptr;
#endif
}
inline double now_us() {
    return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

DFQ_HOST_DEVICE inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
// bytes up to the next multiple of 256: the alignment of every workspace part
DFQ_HOST_DEVICE inline int64_t round256(int64_t b) { return ceil_div(b, (int64_t)256) * 256; }
// at::native's CeilLog2 (the cascade's level step, dfq_common.h)
DFQ_HOST_DEVICE inline int aten_ceil_log2(int64_t x) {
    if (x <= 2) return 1;
    int r = 0;
    for (uint64_t v = (uint64_t)(x - 1); v; v >>= 1) ++r;
    return r;
}

constexpr int kWave = 64;   // gfx950 wave size: the kernels' and every planner's
constexpr int kThreads = 256;
constexpr int kColTileRows = 16;   // W2 rows per column tile (range and rescale tiles)

struct CleRel {
    float* w1;
    float* w2;
    float* b1;
    float* bnw;
    float* bnb;
    float* sacc;
    int64_t c1, len1, o2, i2, khw2, o2g;
    int64_t moff;       // this relation's [W1 | W2] range words inside one parity's mins (and maxs)
    int32_t sacc_init;
    int32_t vec1;       // W1 rows 16-B aligned (float4 path)
    int32_t vec2;       // W2 contiguous channel segments 16-B aligned (i2 == 1)
    int32_t fuse_next;  // >= 0: this relation's W2 is that relation's W1 -- the rescale
                        // of W2 also produces its row ranges (fused schedule)
    int32_t dw_prev;    // >= 0: this relation's W1 is that relation's depthwise W2: its W1 row
                        // ranges are derived (cle_rel_scale) and both run in one launch
    int32_t w1_self;    // 1: its W1 rescale also writes the next iteration's W1 row ranges
    int32_t w2_self;    // 1: its depthwise W2 rescale (kApplyDwBoth) writes the next W2 ranges
};

// Range-launch kinds: W1 rows, W2 contiguous channels (i2 == 1), W2 row tiles
// (i2 > 1, ordered-uint atomics), reset of the OTHER parity's W2 words.
// Rescale-launch kinds: W1 elements, W2 elements, per-channel vectors.
enum : int32_t { kRangeW1 = 0, kRangeW2Contig = 1, kRangeW2Tile = 2, kRangeReset = 3, kRangeResetW1 = 4 };
enum : int32_t { kApplyW1 = 0, kApplyW2Contig = 1, kApplyW2Tile = 2, kApplyChannels = 3, kApplyDwBoth = 4 };

struct CleTask {
    int32_t rel;
    int32_t kind;
    int64_t a, b;     // rows / channels / elements [a, b)
    int64_t c0, c1;   // W2 tiles: columns [c0, c1) (one thread each)
};

struct CleLayer {
    float* w;
    float* snap;
    int64_t n;
    int64_t nt;   // torch.mean's chunks (1: serial sum)
};

// One fp32 torch.mean chunk (a thread's share of at::parallel_for in
// two_pass_reduction): elements [c0, c0 + len) of layer `layer`, slot t.
struct CleChunk {
    int32_t layer;
    int32_t t;
    int64_t c0;
    int64_t len;
};

// One metric tile (dfq_cle_kernels.h, cle_tiles_body): kCleTile contiguous elements of a chunk
struct CleUnit {
    int32_t chunk;
    int32_t tile;     // < nb1: full level-1 tile; == nb1: the chunk's tail tile
};
constexpr int kCleTile = 8192;            // 32 streams x 16 x 16
constexpr int kCleTailWords = 64;         // per chunk: 32 stream partials, 24 row-tail, 8 scalar-tail values

// Short rows (< 64 elements: depthwise filters, the first layers' rows) take a
// group of G lanes each (G = the next power of two >= the length), 64 / G rows
// per wave, instead of a whole wave per row -- 4-7x fewer tasks for MobileNetV2's
// depthwise filters and narrow rows, whose cost is the dependent round trips.
DFQ_HOST_DEVICE inline int row_group_lanes(int64_t len) {
    if (len >= 64) return 64;
    int g = 1;
    while (g < len) g <<= 1;
    return g;
}
// rows (or channel segments) per task: 4 waves x the rows a wave holds
DFQ_HOST_DEVICE inline int64_t rows_per_task(int64_t len) { return 4 * (64 / row_group_lanes(len)); }

constexpr int64_t kCleChansPerTask = 1024;
// Rescale tasks hold rows_per_task rows (one per wave).  W1 tasks of short rows
// (under kCleW1SmallElems elements per task: MobileNetV2's expand convs) take twice
// that: step 0 of MobileNetV2 had 1,648 W1 tasks of ~2 us in 2,433 blocks, more than
// are resident, so its last blocks started 8.7 us into the launch
// (profiles/r06/cle_tl_r06h.log); A/B profiles/r06/cle_ab_rows_r06i.jsonl.
// Diagnostics switches: DFQ_CLE_W1_ROWS (a fixed factor) / DFQ_CLE_DW_ROWS.
constexpr int64_t kCleW1SmallElems = 2048, kCleDwRowsMult = 1;

// W2 row tiles with KH*KW = khw in (1, kTileMaxKhw] and one group are rescaled
// position-parallel (dfq_cle_kernels.h, tile_by_position)
constexpr int kTileMaxKhw = 9;   // 3x3 (and 2x2); larger kernels keep the per-column walk
// Rows per position-parallel rescale tile (<= kColTileRows): their loads are in
// flight together (16-row tiles took ~70 us a task on ResNet-50's 3x3 layers,
// 4-row tiles ~11 us: profiles/r03/cle_tl_*.log)
#ifndef DFQ_CLE_POS_ROWS   // compile-time A/B (scripts/cle_lib_ab.py builds side by side)
#define DFQ_CLE_POS_ROWS 4
#endif
constexpr int kPosTileMaxRows = DFQ_CLE_POS_ROWS;

// The diagnostics library's schedule switches, parsed once per structure build
// (the product library: always the defaults).
struct CleSwitches {
    bool fused = true;                 // DFQ_CLE_FUSED=0: per-step range launches
    int64_t w1_mult = 0;               // DFQ_CLE_W1_ROWS: rows_per_task times this (0: the default rule)
    int64_t dw_mult = kCleDwRowsMult;  // DFQ_CLE_DW_ROWS: likewise for depthwise pairs
    bool lag = true;                   // DFQ_CLE_LAG=0: the round-4 schedule
    bool stop_arrival = false;         // DFQ_CLE_STOP=arrival: the stop rule at the last tile arrival
    int32_t band = -1;                 // DFQ_CLE_BAND: the tiles' band start (< 0: searched)
    static CleSwitches from_env();
    void append_to(std::vector<int64_t>& key) const;
};

// Everything dfq_cle_plan_create derives from the relations' and targets' shapes
// and tensor identities -- chains, steps, tasks, metric chunks and units, the
// placement -- but no address: a plan of the same structure keeps a reference to
// it, reads it at every launch and binds its own tensors (cle_structure_cached).
struct CleStructure {
    std::vector<CleRel> R;   // fused / depthwise / self-range flags set (addresses: the first plan's)
    int64_t M = 0;
    int32_t chains = 0, steps = 0;
    bool fused = false;
    std::vector<CleTask> rt, at;
    std::vector<int64_t> rstep, astep;   // task offsets per step (size steps + 1)
    // per step (size max(steps, 1)): it has W2 row tiles with KH*KW > 1, so its launch is
    // cle_loop_step_kernel<true>, the instantiation with the position-parallel rescale
    // (a wrong value launches the wrong kernel: the structure checker recomputes it)
    std::vector<char> step_pos;
    int64_t ri0 = 0, ri1 = 0;            // fused: each iteration's range tasks (the rest come from the rescales)
    std::vector<CleLayer> layers;   // n, nt (w / snap bound per plan)
    std::vector<CleChunk> chunks;
    int64_t nbig = 0;               // chunks with tiles (len >= 8): the members of the stop rule's last arrival
    std::vector<CleUnit> units;
    std::vector<int64_t> b1off;
    int64_t nb1_total = 0;
    std::vector<int64_t> uoffs, roffs;
    int32_t nlaunch = 0, stop_off = -1;
    bool lagged = false;
    double t_chains = 0, t_tasks = 0, t_chunks = 0, t_place = 0;
    // algorithmic HBM bytes of one iteration (dfq_cle_plan_stats): the rescales
    // (8 B per weight element and per channel of each per-channel vector: read +
    // write; a depthwise pair's filter once), the metric tiles (12 B per target
    // element: W and the snapshot read, the snapshot written) and the range tasks
    // that read weights (4 B per element; self ranges are free)
    int64_t bytes_rescale = 0, bytes_metric = 0, bytes_range = 0;
    uint64_t id = 0;   // unique per built structure: the device pool remembers whose tables it holds
};

// The relations' descriptors as the device's records: shapes checked as
// dfq_cle_relation; each relation's [W1 | W2] range words at moff (M in all).
int cle_rels_from_desc(const dfq_cle_rel* rels, int32_t n_rel, std::vector<CleRel>& R, int64_t& M);
// The structure for these relations and targets, built afresh.
int cle_build_structure(std::vector<CleRel> R, int64_t M, float* const* targets, const int64_t* target_n,
                        int32_t n_targets, int32_t ref_threads, const CleSwitches& sw, CleStructure& S);
// The same through a small cache keyed on shapes, flags, the tensors' sharing
// pattern, the metric's thread count and the switches (null: rc says why).
std::shared_ptr<const CleStructure> cle_structure_cached(const std::vector<CleRel>& R, int64_t M,
                                                         float* const* targets, const int64_t* target_n,
                                                         int32_t n_targets, int32_t ref_threads, int& rc, bool& cached);

}  // namespace dfq
