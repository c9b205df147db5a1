// The sweep planner (dfq_sweep_plan.cpp): host-only code that checks a list of
// tensor descriptors, cuts it into the wave tasks of sweep_main_kernel and
// sweep_reduce_kernel (dfq_sweep.hip) and lays out the two workspaces.  This header
// holds what the planner and the kernels share and includes no HIP header, so the
// planner builds as plain C++ (and on its own, under a sanitizer:
// tests/native/sweep_plan_check.cpp, which checks every invariant the kernels take
// on trust: DESIGN.md 1).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "dfq_cle_plan.h"   // DFQ_HOST_DEVICE, ceil_div, ab_env, kWave
#include "dfq_hip.h"

namespace dfq {

constexpr int kWavesPerBlock = 4;

// Kernel variants: each row is the whole truth about its variant.  The planner reads
// the first three fields (the task table is built for the plan's variant); the rest
// are sweep_main_kernel's template arguments, instantiated from the row.
struct Variant {
    int chunk;       // elements per wave task
    int max_rows;    // rows of one whole-row task; the host caps rows per task at max(64 (one short row
                     // per lane), chunk / 32) (build()): 3 * max_rows floats of row parameters per wave
    bool prefetch;   // LDS-DMA of the wave's next task in flight during compute (two chunk buffers)
    bool nt;         // non-temporal loads and stores
    int espec;       // KH*KW sums with a compile-time length: 2 3x3 / 7x7 / 5x5 / 2x2, 1 3x3, 0 none
    bool timeline;   // per-task timestamps and the ablation word (diagnostics: dfq_debug_timeline / _ablate)
    bool screen;     // the screened reciprocal quantize; false: the IEEE divide on every element
    bool fast;       // the fixed-form quantize loop; false: the generic one (flags tested per float4)
    bool split;      // whole-row tasks in two row batches (compute_task_split)
};
constexpr Variant kVariants[] = {
    //                   nt     E  tl     screen fast  split
    {2048, 64, false,  false, 2, false, true, true, false},   // 0: 8.5 KB LDS / wave, 16 waves / CU
    {1024, 64, true,   false, 2, false, true, true, false},   // 1: 2 x 4 KB, next task's DMA in flight
    {2048, 64, true,   false, 2, false, true, true, false},   // 2: 2 x 8 KB
    {1024, 64, false,  false, 2, false, true, true, false},   // 3: 4.5 KB / wave
    {4096, 128, false, false, 2, false, true, true, false},   // 4: 17 KB / wave, 8 waves / CU
    {2048, 64, false,  true, 2, false, true, true, false},    // 5: variant 0, non-temporal
    {2048, 64, false,  true, 1, false, true, true, false},    // 6: variant 5, 3x3 sums only (fewer VGPRs)
    {2048, 64, false,  true, 0, false, true, true, false},    // 7: variant 5, generic sums only
    {2560, 80, false,  true, 1, false, true, true, false},    // 8: variant 6, 2560-element tasks (12 waves / CU)
    {1024, 64, false,  true, 1, false, true, true, false},    // 9: variant 6, 1024-element tasks
    {1536, 64, false,  true, 1, false, true, true, false},    // 10: variant 6, 1536-element tasks
    {1024, 64, true,   true, 1, false, true, true, false},    // 11: variant 9 with the prefetch
    {1024, 64, false,  true, 0, false, true, true, false},    // 12: variant 9, generic sums (fewer VGPRs)
    {2048, 64, false,  true, 1, true, true, true, false},     // 13: variant 6 + timeline and ablations
    {2048, 64, false,  true, 1, false, false, true, false},   // 14: variant 6, IEEE divide everywhere (round 2)
    {2048, 64, false,  true, 1, false, true, false, false},   // 15: variant 6, generic quantize loop (round 3)
    {2048, 64, false,  true, 1, false, true, true, true},     // 16: variant 6 in two row batches
};
constexpr int kNumVariants = (int)(sizeof(kVariants) / sizeof(kVariants[0]));
// DevTask .nrows <= kGroupTag: a row-group piece of R = kGroupTag - nrows + 1 rows
constexpr int kGroupTag = -64;
constexpr int kGroupMaxRows = 16;
#ifndef DFQ_DEFAULT_VARIANT   // compile-time override for side-by-side A/B builds (scripts/ab_variant_libs.py)
#define DFQ_DEFAULT_VARIANT 6
#endif
constexpr int kDefaultVariant = DFQ_DEFAULT_VARIANT;   // 6 = 5 with 87 instead of 105 VGPRs (profiles/r01/ab_*_v568.json)
static_assert(kDefaultVariant >= 0 && kDefaultVariant < kNumVariants, "DFQ_DEFAULT_VARIANT names no variant");
// Small lists (sweep_plan_tables) run variant 10's 1,536-element tasks; one round
// of resident sweep blocks on the 256-CU part is 4 per CU.
constexpr int kSmallVariant = 10;
constexpr int64_t kResidentBlocks = 4 * 256;

struct alignas(16) DevTensor {
    const float* src;
    float* dst;
    void* codes;
    float* scale;
    float* zero;
    float* esum;
    int64_t rows;
    int64_t row_len;
    int32_t khw;
    int32_t bits;
    int32_t mode;
    int32_t flags;
    float clip_lo;
    float clip_hi;
    double given_min;
    double given_max;
    float inv_len;     // 1/row_len, for the element -> row map inside a task
    int32_t vec4;      // 16-B loads / stores legal
    int32_t code_bytes;
    uint32_t len_magic;  // ceil(2^32 / row_len): element -> row as one v_mul_hi_u32 (row_len >= 2)
    const uint32_t* range_enc;   // DFQ_DEVICE_RANGE
};

// A wave task as the kernels read it: the record carries the address of its first
// element and the tensor's 16-B-vector flag, so a wave issues the task's LDS-DMA as
// soon as the record has landed, while the tensor's 128-B descriptor is still on
// its way (one dependent scalar round trip off every task's critical path).
struct alignas(16) DevTask {
    const float* src;    // T.src + the task's first element (tensor-relative)
    int32_t tensor;
    int32_t n;           // elements in the task
    int32_t row0;        // first row of a whole-row task / the row of a long-row piece
    int32_t nrows;       // > 0: whole rows; 0: slot piece; -2/-4: block-row piece; <= kGroupTag: row group
    int32_t slot;        // workspace (min,max) slot for pieces, -1 = given range
    int32_t flags;       // bit 0: this piece writes scale/zero for its range; bit 1: T.vec4
};
static_assert(sizeof(DevTask) == 32, "one 32-B scalar load per task record");

// Device layout of a plan's tables: [tensors | reduce tasks | main tasks | slots],
// each 256-B aligned (one allocation or one caller workspace).
struct PlanLayout {
    int64_t o_tensors = 0, o_reduce = 0, o_main = 0, o_slots = 0, total = 0;
};
// The single-tensor workspace: [slots | tensor | reduce tasks | main tasks], each
// 64-B aligned; the slots start it.
struct SingleLayout {
    size_t o_tensor = 0, o_reduce = 0, o_main = 0, total = 0;
};

// The finished tables of one list: `slots` mins then `slots` maxs are armed per
// run; the main list holds block-row (and row-group) quads, then the tasks that
// need no reduce, then the slot pieces.
struct SweepTables {
    int variant = kDefaultVariant;
    std::vector<DevTensor> tensors;
    std::vector<DevTask> reduce, main;
    int64_t slots = 0;
    int64_t elems = 0;
    int64_t algo_bytes = 0;   // read x, write dq / codes / E / per-row params once
};

// The plan's variant (the small-list rule, or a diagnostics DFQ_SWEEP_VARIANT), its
// tables and their layout.  descs may be NULL only for n == 0.
int sweep_plan_tables(const dfq_tensor_desc* descs, int32_t n, SweepTables& T, PlanLayout& L);
// The same for dfq_quantize_tensor: one tensor, always the default variant.
int sweep_single_tables(const dfq_tensor_desc& d, SweepTables& T, SingleLayout& L);

}  // namespace dfq
