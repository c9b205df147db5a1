// The graph transforms' planners (dfq_transform_plan.cpp): host-only code that
// turns the descriptor lists of dfq_bn_fold_batch, dfq_bias_absorb_batch and
// dfq_bc_chain into the tables and launch groups their kernels run from
// (dfq_transform.hip, dfq_bc.hip), and checks the bias-correction ops.  This header
// holds what the planners and the kernels share and includes no HIP header, so the
// planners build as plain C++ (and on their own, under a sanitizer:
// tests/native/transform_plan_check.cpp).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "dfq_cle_plan.h"   // DFQ_HOST_DEVICE, ceil_div, round256, kThreads
#include "dfq_hip.h"

namespace dfq {

// Blocks of kThreads for n elements, per_thread each, capped for grid-stride loops.
inline int blocks_for(int64_t n, int per_thread = 1) {
    const int64_t b = ceil_div(std::max<int64_t>(n, 1), (int64_t)kThreads * per_thread);
    return (int)std::min<int64_t>(b, 256 * 8);
}

// ---------------------------------------------------------------------------
// Batched BN fold: every (BN, producer layer) pair of a model in two launches.
// ---------------------------------------------------------------------------
struct BnFoldJob {
    float* w;
    float* bias;
    float* g;
    float* b;
    float* m;
    float* v;
    float* fake_w;
    float* fake_b;
    float eps;
    int32_t flags;    // DFQ_BN_FOLD_ZERO_BIAS
    int64_t rows, row_len;
    uint32_t* range_enc;
};
struct BnFoldChunk {
    int32_t job;
    int32_t pad;
    int64_t e0, e1;   // element range of the job's weight
};

constexpr int64_t kBnFoldMaxRowLen = int64_t(1) << 22;   // fold_row's fp32 row map
constexpr int64_t kBnFoldMaxSpan = int64_t(1) << 20;

// Row of element i of a chunk that starts in row r0 (base = r0 * row_len, inv =
// 1 / row_len in fp32): the chunk-local index times inv, exact after a +-1
// correction.  Holds for row_len <= kBnFoldMaxRowLen and chunk-local indices
// below kBnFoldMaxSpan + row_len (< 2^24: exact as floats); the host check walks
// every such index.  *rem_out = the element's offset in its row.
DFQ_HOST_DEVICE inline int64_t fold_row(int64_t row_len, int64_t r0, int64_t base, float inv, int64_t i,
                                        int* rem_out) {
    const int li = (int)(i - base);
    const int len = (int)row_len;
    int q = (int)((float)li * inv);
    int rem = li - q * len;
    if (rem < 0) {
        --q;
        rem += len;
    } else if (rem >= len) {
        ++q;
        rem -= len;
    }
    *rem_out = rem;
    return r0 + q;
}

// Elements per chunk (one block's work): 8192, or more for batches past 2^27
// elements so the chunk table stays small (<= ~16K chunks of 24 B).
int64_t bn_fold_span(const dfq_bn_fold_desc* d, int32_t n);

// Workspace of one call: [jobs | chunks], each part 256-B aligned.  Sizes only
// (rows, row_len >= 0): dfq_bn_fold_ws_bytes and dfq_bn_fold_batch both take it from here.
struct BnFoldLayout {
    int64_t span = 0, nchunks = 0;
    int64_t o_chunks = 0, total = 0;
};
BnFoldLayout bn_fold_layout(const dfq_bn_fold_desc* d, int32_t n);

// The jobs, and each weight cut into chunks of bn_fold_span elements, in list
// order.  Each weight at most once per list.
int bn_fold_tables(const dfq_bn_fold_desc* d, int32_t n, std::vector<BnFoldJob>& jobs,
                   std::vector<BnFoldChunk>& chunks);

// ---------------------------------------------------------------------------
// Batched absorption
// ---------------------------------------------------------------------------
struct AbsRel {
    const float* w2;
    const float* bn_w;
    float* bn_b;
    int64_t o2, i2, khw2, o2g;
    int64_t wc;    // float offset of this relation's W2sum @ c in the scratch
};
struct AbsRows {   // GEMV task: rows [o0, o1) of relation r, one wave per row
    int32_t r;
    int32_t pad;
    int64_t o0, o1;
};
struct AbsVec {    // a bias vector and its update list
    float* b;
    int64_t n;
    int32_t op0, nops;
};
struct AbsOp {     // kind 0: b += wc[r]; kind 1: b -= c[r] and beta[r] -= c[r]
    int32_t kind;
    int32_t r;
};
struct AbsElems {  // bias walk task: elements [e0, e1) of vector v
    int32_t v;
    int32_t pad;
    int64_t e0, e1;
};
struct AbsTables {
    std::vector<AbsRel> rels;
    std::vector<AbsRows> rows;
    std::vector<AbsVec> vecs;
    std::vector<AbsOp> ops;
    std::vector<AbsElems> elems;
    int64_t wc_floats = 0;
};
// *failed (may be null) = the relation a non-OK code is about, -1 otherwise.
int absorb_tables(const dfq_absorb_desc* d, int32_t n, AbsTables& T, int32_t* failed);

// Workspace: [rels | rows | vecs | ops | elems | wc], each part 256-B aligned; the
// first `host` bytes are uploaded, wc is device scratch.
struct AbsLayout {
    int64_t o_rels, o_rows, o_vecs, o_ops, o_elems, host, o_wc, total;
};
AbsLayout absorb_layout(const AbsTables& T);

// ---------------------------------------------------------------------------
// Bias correction
// ---------------------------------------------------------------------------
constexpr int64_t kBcScratch = 1024;     // floats of a wave's cascade scratch (and wave_full_sum's slots)
constexpr int kBcMaxTerms = 8;
constexpr int64_t kBcMaxExpect = 4096;
// Rows / columns of at most kBcStage values are staged in LDS by bc_layer_kernel;
// longer ones take the per-op kernels.
constexpr int64_t kBcStage = 2048;

// One target layer of the walk for bc_layer_kernel: EXPECT+ -> APPLY (-> PROPAGATE).
struct BcLayerJob {
    const float* ew[kBcMaxTerms];
    const float* eb[kBcMaxTerms];
    int32_t relu[kBcMaxTerms];
    int32_t nterms;
    int32_t threads;            // PROPAGATE: the reference run's intra-op threads
    float* expect_out;          // the EXPECT ops' slot (written by block 0, as they would)
    int64_t f;                  // expect numel
    const float* E;
    int64_t o, i2, bcols;
    float* bias;
    float* vec;                 // APPLY's bias_vec (may be null)
    float* fake_b;              // PROPAGATE target (null: no PROPAGATE in the group)
    int64_t F, nrows;
    int64_t apply_blocks;
};

// Columns of torch's broadcast of [o, i2] + [f]; 0: not broadcastable.
DFQ_HOST_DEVICE inline int64_t bc_bcols(int64_t i2, int64_t f) {
    if (i2 == f || f == 1) return i2;
    return i2 == 1 ? f : 0;
}

// One op's arguments as dfq_bc_expect / dfq_bc_apply / dfq_bc_propagate and
// dfq_bc_chain check them (a COPY: as the chain does).  An EXPECT or COPY of
// n == 0 is valid (and launches nothing).
int bc_check_op(const dfq_bc_op& op);

// ops[k..] as one layer group for bc_layer_kernel: EXPECT (plain) [+ EXPECT
// (accumulate) ...] into one slot, the APPLY reading that slot, and optionally
// the PROPAGATE of that APPLY's bias_vec right after it.  Returns the ops used,
// or 0 (the ops then run one launch each).  Fused only when no op of the group
// writes what another one reads (the launch has no order inside it).
int32_t bc_layer_group(const dfq_bc_op* ops, int32_t n_ops, int32_t k, BcLayerJob& J);

// Up to kCopyBatch consecutive DFQ_BC_OP_COPY ops of a chain in one launch: the
// batch rides in the kernel arguments, blockIdx.y picks the copy.
constexpr int kCopyBatch = 64;   // 1.5 KB of kernel arguments
struct CopyBatch {
    const float* src[kCopyBatch];
    float*       dst[kCopyBatch];
    int64_t      n[kCopyBatch];
};
// The run of COPY ops at ops[k] into b: cnt copies (empty ones left out), the
// longest of `most` floats.  Returns the ops consumed (>= 1; cnt may be 0).
int32_t bc_copy_run(const dfq_bc_op* ops, int32_t n_ops, int32_t k, CopyBatch& b, int& cnt, int64_t& most);

}  // namespace dfq
