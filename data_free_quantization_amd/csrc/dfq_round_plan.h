// The sum-rounding planner (dfq_round_plan.cpp): host-only code that checks the
// descriptors of dfq_sum_round_batch (dfq_round.hip), sizes a workgroup's LDS for a
// (row_len, khw) pair and picks the grid.  This header holds what the planner and
// the kernel share and includes no HIP header, so the planner builds as plain C++
// (and on its own, under a sanitizer: tests/native/round_plan_check.cpp).
//
// One workgroup rounds one row.  Its LDS, in order:
//   S  int32 [G][pitch]   the perturbations P, kernel g's taps at S[g * pitch + k].
//                         pitch = khw | 1 is odd, so the 64 lanes of a wave -- each
//                         walking the taps of its own kernel -- start on 64 different
//                         banks whatever khw is (stride 9 is odd as it is; 4 and 16
//                         take one word of padding).  khw == 1: pitch 1.
//   E  int32 [G]          the kernels' error sums e' (khw == 1: e' = P, E is S)
//   Q  uint8 [row_len]    the nearest codes
// A flip is kept in S itself: a flipped-down element holds P - 2^25 and a flipped-up
// one P + 2^25 (its perturbation after the flip is P -+ 2^24), so flipped elements
// are apart from every unflipped one (|P| <= 2^23) even at an exact tie, and no
// mask is stored.
#pragma once
#include <math.h>
#include <stdint.h>

#include "dfq_cle_plan.h"   // DFQ_HOST_DEVICE, kThreads, round256
#include "dfq_hip.h"

namespace dfq {

constexpr int32_t kSrHalf = 1 << 23;   // half a step in P's fixed point
constexpr int32_t kSrStep = 1 << 24;   // one step
constexpr int32_t kSrMark = 1 << 25;   // what a flip moves the stored word by
constexpr int kSrGridCap = 256;        // workgroups of one call: one per CU
constexpr int kSrRangeBlocks = 64;     // workgroups per TENSOR-mode weight in the range launch
constexpr int64_t kSrLdsLimit = 160 * 1024;

// Step 3: the rounding error of q against t in units of 2^-24 step.
DFQ_HOST_DEVICE inline int32_t sr_perturb(float q, float t) { return (int32_t)rintf(ldexpf(q - t, 24)); }
// Steps 4 and 5: |e| / 2^24 rounded half down (|e| < 2^62).
DFQ_HOST_DEVICE inline int64_t sr_flip_count(int64_t e) { return ((e < 0 ? -e : e) + kSrHalf - 1) >> 24; }
// Step 5's order-preserving key of a kernel's e' (|e'| < 2^31): candidates -- e' on the
// row's side of zero -- order as their unsigned keys, everything else is key 0, below
// every candidate.
DFQ_HOST_DEVICE inline uint32_t sr_key(int32_t e, bool down) {
    const int32_t v = down ? e : -e;
    return v > 0 ? (uint32_t)v : 0u;
}
// The stored word of an element: its code's offset from nearest, and its perturbation.
DFQ_HOST_DEVICE inline int sr_code_offset(int32_t s) { return s > kSrStep ? 1 : (s < -kSrStep ? -1 : 0); }
DFQ_HOST_DEVICE inline int32_t sr_value(int32_t s) { return s - sr_code_offset(s) * kSrStep; }

DFQ_HOST_DEVICE inline int sr_pitch(int khw) { return khw == 1 ? 1 : (khw | 1); }

struct SrLds {
    int32_t o_s, o_e, o_q, total;   // byte offsets into the dynamic LDS, and its size
};
DFQ_HOST_DEVICE inline SrLds sr_lds_layout(int64_t row_len, int khw) {
    const int64_t G = row_len / khw, s_bytes = 4 * G * sr_pitch(khw);
    SrLds L;
    L.o_s = 0;
    L.o_e = khw == 1 ? 0 : (int32_t)s_bytes;
    L.o_q = (int32_t)(khw == 1 ? s_bytes : s_bytes + 4 * G);
    L.total = (int32_t)(L.o_q + (row_len + 15) / 16 * 16);
    return L;
}

// A weight as the kernels see it.
struct SrJob {
    const float* src;
    float* dst;
    void* codes;
    float* scale;
    float* zero;
    int32_t* flips;
    uint32_t* range;   // TENSOR modes: {~enc(min), enc(max)} in the workspace; else NULL
    int64_t rows;
    int64_t row0;      // the weight's first row among the call's rows
    int32_t row_len;
    int32_t khw;
    int32_t bits;
    int32_t sym;
};

// Workspace of one call: [jobs | TENSOR-mode range words, two per weight], each part
// 256-B aligned and both uploaded in one copy (the range words as zeros).
struct SrLayout {
    int64_t total_rows = 0;
    int32_t n_tensor = 0;     // weights in a TENSOR mode (0: no range launch)
    int32_t grid = 0;         // workgroups of the rounding launch
    int32_t lds_bytes = 0;    // its dynamic LDS: the largest row's layout
    int64_t o_jobs = 0, o_range = 0, total = 0;
};

// DFQ_OK or the error the batch call returns for the descriptor.
int sum_round_check(const dfq_sum_round_desc& d);
// The checks of the whole list and the layout.
int sum_round_layout(const dfq_sum_round_desc* d, int32_t n, SrLayout& L);
// jobs[n] as uploaded: `range_base` is the device address of the range words.
void sum_round_jobs(const dfq_sum_round_desc* d, int32_t n, uint32_t* range_base, SrJob* jobs);

}  // namespace dfq
