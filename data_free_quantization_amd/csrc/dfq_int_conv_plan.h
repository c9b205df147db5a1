// The index arithmetic dfq_int_conv2d adds (dfq_int_gemm.hip's conv A and NCHW store):
// dfq_int_linear on the im2col rows of an NCHW activation, gathered in the kernel, with a
// padding tap absent from every sum instead of standing for the code of 0.0.  The tiling and
// the B operand are dfq_int_gemm_plan.h's, which element of x stands at (m, k) and where output
// (m, n) lies in NCHW is dfq_mx_conv_plan.h's (MxcGeom, mxc_row, mxc_tap, mxc_next, mxc_reads,
// mxc_x_offset, mxc_out_offset, mxc_out_quad), both unchanged.  This header adds
//   - which k a lane's run of 16 starts at (ig_lane_k0's) and the 16-bit mask of the run: bit e
//     set iff element k0 + e is read (row < M, k < K, tap inside the image) -- the contract's v,
//   - the mask as the instruction takes it: byte 0x01 where v = 1 (the operand whose product
//     with B's fragment is sum_k v b'), and the fragment's word with every absent element 0
//     in the signed domain (not 0 ^ 0x80),
//   - T[m] = sum_k v, a closed form: C times the kernel rows times the kernel columns that
//     fall inside the image from the row's (ih0, iw0),
//   - the folds, dfq_int_gemm's with T where they had K:
//       P = p + ob ra + oa rbm + T oa ob,   Sa = ra + T oa,   Sb = rbm + T ob
//     from p = sum v a' b', ra = sum v a', rbm = sum v b' (a' = qa - oa, b' = qb - ob).
// The kernel and the host check (tests/native/int_conv_plan_check.cpp) use these helpers and
// nothing else for an address, a mask bit or a fold.  No HIP header: the checks
// (dfq_int_conv_plan.cpp) build as plain C++.
#pragma once
#include "dfq_int_gemm_plan.h"
#include "dfq_mx_conv_plan.h"

namespace dfq {

// Some tap of the geometry can fall in padding: the row sums of B need the mask operand.
DFQ_HOST_DEVICE inline bool igc_masked(const MxcGeom& g) { return (g.ph | g.pw) != 0; }

// A lane's run in K step `step`: its first k and, walked from there, the mask bit of element e.
template <bool PW>
DFQ_HOST_DEVICE inline uint32_t igc_mask_bit(const MxcGeom& g, const MxcRow& r, const MxcTap& t, int64_t k, int64_t K, int e) {
    return mxc_reads<PW>(g, r, t, k, K) ? 1u << e : 0u;
}
// Word j (elements 4 j .. 4 j + 3, one per byte) of the mask operand: 0x01 where the bit is set.
DFQ_HOST_DEVICE inline uint32_t igc_ones_word(uint32_t mask, int j) {
    const uint32_t m = (mask >> (4 * j)) & 0xFu;
    return (m & 1u) | ((m & 2u) << 7) | ((m & 4u) << 14) | ((m & 8u) << 21);
}
// Word j of the A fragment as the instruction takes it: in the signed domain, 0 there wherever
// the mask bit is clear (a padding tap, k >= K, a row >= M).
DFQ_HOST_DEVICE inline uint32_t igc_operand_word(uint32_t raw, uint32_t xor_mask, uint32_t mask, int j) {
    return (raw ^ xor_mask) & (igc_ones_word(mask, j) * 0xFFu);
}

// How many i of 0 .. k - 1 have 0 <= x0 + i * d < n (x0 may be negative: inside the padding).
DFQ_HOST_DEVICE inline int32_t igc_axis_taps(int32_t x0, int32_t n, int32_t k, int32_t d) {
    if (n - 1 - x0 < 0) return 0;
    const int32_t lo = x0 >= 0 ? 0 : (-x0 + d - 1) / d;
    int32_t hi = (n - 1 - x0) / d;
    if (hi > k - 1) hi = k - 1;
    return hi >= lo ? hi - lo + 1 : 0;
}
// T[m]: the taps of row r that lie inside the image.
DFQ_HOST_DEVICE inline int64_t igc_taps(const MxcGeom& g, const MxcRow& r) {
    return (int64_t)g.C * igc_axis_taps(r.ih0, g.H, g.KH, g.dh) * igc_axis_taps(r.iw0, g.W, g.KW, g.dw);
}

// The contract's integers from the signed-domain accumulators.
DFQ_HOST_DEVICE inline int64_t igc_fold_p(int64_t p, int64_t ra, int64_t rbm, int oa, int ob, int64_t T) {
    return ig_fold_p(p, ra, rbm, oa, ob, T);
}
DFQ_HOST_DEVICE inline int64_t igc_fold_s(int64_t r, int o, int64_t T) { return ig_fold_s(r, o, T); }

// dfq_int_conv2d's argument checks (no device call): DFQ_OK with the geometry, M, K and the
// grid, or the error.
int igc_check(const dfq_int_conv2d_desc* d, MxcGeom& g, int64_t& M, int64_t& K, int64_t& grid);

}  // namespace dfq
