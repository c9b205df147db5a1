// The index arithmetic of dfq_int_gemm and dfq_int_linear (dfq_int_gemm.hip): which K
// elements of which operand row a lane holds, where their bytes lie, how packed nibbles
// become bytes, how a fragment reaches the instruction's signed domain, and how the exact
// integers of the contract come back out of the accumulators.  The kernel and the host
// check (tests/native/int_gemm_plan_check.cpp, which walks every block, wave, lane and K
// step of a shape on the CPU) use these helpers and nothing else for an address or a bit
// operation on a fragment, so what the check proves -- every read inside its array, every
// output element stored once, the gathered operands multiply to the contract's P, Sa and
// Sb -- holds for the kernel, up to the instruction's own lane map.  No HIP header: the
// planner (dfq_int_gemm_plan.cpp) builds as plain C++.
//
// The instruction is v_mfma_i32_16x16x64_i8: D[16 x 16] += A[16 x 64] * B[64 x 16], signed
// bytes, every lane holding 16 K elements (four registers) of one row of A and of one
// column of B:
//   A and B operand: row / column  lane & 15,  K elements of lane group  lane >> 4
//   C / D:           column        lane & 15,  row  4 * (lane >> 4) + reg, reg 0..3
// Both operands give lane group g the step's elements [16 g, 16 g + 16) in byte order.  The
// product only needs A and B to agree on which k a (lane group, byte slot) holds -- any
// other assignment the hardware makes is one permutation of k inside a step, applied to
// both, and a sum over k does not see it -- and which operand supplies C's rows is pinned
// by the tests' asymmetric data.
// The tiling is dfq_mx_gemm's (dfq_mx_gemm_plan.h: mxg_wave_m0 / mxg_wave_n0, mxg_lane_row,
// mxg_out_row / mxg_out_col, mxg_stores, mxg_out_offset): a wave owns 32 x 32 outputs as
// 2 x 2 instruction tiles, a block of four waves 64 x 64.
#pragma once
#include <stdint.h>

#include "dfq_mx_gemm_plan.h"

namespace dfq {

constexpr int kIgStepK = 64;      // K elements per instruction
constexpr int kIgLaneK = 16;      // of which a lane holds these, as four 32-bit words
constexpr int64_t kIgMaxK = DFQ_INT_MAX_K;   // 255 * 255 * 32768 < 2^31: P, Sa and Sb fit int32

DFQ_HOST_DEVICE inline int64_t ig_steps(int64_t K) { return ceil_div(K, (int64_t)kIgStepK); }
// First K element of a lane in K step `step`.
DFQ_HOST_DEVICE inline int64_t ig_lane_k0(int64_t step, int lane) { return kIgStepK * step + kIgLaneK * (lane >> 4); }
// How many of the lane's 16 elements exist (0: the lane reads nothing): the first nv.
DFQ_HOST_DEVICE inline int ig_lane_valid(int64_t row, int64_t rows, int64_t k0, int64_t K) {
    if (row >= rows || k0 >= K) return 0;
    return K - k0 >= kIgLaneK ? kIgLaneK : (int)(K - k0);
}
// The wide path: every lane holds all 16 of its elements or none, and its bytes start
// 16-B (packed: 8-B) aligned -- the code bases are 16-B aligned.
DFQ_HOST_DEVICE inline bool ig_wide(int64_t K) { return K % kIgLaneK == 0; }
// Byte offset of element k of `row` in codes[rows][K], and of the byte that holds elements
// k and k + 1 (k even) in packed codes[rows][K / 2] (K even).
DFQ_HOST_DEVICE inline int64_t ig_byte_offset(int64_t row, int64_t k, int64_t K) { return row * K + k; }
DFQ_HOST_DEVICE inline int64_t ig_packed_offset(int64_t row, int64_t k, int64_t K) { return (row * K + k) >> 1; }
// Bytes a lane with nv elements reads of a packed row (K even and k0 even, so nv is even).
DFQ_HOST_DEVICE inline int ig_packed_bytes(int nv) { return nv >> 1; }
DFQ_HOST_DEVICE inline int64_t ig_x_offset(int64_t row, int64_t k, int64_t ldx) { return row * ldx + k; }
// x on the 16-B path: whole aligned groups of four.
DFQ_HOST_DEVICE inline bool ig_x_vec(uintptr_t x, int64_t ldx, int64_t K) { return x % 16 == 0 && ldx % 4 == 0 && K % 4 == 0; }

// Word j (0..3: elements 4 j .. 4 j + 3, one per byte) of the 16 elements that the packed
// words w[0], w[1] (element e in bits [4 e, 4 e + 4) of the pair) hold: every nibble widened
// to a byte, sign-extended when `sign`.
DFQ_HOST_DEVICE inline uint32_t ig_unpack4(const uint32_t (&w)[2], int j, bool sign) {
    const uint32_t h = (w[j >> 1] >> (16 * (j & 1))) & 0xFFFFu;
    uint32_t v = (h & 0xFu) | ((h & 0xF0u) << 4) | ((h & 0xF00u) << 8) | ((h & 0xF000u) << 12);
    if (sign) v |= (v & 0x08080808u) * 0x1Eu;   // 0xF0 into every byte whose bit 3 is set; no carry crosses a byte
    return v;
}
// What moves a fragment's bytes to the instruction's signed domain: unsigned q -> q - 128.
DFQ_HOST_DEVICE inline uint32_t ig_xor_mask(bool is_signed) { return is_signed ? 0u : 0x80808080u; }
DFQ_HOST_DEVICE inline int ig_offset(bool is_signed) { return is_signed ? 0 : 128; }
// Word j of a fragment as the instruction takes it: in the signed domain, the elements past
// nv zero there (so they add nothing to a product or a row sum).
DFQ_HOST_DEVICE inline uint32_t ig_operand_word(uint32_t raw, uint32_t xor_mask, int nv, int j) {
    const int vb = nv - 4 * j;
    const uint32_t keep = vb >= 4 ? 0xFFFFFFFFu : vb <= 0 ? 0u : (1u << (8 * vb)) - 1u;
    return (raw ^ xor_mask) & keep;
}
// The contract's integers from the signed-domain accumulators p = sum a' b', ra = sum a',
// rb = sum b' (a' = qa - oa, b' = qb - ob over the K real elements).
DFQ_HOST_DEVICE inline int64_t ig_fold_p(int64_t p, int64_t ra, int64_t rb, int oa, int ob, int64_t K) {
    return p + ob * ra + oa * rb + K * oa * ob;
}
DFQ_HOST_DEVICE inline int64_t ig_fold_s(int64_t r, int o, int64_t K) { return r + K * o; }

// The argument checks both entry points share (no device call): DFQ_OK and the grid, or the
// error.  a_ok: A's own pointers are there, aligned, and its fields in range; lda: x's row
// stride (K for stored codes, so that its check passes whenever K's do).
template <class Desc>
inline int ig_check_common(const Desc& d, bool a_ok, int64_t lda, int32_t known_flags, int64_t& grid) {
    const auto addr = [](const void* p) { return reinterpret_cast<uintptr_t>(p); };
    if (!a_ok || !d.b_codes || !d.b_scale || !d.out) return DFQ_ERR_INVALID;
    if ((d.flags & ~known_flags) != 0 || d.reserved != 0) return DFQ_ERR_INVALID;
    if (d.b_signed != 0 && d.b_signed != 1) return DFQ_ERR_INVALID;
    if (d.M < 1 || d.N < 1 || d.K < 1) return DFQ_ERR_INVALID;
    if (d.M > (int64_t(1) << 40) || d.N > (int64_t(1) << 40) || d.ldo > (int64_t(1) << 40) || lda > (int64_t(1) << 40))
        return DFQ_ERR_INVALID;
    if (addr(d.b_codes) % 16) return DFQ_ERR_INVALID;
    if (addr(d.out) % 4 || addr(d.bias) % 4 || addr(d.b_scale) % 4 || addr(d.b_zero) % 4) return DFQ_ERR_INVALID;
    if (lda < d.K || d.ldo < d.N) return DFQ_ERR_SHAPE;
    if (d.M > (int64_t(1) << 50) / lda || d.M > (int64_t(1) << 50) / d.ldo) return DFQ_ERR_INVALID;   // row * ld + col
    if (d.K > kIgMaxK) return DFQ_ERR_UNSUPPORTED;
    if ((d.flags & DFQ_INT_B_PACK4) && d.K % 2) return DFQ_ERR_UNSUPPORTED;
    const int64_t g = mxg_grid(d.M, d.N);
    if (g > 0x7fffffff) return DFQ_ERR_UNSUPPORTED;
    grid = g;
    return DFQ_OK;
}

int ig_check(const dfq_int_gemm_desc* d, int64_t& grid);
int igl_check(const dfq_int_linear_desc* d, int64_t& grid);

}  // namespace dfq
