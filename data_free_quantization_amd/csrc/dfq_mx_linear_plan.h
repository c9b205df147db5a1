// The index arithmetic and the per-lane quantizer of dfq_mx_linear (dfq_mx_gemm.hip's fp32 A):
// dfq_mx_gemm with the A operand built in the kernel from an fp32 activation.  Tiling, the B
// operand, the accumulators and the stores are dfq_mx_gemm_plan.h's, unchanged; this header
// adds which fp32 elements of x a lane reads, how it turns them into the operand registers and
// the scale byte the instruction expects, and -- for FP8 -- which lanes exchange what.  The
// kernel and the host check (tests/native/mx_linear_plan_check.cpp) use these helpers and
// nothing else for it, so what the check proves on the CPU -- every fp32 read inside its row,
// registers and scale byte equal, byte for byte, to what dfq_mx_gemm's helpers gather from
// the stored codes of the same x -- holds for the kernel, up to the cross-lane instruction
// itself.  No HIP header: the checks (dfq_mx_linear_plan.cpp) build as plain C++.
//
// FP4 / FP6: a lane's operand is one MX block of its row (32 consecutive K elements) and that
// block's scale byte, so the lane reads its 32 floats, takes their amax, derives the floor
// rule's exponent, encodes and packs: no other lane is involved.
// FP8 ("split", dfq_mx_gemm_plan.h): lane group g = lane >> 4 holds the 16-element half
// g & 1 of MX block g >> 1 (registers 0..3) and of MX block 2 + (g >> 1) (registers 4..7) of
// the K step, and its scale register block g's byte.  So
//   - the other half of both of its blocks is held by lane ^ 16 (same row, group g ^ 1): the
//     two lanes exchange their halves' amax bits, after which both know both blocks' exponents;
//   - block g's exponent is known to lane group 2 * (g & 1) (and its neighbour): as the
//     exponent of its first block if g < 2, of its second if g >= 2.  Every lane offers both
//     of its exponents' bytes packed in one word, reads the word of lane
//     (lane & 15) + 32 * (g & 1) and keeps byte g >> 1.
// Both exchanges are one ds_bpermute each (no LDS memory, no barrier); every lane of the wave
// takes part, which the kernel's only early return (wave-uniform, before the loop) allows.
#pragma once
#include "dfq_mx_encode.h"
#include "dfq_mx_gemm_plan.h"

namespace dfq {

// The DFQ_MX_* format of the instruction's format field.
DFQ_HOST_DEVICE constexpr int mxl_format_of_hw(int hw) {
    return hw == 4 ? (int)DFQ_MX_FP4_E2M1 : hw == 2 ? (int)DFQ_MX_FP6_E2M3 : hw == 3 ? (int)DFQ_MX_FP6_E3M2 : (int)DFQ_MX_FP8_E4M3;
}
DFQ_HOST_DEVICE constexpr int mxl_elem_bits(int hw) { return hw == 4 ? 4 : mxg_hw_split(hw) ? 8 : 6; }

// A lane's 32 elements of one K step come in `parts` runs of consecutive K elements: one MX
// block, or (FP8) two 16-element halves of two blocks.  Slot 32 / parts * part + j of the
// operand (mxg_hw_slot's numbering) is element j of run `part`.
DFQ_HOST_DEVICE constexpr int mxl_parts(int hw) { return mxg_hw_split(hw) ? 2 : 1; }
DFQ_HOST_DEVICE constexpr int mxl_part_len(int hw) { return DFQ_MX_BLOCK / mxl_parts(hw); }
// The MX block of run `part` and the run's first K element.
DFQ_HOST_DEVICE inline int64_t mxl_part_kblock(int hw, int64_t step, int lane, int part) {
    return mxg_hw_split(hw) ? mxg_split_kblock(step, lane, part) : mxg_lane_kblock(step, lane);
}
DFQ_HOST_DEVICE inline int64_t mxl_part_k(int hw, int64_t step, int lane, int part) {
    return DFQ_MX_BLOCK * mxl_part_kblock(hw, step, lane, part) + (mxg_hw_split(hw) ? mxl_part_len(hw) * mxg_split_chunk(lane) : 0);
}
// Element (row, k) of x is read iff it exists; everything else is +0.
DFQ_HOST_DEVICE inline bool mxl_reads(int64_t row, int64_t M, int64_t k, int64_t K) { return row < M && k < K; }
DFQ_HOST_DEVICE inline int64_t mxl_x_offset(int64_t row, int64_t k, int64_t ldx) { return row * ldx + k; }
// The 16-B path: every row of x starts 16-B aligned and K is a multiple of 4, so four elements at
// k % 4 == 0 exist together or not at all and are one 16-B load.  Every other case reads
// element by element.
DFQ_HOST_DEVICE inline bool mxl_vec(uintptr_t x, int64_t ldx, int64_t K) { return x % 16 == 0 && ldx % 4 == 0 && K % 4 == 0; }

// FP8: the lane that holds the other half of both of this lane's blocks.
DFQ_HOST_DEVICE inline int mxl_split_partner(int lane) { return lane ^ 16; }
// FP8: the lane whose packed exponent bytes hold this lane group's block's, and which byte.
DFQ_HOST_DEVICE inline int mxl_split_scale_lane(int lane) { return (lane & 15) + 32 * ((lane >> 4) & 1); }
DFQ_HOST_DEVICE inline int mxl_split_scale_byte(int lane) { return lane >> 5; }

// The largest magnitude's bits of one run (integer compares on the bit patterns, as the
// quantizer's: no NaN rule, no canonicalisation).
template <int HW>
DFQ_MX_INLINE uint32_t mxl_part_amax(const float (&v)[DFQ_MX_BLOCK], int part) {
    constexpr int n = mxl_part_len(HW);
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < n; ++j) {
        const uint32_t b = mx_bits(v[n * part + j]) & 0x7fffffffu;
        m = b > m ? b : m;
    }
    return m;
}
// The scale byte of a block with those amax bits (0 for an all-zero block).
template <int HW>
DFQ_MX_INLINE int mxl_scale_byte(uint32_t amax_bits) { return mx_exponent<mxl_format_of_hw(HW)>(amax_bits) + 127; }

// Slot `slot` (0..31) of the operand registers takes `code`: bits [w slot, w slot + w), w the
// element width -- the stored block's bit order for FP4 / FP6, a byte per slot for FP8.
template <int HW>
DFQ_MX_INLINE void mxl_put(uint32_t (&regs)[8], int slot, uint32_t code) {
    constexpr int w = mxl_elem_bits(HW);
    const int bit = w * slot, r = bit >> 5, sh = bit & 31;
    regs[r] |= code << sh;
    if (sh + w > 32) regs[r + 1] |= code >> (32 - sh);
}
// Run `part` of the lane's elements under the scale byte `byte` of its block, into its slots.
template <int HW>
DFQ_MX_INLINE void mxl_encode_part(uint32_t (&regs)[8], const float (&v)[DFQ_MX_BLOCK], int part, int byte) {
    constexpr int n = mxl_part_len(HW);
    const float inv = pow2f(127 - byte), up = pow2f(byte - 127);
#pragma unroll
    for (int j = 0; j < n; ++j) {
        float y;
        mxl_put<HW>(regs, n * part + j, mx_encode<mxl_format_of_hw(HW)>(v[n * part + j], inv, up, y));
    }
}

// dfq_mx_linear's argument checks (no device call); DFQ_OK and the grid, or the error.
int mxl_check(const dfq_mx_linear_desc* d, int64_t& grid);

}  // namespace dfq
