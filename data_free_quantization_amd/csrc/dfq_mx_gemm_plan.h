// The index arithmetic of dfq_mx_gemm (dfq_mx_gemm.hip): which output tile a block and
// a wave own, which row and MX block of an operand a lane holds, where the lane's code
// bytes and scale byte lie, and which output elements it stores.  The kernel and the
// host check (tests/native/mx_gemm_plan_check.cpp, which walks every block, wave, lane
// and K step of a shape on the CPU) use these helpers and nothing else for an address,
// so what the check proves -- every read inside its array, every output element
// stored once, the gathered operands multiply to the product -- holds for the kernel,
// up to the instruction's own lane map and bit order.  No HIP header: the planner
// (dfq_mx_gemm_plan.cpp) builds as plain C++.
//
// The instruction is v_mfma_scale_f32_16x16x128_f8f6f4: D[16 x 16] += A[16 x 128] *
// B[128 x 16], every lane holding 32 consecutive K elements (one MX block) of one row
// of A and of one column of B with one E8M0 scale byte each:
//   A and B operand: row / column  lane & 15,  MX block  lane >> 4  of the K step's four
//                    (FP8 elements: two 16-element halves of two blocks, see "split" below)
//   C / D:           column        lane & 15,  row       4 * (lane >> 4) + reg, reg 0..3
// A wave owns a 32 x 32 output tile (2 x 2 instruction tiles: each loaded fragment feeds
// two instructions), a block of four waves 64 x 64; blocks number the output's 64 x 64
// tiles row by row.
#pragma once
#include <stdint.h>

#include "dfq_cle_plan.h"   // DFQ_HOST_DEVICE, ceil_div
#include "dfq_hip.h"

namespace dfq {

constexpr int kMxgMfma = 16;         // the instruction's M and N
constexpr int kMxgSub = 2;           // instruction tiles per wave tile, each way
constexpr int kMxgWaveTile = kMxgMfma * kMxgSub;
constexpr int kMxgWavesM = 2, kMxgWavesN = 2;
constexpr int kMxgWaves = kMxgWavesM * kMxgWavesN;
constexpr int kMxgBlockM = kMxgWaveTile * kMxgWavesM, kMxgBlockN = kMxgWaveTile * kMxgWavesN;
constexpr int kMxgStepBlocks = 4;    // MX blocks per K step (128 elements)

// The instruction's format field (cbsz for A, blgp for B) of a DFQ_MX_* format; -1: unknown.
DFQ_HOST_DEVICE inline int mxg_hw_format(int32_t format) {
    return format == DFQ_MX_FP8_E4M3 ? 0 : format == DFQ_MX_FP6_E2M3 ? 2 : format == DFQ_MX_FP6_E3M2 ? 3
           : format == DFQ_MX_FP4_E2M1 ? 4 : -1;
}
// Code bytes of one MX block, by the instruction's format field.
DFQ_HOST_DEVICE constexpr int mxg_hw_code_bytes(int hw) { return hw == 4 ? 16 : hw == 0 || hw == 1 ? 32 : 24; }
DFQ_HOST_DEVICE inline int mxg_code_bytes(int32_t format) { return mxg_hw_code_bytes(mxg_hw_format(format)); }
// Alignment a code base needs: a block is read as 16-B words (FP6: three 8-B words).
DFQ_HOST_DEVICE inline int mxg_code_align(int32_t format) { return mxg_code_bytes(format) == 24 ? 8 : 16; }

DFQ_HOST_DEVICE inline int64_t mxg_blocks(int64_t K) { return ceil_div(K, (int64_t)DFQ_MX_BLOCK); }
DFQ_HOST_DEVICE inline int64_t mxg_steps(int64_t nb) { return ceil_div(nb, (int64_t)kMxgStepBlocks); }
DFQ_HOST_DEVICE inline int64_t mxg_grid_m(int64_t M) { return ceil_div(M, (int64_t)kMxgBlockM); }
DFQ_HOST_DEVICE inline int64_t mxg_grid_n(int64_t N) { return ceil_div(N, (int64_t)kMxgBlockN); }
DFQ_HOST_DEVICE inline int64_t mxg_grid(int64_t M, int64_t N) { return mxg_grid_m(M) * mxg_grid_n(N); }

// First output row / column of wave `wave` (0..3) of block `block`.
DFQ_HOST_DEVICE inline int64_t mxg_wave_m0(int64_t block, int wave, int64_t N) {
    return block / mxg_grid_n(N) * kMxgBlockM + (wave % kMxgWavesM) * kMxgWaveTile;
}
DFQ_HOST_DEVICE inline int64_t mxg_wave_n0(int64_t block, int wave, int64_t N) {
    return block % mxg_grid_n(N) * kMxgBlockN + (wave / kMxgWavesM) * kMxgWaveTile;
}
// A wave whose tile lies outside the output has nothing to do.
DFQ_HOST_DEVICE inline bool mxg_wave_works(int64_t m0, int64_t n0, int64_t M, int64_t N) { return m0 < M && n0 < N; }

// The operand row (A: m, B: n) a lane holds for instruction tile `sub` of a wave tile that
// starts at row t0, and its MX block in K step `step`.
DFQ_HOST_DEVICE inline int64_t mxg_lane_row(int64_t t0, int sub, int lane) { return t0 + kMxgMfma * sub + (lane & 15); }
DFQ_HOST_DEVICE inline int64_t mxg_lane_kblock(int64_t step, int lane) { return kMxgStepBlocks * step + (lane >> 4); }
// The lane reads that block (otherwise it holds zero codes and scale byte 127).
DFQ_HOST_DEVICE inline bool mxg_lane_loads(int64_t row, int64_t rows, int64_t kb, int64_t nb) { return row < rows && kb < nb; }
// Byte offsets of the block's cb code bytes in codes[rows][nb][cb] and of its byte in scales[rows][nb].
DFQ_HOST_DEVICE inline int64_t mxg_code_offset(int64_t row, int64_t kb, int64_t nb, int cb) { return (row * nb + kb) * cb; }
DFQ_HOST_DEVICE inline int64_t mxg_scale_offset(int64_t row, int64_t kb, int64_t nb) { return row * nb + kb; }

// Where the instruction expects K position k (0..127) of a K step, measured on the hardware
// with exact data.  The scale byte of MX block k / 32 always comes from lane
// group k / 32 (lane group = lane >> 4).  The element does so too for FP6 and FP4: lane
// group g holds MX block g as stored, slot e = k % 32 at bits [w e, w e + w) of its
// registers.  An FP8 operand is laid out in two passes of 64: lane group g holds K
// [16 g, 16 g + 16) in registers 0..3 and K [64 + 16 g, 64 + 16 g + 16) in registers
// 4..7 -- the 16-byte half (g & 1) of MX block g >> 1 and of MX block 2 + (g >> 1), while
// its scale register still holds block g's byte.  So an FP8 lane loads two stored 16-byte
// halves ("split") instead of one stored 32-byte block; the bytes are the stored ones,
// placed by address alone, and one instruction serves every format pair.
DFQ_HOST_DEVICE constexpr bool mxg_hw_split(int hw) { return hw == 0 || hw == 1; }
constexpr int kMxgHalfBytes = 16;   // 16 FP8 codes
// The MX block whose half a split lane holds in registers 4 * half .. 4 * half + 3, and which half of it.
DFQ_HOST_DEVICE inline int64_t mxg_split_kblock(int64_t step, int lane, int half) {
    return kMxgStepBlocks * step + 2 * half + (lane >> 5);
}
DFQ_HOST_DEVICE inline int mxg_split_chunk(int lane) { return (lane >> 4) & 1; }
DFQ_HOST_DEVICE inline int64_t mxg_split_code_offset(int64_t row, int64_t kb, int64_t nb, int lane) {
    return mxg_code_offset(row, kb, nb, 2 * kMxgHalfBytes) + kMxgHalfBytes * mxg_split_chunk(lane);
}
// The instruction's own map, for the host emulation: the lane group and the slot (0..31) of K position k.
DFQ_HOST_DEVICE inline int mxg_hw_group(bool split, int k) { return split ? (k / 16) % 4 : k / 32; }
DFQ_HOST_DEVICE inline int mxg_hw_slot(bool split, int k) { return split ? 16 * (k / 64) + k % 16 : k % 32; }

// Output element of accumulator register `reg` (0..3) of instruction tile (sub_m, sub_n).
DFQ_HOST_DEVICE inline int64_t mxg_out_row(int64_t m0, int sub_m, int lane, int reg) {
    return m0 + kMxgMfma * sub_m + 4 * (lane >> 4) + reg;
}
DFQ_HOST_DEVICE inline int64_t mxg_out_col(int64_t n0, int sub_n, int lane) { return n0 + kMxgMfma * sub_n + (lane & 15); }
DFQ_HOST_DEVICE inline bool mxg_stores(int64_t row, int64_t col, int64_t M, int64_t N) { return row < M && col < N; }
DFQ_HOST_DEVICE inline int64_t mxg_out_offset(int64_t row, int64_t col, int64_t ldo) { return row * ldo + col; }

// The argument checks of dfq_mx_gemm and dfq_mx_linear (no device call), whose descriptors name
// what they share alike: DFQ_OK and the grid, or the error.  A's part is the caller's: a_ok, its
// pointers are there; a_hw, its format field; a_aligned, its base is; lda, the row stride of an
// fp32 A -- K for stored codes, whose rows have no stride of their own, so that the checks of
// lda pass whenever those of K do.
template <class Desc>
inline int mxm_check(const Desc& d, bool a_ok, int a_hw, bool a_aligned, int64_t lda, int64_t& grid) {
    const auto addr = [](const void* p) { return reinterpret_cast<uintptr_t>(p); };
    if (!a_ok || !d.b_codes || !d.b_scales || !d.out) return DFQ_ERR_INVALID;
    if (a_hw < 0 || mxg_hw_format(d.b_format) < 0) return DFQ_ERR_INVALID;
    if (d.flags != 0 || d.reserved != 0) return DFQ_ERR_INVALID;
    if (d.M < 1 || d.N < 1 || d.K < 1) return DFQ_ERR_INVALID;
    // byte and element offsets and the block count stay far inside int64 and the grid inside int32
    if (d.M > (int64_t(1) << 31) || d.N > (int64_t(1) << 31) || d.K > (int64_t(1) << 40) ||
        d.ldo > (int64_t(1) << 40) || lda > (int64_t(1) << 40))
        return DFQ_ERR_INVALID;
    if (d.M > (int64_t(1) << 50) / d.K || d.N > (int64_t(1) << 50) / d.K) return DFQ_ERR_INVALID;
    if (lda < d.K || d.ldo < d.N) return DFQ_ERR_SHAPE;
    if (d.M > (int64_t(1) << 50) / lda) return DFQ_ERR_INVALID;   // row * lda + k
    if (!a_aligned || addr(d.b_codes) % mxg_code_align(d.b_format)) return DFQ_ERR_INVALID;
    if (addr(d.out) % 4 || addr(d.bias) % 4) return DFQ_ERR_INVALID;
    const int64_t g = mxg_grid(d.M, d.N);
    if (g > 0x7fffffff) return DFQ_ERR_UNSUPPORTED;
    grid = g;
    return DFQ_OK;
}

int mxg_check(const dfq_mx_gemm_desc* d, int64_t& grid);

}  // namespace dfq
