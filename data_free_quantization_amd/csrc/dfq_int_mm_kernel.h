// The integer matrix multiply kernel (dfq_int_gemm.hip has the design): the __global__ template itself,
// over the A source, the B source, the store and a trailing parameter pack -- empty for the old
// entries, whose kernels so keep their one argument and their code, IgOutQ for a code store -- so
// that the code-in / code-out variants (dfq_int_io.hip) are instantiated in a translation unit of
// their own.  Device code: included by those two files and nothing else.
#pragma once
#include "dfq_int_mm_sources.h"

namespace dfq {
namespace {

// A: IgStoredA, IgFp32A, IgConvA or IgConvCodesA.  B: IgBytesB or IgPackedB.  Store: IgRowMajorStore,
// IgNchwStore, or a code store with OutQ = IgOutQ (else no OutQ).
//
// The epilogue of a code store.  ig_codes4 holds a ballot and must sit in wave-uniform control
// flow, so nothing between the K loop and it may leave by lane: a column >= N and a row >= M
// compute 0 instead of being skipped (their parameter loads read column n0's, which exists in a
// working wave), every lane of the wave reaches the quantizer once per instruction tile, and only
// the store is guarded.  The fp32 stores keep their lane-divergent skips.
template <class A, class B, class Store, class... OutQ>
__global__ __launch_bounds__(kThreads) void int_mm_kernel(const typename A::Args g, const OutQ... oq) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int64_t m0 = mxg_wave_m0(blockIdx.x, wave, g.N), n0 = mxg_wave_n0(blockIdx.x, wave, g.N);
    if (!mxg_wave_works(m0, n0, g.M, g.N)) return;   // wave-uniform; the kernel has no barrier
    const IgAParams pa = A::params(g);
    const uint32_t xb = ig_xor_mask(g.b_signed != 0);
    const ig_v4i zero4 = {0, 0, 0, 0}, ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101};
    // rb: sum_k b' of C's columns -- one per column tile, or, under a mask, one per tile: sum_k v b'
    constexpr int kRb = A::kMask ? kMxgSub : 1;
    ig_v4i acc[kMxgSub][kMxgSub], ra[kMxgSub], rb[kRb][kMxgSub];
    const typename A::Rows rows(g, m0, lane);
    int64_t brow[kMxgSub];
#pragma unroll
    for (int i = 0; i < kMxgSub; ++i) {
        ra[i] = zero4;
        brow[i] = mxg_lane_row(n0, i, lane);
#pragma unroll
        for (int j = 0; j < kMxgSub; ++j) acc[i][j] = zero4;
#pragma unroll
        for (int t = 0; t < kRb; ++t) rb[t][i] = zero4;
    }
    const int64_t steps = ig_steps(g.K);
    typename A::Fetched fa[kMxgSub];
    typename B::Fetched fb[kMxgSub];
#pragma unroll
    for (int i = 0; i < kMxgSub; ++i) {
        A::fetch(fa[i], g, rows.at(i), 0, lane);
        B::fetch(fb[i], g, brow[i], 0, lane);
    }
    for (int64_t s = 0; s < steps; ++s) {
        const int64_t k0 = ig_lane_k0(s, lane);
        ig_v4i a[kMxgSub], b[kMxgSub], am[kMxgSub];
#pragma unroll
        for (int i = 0; i < kMxgSub; ++i) {
            a[i] = A::operand(fa[i], pa, ig_lane_valid(rows.m(i), g.M, k0, g.K));
            b[i] = B::operand(fb[i], xb, ig_lane_valid(brow[i], g.N, k0, g.K));
            if constexpr (A::kMask) am[i] = A::mask(fa[i]);
        }
        if (s + 1 < steps) {
#pragma unroll
            for (int i = 0; i < kMxgSub; ++i) {
                A::fetch(fa[i], g, rows.at(i), s + 1, lane);
                B::fetch(fb[i], g, brow[i], s + 1, lane);
            }
        }
#pragma unroll
        for (int i = 0; i < kMxgSub; ++i) {
#pragma unroll
            for (int j = 0; j < kMxgSub; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[i], b[j], acc[i][j], 0, 0, 0);
            ra[i] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[i], ones, ra[i], 0, 0, 0);   // sum_k a' of C's rows
            if constexpr (A::kMask) {
#pragma unroll
                for (int j = 0; j < kMxgSub; ++j) rb[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(am[i], b[j], rb[i][j], 0, 0, 0);
            } else {
                rb[0][i] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, b[i], rb[0][i], 0, 0, 0);   // sum_k b' of C's columns
            }
        }
    }
    // the contract's integers, then its fp64 steps in its order
    const DFQ_GLOBAL float* bias = (const DFQ_GLOBAL float*)g.bias;
    const DFQ_GLOBAL float* b_scale = (const DFQ_GLOBAL float*)g.b_scale;
    const DFQ_GLOBAL float* b_zero = (const DFQ_GLOBAL float*)g.b_zero;
    const int ob = ig_offset(g.b_signed != 0);
    const bool has_zb = b_zero != nullptr;
    const double sa = (double)pa.s, za = (double)pa.z;
    int64_t T[kMxgSub][4];   // the contract's T of the lane's output rows: K unless a mask is on
#pragma unroll
    for (int i = 0; i < kMxgSub; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) T[i][r] = A::taps(g, mxg_out_row(m0, i, lane, r));
    IgAParams po;
    if constexpr (Store::kCodes) po = ig_out_params(oq...);   // once per wave, before the epilogue
#pragma unroll
    for (int j = 0; j < kMxgSub; ++j) {
        int64_t col = mxg_out_col(n0, j, lane);
        if constexpr (Store::kCodes) {
            if (col >= g.N) col = n0;   // computes column n0's values and stores nothing (the store looks at the real column)
        } else {
            if (col >= g.N) continue;
        }
        const int64_t pc = g.per_row ? col : 0;
        const double sb = (double)b_scale[pc], zb = has_zb ? (double)b_zero[pc] : 0.0;
        const double ss = sa * sb, sz = sa * zb, zs = za * sb, zz = za * zb;
        const double bv = bias != nullptr ? (double)bias[col] : 0.0;
#pragma unroll
        for (int i = 0; i < kMxgSub; ++i) {
            float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t row = mxg_out_row(m0, i, lane, r);
                if (!mxg_stores(row, col, g.M, g.N)) continue;   // no ballot inside this loop
                const int rbv = rb[A::kMask ? i : 0][j][r];
                const int64_t P = igc_fold_p(acc[i][j][r], ra[i][r], rbv, pa.off, ob, T[i][r]);
                double t = ss * (double)P;
                if (has_zb) t += sz * (double)igc_fold_s(ra[i][r], pa.off, T[i][r]);
                if (pa.has_z) t += zs * (double)igc_fold_s(rbv, ob, T[i][r]);
                if (has_zb && pa.has_z) t += zz * (double)T[i][r];
                if (bias != nullptr) t += bv;
                v[r] = (float)t;
                if constexpr (!Store::kGroups) Store::store(v[r], g, row, col);
            }
            if constexpr (Store::kCodes) Store::store(ig_codes4(v, po), g, mxg_out_row(m0, i, lane, 0), mxg_out_col(n0, j, lane));
            else if constexpr (Store::kGroups) Store::store(v, g, mxg_out_row(m0, i, lane, 0), col);
        }
    }
}

}  // namespace
}  // namespace dfq
