// dfq_int_gemm_grouped, dfq_int_linear_grouped and dfq_int_conv2d_grouped: the integer matrix
// multiply, linear and convolution of dfq_int_gemm.hip with group-wise B parameters -- an fp32
// scale and zero per g consecutive elements of a row of B, b_scale / b_zero [N][G], G = ceil(K / g)
// (include/dfq_hip.h).  A group's scale cannot be applied after the K loop, so the
// accumulation has two levels: the int32 accumulators of int_mm_kernel hold one group's exact
// sums, and every one of the lane's 16 outputs has a double running sum (32 registers) that takes
// the contract's four fp64 steps of a group when the group closes, groups in ascending order;
// the integer accumulators then restart from zero.  The tiling, the fragment sources, the fetch
// pipeline and the folds are int_mm_kernel's (dfq_int_mm_sources.h, dfq_int_gemm_plan.h,
// dfq_int_conv_plan.h); which group a step adds to and where it closes is dfq_int_gemm_plan.h's
// igg_*.
//
// g a multiple of 64: a group closes between two K steps; a step issues int_mm_kernel's
// instructions (eight; under a tap mask twelve, below).  g = 32: half a step.  A lane holds
// k = 64 s + 16 (lane >> 4), so lanes 0..31 hold the step's first group and lanes 32..63 its
// second: the step runs as two passes over the same fetched fragments, pass h with the A-side
// operands (the A fragment, the all-ones operand of the column sums, the tap mask) zero in the
// lanes of the other half, so its products are the sums over group 2 s + h alone, and the group
// closes after the pass.  One set of integer accumulators serves both passes; sixteen
// instructions a step (twenty-four under a mask).  g is a kernel argument, every branch on it
// is wave-uniform, and the two designs share one code object per fragment source.
//
// Under a tap mask (a convolution with padding) T_j[m] = sum_{k in j} v is no closed form of the
// row alone: it comes from one more instruction per row tile, mask operand x all-ones, which
// leaves it in the lane and register that stores the row, as A x ones leaves sum_k a'.  Without a
// mask T_j is the group's element count K_j.
//
// No LDS, no workspace, no atomics, no split of K: an output is one double of one lane, the
// groups in order, and inside a group one int32 accumulator, the K steps in order.
#include "dfq_int_mm_sources.h"

namespace dfq {
namespace {

// A lane's registers of an A-side operand in a pass: zero where the lane's k belong to the other half.
__device__ __forceinline__ ig_v4i igg_in_pass(const ig_v4i& v, bool in) {
    ig_v4i r;
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = in ? v[j] : 0;
    return r;
}

// A, B, Store: int_mm_kernel's.  bg: the group size (igg_allowed).
template <class A, class B, class Store>
__global__ __launch_bounds__(kThreads) void int_mm_group_kernel(const typename A::Args g, const int bg) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int64_t m0 = mxg_wave_m0(blockIdx.x, wave, g.N), n0 = mxg_wave_n0(blockIdx.x, wave, g.N);
    if (!mxg_wave_works(m0, n0, g.M, g.N)) return;   // wave-uniform; the kernel has no barrier
    const IgAParams pa = A::params(g);
    const uint32_t xb = ig_xor_mask(g.b_signed != 0);
    const ig_v4i zero4 = {0, 0, 0, 0}, ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101};
    constexpr int kRb = A::kMask ? kMxgSub : 1;
    // one group's sums: int_mm_kernel's acc, ra and rb, and under a mask rt: sum_k v of C's rows
    ig_v4i acc[kMxgSub][kMxgSub], ra[kMxgSub], rb[kRb][kMxgSub], rt[kMxgSub];
    double sum[kMxgSub][kMxgSub][4];   // the contract's acc of the lane's outputs: [row tile][column tile][register]
    const typename A::Rows rows(g, m0, lane);
    int64_t brow[kMxgSub], pcol[kMxgSub];
    const DFQ_GLOBAL float* b_scale = (const DFQ_GLOBAL float*)g.b_scale;
    const DFQ_GLOBAL float* b_zero = (const DFQ_GLOBAL float*)g.b_zero;
    const int64_t G = igg_groups(g.K, bg);
#pragma unroll
    for (int i = 0; i < kMxgSub; ++i) {
        ra[i] = rt[i] = zero4;
        brow[i] = mxg_lane_row(n0, i, lane);
        const int64_t col = mxg_out_col(n0, i, lane);
        pcol[i] = igg_param_offset(col < g.N ? col : n0, 0, G);   // a column past N is never stored: it reads column n0's
#pragma unroll
        for (int j = 0; j < kMxgSub; ++j) {
            acc[i][j] = zero4;
#pragma unroll
            for (int r = 0; r < 4; ++r) sum[i][j][r] = 0.0;
        }
#pragma unroll
        for (int t = 0; t < kRb; ++t) rb[t][i] = zero4;
    }
    const int ob = ig_offset(g.b_signed != 0);
    const bool has_zb = b_zero != nullptr;
    const double sa = (double)pa.s, za = (double)pa.z;
    const int steps = (int)ig_steps(g.K), passes = igg_passes(bg);
    typename A::Fetched fa[kMxgSub];
    typename B::Fetched fb[kMxgSub];
#pragma unroll
    for (int i = 0; i < kMxgSub; ++i) {
        A::fetch(fa[i], g, rows.at(i), 0, lane);
        B::fetch(fb[i], g, brow[i], 0, lane);
    }
    for (int s = 0; s < steps; ++s) {
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
        for (int pass = 0; pass < passes; ++pass) {
            const int grp = igg_group(s, pass, bg), len = igg_group_len(grp, bg, g.K);
            if (len <= 0) break;   // K ends in the step's first half
            const bool in = igg_lane_in_pass(lane, pass, bg);
            const ig_v4i ones_p = igg_in_pass(ones, in);
#pragma unroll
            for (int i = 0; i < kMxgSub; ++i) {
                const ig_v4i ap = igg_in_pass(a[i], in);
#pragma unroll
                for (int j = 0; j < kMxgSub; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ap, b[j], acc[i][j], 0, 0, 0);
                ra[i] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ap, ones, ra[i], 0, 0, 0);
                if constexpr (A::kMask) {
                    const ig_v4i mp = igg_in_pass(am[i], in);
#pragma unroll
                    for (int j = 0; j < kMxgSub; ++j) rb[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(mp, b[j], rb[i][j], 0, 0, 0);
                    rt[i] = __builtin_amdgcn_mfma_i32_16x16x64_i8(mp, ones, rt[i], 0, 0, 0);
                } else {
                    rb[0][i] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones_p, b[i], rb[0][i], 0, 0, 0);
                }
            }
            if (!igg_closes(s, steps, bg)) continue;
            // the group's integers, then its fp64 steps in the contract's order
#pragma unroll
            for (int j = 0; j < kMxgSub; ++j) {
                const double sb = (double)b_scale[pcol[j] + grp], zb = has_zb ? (double)b_zero[pcol[j] + grp] : 0.0;
                const double ss = sa * sb, sz = sa * zb, zs = za * sb, zz = za * zb;
#pragma unroll
                for (int i = 0; i < kMxgSub; ++i) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int64_t T = A::kMask ? (int64_t)rt[i][r] : (int64_t)len;
                        const int rbv = rb[A::kMask ? i : 0][j][r];
                        const double p = ss * (double)igc_fold_p(acc[i][j][r], ra[i][r], rbv, pa.off, ob, T);
                        double t = grp == 0 ? p : sum[i][j][r] + p;   // the first term assigns: no 0.0 + (-0.0)
                        if (has_zb) t += sz * (double)igc_fold_s(ra[i][r], pa.off, T);
                        if (pa.has_z) t += zs * (double)igc_fold_s(rbv, ob, T);
                        if (has_zb && pa.has_z) t += zz * (double)T;
                        sum[i][j][r] = t;
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < kMxgSub; ++i) {
                ra[i] = rt[i] = zero4;
#pragma unroll
                for (int j = 0; j < kMxgSub; ++j) acc[i][j] = zero4;
#pragma unroll
                for (int t = 0; t < kRb; ++t) rb[t][i] = zero4;
            }
        }
    }
    const DFQ_GLOBAL float* bias = (const DFQ_GLOBAL float*)g.bias;
#pragma unroll
    for (int j = 0; j < kMxgSub; ++j) {
        const int64_t col = mxg_out_col(n0, j, lane);
        if (col >= g.N) continue;
        const double bv = bias != nullptr ? (double)bias[col] : 0.0;
#pragma unroll
        for (int i = 0; i < kMxgSub; ++i) {
            float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t row = mxg_out_row(m0, i, lane, r);
                if (!mxg_stores(row, col, g.M, g.N)) continue;
                double t = sum[i][j][r];
                if (bias != nullptr) t += bv;
                v[r] = (float)t;
                if constexpr (!Store::kGroups) Store::store(v[r], g, row, col);
            }
            if constexpr (Store::kGroups) Store::store(v, g, mxg_out_row(m0, i, lane, 0), col);
        }
    }
}

template <class A, class Store, class G>
void igg_launch_b(const G& g, int bg, bool packed, bool wide, int64_t grid, hipStream_t s) {
    const dim3 blocks((unsigned)grid), threads(kThreads);
    if (packed) {
        if (wide) hipLaunchKernelGGL((int_mm_group_kernel<A, IgPackedB<true>, Store>), blocks, threads, 0, s, g, bg);
        else hipLaunchKernelGGL((int_mm_group_kernel<A, IgPackedB<false>, Store>), blocks, threads, 0, s, g, bg);
    } else {
        if (wide) hipLaunchKernelGGL((int_mm_group_kernel<A, IgBytesB<true>, Store>), blocks, threads, 0, s, g, bg);
        else hipLaunchKernelGGL((int_mm_group_kernel<A, IgBytesB<false>, Store>), blocks, threads, 0, s, g, bg);
    }
}

}  // namespace
}  // namespace dfq

using namespace dfq;

extern "C" int dfq_int_gemm_grouped(const dfq_int_gemm_desc* d, int32_t b_group, void* stream) {
    int64_t grid = 0;
    int rc = ig_check(d, grid);
    if (rc == DFQ_OK) rc = igg_check(b_group, d->flags);
    if (rc != DFQ_OK) return rc;
    const IgArgs g = ig_args(d);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool packed = (d->flags & DFQ_INT_B_PACK4) != 0, wide = ig_wide(d->K);
    if (wide) igg_launch_b<IgStoredA<true>, IgRowMajorStore>(g, b_group, packed, wide, grid, s);
    else igg_launch_b<IgStoredA<false>, IgRowMajorStore>(g, b_group, packed, wide, grid, s);
    DFQ_LAUNCH_CHECK();
    return DFQ_OK;
}

extern "C" int dfq_int_linear_grouped(const dfq_int_linear_desc* d, int32_t b_group, void* stream) {
    int64_t grid = 0;
    int rc = igl_check(d, grid);
    if (rc == DFQ_OK) rc = igg_check(b_group, d->flags);
    if (rc != DFQ_OK) return rc;
    const IgArgs g = ig_args(d);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool packed = (d->flags & DFQ_INT_B_PACK4) != 0, wide = ig_wide(d->K);
    if (ig_x_vec(reinterpret_cast<uintptr_t>(d->x), d->ldx, d->K)) igg_launch_b<IgFp32A<true>, IgRowMajorStore>(g, b_group, packed, wide, grid, s);
    else igg_launch_b<IgFp32A<false>, IgRowMajorStore>(g, b_group, packed, wide, grid, s);
    DFQ_LAUNCH_CHECK();
    return DFQ_OK;
}

extern "C" int dfq_int_conv2d_grouped(const dfq_int_conv2d_desc* d, int32_t b_group, void* stream) {
    IgcArgs g{};
    int64_t grid = 0;
    int rc = igc_check(d, g.c, g.M, g.K, grid);
    if (rc == DFQ_OK) rc = igg_check(b_group, d->flags);
    if (rc != DFQ_OK) return rc;
    ig_fill(g, d);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool packed = (d->flags & DFQ_INT_B_PACK4) != 0, wide = ig_wide(g.K);
    if (igc_masked(g.c)) igg_launch_b<IgConvA<false, true>, IgNchwStore>(g, b_group, packed, wide, grid, s);
    else if (mxc_pointwise(g.c)) igg_launch_b<IgConvA<true, false>, IgNchwStore>(g, b_group, packed, wide, grid, s);
    else igg_launch_b<IgConvA<false, false>, IgNchwStore>(g, b_group, packed, wide, grid, s);
    DFQ_LAUNCH_CHECK();
    return DFQ_OK;
}
