// dfq_int_gemm, dfq_int_linear and dfq_int_conv2d: out[m][n] = sum_k A[m][k] * B[n][k] (+ bias[n])
// of the affine values A = qa * sa + za, B = qb * sb[n] + zb[n] that the sweep's integer codes
// stand for, on the integer matrix instruction v_mfma_i32_16x16x64_i8 (include/dfq_hip.h;
// DESIGN.md 3.9).  One kernel template over how a lane obtains the 16 bytes of its A fragment --
// stored codes (dfq_int_gemm), fp32 x quantized on the way (dfq_int_linear: dfq_fake_quant_given's
// quantizer, the code being its q), or the im2col rows of an NCHW x gathered and quantized on the
// way (dfq_int_conv2d) -- of its B fragment: 16 stored bytes, or 8 packed bytes widened -- and
// over where the result goes: row-major, or NCHW.
//
// The convolution pads with the real value 0: a padding tap is absent from every sum (0 in the
// signed domain), so sum_k b' over the taps inside the image depends on the output row.  Where
// the geometry has padding the two ones x B-fragment instructions become four mask x B-fragment
// instructions (the mask operand holds 0x01 where the tap is inside), ten a step, and the folds
// take T[m] = sum_k v, a closed form of the row's position, where they had K
// (dfq_int_conv_plan.h).
//
// All addressing and every bit operation on a fragment is dfq_int_gemm_plan.h's (the convolution's:
// dfq_mx_conv_plan.h's and dfq_int_conv_plan.h's); the tiling is
// dfq_mx_gemm's: a wave owns a 32 x 32 output tile, so each of its two A and two B fragments of a
// K step (64 elements) feeds two product instructions, and four waves make a 64 x 64 block.  The
// instruction multiplies signed bytes.  An unsigned code q enters as q - 128 (xor 0x80); elements
// at k >= K and rows past M / N enter as 0 in that domain.  Next to the four products a step
// issues four more instructions against an all-ones operand: A-fragment x ones leaves sum_k a' in
// every column of C -- already in the lane and register that stores that row -- and ones x
// B-fragment leaves sum_k b' in every row.  The epilogue folds the two offsets back in integers
// (ig_fold_p / ig_fold_s: the contract's P, Sa and Sb, exact) and then runs the contract's fp64
// steps in its order; the library builds with -ffp-contract=off.  No LDS, no workspace, no
// atomics, no split of K: an output element is one accumulator of one lane, K steps in order.
//
// K % 16 == 0: a lane's bytes are one aligned 16-B (packed: 8-B) load and all exist or none do.
// Otherwise: guarded byte loads into the same words.  fp32 A: 16-B loads where x's rows allow
// (ig_x_vec), else 4-B loads.  The A fragment of dfq_int_linear is re-quantized by every wave that
// needs it (once per 32 output columns): the kernel is aimed at layer-sized calls.
//
// A K step: turn what was fetched for step s into operand registers, issue the loads of step
// s + 1, then the step's eight instructions.
#include "dfq_int_mm_sources.h"

namespace dfq {
namespace {

// A: IgStoredA, IgFp32A or IgConvA.  B: IgBytesB or IgPackedB.  Store: IgRowMajorStore or IgNchwStore.
template <class A, class B, class Store>
__global__ __launch_bounds__(kThreads) void int_mm_kernel(const typename A::Args g) {
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
#pragma unroll
    for (int j = 0; j < kMxgSub; ++j) {
        const int64_t col = mxg_out_col(n0, j, lane);
        if (col >= g.N) continue;
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
                if (!mxg_stores(row, col, g.M, g.N)) continue;
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
            if constexpr (Store::kGroups) Store::store(v, g, mxg_out_row(m0, i, lane, 0), col);
        }
    }
}

template <class A, class Store, class G>
void ig_launch_b(const G& g, bool packed, bool wide, int64_t grid, hipStream_t s) {
    const dim3 blocks((unsigned)grid), threads(kThreads);
    if (packed) {
        if (wide) hipLaunchKernelGGL((int_mm_kernel<A, IgPackedB<true>, Store>), blocks, threads, 0, s, g);
        else hipLaunchKernelGGL((int_mm_kernel<A, IgPackedB<false>, Store>), blocks, threads, 0, s, g);
    } else {
        if (wide) hipLaunchKernelGGL((int_mm_kernel<A, IgBytesB<true>, Store>), blocks, threads, 0, s, g);
        else hipLaunchKernelGGL((int_mm_kernel<A, IgBytesB<false>, Store>), blocks, threads, 0, s, g);
    }
}

}  // namespace
}  // namespace dfq

using namespace dfq;

extern "C" int dfq_int_gemm(const dfq_int_gemm_desc* d, void* stream) {
    static_assert(kMxgWaves * kWave == kThreads, "four waves per block");
    int64_t grid = 0;
    const int rc = ig_check(d, grid);
    if (rc != DFQ_OK) return rc;
    const IgArgs g = ig_args(d);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool packed = (d->flags & DFQ_INT_B_PACK4) != 0, wide = ig_wide(d->K);
    if (wide) ig_launch_b<IgStoredA<true>, IgRowMajorStore>(g, packed, wide, grid, s);
    else ig_launch_b<IgStoredA<false>, IgRowMajorStore>(g, packed, wide, grid, s);
    DFQ_LAUNCH_CHECK();
    return DFQ_OK;
}

extern "C" int dfq_int_linear(const dfq_int_linear_desc* d, void* stream) {
    int64_t grid = 0;
    const int rc = igl_check(d, grid);
    if (rc != DFQ_OK) return rc;
    const IgArgs g = ig_args(d);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool packed = (d->flags & DFQ_INT_B_PACK4) != 0, wide = ig_wide(d->K);
    if (ig_x_vec(reinterpret_cast<uintptr_t>(d->x), d->ldx, d->K)) ig_launch_b<IgFp32A<true>, IgRowMajorStore>(g, packed, wide, grid, s);
    else ig_launch_b<IgFp32A<false>, IgRowMajorStore>(g, packed, wide, grid, s);
    DFQ_LAUNCH_CHECK();
    return DFQ_OK;
}

extern "C" int dfq_int_conv2d(const dfq_int_conv2d_desc* d, void* stream) {
    IgcArgs g{};
    int64_t grid = 0;
    const int rc = igc_check(d, g.c, g.M, g.K, grid);
    if (rc != DFQ_OK) return rc;
    ig_fill(g, d);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool packed = (d->flags & DFQ_INT_B_PACK4) != 0, wide = ig_wide(g.K);
    if (igc_masked(g.c)) ig_launch_b<IgConvA<false, true>, IgNchwStore>(g, packed, wide, grid, s);
    else if (mxc_pointwise(g.c)) ig_launch_b<IgConvA<true, false>, IgNchwStore>(g, packed, wide, grid, s);
    else ig_launch_b<IgConvA<false, false>, IgNchwStore>(g, packed, wide, grid, s);
    DFQ_LAUNCH_CHECK();
    return DFQ_OK;
}
