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
#include "dfq_int_mm_kernel.h"

namespace dfq {
namespace {

// int_mm_kernel<A, B, Store> is dfq_int_mm_kernel.h's.  A: IgStoredA, IgFp32A or IgConvA.  B: IgBytesB or IgPackedB.
// Store: IgRowMajorStore or IgNchwStore.
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
