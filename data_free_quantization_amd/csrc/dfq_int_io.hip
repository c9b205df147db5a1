// dfq_int_gemm_q, dfq_int_linear_q and dfq_int_conv2d_q: the integer matrix multiply, linear and
// convolution of dfq_int_gemm.hip with stored activation codes at either end (include/dfq_hip.h;
// DESIGN.md 3.9.1) -- what an integer deployment computes: codes in, exact integer sums, the
// affine terms, requantize, codes out.  The K loop, the tiling, the B operand and the folds are
// int_mm_kernel's (dfq_int_mm_kernel.h), unchanged; this file instantiates it, with an IgOutQ argument, with
//   - IgConvCodesA: the convolution's A fragment gathered from a uint8 / int8 NCHW tensor as
//     bytes -- no quantizer, no ballot, 16 bytes held between the loads and the step where the
//     fp32 source holds 16 floats;
//   - IgRowMajorCodeStore / IgNchwCodeStore: the epilogue's (float)acc quantized on the output
//     range by ig_codes4, the next layer's code byte stored in its place -- a lane's four rows of
//     a column are four consecutive bytes of an NCHW plane, one 4-B store where the address
//     allows.
// Its own translation unit, so int_mm_kernel's instantiations keep their code and the library's
// files compile in parallel.  With neither option the entries call the old ones.  No LDS, no
// workspace, no atomics, no split of K: one accumulator per output, as there.
#include "dfq_int_mm_kernel.h"

namespace dfq {
namespace {

// wide: K % 16 == 0, B's (and stored A's) 16-B path
template <class A, class Store, class G>
void igq_launch_b(const G& g, const IgOutQ& oq, bool packed, bool wide, int64_t grid, hipStream_t s) {
    const dim3 blocks((unsigned)grid), threads(kThreads);
    if (packed) {
        if (wide) hipLaunchKernelGGL((int_mm_kernel<A, IgPackedB<true>, Store, IgOutQ>), blocks, threads, 0, s, g, oq);
        else hipLaunchKernelGGL((int_mm_kernel<A, IgPackedB<false>, Store, IgOutQ>), blocks, threads, 0, s, g, oq);
    } else {
        if (wide) hipLaunchKernelGGL((int_mm_kernel<A, IgBytesB<true>, Store, IgOutQ>), blocks, threads, 0, s, g, oq);
        else hipLaunchKernelGGL((int_mm_kernel<A, IgBytesB<false>, Store, IgOutQ>), blocks, threads, 0, s, g, oq);
    }
}
// The convolution's three gathers: masked, pointwise, general.
template <template <bool, bool> class A, class Store>
void igq_launch_conv(const IgcArgs& g, const IgOutQ& oq, bool packed, bool wide, int64_t grid, hipStream_t s) {
    if (igc_masked(g.c)) igq_launch_b<A<false, true>, Store>(g, oq, packed, wide, grid, s);
    else if (mxc_pointwise(g.c)) igq_launch_b<A<true, false>, Store>(g, oq, packed, wide, grid, s);
    else igq_launch_b<A<false, false>, Store>(g, oq, packed, wide, grid, s);
}

}  // namespace
}  // namespace dfq

using namespace dfq;

extern "C" int dfq_int_gemm_q(const dfq_int_gemm_desc* d, const dfq_int_io* io, void* stream) {
    int64_t grid = 0;
    int rc = ig_check(d, grid, igio_bytes(io));
    if (rc == DFQ_OK) rc = igio_check(io, false);
    if (rc != DFQ_OK) return rc;
    if (io->out_bits == 0) return dfq_int_gemm(d, stream);
    const IgArgs g = ig_args(d);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool packed = (d->flags & DFQ_INT_B_PACK4) != 0, wide = ig_wide(d->K);
    if (wide) igq_launch_b<IgStoredA<true>, IgRowMajorCodeStore>(g, ig_out_q(io), packed, wide, grid, s);
    else igq_launch_b<IgStoredA<false>, IgRowMajorCodeStore>(g, ig_out_q(io), packed, wide, grid, s);
    DFQ_LAUNCH_CHECK();
    return DFQ_OK;
}

extern "C" int dfq_int_linear_q(const dfq_int_linear_desc* d, const dfq_int_io* io, void* stream) {
    int64_t grid = 0;
    int rc = igl_check(d, grid, igio_bytes(io));
    if (rc == DFQ_OK) rc = igio_check(io, false);
    if (rc != DFQ_OK) return rc;
    if (io->out_bits == 0) return dfq_int_linear(d, stream);
    const IgArgs g = ig_args(d);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool packed = (d->flags & DFQ_INT_B_PACK4) != 0, wide = ig_wide(d->K);
    if (ig_x_vec(reinterpret_cast<uintptr_t>(d->x), d->ldx, d->K)) igq_launch_b<IgFp32A<true>, IgRowMajorCodeStore>(g, ig_out_q(io), packed, wide, grid, s);
    else igq_launch_b<IgFp32A<false>, IgRowMajorCodeStore>(g, ig_out_q(io), packed, wide, grid, s);
    DFQ_LAUNCH_CHECK();
    return DFQ_OK;
}

extern "C" int dfq_int_conv2d_q(const dfq_int_conv2d_desc* d, const dfq_int_io* io, void* stream) {
    IgcArgs g{};
    int64_t grid = 0;
    int rc = igc_check(d, g.c, g.M, g.K, grid, igio_bytes(io));
    if (rc == DFQ_OK) rc = igio_check(io, true);
    if (rc != DFQ_OK) return rc;
    if (io->x_codes == 0 && io->out_bits == 0) return dfq_int_conv2d(d, stream);
    ig_fill(g, d);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool packed = (d->flags & DFQ_INT_B_PACK4) != 0, wide = ig_wide(g.K);
    const IgOutQ oq = ig_out_q(io);
    if (io->x_codes == 0) igq_launch_conv<IgConvA, IgNchwCodeStore>(g, oq, packed, wide, grid, s);
    else if (io->out_bits == 0) igq_launch_conv<IgConvCodesA, IgNchwStore>(g, oq, packed, wide, grid, s);
    else igq_launch_conv<IgConvCodesA, IgNchwCodeStore>(g, oq, packed, wide, grid, s);
    DFQ_LAUNCH_CHECK();
    return DFQ_OK;
}
