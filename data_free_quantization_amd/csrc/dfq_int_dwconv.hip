// dfq_int_dwconv2d: the depthwise convolution (groups == C, N = C * mult) of the affine values
// that the activation codes and the weight's integer codes stand for, in one launch on the packed
// 8-bit dot instruction v_dot4c_i32_i8 (include/dfq_hip.h).  A depthwise layer has
// K = KH * KW products per output and one output column per channel: it is bound by bandwidth and
// by the quantizer, not by the matrix instruction, so it does not go through dfq_int_gemm.hip's
// tiles.
//
// A workgroup owns a tile of outputs of one (b, c) plane -- several whole planes where a plane is
// one tile -- for all mult output channels (dfq_int_dwconv_plan.h):
//   1. it reads the tile's input footprint with its halo, four consecutive columns a lane
//      (4-B loads, coalesced along W), quantizes every element ONCE (dfq_int_quant.h: the sweep's
//      screened quotient; the ballot sits in a loop whose trip count is the block's, so every lane
//      reaches it and lanes outside the image or the footprint carry a dummy 0 that is masked
//      afterwards) and writes the code bytes, a word a lane, to LDS -- 0 outside the image;
//   2. per round of mc output channels it writes the planes' weight bytes to LDS as operand
//      words (signed domain, four taps a word);
//   3. a lane takes four consecutive outputs of a row at a time: per word of four taps it
//      gathers the four code bytes of each output from LDS, moves them to the signed domain on
//      the taps inside the image (the tap mask: row bits x column bits) and issues three dot
//      instructions an output -- a' . b', a' . ones, mask . b' -- then folds the offsets back in
//      integers (ig_fold_p / ig_fold_s with T) and runs the contract's fp64 steps in its order;
//      the four results go out as one 16-B store (4-B aligned) where all four exist, else one by
//      one.
// One accumulator per output element, the taps in order, no atomics, no workspace.  All addressing,
// every mask bit and the folds are dfq_int_dwconv_plan.h's.  The kernel is dfq_int_dwconv_kernel.h's
// template, here with fp32 at both ends; dfq_int_dwconv_io.hip has the stored-code variants.
#include "dfq_int_dwconv_kernel.h"

using namespace dfq;

extern "C" int dfq_int_dwconv2d(const dfq_int_dwconv2d_desc* d, void* stream) {
    static_assert(kThreads == 256, "dfq_int_dwconv_plan.h sizes a workgroup's quads for 256 lanes");
    DwArgs a{};
    int64_t grid = 0;
    const int rc = dwc_check(d, a.g, grid);
    if (rc != DFQ_OK) return rc;
    dw_fill(a, d);
    hipLaunchKernelGGL((int_dwconv_kernel<false, false>), dim3((unsigned)grid), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
    DFQ_LAUNCH_CHECK();
    return DFQ_OK;
}
