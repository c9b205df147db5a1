// dfq_int_dwconv2d_q: the integer depthwise convolution of dfq_int_dwconv.hip with stored
// activation codes at either end (include/dfq_hip.h): codes in -> fp32 out,
// fp32 in -> codes out, codes in -> codes out.  The kernel is dfq_int_dwconv_kernel.h's template
// (phase 1 copies bytes instead of quantizing, phase 3 quantizes a lane's four outputs and stores
// a word of code bytes); its own translation unit, so dfq_int_dwconv2d's kernel keeps its code.
// With neither option the entry calls the old one.
#include "dfq_int_dwconv_kernel.h"

using namespace dfq;

extern "C" int dfq_int_dwconv2d_q(const dfq_int_dwconv2d_desc* d, const dfq_int_io* io, void* stream) {
    DwArgs a{};
    int64_t grid = 0;
    int rc = dwc_check(d, a.g, grid, igio_bytes(io));   // the old entry's checks: a byte tensor needs no alignment
    if (rc == DFQ_OK) rc = igio_check(io, true);
    if (rc != DFQ_OK) return rc;
    if (io->x_codes == 0 && io->out_bits == 0) return dfq_int_dwconv2d(d, stream);
    dw_fill(a, d);
    a.out_min_dev = io->out_min_dev;
    a.out_max_dev = io->out_max_dev;
    a.out_gmin = io->out_given_min;
    a.out_gmax = io->out_given_max;
    a.out_bits = io->out_bits;
    a.out_symmetric = io->out_symmetric;
    a.out_flags = io->out_flags;
    const dim3 blocks((unsigned)grid), threads(kThreads);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (io->x_codes == 0) hipLaunchKernelGGL((int_dwconv_kernel<false, true>), blocks, threads, 0, s, a);
    else if (io->out_bits == 0) hipLaunchKernelGGL((int_dwconv_kernel<true, false>), blocks, threads, 0, s, a);
    else hipLaunchKernelGGL((int_dwconv_kernel<true, true>), blocks, threads, 0, s, a);
    DFQ_LAUNCH_CHECK();
    return DFQ_OK;
}
