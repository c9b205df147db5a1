// The activation quantizer the one-launch integer kernels share (dfq_int_linear, dfq_int_conv2d:
// dfq_int_gemm.hip; dfq_int_dwconv2d: dfq_int_dwconv.hip): dfq_fake_quant_given's parameters and
// the code bytes of four fp32 elements.  Device code.
#pragma once
#include "dfq_common.h"

#include "dfq_int_gemm_plan.h"

namespace dfq {

struct IgAParams {
    float s, z;
    bool has_z;
    uint32_t xm;   // ig_xor_mask of A's signedness
    int off;       // ig_offset
    QParams q;     // fp32 A only
    float rs;      // fp32 A only: rcp(q.s), qdq_screen's
    float band;    // fp32 A only: qdq_screen's band factor (screen_rcp)
};

// The parameters as fq_given_kernel builds them: the range from min_dev[0] / max_dev[0] (device
// floats read as exact doubles) or gmin / gmax; x_flags holds DFQ_SCALE_F32 or 0.
__device__ __forceinline__ IgAParams ig_quant_params(const float* min_dev, const float* max_dev, double gmin, double gmax,
                                                     int x_bits, int x_symmetric, int x_flags) {
    if (min_dev) gmin = (double)((const DFQ_GLOBAL float*)min_dev)[0];
    if (max_dev) gmax = (double)((const DFQ_GLOBAL float*)max_dev)[0];
    IgAParams p;
    p.q = make_qparams((float)gmin, (float)gmax, x_bits, x_symmetric != 0, x_flags | DFQ_GIVEN_RANGE, gmin, gmax);
    p.rs = screen_rcp(p.q.s, p.band);
    p.s = p.q.s;
    p.z = p.q.mn;
    p.has_z = true;
    p.xm = ig_xor_mask(x_symmetric != 0);
    p.off = ig_offset(x_symmetric != 0);
    return p;
}

// qdq's q of x[0 .. 3], four at a time as the sweep takes them: the screened reciprocal
// quotient, the IEEE divide only where a lane of the wave sits near a rounding boundary
// (qdq_screen; the same codes).  Every lane of a working wave gets here: the ballot is in
// wave-uniform control flow.  The word holds the bytes dfq_quantize_tensor stores.
__device__ __forceinline__ uint32_t ig_codes4(const float* x, const IgAParams& p) {
    float t[4];
    bool need[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) t[e] = qdq_screen(x[e], p.q, p.rs, p.band, need[e]);
    if (__builtin_amdgcn_ballot_w64(need[0] | need[1] | need[2] | need[3])) {   // wave-uniform, rare
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (need[e]) t[e] = qdq_exact_t(x[e], p.q);
    }
    uint32_t w = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float q;
        qdq_finish(t[e], p.q, q);
        w |= ((uint32_t)(int)q & 0xFFu) << (8 * e);
    }
    return w;
}

}  // namespace dfq
