// The MX element encoder (include/dfq_hip.h's contract), shared by the quantizer
// (dfq_mx.hip) and the fused linear (dfq_mx_gemm.hip): the element formats' constants,
// the floor rule's exponent and one element's code.  Plain integer / fp32 arithmetic with
// no HIP-only intrinsic, so a host program compiles it too
// (tests/native/mx_linear_plan_check.cpp encodes the case files with it): exact
// power-of-two scalings, one round-to-nearest-even (rintf: v_rndne_f32 on the device,
// the default rounding mode on the host) and a saturating integer min.  Build without FMA
// contraction (-ffp-contract=off), as the library does.
#pragma once
#include <math.h>
#include <stdint.h>

#include "dfq_cle_plan.h"   // DFQ_HOST_DEVICE
#include "dfq_hip.h"

#ifdef __HIPCC__
#define DFQ_MX_INLINE __host__ __device__ __forceinline__
#else
#define DFQ_MX_INLINE inline
#endif

namespace dfq {

template <int FMT>
struct MxFmt;
template <>
struct MxFmt<DFQ_MX_FP4_E2M1> {
    static constexpr int mbits = 1, emin = 0, emax = 2, max_code = 0x7, sign = 0x8;
    static constexpr float qmax = 6.0f;   // the magnitude of max_code
};
template <>
struct MxFmt<DFQ_MX_FP8_E4M3> {
    static constexpr int mbits = 3, emin = -6, emax = 8, max_code = 0x7E, sign = 0x80;   // 0x7F is NaN
    static constexpr float qmax = 448.0f;
};
template <>
struct MxFmt<DFQ_MX_FP6_E2M3> {   // s ee mmm, bias 1: every code is finite
    static constexpr int mbits = 3, emin = 0, emax = 2, max_code = 0x1F, sign = 0x20;
    static constexpr float qmax = 7.5f;
};
template <>
struct MxFmt<DFQ_MX_FP6_E3M2> {   // s eee mm, bias 3: every code is finite
    static constexpr int mbits = 2, emin = -2, emax = 4, max_code = 0x1F, sign = 0x20;
    static constexpr float qmax = 28.0f;
};
template <int FMT>
constexpr bool kMxFp6 = FMT == DFQ_MX_FP6_E2M3 || FMT == DFQ_MX_FP6_E3M2;

DFQ_MX_INLINE uint32_t mx_bits(float x) { return __builtin_bit_cast(uint32_t, x); }
DFQ_MX_INLINE float mx_float(uint32_t b) { return __builtin_bit_cast(float, b); }

DFQ_MX_INLINE float pow2f(int e) { return mx_float((uint32_t)(e + 127) << 23); }   // -127 <= e <= 127; -127: +0

// The shared exponent X of a block whose largest magnitude has the bits `amax_bits`.
template <int FMT>
DFQ_MX_INLINE int mx_exponent(uint32_t amax_bits) {
    if (amax_bits == 0) return -127;
    const int x = (int)(amax_bits >> 23) - 127 - MxFmt<FMT>::emax;   // floor(log2 amax) is the fp32 exponent
    return x < -127 ? -127 : x;                                      // <= 127 - emax
}

// One element: its code and y = +-q * 2^X.  inv = 2^-X, up = 2^X.
//   v = |x| * 2^-X in [0, 2^(emax+1));  e = max(exponent(v), emin);  n = rne(v * 2^(mbits-e)), an
//   integer in [0, 2^(mbits+1)];  magnitude code = n + ((e - emin) << mbits): n < 2^mbits only in the
//   subnormal binade (exponent field 0), n == 2^(mbits+1) carries into the next binade's first code,
//   and an even n is an even code, so round-half-even on n is ties-to-even-code.  The codes ascend
//   with the magnitudes, so the integer min with the largest finite code saturates.
template <int FMT>
DFQ_MX_INLINE uint32_t mx_encode(float x, float inv, float up, float& y) {
    using F = MxFmt<FMT>;
    const uint32_t xb = mx_bits(x);
    const float v = mx_float(xb & 0x7fffffffu) * inv;
    int e = (int)(mx_bits(v) >> 23) - 127;
    e = e < F::emin ? F::emin : e;
    const float n = rintf(v * pow2f(F::mbits - e));
    uint32_t code = (uint32_t)(int)n + ((uint32_t)(e - F::emin) << F::mbits);
    float q = n * pow2f(e - F::mbits);
    if (code > (uint32_t)F::max_code) {
        code = F::max_code;
        q = F::qmax;
    }
    const uint32_t sb = xb & 0x80000000u;
    y = mx_float(mx_bits(q * up) | sb);
    return code | (sb ? (uint32_t)F::sign : 0u);
}

}  // namespace dfq
