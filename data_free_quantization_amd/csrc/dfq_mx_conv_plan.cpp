// Host-only part of dfq_mx_conv2d: the argument checks, the geometry and the grid
// (dfq_mx_conv_plan.h).  Plain C++: no HIP header, no device code.
#include <initializer_list>

#include "dfq_mx_conv_plan.h"

namespace dfq {

int mxc_check(const dfq_mx_conv2d_desc* d, MxcGeom& g, int64_t& M, int64_t& K, int64_t& grid) {
    const auto addr = [](const void* p) { return reinterpret_cast<uintptr_t>(p); };
    g = MxcGeom{};
    M = K = grid = 0;
    if (!d) return DFQ_ERR_INVALID;
    if (!d->x || !d->b_codes || !d->b_scales || !d->out) return DFQ_ERR_INVALID;
    if (mxg_hw_format(d->x_format) < 0 || mxg_hw_format(d->b_format) < 0) return DFQ_ERR_INVALID;
    if (d->flags != 0 || d->reserved != 0) return DFQ_ERR_INVALID;
    // every extent, stride, dilation and padding: at least 1 (padding 0), at most 2^28, so that
    // H + 2 ph + dh (and W's) stays inside int32
    constexpr int64_t kMax = int64_t(1) << 28;
    for (int64_t v : {d->B, d->C, d->H, d->W, d->N, d->KH, d->KW, d->stride_h, d->stride_w, d->dil_h, d->dil_w})
        if (v < 1 || v > kMax) return DFQ_ERR_INVALID;
    for (int64_t v : {d->pad_h, d->pad_w})
        if (v < 0 || v > kMax) return DFQ_ERR_INVALID;
    constexpr int64_t k31 = int64_t(1) << 31;
    // offsets inside one image of x and the im2col column inside int32 (factor by factor: no product overflows)
    if (d->H * d->W >= k31 || d->C * (d->H * d->W) >= k31) return DFQ_ERR_INVALID;
    if (d->KH * d->KW >= k31 || d->C * (d->KH * d->KW) >= k31) return DFQ_ERR_INVALID;
    if (addr(d->x) % 4 || addr(d->out) % 4 || addr(d->bias) % 4) return DFQ_ERR_INVALID;
    if (addr(d->b_codes) % mxg_code_align(d->b_format)) return DFQ_ERR_INVALID;
    const int64_t OH = mxc_out_extent(d->H, d->pad_h, d->dil_h, d->KH, d->stride_h);
    const int64_t OW = mxc_out_extent(d->W, d->pad_w, d->dil_w, d->KW, d->stride_w);
    if (OH < 1 || OW < 1) return DFQ_ERR_SHAPE;
    if (OH * OW >= k31 || d->N * (OH * OW) >= k31) return DFQ_ERR_INVALID;   // offsets inside one image of out
    if (d->B * (OH * OW) > k31) return DFQ_ERR_INVALID;                      // M, as dfq_mx_gemm's
    K = d->C * d->KH * d->KW;
    M = d->B * OH * OW;
    if (d->N > (int64_t(1) << 50) / K) return DFQ_ERR_INVALID;               // B's code offsets
    g.C = (int32_t)d->C; g.H = (int32_t)d->H; g.W = (int32_t)d->W; g.N = (int32_t)d->N;
    g.KH = (int32_t)d->KH; g.KW = (int32_t)d->KW; g.OH = (int32_t)OH; g.OW = (int32_t)OW;
    g.sh = (int32_t)d->stride_h; g.sw = (int32_t)d->stride_w; g.ph = (int32_t)d->pad_h; g.pw = (int32_t)d->pad_w;
    g.dh = (int32_t)d->dil_h; g.dw = (int32_t)d->dil_w;
    g.HW = g.H * g.W; g.OHW = g.OH * g.OW; g.KHW = g.KH * g.KW;
    g.CHW = (int64_t)g.C * g.HW;
    g.NOHW = (int64_t)g.N * g.OHW;
    const int64_t n = mxg_grid(M, d->N);
    if (n > 0x7fffffff) return DFQ_ERR_UNSUPPORTED;
    grid = n;
    return DFQ_OK;
}

}  // namespace dfq
