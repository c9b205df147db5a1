// The index arithmetic of dfq_mx_conv2d (dfq_mx_gemm.hip's conv A and NCHW store): dfq_mx_linear
// on the im2col rows of an NCHW activation, gathered in the kernel.  Tiling, the B operand, the
// per-lane quantizer and the accumulators are dfq_mx_gemm_plan.h's and dfq_mx_linear_plan.h's,
// unchanged; this header adds which element of x stands at (m, k) of the im2col matrix and
// where output element (m, n) lies in NCHW:
//   m = (b * OH + oh) * OW + ow        k = (c * KH + i) * KW + j
//   A[m][k] = x[b][c][oh * sh - ph + i * dh][ow * sw - pw + j * dw], +0 outside the image
//   out[b][n][oh][ow] at b * N * OH * OW + n * OH * OW + (oh * OW + ow)
// The kernel and the host check (tests/native/mx_conv_plan_check.cpp) use these helpers and
// nothing else for an address, so what the check proves on the CPU -- every read inside x, the
// gathered element the im2col definition's, every output element stored once at its NCHW
// offset -- holds for the kernel.  No HIP header: the checks (dfq_mx_conv_plan.cpp) build as
// plain C++.
//
// A lane's row m is the same for the whole K loop: mxc_row decomposes it once.  A lane's run of
// consecutive k (32, FP8: 2 x 16) starts at mxl_part_k: mxc_tap decomposes that k once per K
// step and mxc_next walks j -> i -> c with carries, so the gather divides nothing per element.
// PW, a compile-time variant for pointwise layers (1 x 1 kernel, zero padding, dilation 1, any
// stride): k = c, the element lies at the row's base + c * H * W and is inside the image
// whenever the row exists.
#pragma once
#include "dfq_mx_linear_plan.h"

namespace dfq {

// The convolution's geometry as the kernel takes it (mxc_check derives it from the descriptor).
struct MxcGeom {
    int32_t C, H, W, N, KH, KW, OH, OW;
    int32_t sh, sw, ph, pw, dh, dw;
    int32_t HW, OHW;      // H * W, OH * OW: a channel's plane of x and of out
    int32_t KHW;          // KH * KW
    int32_t reserved;
    int64_t CHW, NOHW;    // an image of x and of out (each below 2^31)
};

// Output extent along one axis; < 1 when the dilated kernel does not fit the padded image.
DFQ_HOST_DEVICE inline int64_t mxc_out_extent(int64_t in, int64_t pad, int64_t dil, int64_t k, int64_t stride) {
    const int64_t span = in + 2 * pad - dil * (k - 1) - 1;
    return span < 0 ? 0 : span / stride + 1;
}
DFQ_HOST_DEVICE inline bool mxc_pointwise(const MxcGeom& g) {
    return g.KH == 1 && g.KW == 1 && g.ph == 0 && g.pw == 0 && g.dh == 1 && g.dw == 1;
}

// Row m of the im2col matrix: its image's first element of x, the input coordinates of tap
// (i, j) = (0, 0) (negative inside the padding) and those as an offset into a channel's plane.
// A row >= M reads nothing and stands for row 0, so that its arithmetic stays in range.
struct MxcRow {
    int64_t m;
    int64_t base;       // b * C * H * W + ih0 * W + iw0
    int32_t ih0, iw0;   // oh * sh - ph, ow * sw - pw
    bool on;            // m < M
};
DFQ_HOST_DEVICE inline MxcRow mxc_row(const MxcGeom& g, int64_t m, int64_t M) {
    MxcRow r;
    r.m = m;
    r.on = m < M;
    const uint32_t mm = r.on ? (uint32_t)m : 0u;   // M <= 2^31
    const uint32_t b = mm / (uint32_t)g.OHW, p = mm % (uint32_t)g.OHW;
    const int32_t oh = (int32_t)(p / (uint32_t)g.OW), ow = (int32_t)(p % (uint32_t)g.OW);
    r.ih0 = oh * g.sh - g.ph;
    r.iw0 = ow * g.sw - g.pw;
    r.base = (int64_t)b * g.CHW + (int64_t)r.ih0 * g.W + r.iw0;
    return r;
}

// Column k of the im2col matrix: tap (c, i, j), its displacement (i * dh, j * dw) from the
// row's (ih0, iw0) and that as an offset, (c * H + i * dh) * W + j * dw.  Columns >= K (the
// padding of the last block and K step) decompose like any other and are never read.
struct MxcTap {
    int32_t c, i, j;
    int32_t ih, iw;   // i * dh, j * dw
    int64_t off;
};
template <bool PW>
DFQ_HOST_DEVICE inline MxcTap mxc_tap(const MxcGeom& g, int64_t k) {
    MxcTap t;
    const uint32_t kk = (uint32_t)k;   // K < 2^31, and a K step ends less than 128 past it
    if (PW) {
        t.c = (int32_t)kk;
        t.i = t.j = t.ih = t.iw = 0;
        t.off = (int64_t)kk * g.HW;
    } else {
        const uint32_t c = kk / (uint32_t)g.KHW, r = kk % (uint32_t)g.KHW;
        t.c = (int32_t)c;
        t.i = (int32_t)(r / (uint32_t)g.KW);
        t.j = (int32_t)(r % (uint32_t)g.KW);
        t.ih = t.i * g.dh;
        t.iw = t.j * g.dw;
        t.off = ((int64_t)c * g.H + t.ih) * g.W + t.iw;
    }
    return t;
}
// The tap of k + 1 from the tap of k: j, then i, then c, each with its carry.
template <bool PW>
DFQ_HOST_DEVICE inline void mxc_next(const MxcGeom& g, MxcTap& t) {
    if (PW) {
        ++t.c;
        t.off += g.HW;
        return;
    }
    ++t.j;
    t.iw += g.dw;
    t.off += g.dw;
    if (t.j == g.KW) {
        t.off -= t.iw;
        t.j = 0;
        t.iw = 0;
        ++t.i;
        t.ih += g.dh;
        t.off += (int64_t)g.dh * g.W;
        if (t.i == g.KH) {
            t.off += (int64_t)g.HW - (int64_t)t.ih * g.W;
            t.i = 0;
            t.ih = 0;
            ++t.c;
        }
    }
}
// Element (m, k) is read iff the row and the column exist and the tap lies inside the image;
// everything else is +0.
template <bool PW>
DFQ_HOST_DEVICE inline bool mxc_reads(const MxcGeom& g, const MxcRow& r, const MxcTap& t, int64_t k, int64_t K) {
    if (!(r.on && k < K)) return false;
    if (PW) return true;
    return (uint32_t)(r.ih0 + t.ih) < (uint32_t)g.H && (uint32_t)(r.iw0 + t.iw) < (uint32_t)g.W;
}
DFQ_HOST_DEVICE inline int64_t mxc_x_offset(const MxcRow& r, const MxcTap& t) { return r.base + t.off; }

// Output element (m, n) in NCHW.
DFQ_HOST_DEVICE inline int64_t mxc_out_offset(const MxcGeom& g, int64_t m, int64_t n) {
    const uint32_t b = (uint32_t)m / (uint32_t)g.OHW, p = (uint32_t)m % (uint32_t)g.OHW;
    return (int64_t)b * g.NOHW + n * g.OHW + p;
}
// Rows m .. m + 3 of one column (a lane's four accumulator registers) are four consecutive
// floats of out iff all exist and lie in one image: one 16-B store at (m, n)'s offset.  Every
// other group is stored element by element.
DFQ_HOST_DEVICE inline bool mxc_out_quad(const MxcGeom& g, int64_t m, int64_t M) {
    return m + 3 < M && (uint32_t)m % (uint32_t)g.OHW + 3 < (uint32_t)g.OHW;
}

// The geometry checks of dfq_mx_conv2d and dfq_int_conv2d (no device call), whose descriptors
// name the geometry alike.  mxc_check_extents: every extent, stride, dilation and padding at
// least 1 (padding 0) and at most 2^28, so that H + 2 ph + dh (and W's) stays inside int32, and
// the offsets inside one image of x and the im2col column inside int32 (factor by factor: no
// product overflows).  mxc_check_geometry, after it: the output extents, M, K, the geometry as
// the kernel takes it and the grid.
template <class Desc>
inline int mxc_check_extents(const Desc& d) {
    constexpr int64_t kMax = int64_t(1) << 28;
    const int64_t least_one[] = {d.B, d.C, d.H, d.W, d.N, d.KH, d.KW, d.stride_h, d.stride_w, d.dil_h, d.dil_w};
    for (int64_t v : least_one)
        if (v < 1 || v > kMax) return DFQ_ERR_INVALID;
    const int64_t least_zero[] = {d.pad_h, d.pad_w};
    for (int64_t v : least_zero)
        if (v < 0 || v > kMax) return DFQ_ERR_INVALID;
    constexpr int64_t k31 = int64_t(1) << 31;
    if (d.H * d.W >= k31 || d.C * (d.H * d.W) >= k31) return DFQ_ERR_INVALID;
    if (d.KH * d.KW >= k31 || d.C * (d.KH * d.KW) >= k31) return DFQ_ERR_INVALID;
    return DFQ_OK;
}
template <class Desc>
inline int mxc_check_geometry(const Desc& d, MxcGeom& g, int64_t& M, int64_t& K, int64_t& grid) {
    constexpr int64_t k31 = int64_t(1) << 31;
    const int64_t OH = mxc_out_extent(d.H, d.pad_h, d.dil_h, d.KH, d.stride_h);
    const int64_t OW = mxc_out_extent(d.W, d.pad_w, d.dil_w, d.KW, d.stride_w);
    if (OH < 1 || OW < 1) return DFQ_ERR_SHAPE;
    if (OH * OW >= k31 || d.N * (OH * OW) >= k31) return DFQ_ERR_INVALID;   // offsets inside one image of out
    if (d.B * (OH * OW) > k31) return DFQ_ERR_INVALID;                      // M, as dfq_mx_gemm's
    K = d.C * d.KH * d.KW;
    M = d.B * OH * OW;
    if (d.N > (int64_t(1) << 50) / K) return DFQ_ERR_INVALID;               // B's code offsets
    g.C = (int32_t)d.C; g.H = (int32_t)d.H; g.W = (int32_t)d.W; g.N = (int32_t)d.N;
    g.KH = (int32_t)d.KH; g.KW = (int32_t)d.KW; g.OH = (int32_t)OH; g.OW = (int32_t)OW;
    g.sh = (int32_t)d.stride_h; g.sw = (int32_t)d.stride_w; g.ph = (int32_t)d.pad_h; g.pw = (int32_t)d.pad_w;
    g.dh = (int32_t)d.dil_h; g.dw = (int32_t)d.dil_w;
    g.HW = g.H * g.W; g.OHW = g.OH * g.OW; g.KHW = g.KH * g.KW;
    g.CHW = (int64_t)g.C * g.HW;
    g.NOHW = (int64_t)g.N * g.OHW;
    const int64_t n = mxg_grid(M, d.N);
    if (n > 0x7fffffff) return DFQ_ERR_UNSUPPORTED;
    grid = n;
    return DFQ_OK;
}

// dfq_mx_conv2d's argument checks (no device call): DFQ_OK with the geometry, M, K and the
// grid, or the error.
int mxc_check(const dfq_mx_conv2d_desc* d, MxcGeom& g, int64_t& M, int64_t& K, int64_t& grid);

}  // namespace dfq
