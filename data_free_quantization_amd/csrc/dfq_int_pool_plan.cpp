// Host-only part of dfq_int_mean_q and dfq_int_maxpool2d_q: the argument checks, the mean's regime
// and rows of a workgroup, the max pool's tiles and the grids (dfq_int_pool_plan.h).  Plain C++: no
// HIP header, no device code.
#include "dfq_int_pool_plan.h"

namespace dfq {
namespace {

uintptr_t addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }

// What the two descriptors share: the pointers, the flags and the two grids.
template <class Desc>
int pool_check_common(const Desc* d) {
    if (!d) return DFQ_ERR_INVALID;
    if (!d->x || !d->out) return DFQ_ERR_INVALID;
    if (d->flags != 0 || d->reserved != 0) return DFQ_ERR_INVALID;
    if (int rc = mb_check_quant(d->x_quant, false)) return rc;
    if (int rc = mb_check_quant(d->out_quant, true)) return rc;
    if (!mb_quant_aligned(d->x_quant) || !mb_quant_aligned(d->out_quant)) return DFQ_ERR_INVALID;
    return DFQ_OK;
}

}  // namespace

int mean_check(const dfq_int_mean_desc* d, MeanGeom& g, int64_t& grid) {
    g = MeanGeom{};
    grid = 0;
    if (int rc = pool_check_common(d)) return rc;
    if (d->rows < 1 || d->plane < 1 || d->rows > kMeanMaxN || d->plane > kMeanMaxN) return DFQ_ERR_INVALID;
    if (d->rows > kMeanMaxN / d->plane) return DFQ_ERR_INVALID;   // rows * plane <= 2^40, no overflow
    if (d->out_quant.bits == 0 && addr(d->out) % 4) return DFQ_ERR_INVALID;
    if (d->plane > kMeanMaxP) return DFQ_ERR_UNSUPPORTED;

    g.R = d->rows;
    g.P = d->plane;
    g.small = d->plane <= kMeanSmallP;
    int64_t rb = 1;
    if (g.small) {
        rb = kMeanSpanBytes / d->plane;
        if (rb > kMeanMaxRows) rb = kMeanMaxRows;
    }
    g.rb = (int32_t)rb;
    g.x16 = (int32_t)(addr(d->x) & 15u);
    g.out_codes = d->out_quant.bits > 0;
    const int64_t blocks = ceil_div(d->rows, rb);
    if (blocks > 0x7fffffff) return DFQ_ERR_UNSUPPORTED;
    grid = blocks;
    return DFQ_OK;
}

int maxpool_check(const dfq_int_maxpool2d_desc* d, DwcGeom& g, int64_t& grid) {
    g = DwcGeom{};
    grid = 0;
    if (int rc = pool_check_common(d)) return rc;
    constexpr int64_t kMax = int64_t(1) << 28, k31 = int64_t(1) << 31;
    const int64_t least_one[] = {d->B, d->C, d->H, d->W, d->KH, d->KW, d->stride_h, d->stride_w};
    for (int64_t v : least_one)
        if (v < 1 || v > kMax) return DFQ_ERR_INVALID;
    if (d->pad_h < 0 || d->pad_w < 0) return DFQ_ERR_INVALID;
    if (d->pad_h > d->KH / 2 || d->pad_w > d->KW / 2) return DFQ_ERR_INVALID;   // every window holds a tap of the image
    if (d->H * d->W >= k31) return DFQ_ERR_INVALID;
    const int64_t OH = mxc_out_extent(d->H, d->pad_h, 1, d->KH, d->stride_h);
    const int64_t OW = mxc_out_extent(d->W, d->pad_w, 1, d->KW, d->stride_w);
    if (OH < 1 || OW < 1) return DFQ_ERR_SHAPE;
    if (OH * OW >= k31) return DFQ_ERR_INVALID;
    if (d->KH * d->KW > kDwMaxTaps) return DFQ_ERR_UNSUPPORTED;
    const DwcWindow w{d->B, d->C, d->H, d->W, 1, d->KH, d->KW, d->stride_h, d->stride_w, d->pad_h, d->pad_w, 1, 1, OH, OW};
    return dwc_tiles(w, g, grid);
}

}  // namespace dfq
