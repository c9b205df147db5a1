// Host-only part of dfq_int_dwconv2d: the argument checks, the tile decomposition and the grid
// (dfq_int_dwconv_plan.h).  Plain C++: no HIP header, no device code.
#include "dfq_int_dwconv_plan.h"

namespace dfq {

int dwc_check(const dfq_int_dwconv2d_desc* d, DwcGeom& g, int64_t& grid) {
    const auto addr = [](const void* p) { return reinterpret_cast<uintptr_t>(p); };
    g = DwcGeom{};
    grid = 0;
    if (!d) return DFQ_ERR_INVALID;
    if (!d->x || !d->b_codes || !d->b_scale || !d->out) return DFQ_ERR_INVALID;
    // dfq_int_conv2d's checks of the quantizer and of B
    if ((d->flags & ~(DFQ_INT_B_PACK4 | DFQ_INT_B_PER_ROW | DFQ_SCALE_F32)) != 0 || d->reserved != 0 || d->reserved2 != 0)
        return DFQ_ERR_INVALID;
    if (d->b_signed != 0 && d->b_signed != 1) return DFQ_ERR_INVALID;
    if (d->x_symmetric != 0 && d->x_symmetric != 1) return DFQ_ERR_INVALID;
    if (d->x_bits < 2 || d->x_bits > 8) return DFQ_ERR_INVALID;
    // its extents, with N = C * mult
    constexpr int64_t kMax = int64_t(1) << 28, k31 = int64_t(1) << 31;
    const int64_t least_one[] = {d->B, d->C, d->H, d->W, d->mult, d->KH, d->KW, d->stride_h, d->stride_w, d->dil_h, d->dil_w};
    for (int64_t v : least_one)
        if (v < 1 || v > kMax) return DFQ_ERR_INVALID;
    if (d->pad_h < 0 || d->pad_h > kMax || d->pad_w < 0 || d->pad_w > kMax) return DFQ_ERR_INVALID;
    const int64_t N = d->C * d->mult;
    if (N > kMax) return DFQ_ERR_INVALID;
    if (d->H * d->W >= k31 || d->C * (d->H * d->W) >= k31) return DFQ_ERR_INVALID;
    if (addr(d->x) % 4 || addr(d->out) % 4 || addr(d->bias) % 4 || addr(d->min_dev) % 4 || addr(d->max_dev) % 4) return DFQ_ERR_INVALID;
    if (addr(d->b_codes) % 16 || addr(d->b_scale) % 4 || addr(d->b_zero) % 4) return DFQ_ERR_INVALID;
    const int64_t OH = mxc_out_extent(d->H, d->pad_h, d->dil_h, d->KH, d->stride_h);
    const int64_t OW = mxc_out_extent(d->W, d->pad_w, d->dil_w, d->KW, d->stride_w);
    if (OH < 1 || OW < 1) return DFQ_ERR_SHAPE;
    if (OH * OW >= k31 || N * (OH * OW) >= k31) return DFQ_ERR_INVALID;   // offsets inside one image of out
    if (d->B * (OH * OW) > k31) return DFQ_ERR_INVALID;
    const int64_t K = d->KH * d->KW;
    if (K > kDwMaxTaps) return DFQ_ERR_UNSUPPORTED;
    if ((d->flags & DFQ_INT_B_PACK4) && K % 2) return DFQ_ERR_UNSUPPORTED;

    // the tile: a plane's rows and columns split evenly over the fewest tiles of at most kDwTileH x
    // kDwTileW (whole quads a tile where a row has several), shrunk until one plane's footprint fits the code bytes
    int64_t th = ceil_div(OH, ceil_div(OH, (int64_t)kDwTileH)), tw = ceil_div(OW, ceil_div(OW, (int64_t)kDwTileW));
    if (tw < OW) tw = ceil_div(tw, (int64_t)kDwQuad) * kDwQuad;
    int64_t fh, fw, fwp;
    for (;;) {
        fh = (th - 1) * d->stride_h + (d->KH - 1) * d->dil_h + 1;
        fw = (tw - 1) * d->stride_w + (d->KW - 1) * d->dil_w + 1;
        fwp = (fw + 3) / 4 * 4;
        if (fh <= kDwCodeBytes && fwp <= kDwCodeBytes && fh * fwp <= kDwCodeBytes) break;   // factor by factor: no overflow
        if (th == 1 && tw == 1) return DFQ_ERR_UNSUPPORTED;   // one output's footprint does not fit
        if (tw == 1 || (th > 1 && fh >= fwp)) th = (th + 1) / 2;
        else tw = (tw + 1) / 2;
    }
    const int64_t tiles_h = ceil_div(OH, th), tiles_w = ceil_div(OW, tw), tqw = ceil_div(tw, (int64_t)kDwQuad);
    const int64_t planes = d->B * d->C, words = ceil_div(K, (int64_t)4);
    // planes of a workgroup: where a plane is one tile, as many as fill two quads a lane
    int64_t pp = 1;
    if (tiles_h * tiles_w == 1) {
        pp = kDwTargetQuads / (th * tqw);
        if (pp > kDwMaxPlanes) pp = kDwMaxPlanes;
        if (pp > kDwCodeBytes / (fh * fwp)) pp = kDwCodeBytes / (fh * fwp);
        if (pp > planes) pp = planes;
        if (pp < 1) pp = 1;
    }
    int64_t mc = kDwWeightWords / (pp * words);
    if (mc > d->mult) mc = d->mult;
    const int64_t n = ceil_div(planes, pp) * tiles_h * tiles_w;
    if (n > 0x7fffffff) return DFQ_ERR_UNSUPPORTED;

    g.C = (int32_t)d->C; g.H = (int32_t)d->H; g.W = (int32_t)d->W; g.mult = (int32_t)d->mult;
    g.KH = (int32_t)d->KH; g.KW = (int32_t)d->KW; g.OH = (int32_t)OH; g.OW = (int32_t)OW;
    g.sh = (int32_t)d->stride_h; g.sw = (int32_t)d->stride_w; g.ph = (int32_t)d->pad_h; g.pw = (int32_t)d->pad_w;
    g.dh = (int32_t)d->dil_h; g.dw = (int32_t)d->dil_w;
    g.HW = g.H * g.W; g.OHW = g.OH * g.OW;
    g.K = (int32_t)K; g.words = (int32_t)words;
    g.th = (int32_t)th; g.tw = (int32_t)tw; g.tqw = (int32_t)tqw;
    g.fh = (int32_t)fh; g.fw = (int32_t)fw; g.fwp = (int32_t)fwp;
    g.fwords = (int32_t)(fh * fwp / 4);
    g.pp = (int32_t)pp; g.mc = (int32_t)mc;
    g.tiles_h = (int32_t)tiles_h; g.tiles_w = (int32_t)tiles_w;
    g.masked = (d->pad_h | d->pad_w) != 0;
    g.planes = planes;
    grid = n;
    return DFQ_OK;
}

}  // namespace dfq
