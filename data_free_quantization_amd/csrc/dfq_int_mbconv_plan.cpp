// Host-only part of dfq_int_mbconv_q: the argument checks, the tile, the LDS map and the grid
// (dfq_int_mbconv_plan.h).  Plain C++: no HIP header, no device code.
#include "dfq_int_mbconv_plan.h"

namespace dfq {
namespace {

uintptr_t addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }

int mb_check_layer(const dfq_int_mbconv_layer& l) {
    if (!l.b_codes || !l.b_scale) return DFQ_ERR_INVALID;
    if ((l.flags & ~(DFQ_INT_B_PACK4 | DFQ_INT_B_PER_ROW)) != 0) return DFQ_ERR_INVALID;
    if (l.b_signed != 0 && l.b_signed != 1) return DFQ_ERR_INVALID;
    return DFQ_OK;
}
}  // namespace

int mb_res_check(const dfq_int_mbconv_desc* d, const dfq_int_mbconv_res* r, MbGeom& g, int64_t& grid) {
    if (int rc = mb_check(d, g, grid)) return rc;
    if (!r || r->flags != 0 || r->reserved != 0) return DFQ_ERR_INVALID;
    if (int rc = mb_check_quant(r->proj_quant, false)) return rc;
    if (!mb_quant_aligned(r->proj_quant)) return DFQ_ERR_INVALID;
    if (d->stride != 1 || d->pad != 1 || d->Cin != d->Cout) return DFQ_ERR_SHAPE;   // x and out: one shape
    return DFQ_OK;
}

int mb_check(const dfq_int_mbconv_desc* d, MbGeom& g, int64_t& grid) {
    g = MbGeom{};
    grid = 0;
    if (!d) return DFQ_ERR_INVALID;
    if (!d->x || !d->out) return DFQ_ERR_INVALID;
    const dfq_int_mbconv_layer* layers[] = {&d->expand, &d->depthwise, &d->project};
    const dfq_int_mbconv_quant* quants[] = {&d->x_quant, &d->hidden1, &d->hidden2, &d->out_quant};
    if (d->flags != 0 || d->reserved != 0) return DFQ_ERR_INVALID;
    for (const auto* l : layers)
        if (int rc = mb_check_layer(*l)) return rc;
    for (int i = 0; i < 4; ++i)
        if (int rc = mb_check_quant(*quants[i], i == 3)) return rc;
    constexpr int64_t kMax = int64_t(1) << 28, k31 = int64_t(1) << 31;
    const int64_t least_one[] = {d->B, d->Cin, d->H, d->W, d->Ch, d->Cout, d->stride};
    for (int64_t v : least_one)
        if (v < 1 || v > kMax) return DFQ_ERR_INVALID;
    if (d->pad < 0 || d->pad > kMax) return DFQ_ERR_INVALID;
    if (d->H * d->W >= k31 || d->Cin * (d->H * d->W) >= k31) return DFQ_ERR_INVALID;
    if (d->out_quant.bits == 0 && addr(d->out) % 4) return DFQ_ERR_INVALID;
    for (const auto* l : layers)
        if (addr(l->b_codes) % 16 || addr(l->b_scale) % 4 || addr(l->b_zero) % 4 || addr(l->bias) % 4) return DFQ_ERR_INVALID;
    for (const auto* q : quants)
        if (addr(q->min_dev) % 4 || addr(q->max_dev) % 4) return DFQ_ERR_INVALID;
    const int64_t OH = mxc_out_extent(d->H, d->pad, 1, 3, d->stride), OW = mxc_out_extent(d->W, d->pad, 1, 3, d->stride);
    if (OH < 1 || OW < 1) return DFQ_ERR_SHAPE;
    if (OH * OW >= k31 || d->Cout * (OH * OW) >= k31) return DFQ_ERR_INVALID;   // offsets inside one image of out
    if (d->B * (OH * OW) > k31) return DFQ_ERR_INVALID;
    if (d->stride > 2 || d->pad > 1) return DFQ_ERR_UNSUPPORTED;
    for (const auto* l : layers)
        if (l->flags & DFQ_INT_B_PACK4) return DFQ_ERR_UNSUPPORTED;
    if (d->Cin > DFQ_INT_MB_MAX_CIN || d->Cout > DFQ_INT_MB_MAX_COUT || d->Ch > kIgMaxK) return DFQ_ERR_UNSUPPORTED;

    // the tile: a plane's rows and columns split evenly over the fewest tiles
    const int64_t s = d->stride, max_h = s == 1 ? kMbTile : kMbTile / 2;
    const int64_t th = ceil_div(OH, ceil_div(OH, max_h)), tw = ceil_div(OW, ceil_div(OW, (int64_t)kMbTile));
    const int64_t fh = (th - 1) * s + 3, fw = (tw - 1) * s + 3, fr = fh * fw, frt = ceil_div(fr, (int64_t)16);
    if (frt > kMbMaxRowTiles) return DFQ_ERR_UNSUPPORTED;   // not reached by the tiles above
    const int64_t cinp = ceil_div(d->Cin, (int64_t)kIgStepK) * kIgStepK, frp = frt * 16;
    const int64_t tpn = max_h * kMbTile;
    const int64_t tiles_h = ceil_div(OH, th), tiles_w = ceil_div(OW, tw);
    const int64_t n = d->B * tiles_h * tiles_w;
    if (n > 0x7fffffff) return DFQ_ERR_UNSUPPORTED;

    g.Cin = (int32_t)d->Cin; g.H = (int32_t)d->H; g.W = (int32_t)d->W; g.Ch = (int32_t)d->Ch; g.Cout = (int32_t)d->Cout;
    g.OH = (int32_t)OH; g.OW = (int32_t)OW; g.HW = g.H * g.W; g.OHW = g.OH * g.OW;
    g.s = (int32_t)s; g.p = (int32_t)d->pad;
    g.cinp = (int32_t)cinp; g.ksteps = (int32_t)(cinp / kIgStepK);
    g.chunks = (int32_t)ceil_div(d->Ch, (int64_t)kMbChunk);
    g.nt = (int32_t)ceil_div(d->Cout, (int64_t)16);
    g.th = (int32_t)th; g.tw = (int32_t)tw; g.tpn = (int32_t)tpn; g.tp_shift = tpn == 64 ? 6 : 5; g.rt = (int32_t)(tpn / 16);
    g.fh = (int32_t)fh; g.fw = (int32_t)fw; g.fr = (int32_t)fr; g.frp = (int32_t)frp; g.frt = (int32_t)frt;
    g.tiles_h = (int32_t)tiles_h; g.tiles_w = (int32_t)tiles_w;
    g.e_wide = ig_wide(d->Cin); g.p_wide = ig_wide(d->Ch);
    g.xp = g.cinp + 16; g.pp = g.frp;
    g.xsum_off = g.frp * g.xp;
    g.hid_off = g.xsum_off + 4 * g.frp;
    g.wts_off = g.hid_off + kMbChunk * g.pp;
    g.pa_off = g.wts_off + kMbChunk * 3 * 4;
    g.lds_bytes = g.pa_off + g.tpn * kMbPaPitch;
    if (g.lds_bytes > kMbLdsBytes) return DFQ_ERR_UNSUPPORTED;
    DwcGeom& w = g.dw;
    w.C = g.Ch; w.H = g.H; w.W = g.W; w.mult = 1; w.KH = w.KW = 3; w.OH = g.OH; w.OW = g.OW;
    w.sh = w.sw = g.s; w.ph = w.pw = g.p; w.dh = w.dw = 1;
    w.HW = g.HW; w.OHW = g.OHW; w.K = 9; w.words = 3;
    w.masked = g.p != 0;
    grid = n;
    return DFQ_OK;
}

}  // namespace dfq
