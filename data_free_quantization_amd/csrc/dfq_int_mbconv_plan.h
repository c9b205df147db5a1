// The index arithmetic of dfq_int_mbconv_q (dfq_int_mbconv.hip): the integer inverted-residual
// block -- expand 1x1, depthwise 3x3, project 1x1 on stored codes -- in one launch with the two
// hidden tensors in LDS.
//
// A workgroup (kThreads lanes, four waves) owns one image b, one tile of th x tw outputs (at most
// 8 x 8, 4 x 8 at stride 2; a ragged plane is split evenly) and all Cout channels:
//   block = (b * tiles_h + tile_h) * tiles_w + tile_w
// The tile's input footprint is fh x fw pixels (fh = (th - 1) s + 3; fw alike) from (ih0, iw0) =
// (oh0 s - p, ow0 s - p); footprint row fr = r * fw + c, fr < FR = fh * fw, padded to frp = 16 frt
// rows of the matrix instruction.  A tile pixel is tp = r * 8 + c < tpn (64, or 32 at stride 2).
// LDS, all offsets multiples of 16:
//   xs    [frp][xp]      x's codes in the signed domain, k contiguous, xp = Cin rounded up to 64,
//                        plus 16; 0 where the pixel lies outside the image, fr >= FR or k >= Cin
//   xsum  [frp] int32    sum_k of a row of xs (the expand's sum of a')
//   hid   [64][pp]       the chunk's expand output: the code byte of footprint row fr of chunk
//                        channel nl at nl * pp + fr (pp = frp), raw 0 outside the image
//   wts   [64][3]        the chunk's depthwise weights as operand words (dwc_operand_word)
//   pa    [tpn][kMbPaPitch]  the chunk's depthwise output in the signed domain: the project's A
//                        operand, k = chunk channel; 0 at a channel >= Ch
// A chunk is 64 consecutive hidden channels; chunks = ceil(Ch / 64).
// The expand gives wave w the chunk's columns 16 w .. 16 w + 15 for every row tile; the project
// gives wave w the column tiles w, w + 4, ... of Cout for every row tile of the pixels.
// The kernel and the host check (tests/native/int_mbconv_plan_check.cpp) use these helpers and
// nothing else for an address or a predicate.  No HIP header: the checks (dfq_int_mbconv_plan.cpp)
// build as plain C++.
#pragma once
#include "dfq_int_io_plan.h"

namespace dfq {

constexpr int kMbChunk = 64;                          // hidden channels of a chunk
constexpr int kMbTile = 8;                            // the tile's largest side, and tp's row pitch
constexpr int kMbMaxKSteps = DFQ_INT_MB_MAX_CIN / kIgStepK;   // the expand's K steps, B fragments in registers
constexpr int kMbMaxRowTiles = 16;                    // frt: a lane's inside-the-image bits are one 64-bit word
constexpr int kMbPaPitch = kMbChunk + 16;             // bytes of a pa row
constexpr int kMbLdsBytes = DFQ_INT_MB_LDS_BYTES;
constexpr int kMbWaves = 4;

struct MbGeom {
    int32_t Cin, H, W, Ch, Cout, OH, OW;
    int32_t HW, OHW;
    int32_t s, p;
    int32_t cinp, ksteps;         // Cin rounded up to 64; cinp / 64
    int32_t chunks;               // ceil(Ch / 64)
    int32_t nt;                   // the project's column tiles, ceil(Cout / 16)
    int32_t th, tw, tpn, tp_shift, rt;   // the tile; its pixel slots (64 / 32), log2, and row tiles tpn / 16
    int32_t fh, fw, fr, frp, frt; // the footprint; its rows, padded rows and row tiles
    int32_t tiles_h, tiles_w;
    int32_t e_wide, p_wide;       // the expand's / project's weight rows on the 16-B path (ig_wide)
    int32_t xp, pp;               // pitches of xs and hid
    int32_t xsum_off, hid_off, wts_off, pa_off, lds_bytes;
    DwcGeom dw;                   // the depthwise window for dwc_tap_mask / dwc_taps (C = Ch, K = 9)
};

struct MbBlock {
    int32_t b, oh0, ow0, ih0, iw0;
};
DFQ_HOST_DEVICE inline MbBlock mb_block(const MbGeom& g, uint32_t block) {
    MbBlock k;
    const uint32_t tw_i = block % (uint32_t)g.tiles_w, rest = block / (uint32_t)g.tiles_w;
    k.b = (int32_t)(rest / (uint32_t)g.tiles_h);
    k.oh0 = (int32_t)(rest % (uint32_t)g.tiles_h) * g.th;
    k.ow0 = (int32_t)tw_i * g.tw;
    k.ih0 = k.oh0 * g.s - g.p;
    k.iw0 = k.ow0 * g.s - g.p;
    return k;
}

// Footprint row fr: its pixel of the image, and whether it exists there.
struct MbPixel {
    int32_t ih, iw;
    bool inside;
};
DFQ_HOST_DEVICE inline MbPixel mb_pixel(const MbGeom& g, const MbBlock& k, int32_t fr) {
    MbPixel q;
    const uint32_t r = (uint32_t)fr / (uint32_t)g.fw, c = (uint32_t)fr % (uint32_t)g.fw;
    q.ih = k.ih0 + (int32_t)r;
    q.iw = k.iw0 + (int32_t)c;
    q.inside = fr < g.fr && (uint32_t)q.ih < (uint32_t)g.H && (uint32_t)q.iw < (uint32_t)g.W;
    return q;
}
DFQ_HOST_DEVICE inline int64_t mb_x_offset(const MbGeom& g, int32_t b, int32_t k, int32_t ih, int32_t iw) {
    return ((int64_t)b * g.Cin + k) * g.HW + (int64_t)ih * g.W + iw;
}

// ---- staging: a cell is four consecutive k of one footprint row, one LDS word ----
DFQ_HOST_DEVICE inline int32_t mb_cells(const MbGeom& g) { return (g.cinp >> 2) * g.frp; }
DFQ_HOST_DEVICE inline int32_t mb_cell_k(const MbGeom& g, int32_t cell) { return (int32_t)((uint32_t)cell / (uint32_t)g.frp) * 4; }
DFQ_HOST_DEVICE inline int32_t mb_cell_fr(const MbGeom& g, int32_t cell) { return (int32_t)((uint32_t)cell % (uint32_t)g.frp); }

// ---- LDS bytes ----
DFQ_HOST_DEVICE inline int32_t mb_xs_byte(const MbGeom& g, int32_t fr, int32_t k) { return fr * g.xp + k; }
DFQ_HOST_DEVICE inline int32_t mb_xsum_byte(const MbGeom& g, int32_t fr) { return g.xsum_off + 4 * fr; }
DFQ_HOST_DEVICE inline int32_t mb_hid_byte(const MbGeom& g, int32_t nl, int32_t fr) { return g.hid_off + nl * g.pp + fr; }
DFQ_HOST_DEVICE inline int32_t mb_wts_byte(const MbGeom& g, int32_t nl, int32_t w) { return g.wts_off + 4 * (nl * 3 + w); }
DFQ_HOST_DEVICE inline int32_t mb_pa_byte(const MbGeom& g, int32_t tp, int32_t k) { return g.pa_off + tp * kMbPaPitch + k; }
// A lane's 16 bytes of an A fragment: row (lane & 15) of row tile i, k from ig_lane_k0.
DFQ_HOST_DEVICE inline int32_t mb_xs_frag(const MbGeom& g, int32_t i, int32_t step, int lane) {
    return mb_xs_byte(g, i * 16 + (lane & 15), (int32_t)ig_lane_k0(step, lane));
}
DFQ_HOST_DEVICE inline int32_t mb_pa_frag(const MbGeom& g, int32_t i, int lane) {
    return mb_pa_byte(g, i * 16 + (lane & 15), (int32_t)ig_lane_k0(0, lane));
}
// The first of a lane's four accumulator rows of row tile i (the instruction's C layout).
DFQ_HOST_DEVICE inline int32_t mb_acc_row(int32_t i, int lane) { return i * 16 + 4 * (lane >> 4); }

// ---- the depthwise: a unit is one tile pixel and four consecutive chunk channels ----
DFQ_HOST_DEVICE inline int32_t mb_units(const MbGeom& g) { return g.tpn * (kMbChunk / 4); }
struct MbUnit {
    int32_t tp, cq;           // pixel slot, channel quad
    int32_t oh, ow;
    bool on;                  // the pixel is an output of this tile
    int32_t at;               // the footprint row of its tap (0, 0); 0 when off
};
DFQ_HOST_DEVICE inline bool mb_tp_on(const MbGeom& g, const MbBlock& k, int32_t tp) {
    const int32_t r = tp >> 3, c = tp & 7;
    return r < g.th && c < g.tw && k.oh0 + r < g.OH && k.ow0 + c < g.OW;
}
DFQ_HOST_DEVICE inline MbUnit mb_unit(const MbGeom& g, const MbBlock& k, int32_t u) {
    MbUnit q;
    q.tp = u & (g.tpn - 1);
    q.cq = u >> g.tp_shift;
    const int32_t r = q.tp >> 3, c = q.tp & 7;
    q.oh = k.oh0 + r;
    q.ow = k.ow0 + c;
    q.on = mb_tp_on(g, k, q.tp);
    q.at = q.on ? r * g.s * g.fw + c * g.s : 0;
    return q;
}
// Tap k = 3 i + j of a unit, as a displacement in footprint rows.
DFQ_HOST_DEVICE inline int32_t mb_tap(const MbGeom& g, int k) { return (k / 3) * g.fw + k % 3; }

DFQ_HOST_DEVICE inline int64_t mb_out_offset(const MbGeom& g, int32_t b, int64_t n, int32_t oh, int32_t ow) {
    return ((int64_t)b * g.Cout + n) * g.OHW + (int64_t)oh * g.OW + ow;
}

// ---- the residual (dfq_int_mbconv_res_q): stride 1, pad 1, Cin == Cout ----
// The footprint row that holds x at tile pixel tp: the footprint starts one pixel above and left
// of the tile.  Row 0 for a pixel that is off (its value is never stored).
DFQ_HOST_DEVICE inline int32_t mb_res_fr(const MbGeom& g, int32_t tp, bool on) {
    return on ? ((tp >> 3) + 1) * g.fw + (tp & 7) + 1 : 0;
}

// A grid's checks (dfq_int_mbconv_quant): its fields, then its range pointers' alignment.
inline int mb_check_quant(const dfq_int_mbconv_quant& q, bool optional) {
    if (q.reserved != 0 || (q.flags & ~DFQ_SCALE_F32) != 0) return DFQ_ERR_INVALID;
    if (q.symmetric != 0 && q.symmetric != 1) return DFQ_ERR_INVALID;
    if (optional && q.bits == 0) return DFQ_OK;
    if (q.bits < 2 || q.bits > 8) return DFQ_ERR_INVALID;
    if (!q.min_dev && !q.max_dev && !(q.given_max > q.given_min)) return DFQ_ERR_INVALID;
    return DFQ_OK;
}
inline bool mb_quant_aligned(const dfq_int_mbconv_quant& q) {
    return reinterpret_cast<uintptr_t>(q.min_dev) % 4 == 0 && reinterpret_cast<uintptr_t>(q.max_dev) % 4 == 0;
}

// dfq_int_mbconv_q's argument checks (no device call): DFQ_OK with the geometry and the grid, or
// the error.
int mb_check(const dfq_int_mbconv_desc* d, MbGeom& g, int64_t& grid);
// dfq_int_mbconv_res_q's: mb_check, then the residual struct's and the shapes the add needs.
int mb_res_check(const dfq_int_mbconv_desc* d, const dfq_int_mbconv_res* r, MbGeom& g, int64_t& grid);

}  // namespace dfq
