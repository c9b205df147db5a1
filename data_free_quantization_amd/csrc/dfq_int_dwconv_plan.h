// The index arithmetic of dfq_int_dwconv2d (dfq_int_dwconv.hip): the depthwise convolution of
// the affine values the codes stand for, on the packed 8-bit dot instruction.
//
// A plane is one (b, c) image of x, p = b * C + c; its mult output channels are planes
// p * mult + m of out.  A workgroup (a block of kThreads) owns one tile of th x tw outputs of
// pp consecutive planes (pp > 1 only where a plane is one tile) for all mult channels:
//   block = (group * tiles_h + tile_h) * tiles_w + tile_w,   planes group * pp .. + pp - 1
// Phase 1 -- the footprint.  A tile reads rows ih0 .. ih0 + fh - 1 and columns iw0 .. iw0 + fw - 1
// of each of its planes (ih0 = oh0 * sh - ph, fh = (th - 1) sh + (KH - 1) dh + 1; W alike), halo
// included.  The code bytes lie in LDS at  pl * 4 fwords + r * fwp + col,  fwp = fw rounded up to
// 4: one lane quantizes the four consecutive columns of one 32-bit word (cell wq = (pl, r, col))
// and stores the word, byte t = 0 where column col + t lies outside the image, past fw or in a
// plane past the last.  Every word of the pp * fwords is written once, by lane wq % kThreads of
// round wq / kThreads.
// Phase 2 -- the outputs.  A lane takes quads: four consecutive outputs (r, c0 .. c0 + 3) of
// plane pl, q = (pl * th + r) * tqw + c0 / 4.  Tap k = i * KW + j of output (r, c) is the byte at
// dwc_lds_byte(pl, r * sh + i * dh, c * sw + j * dw); word w of an output's operand holds taps
// 4 w .. 4 w + 3, one per byte.  The tap mask (bit k: the tap lies inside the image) is the
// product of a row and a column bit set; T is igc_axis_taps' closed form, and the host check
// proves it is the mask's population count.  The weights of the tile's planes -- mc output
// channels at a time -- lie in LDS as operand words, in the signed domain, 0 at k >= K.
// The instruction multiplies signed bytes: an unsigned code enters as q - 128 (xor 0x80) on the
// taps whose mask bit is set, every other byte as 0, and ig_fold_p / ig_fold_s give the
// contract's P, Sa and Sb back with T where dfq_int_gemm has K.
// The kernel and the host check (tests/native/int_dwconv_plan_check.cpp) use these helpers and
// nothing else for an address, a mask bit, a fold or the dot product's lane arithmetic.  No HIP
// header: the checks (dfq_int_dwconv_plan.cpp) build as plain C++.
#pragma once
#include "dfq_int_conv_plan.h"

namespace dfq {

constexpr int kDwTileH = DFQ_INT_DW_TILE_H, kDwTileW = DFQ_INT_DW_TILE_W;
constexpr int kDwQuad = 4;                            // outputs of a lane along OW
constexpr int kDwMaxTaps = DFQ_INT_DW_MAX_TAPS;       // a tap mask is one 64-bit word
constexpr int kDwMaxWords = kDwMaxTaps / 4;
constexpr int kDwCodeBytes = DFQ_INT_DW_LDS_BYTES;    // LDS: the footprints' code bytes
constexpr int kDwWeightWords = 2048;                  // LDS: the weights' operand words
constexpr int kDwMaxPlanes = 64;                      // planes of a workgroup
constexpr int kDwTargetQuads = 2 * 256;               // quads of a workgroup: two per lane
static_assert(kDwMaxPlanes * kDwMaxWords <= kDwWeightWords, "one output channel of every plane fits");

struct DwcGeom {
    int32_t C, H, W, mult, KH, KW, OH, OW;
    int32_t sh, sw, ph, pw, dh, dw;
    int32_t HW, OHW;          // a plane of x and of out
    int32_t K, words;         // KH * KW; operand words of an output, ceil(K / 4)
    int32_t th, tw, tqw;      // the tile's outputs; quads per tile row, ceil(tw / 4)
    int32_t fh, fw, fwp;      // the footprint's rows, columns and LDS pitch
    int32_t fwords;           // LDS words of one plane's footprint, fh * fwp / 4
    int32_t pp, mc;           // planes of a workgroup; output channels per weight round
    int32_t tiles_h, tiles_w;
    int32_t masked;           // some tap of the geometry can fall in padding
    int64_t planes;           // B * C
};

// ---- the block ----
struct DwcBlock {
    int64_t p0;               // first plane
    int32_t oh0, ow0;         // the tile's first output
    int32_t ih0, iw0;         // the footprint's first input row and column (negative inside the padding)
};
DFQ_HOST_DEVICE inline DwcBlock dwc_block(const DwcGeom& g, uint32_t block) {
    DwcBlock b;
    const uint32_t tw_i = block % (uint32_t)g.tiles_w, rest = block / (uint32_t)g.tiles_w;
    const uint32_t th_i = rest % (uint32_t)g.tiles_h, group = rest / (uint32_t)g.tiles_h;
    b.p0 = (int64_t)group * g.pp;
    b.oh0 = (int32_t)th_i * g.th;
    b.ow0 = (int32_t)tw_i * g.tw;
    b.ih0 = b.oh0 * g.sh - g.ph;
    b.iw0 = b.ow0 * g.sw - g.pw;
    return b;
}

// ---- phase 1: the footprint ----
DFQ_HOST_DEVICE inline int32_t dwc_cells(const DwcGeom& g) { return g.pp * g.fwords; }
struct DwcCell {
    int32_t pl, r, col;       // plane of the block, footprint row, first of the word's four columns
};
DFQ_HOST_DEVICE inline DwcCell dwc_cell(const DwcGeom& g, int32_t wq) {
    DwcCell c;
    const uint32_t row_words = (uint32_t)g.fwp >> 2;
    const uint32_t pl = (uint32_t)wq / (uint32_t)g.fwords, rem = (uint32_t)wq % (uint32_t)g.fwords;
    c.pl = (int32_t)pl;
    c.r = (int32_t)(rem / row_words);
    c.col = (int32_t)(rem % row_words) * 4;
    return c;
}
DFQ_HOST_DEVICE inline int32_t dwc_lds_byte(const DwcGeom& g, int32_t pl, int32_t r, int32_t col) {
    return pl * g.fwords * 4 + r * g.fwp + col;
}
// Footprint element (row r, column col) of plane p is read iff the plane exists, the column is the
// footprint's and the element lies inside the image; every other byte of the word is 0.
DFQ_HOST_DEVICE inline bool dwc_x_reads(const DwcGeom& g, const DwcBlock& b, int64_t p, int32_t r, int32_t col) {
    return p < g.planes && col < g.fw && (uint32_t)(b.ih0 + r) < (uint32_t)g.H && (uint32_t)(b.iw0 + col) < (uint32_t)g.W;
}
DFQ_HOST_DEVICE inline int64_t dwc_x_offset(const DwcGeom& g, const DwcBlock& b, int64_t p, int32_t r, int32_t col) {
    return p * g.HW + (int64_t)(b.ih0 + r) * g.W + (b.iw0 + col);
}

// ---- the weights ----
// The code of element k of row n as a byte: the stored byte, or its nibble widened (sign-extended
// when b_signed; K even, so a row starts on a byte and element k sits in nibble k & 1).
DFQ_HOST_DEVICE inline uint32_t dwc_b_code(const uint8_t* codes, int64_t n, int32_t k, int32_t K, bool packed, bool b_signed) {
    if (!packed) return codes[ig_byte_offset(n, k, K)];
    const uint32_t byte = codes[ig_packed_offset(n, k, K)];
    const uint32_t nib = (k & 1) ? byte >> 4 : byte & 0xFu;
    return b_signed && (nib & 8u) ? nib | 0xF0u : nib;
}
// Where word w of output channel m (of the round) of plane pl lies in the weights' LDS.
DFQ_HOST_DEVICE inline int32_t dwc_w_index(const DwcGeom& g, int32_t pl, int32_t m, int32_t w) {
    return (pl * g.mc + m) * g.words + w;
}
// The mask of the K real taps (no padding anywhere, and what a weight word keeps).
DFQ_HOST_DEVICE inline uint64_t dwc_full_mask(int32_t K) { return K >= 64 ? ~uint64_t(0) : (uint64_t(1) << K) - 1; }

// ---- phase 2: the outputs ----
DFQ_HOST_DEVICE inline int32_t dwc_quads(const DwcGeom& g) { return g.pp * g.th * g.tqw; }
struct DwcQuad {
    int32_t pl, r, c0;        // plane of the block, tile row, first tile column
};
DFQ_HOST_DEVICE inline DwcQuad dwc_quad(const DwcGeom& g, int32_t q) {
    DwcQuad d;
    const uint32_t per_plane = (uint32_t)(g.th * g.tqw);
    const uint32_t pl = (uint32_t)q / per_plane, rem = (uint32_t)q % per_plane;
    d.pl = (int32_t)pl;
    d.r = (int32_t)(rem / (uint32_t)g.tqw);
    d.c0 = (int32_t)(rem % (uint32_t)g.tqw) * kDwQuad;
    return d;
}
// Output e of the quad exists: inside the tile and inside the image.
DFQ_HOST_DEVICE inline bool dwc_out_on(const DwcGeom& g, const DwcBlock& b, const DwcQuad& d, int e) {
    return d.c0 + e < g.tw && b.ow0 + d.c0 + e < g.OW;
}
// Bit i set iff 0 <= x0 + i * d < n, i < k.
DFQ_HOST_DEVICE inline uint64_t dwc_axis_bits(int32_t x0, int32_t n, int32_t k, int32_t d) {
    uint64_t bits = 0;
    int64_t x = x0;
    for (int i = 0; i < k; ++i, x += d)
        if (x >= 0 && x < n) bits |= uint64_t(1) << i;
    return bits;
}
// Bit k = i * KW + j of the tap mask: row bit i and column bit j.
DFQ_HOST_DEVICE inline uint64_t dwc_tap_mask(const DwcGeom& g, uint64_t row_bits, uint64_t col_bits) {
    uint64_t mask = 0;
    for (int i = 0; i < g.KH; ++i)
        if ((row_bits >> i) & 1u) mask |= col_bits << (i * g.KW);
    return mask;
}
// T of output (oh, ow): the closed form.
DFQ_HOST_DEVICE inline int32_t dwc_taps(const DwcGeom& g, int32_t oh, int32_t ow) {
    return igc_axis_taps(oh * g.sh - g.ph, g.H, g.KH, g.dh) * igc_axis_taps(ow * g.sw - g.pw, g.W, g.KW, g.dw);
}
// Word w of the mask operand (0x01 where the bit is set) and of the A operand as the instruction
// takes it (signed domain, 0 wherever the bit is clear).
DFQ_HOST_DEVICE inline uint32_t dwc_ones_word(uint64_t mask, int w) { return igc_ones_word((uint32_t)(mask >> (4 * w)) & 0xFu, 0); }
DFQ_HOST_DEVICE inline uint32_t dwc_operand_word(uint32_t raw, uint32_t xor_mask, uint64_t mask, int w) {
    return (raw ^ xor_mask) & (dwc_ones_word(mask, w) * 0xFFu);
}
// The taps walked in order: k -> (i, j) and the tap's displacement in the footprint's LDS bytes.
struct DwcTap {
    int32_t i, j, off;        // off = i * dh * fwp + j * dw
};
DFQ_HOST_DEVICE inline DwcTap dwc_tap0() { return DwcTap{0, 0, 0}; }
DFQ_HOST_DEVICE inline void dwc_tap_next(const DwcGeom& g, DwcTap& t) {
    ++t.j;
    t.off += g.dw;
    if (t.j == g.KW) {
        t.off += g.dh * g.fwp - g.KW * g.dw;
        t.j = 0;
        ++t.i;
    }
}
// LDS byte of tap t of tile output (r, c) of plane pl.
DFQ_HOST_DEVICE inline int32_t dwc_tap_byte(const DwcGeom& g, int32_t pl, int32_t r, int32_t c, const DwcTap& t) {
    return dwc_lds_byte(g, pl, r * g.sh, c * g.sw) + t.off;
}
// The instruction: c + sum of the four signed byte products.
DFQ_HOST_DEVICE inline int32_t dwc_dot4(uint32_t a, uint32_t b, int32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_sdot4((int)a, (int)b, c, false);
#else
    for (int e = 0; e < 4; ++e) c += (int32_t)(int8_t)(a >> (8 * e)) * (int32_t)(int8_t)(b >> (8 * e));
    return c;
#endif
}
// Output (oh, ow) of channel m of plane p in NCHW: plane p * mult + m of out.
DFQ_HOST_DEVICE inline int64_t dwc_out_offset(const DwcGeom& g, int64_t p, int32_t m, int32_t oh, int32_t ow) {
    return (p * g.mult + m) * g.OHW + (int64_t)oh * g.OW + ow;
}

// dfq_int_dwconv2d's argument checks (no device call): DFQ_OK with the geometry and the grid, or
// the error.
int dwc_check(const dfq_int_dwconv2d_desc* d, DwcGeom& g, int64_t& grid);

}  // namespace dfq
