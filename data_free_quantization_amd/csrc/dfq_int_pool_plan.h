// The index arithmetic of the pooling entries on stored codes (dfq_int_pool.hip): dfq_int_mean_q,
// the mean over a plane, and dfq_int_maxpool2d_q.
//
// The mean.  x is R rows of P code bytes; a workgroup (kThreads lanes) owns nr consecutive rows
// from r0, whose bytes are one span of n = nr * P bytes at byte b0 = r0 * P of x:
//   small planes (P <= kMeanSmallP)  nr = rb = kMeanSpanBytes / P rows (at most kMeanMaxRows): two
//                                    chunks a lane; block = r0 / rb
//   large planes                     nr = 1: block = r0
// Chunks are counted from the span's first 16-B boundary, as the add's are: with ha = (x + b0) mod
// 16, chunk c holds the span's bytes e0 = 16 c - ha .. e0 + 15, c < chunks = ceil((n + ha) / 16),
// and its address is a multiple of 16.  A chunk all of whose 16 bytes lie inside x -- in this span
// or in a neighbour's -- is one 16-B load (mean_chunk_vector); the first chunk of the first span
// and the last of the last are predicated byte loads of the bytes that are the span's
// (mean_byte_on).  No byte outside [x, x + R P) is read.
// A chunk's bytes of the span, [lo, hi) of its 16 (mean_chunk_lo / _hi), are cut at the row
// boundaries inside them into pieces (mean_piece): a piece is the bytes of one row, at most two
// pieces a chunk when P >= 16, at most 16 when P < 16.  A piece's sum is the packed 8-bit dot
// instruction of the chunk's four words, in the signed domain and masked to the piece
// (mean_piece_word), against a word of ones; the offset the signed domain took out comes back
// once a row, in the epilogue (mean_row_sum).  Small planes add every piece into its row's int32
// in LDS; large planes keep one int32 a lane, reduce it over the wave and add the waves' sums in
// LDS.  |S| <= 255 P < 2^31 for P <= kMeanMaxP.
// The epilogue takes the block's rows four at a time (a quad: rows 4 t .. 4 t + 3 of the block, a
// lane each), so that a code output's four bytes are one ig_codes4 call and one word where the
// address allows; the quad loop's trip count is the block's.
//
// The max pool.  The planes are tiled as dfq_int_dwconv2d's are (dwc_tiles with mult = 1 and
// dilation 1), and the footprint's cells, the quads, the row and column tap bits and every offset
// are dfq_int_dwconv_plan.h's and dfq_int_io_plan.h's.  The LDS holds a code in the order domain --
// the stored byte xor pool_order_mask -- in which the grid's order is the unsigned one for int8 as
// for uint8.  A tap outside the image is a clear bit of the row or column bits and takes no part;
// the byte at its place in LDS is never compared.
// The kernels and the host check (tests/native/int_pool_plan_check.cpp) use these helpers and
// nothing else for an address or a predicate.  No HIP header: the checks (dfq_int_pool_plan.cpp)
// build as plain C++.
#pragma once
#include "dfq_int_mbconv_plan.h"

namespace dfq {

constexpr int kMeanChunk = 16;                        // bytes of a lane's chunk
constexpr int64_t kMeanMaxP = int64_t(1) << 23;       // 255 P stays inside int32
constexpr int64_t kMeanMaxN = int64_t(1) << 40;
constexpr int kMeanSmallP = 4096;                     // the largest plane of the small regime
constexpr int kMeanSpanBytes = 2 * kMeanChunk * kThreads;   // a small workgroup's span: two chunks a lane
constexpr int kMeanMaxRows = 1024;                    // rows of a workgroup: its int32 sums in LDS
constexpr int kMeanQuad = 4;                          // rows of a lane's epilogue
static_assert(kMeanSpanBytes / kMeanSmallP >= 1, "a small plane fits a span");

struct MeanGeom {
    int64_t R, P;             // rows, bytes of a row
    int32_t rb;               // rows of a workgroup
    int32_t small;            // the regime
    int32_t x16;              // x mod 16
    int32_t out_codes;
};

struct MeanBlock {
    int64_t r0, b0;           // first row; its byte offset in x
    int32_t nr, n;            // rows and bytes of the span
    int32_t ha;               // (x + b0) mod 16: the bytes of chunk 0 before the span
    int32_t chunks;
};
DFQ_HOST_DEVICE inline MeanBlock mean_block(const MeanGeom& g, uint32_t block) {
    MeanBlock b;
    b.r0 = (int64_t)block * g.rb;
    b.b0 = b.r0 * g.P;
    const int64_t left = g.R - b.r0;
    b.nr = (int32_t)(left < g.rb ? left : g.rb);
    b.n = b.nr * (int32_t)g.P;
    b.ha = (int32_t)(((int64_t)g.x16 + b.b0) & 15);
    b.chunks = (b.n + b.ha + kMeanChunk - 1) / kMeanChunk;
    return b;
}
// Chunk c's first byte, in bytes of the span (negative inside chunk 0's head).
DFQ_HOST_DEVICE inline int32_t mean_chunk_e0(const MeanBlock& b, int32_t c) { return c * kMeanChunk - b.ha; }
// All 16 bytes of the chunk lie inside x: one 16-B load.
DFQ_HOST_DEVICE inline bool mean_chunk_vector(const MeanGeom& g, const MeanBlock& b, int32_t e0) {
    return b.b0 + e0 >= 0 && b.b0 + e0 + kMeanChunk <= g.R * g.P;
}
// Byte i of the chunk is the span's.
DFQ_HOST_DEVICE inline bool mean_byte_on(const MeanBlock& b, int32_t e0, int i) { return e0 + i >= 0 && e0 + i < b.n; }
// The chunk's bytes of the span: [lo, hi) of its 16 (empty for a chunk past the last).
DFQ_HOST_DEVICE inline int32_t mean_chunk_lo(int32_t e0) { return e0 < 0 ? -e0 : 0; }
DFQ_HOST_DEVICE inline int32_t mean_chunk_hi(const MeanBlock& b, int32_t e0) {
    const int32_t left = b.n - e0;
    return left < 0 ? 0 : left < kMeanChunk ? left : kMeanChunk;
}
// The piece that starts at byte `lo` of the chunk: its row of the block and its end.
struct MeanPiece {
    int32_t row, hi;
};
DFQ_HOST_DEVICE inline MeanPiece mean_piece(const MeanGeom& g, int32_t e0, int32_t lo, int32_t hi) {
    MeanPiece p;
    p.row = (int32_t)((uint32_t)(e0 + lo) / (uint32_t)g.P);
    const int64_t end = ((int64_t)p.row + 1) * g.P - e0;   // the row's end, in bytes of the chunk
    p.hi = end < hi ? (int32_t)end : hi;
    return p;
}
// Word j of the chunk as the dot instruction takes it: in the signed domain, 0 outside [lo, hi).
DFQ_HOST_DEVICE inline uint32_t mean_piece_word(uint32_t raw, uint32_t xor_mask, int32_t lo, int32_t hi, int j) {
    const uint32_t bits = ((1u << hi) - 1u) & ~((1u << lo) - 1u);
    return (raw ^ xor_mask) & (igc_ones_word(bits, j) * 0xFFu);
}
// A row's S from the sum of its pieces' dot products: the signed domain's offset back, P times.
DFQ_HOST_DEVICE inline int32_t mean_row_sum(const MeanGeom& g, int32_t dots, int off) { return dots + off * (int32_t)g.P; }

// The epilogue's quads of a block, and row e of quad t.
DFQ_HOST_DEVICE inline int32_t mean_quads(const MeanBlock& b) { return (b.nr + kMeanQuad - 1) / kMeanQuad; }
DFQ_HOST_DEVICE inline bool mean_row_on(const MeanBlock& b, int32_t t, int e) { return t * kMeanQuad + e < b.nr; }
// The quad's four code bytes, the first at out + r, go out as one word.
DFQ_HOST_DEVICE inline bool mean_out_word(const MeanBlock& b, int32_t t, uintptr_t out) {
    return mean_row_on(b, t, kMeanQuad - 1) && igio_word_at(out, b.r0 + (int64_t)t * kMeanQuad);
}

// The order domain of the max pool: xor this and the grid's integers compare as unsigned bytes.
DFQ_HOST_DEVICE inline uint32_t pool_order_mask(bool is_signed) { return ig_xor_mask(is_signed) ^ 0x80808080u; }

// The entries' argument checks (no device call): DFQ_OK with the geometry and the grid, or the error.
int mean_check(const dfq_int_mean_desc* d, MeanGeom& g, int64_t& grid);
int maxpool_check(const dfq_int_maxpool2d_desc* d, DwcGeom& g, int64_t& grid);

}  // namespace dfq
