// Host walk of dfq_int_mean_q's planner (dfq_int_pool_plan.h), built with the plan files alone under sanitizers.  shapes.txt: a line
// "R P x16" a shape.  Every block, chunk and piece is walked with the kernel's helpers: a chunk and a piece lie inside [0, R P), a
// 16-B load is aligned, the pieces of a row partition it, every byte is summed once and every row stored once.  Silent when so.
// (The max pool's cells, quads and taps are the depthwise convolution's: int_dwconv_plan_check.cpp and int_io_plan_check.cpp.)
#include <cstdio>
#include <vector>

#include "dfq_int_pool_plan.h"

using namespace dfq;

namespace {

int failures = 0;
void fail(const char* what, long a, long b) { if (failures++ < 20) std::printf("%s: %ld %ld\n", what, a, b); }

void walk_mean(int64_t R, int64_t P, int x16) {
    dfq_int_mean_desc d{};   // made-up pointers: nothing is dereferenced
    d.x = reinterpret_cast<void*>(0x10000 + x16);
    d.out = reinterpret_cast<void*>(0x20000);
    d.x_quant.bits = 8, d.x_quant.given_max = 6.0;
    d.rows = R, d.plane = P;
    MeanGeom g;
    int64_t grid = 0;
    if (mean_check(&d, g, grid) != DFQ_OK) return fail("mean_check refuses", R, P);
    if (g.rb > kMeanMaxRows || g.small != (P <= kMeanSmallP)) fail("limits", g.rb, g.small);
    const int64_t n = R * P;
    std::vector<int> summed((size_t)n, 0), stored((size_t)R, 0);
    for (int64_t block = 0; block < grid; ++block) {
        const MeanBlock b = mean_block(g, (uint32_t)block);
        if (b.nr < 1 || b.nr > g.rb || b.r0 + b.nr > R) fail("a block's rows", b.r0, b.nr);
        for (int32_t c = 0; c < b.chunks + 2; ++c) {   // two chunks past the last: a lane's of a ragged round
            const int32_t e0 = mean_chunk_e0(b, c);
            if (c < b.chunks) {
                if (mean_chunk_vector(g, b, e0)) {
                    if ((0x10000 + x16 + b.b0 + e0) % 16 || b.b0 + e0 < 0 || b.b0 + e0 + 16 > n) fail("a 16-B load", b.b0, e0);
                } else {
                    for (int i = 0; i < kMeanChunk; ++i)
                        if (mean_byte_on(b, e0, i) && (b.b0 + e0 + i < 0 || b.b0 + e0 + i >= n)) fail("a byte load", b.b0, e0 + i);
                }
            }
            const int32_t hi = mean_chunk_hi(b, e0);
            if (c >= b.chunks && mean_chunk_lo(e0) < hi) fail("a chunk past the last holds bytes", c, hi);
            int pieces = 0;
            for (int32_t lo = mean_chunk_lo(e0); lo < hi; ++pieces) {
                const MeanPiece pc = mean_piece(g, e0, lo, hi);
                if (pc.row < 0 || pc.row >= (g.small ? b.nr : 1) || pc.hi <= lo || pc.hi > hi) return fail("a piece", pc.row, pc.hi);
                for (int i = lo; i < pc.hi; ++i) {
                    if ((e0 + i) / P != pc.row) fail("a piece's byte in another row", e0 + i, pc.row);
                    if (!((mean_piece_word(0xFFFFFFFFu, 0, lo, pc.hi, i >> 2) >> (8 * (i & 3))) & 1u)) fail("a masked byte of the piece", lo, i);
                    ++summed[(size_t)(b.b0 + e0 + i)];
                }
                uint32_t kept = 0;
                for (int j = 0; j < 4; ++j) kept += (uint32_t)dwc_dot4(mean_piece_word(0x01010101u, 0, lo, pc.hi, j), 0x01010101u, 0);
                if ((int32_t)kept != pc.hi - lo) fail("the mask keeps other bytes", kept, pc.hi - lo);
                lo = pc.hi;
            }
            if (P >= kMeanChunk && pieces > 2) fail("more than two pieces", pieces, P);
        }
        for (int32_t t = 0; t < mean_quads(b); ++t) {
            for (int e = 0; e < kMeanQuad; ++e)
                if (mean_row_on(b, t, e)) ++stored[(size_t)(b.r0 + t * kMeanQuad + e)];
            for (uintptr_t out : {uintptr_t(0x20000), uintptr_t(0x20001)})
                if (mean_out_word(b, t, out) && ((out + b.r0 + t * kMeanQuad) % 4 || !mean_row_on(b, t, 3))) fail("a word store", b.r0, t);
        }
    }
    for (int64_t i = 0; i < n; ++i)
        if (summed[(size_t)i] != 1) return fail("a byte not summed once", i, summed[(size_t)i]);
    for (int64_t r = 0; r < R; ++r)
        if (stored[(size_t)r] != 1) return fail("a row not stored once", r, stored[(size_t)r]);
}

}  // namespace

int main(int argc, char** argv) {
    std::FILE* f = argc > 1 ? std::fopen(argv[1], "r") : nullptr;
    if (!f) return 2;
    long v[3];
    while (std::fscanf(f, "%ld %ld %ld", &v[0], &v[1], &v[2]) == 3) walk_mean(v[0], v[1], (int)v[2]);
    std::fclose(f);
    return failures ? 1 : 0;
}
