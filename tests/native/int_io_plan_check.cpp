// The three 4-B access predicates of the code-in / code-out integer entries (dfq_int_io_plan.h) on the CPU
// under ASan / UBSan (tests/test_int_io_host.py); links dfq_int_dwconv_plan.cpp only.  shapes.txt: lines
// `c B C H W N KH KW sh sw ph pw dh dw` (dfq_int_conv2d_q) or `d B C H W mult KH KW ...` (dfq_int_dwconv2d_q),
// each taken at every address mod 4: a 4-B access is granted only at a 4-aligned address inside the array,
// over the four bytes the byte path touches, and every output byte is stored once.  Silent unless it fails.
#include <cstdio>
#include <vector>

#include "dfq_int_io_plan.h"

using namespace dfq;

namespace {

#define FAIL(...) return fprintf(stderr, __VA_ARGS__), fprintf(stderr, "\n"), false

struct Shape { long long B, C, H, W, N, KH, KW, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w; };   // the descriptors' names (N: mult on a `d` line)
long long g_words = 0;   // 4-B accesses granted over the whole file: the walk is not vacuous

// igio_out_word over every group of four rows a lane can hold (m % 4 == 0) and every column
bool conv(const Shape& s, uintptr_t out) {
    MxcGeom g;
    int64_t M = 0, K = 0, grid = 0;
    if (mxc_check_geometry(s, g, M, K, grid) != DFQ_OK) FAIL("the geometry is refused");
    std::vector<int> stored((size_t)(s.B * s.N * g.OHW), 0);
    for (int64_t m = 0; m < M; m += 4)
        for (int64_t n = 0; n < s.N; ++n) {
            const bool word = igio_out_word(g, m, M, n, out);
            if (word && (((out + (uintptr_t)mxc_out_offset(g, m, n)) & 3u) != 0 || m + 3 >= M)) FAIL("a 4-B store off its alignment or past M");
            for (int r = 0; r < 4 && m + r < M; ++r) {
                const int64_t o = mxc_out_offset(g, m + r, n);
                if (word && o != mxc_out_offset(g, m, n) + r) FAIL("the word at (%lld, %lld) is not rows m .. m + 3", (long long)m, (long long)n);
                if (o < 0 || o >= (int64_t)stored.size() || stored[(size_t)o]++) FAIL("byte %lld stored twice or outside out", (long long)o);
            }
            g_words += word;
        }
    return true;
}

// dwio_x_word over every cell of every block; dwio_out_word over a few offsets
bool dwconv(const Shape& s, uintptr_t x, uintptr_t out) {
    dfq_int_dwconv2d_desc d{};
    d.x = reinterpret_cast<const float*>(x & ~uintptr_t(3));
    d.out = reinterpret_cast<float*>(out & ~uintptr_t(3));
    d.b_codes = d.b_scale = d.x;
    d.B = s.B; d.C = s.C; d.H = s.H; d.W = s.W; d.mult = s.N; d.KH = s.KH; d.KW = s.KW; d.x_bits = 8;
    d.stride_h = s.stride_h; d.stride_w = s.stride_w; d.pad_h = s.pad_h; d.pad_w = s.pad_w; d.dil_h = s.dil_h; d.dil_w = s.dil_w;
    DwcGeom g;
    int64_t grid = 0;
    if (dwc_check(&d, g, grid) != DFQ_OK) FAIL("dwc_check refuses a good descriptor");
    const int64_t xsize = s.B * s.C * s.H * s.W;
    for (int64_t block = 0; block < grid; ++block) {
        const DwcBlock blk = dwc_block(g, (uint32_t)block);
        for (int32_t wq = 0; wq < dwc_cells(g); ++wq) {
            const DwcCell c = dwc_cell(g, wq);
            const int64_t p = blk.p0 + c.pl, off = dwc_x_offset(g, blk, p, c.r, c.col);
            if (!dwio_x_word(g, blk, p, c.r, c.col, x)) continue;
            if (off < 0 || off + 3 >= xsize || ((x + (uintptr_t)off) & 3u) != 0) FAIL("a 4-B load at %lld", (long long)off);
            for (int t = 0; t < 4; ++t)   // the byte path reads the same four
                if (!dwc_x_reads(g, blk, p, c.r, c.col + t) || dwc_x_offset(g, blk, p, c.r, c.col + t) != off + t) FAIL("cell %d: byte %d of the word is no read", wq, t);
            ++g_words;
        }
    }
    for (int64_t o = 0; o < 8; ++o)
        if (dwio_out_word(false, out, o) || dwio_out_word(true, out, o) != (((out + (uintptr_t)o) & 3u) == 0)) FAIL("dwio_out_word at %lld", (long long)o);
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    FILE* f = argc == 2 ? fopen(argv[1], "r") : nullptr;
    if (!f) return fprintf(stderr, "usage: %s shapes.txt\n", argv[0]), 2;
    Shape s;
    char kind;
    while (fscanf(f, " %c %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld", &kind, &s.B, &s.C, &s.H, &s.W, &s.N, &s.KH, &s.KW, &s.stride_h,
                  &s.stride_w, &s.pad_h, &s.pad_w, &s.dil_h, &s.dil_w) == 14)
        for (uintptr_t align = 0; align < 4; ++align)
            if (!(kind == 'd' ? dwconv(s, 0x10000 + align, 0x40000 + align) : conv(s, 0x40000 + align)))
                return fprintf(stderr, "%c geometry %lld %lld %lld %lld -> %lld, %lldx%lld, alignment %d\n", kind, s.B, s.C, s.H, s.W, s.N, s.KH, s.KW, (int)align), 1;
    fclose(f);
    return g_words > 0 ? 0 : (fprintf(stderr, "no 4-B access was granted anywhere\n"), 1);
}
