// dfq_int_dwconv2d's index arithmetic on its own: dfq_int_dwconv_plan.h / .cpp (with the headers
// they build on) linked with this main and nothing else, so it runs under AddressSanitizer / UBSan
// on a machine without a GPU (tests/test_int_dwconv_host.py builds and runs it).
//
//   int_dwconv_plan_check shapes.txt
//
// shapes.txt: lines `B C H W mult KH KW sh sw ph pw dh dw`.  For every geometry, each
// (x_symmetric, b_signed) and, where K is even, packed B as well, every element of x carries a
// random code over the full byte range (what the quantizer would give it), B's codes are random,
// and the program walks every block, round and lane through the header's helpers exactly as the
// kernel does -- the footprint cells, the weight words, the quads, the tap walk, the dot
// instruction's host form, the folds, the stores -- and checks that
//   - every global read lies inside x and is the element (plane, ih0 + r, iw0 + col) found here
//     with plain arithmetic,
//   - every LDS word is written at most once a block and inside the declared extents, and every
//     LDS byte or weight word that is read was written (a lane that reads nothing carries a junk
//     code before the keep mask, so only the mask can remove it),
//   - the byte at each (output, tap) is the code of the im2col definition's element -- found here
//     from (b, c, oh, ow, i, j) with plain arithmetic -- or 0 for a padding tap, and the tap's mask
//     bit is the definition's v,
//   - T (dwc_taps) is the mask's population count,
//   - the folds give the contract's P, Sa and Sb -- computed directly from the codes and v in
//     int64 -- back from the signed-domain dot products,
//   - every output element is stored exactly once, at its NCHW offset (found here from
//     (b, n, oh, ow)), the 16-B groups only where all four are consecutive.
// Output per (geometry, signs, packed):
//   `ok <13 numbers> xs <0|1> bs <0|1> packed <0|1> K <K> OH <n> OW <n> th <n> tw <n> pp <n> mc <n> grid <n>
//    cells <n> reads <n> distinct <n> taps <n> stores <n> quads <n>`.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dfq_int_dwconv_plan.h"

using namespace dfq;

namespace {

#define FAIL(...) return fprintf(stderr, __VA_ARGS__), fprintf(stderr, "\n"), false

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 32);
}

struct Shape {
    long long B, C, H, W, mult, KH, KW, sh, sw, ph, pw, dh, dw;
};

// the definition: the offset into x of tap (i, j) of output (b, c, oh, ow), or -1 for a padding tap
long long definition(const Shape& s, long long b, long long c, long long oh, long long ow, long long i, long long j) {
    const long long ih = oh * s.sh - s.ph + i * s.dh, iw = ow * s.sw - s.pw + j * s.dw;
    if (ih < 0 || ih >= s.H || iw < 0 || iw >= s.W) return -1;
    return ((b * s.C + c) * s.H + ih) * s.W + iw;
}

constexpr int kThreadsHere = 256;   // the kernel's block

bool walk(const Shape& s, const DwcGeom& g, int64_t grid, bool x_sym, bool b_signed, bool packed) {
    const long long N = s.C * s.mult, K = s.KH * s.KW;
    const long long xsize = s.B * s.C * s.H * s.W, osize = s.B * N * g.OH * g.OW;
    const int alo = x_sym ? -128 : 0;
    std::vector<int> qx((size_t)xsize);
    for (auto& q : qx) q = alo + (int)(rnd() % 256u);
    qx[0] = alo + 255;
    // B: its codes and the bytes as stored
    const int bspan = packed ? 16 : 256, blo = b_signed ? -(bspan / 2) : 0;
    std::vector<int> qb((size_t)(N * K));
    for (auto& q : qb) q = blo + (int)(rnd() % (uint32_t)bspan);
    for (long long k = 0; k < K; ++k) qb[(size_t)k] = N > 1 ? blo : blo + bspan - 1;
    std::vector<uint8_t> bbytes((size_t)(packed ? N * K / 2 : N * K));   // exactly the rows: a read past them is ASan's
    for (long long t = 0; t < N * K; ++t) {
        if (!packed) bbytes[(size_t)t] = (uint8_t)(qb[(size_t)t] & 0xFF);
        else if (t % 2 == 0) bbytes[(size_t)(t / 2)] = (uint8_t)((qb[(size_t)t] & 0xF) | ((qb[(size_t)(t + 1)] & 0xF) << 4));
    }
    const int oa = ig_offset(x_sym), ob = ig_offset(b_signed);
    const uint32_t xa = ig_xor_mask(x_sym), xb = ig_xor_mask(b_signed);
    const uint64_t full = dwc_full_mask(g.K);
    if (g.K != K || g.words != (K + 3) / 4 || K > kDwMaxTaps) FAIL("K or the word count");
    if ((long long)g.pp * g.fwords * 4 > kDwCodeBytes) FAIL("the footprints leave the declared code bytes");
    if ((long long)g.pp * g.mc * g.words > kDwWeightWords) FAIL("the weights leave the declared words");
    if (g.th > kDwTileH || g.tw > kDwTileW || g.th < 1 || g.tw < 1 || g.mc < 1 || g.pp < 1 || g.pp > kDwMaxPlanes) FAIL("tile");
    if (g.fh != (g.th - 1) * s.sh + (s.KH - 1) * s.dh + 1 || g.fw != (g.tw - 1) * s.sw + (s.KW - 1) * s.dw + 1) FAIL("footprint");
    if (g.fwp % 4 || g.fwp < g.fw || g.fwp >= g.fw + 4 || g.fwords * 4 != g.fh * g.fwp) FAIL("pitch");
    if (grid != ceil_div(g.planes, (int64_t)g.pp) * g.tiles_h * g.tiles_w) FAIL("grid");
    if (g.pp > 1 && g.tiles_h * g.tiles_w != 1) FAIL("several planes of several tiles");

    std::vector<int> stored((size_t)osize, 0), xread((size_t)xsize, 0);
    long long cells = 0, reads = 0, taps = 0, stores = 0, quads16 = 0;
    std::vector<uint8_t> lds((size_t)kDwCodeBytes), ldsw((size_t)kDwCodeBytes);
    std::vector<long long> ldssrc((size_t)kDwCodeBytes);   // offset + 1 of the element a byte stands for, 0: none
    std::vector<uint32_t> wts((size_t)kDwWeightWords);
    std::vector<uint8_t> wtsw((size_t)kDwWeightWords);
    for (int64_t block = 0; block < grid; ++block) {
        const DwcBlock blk = dwc_block(g, (uint32_t)block);
        if (blk.p0 >= g.planes || blk.oh0 >= g.OH || blk.ow0 >= g.OW) FAIL("block %lld owns nothing", (long long)block);
        std::fill(ldsw.begin(), ldsw.end(), 0);
        // 1. the footprint
        const int32_t ncells = dwc_cells(g);
        for (int32_t base = 0; base < ncells; base += kThreadsHere)
            for (int tid = 0; tid < kThreadsHere; ++tid) {
                const int32_t wq = base + tid;
                const bool active = wq < ncells;
                const DwcCell c = dwc_cell(g, active ? wq : 0);
                if (c.pl < 0 || c.pl >= g.pp || c.r < 0 || c.r >= g.fh || c.col < 0 || c.col >= g.fwp || c.col % 4) FAIL("cell %d", wq);
                const int64_t p = blk.p0 + c.pl;
                uint32_t word = 0, keep = 0;
                long long src[4] = {0, 0, 0, 0};
                for (int t = 0; t < 4; ++t) {
                    const bool on = active && dwc_x_reads(g, blk, p, c.r, c.col + t);
                    int code = 0x5A;   // junk: only the keep mask removes it
                    if (on) {
                        const int64_t off = dwc_x_offset(g, blk, p, c.r, c.col + t);
                        if (off < 0 || off >= xsize) FAIL("read of x at %lld", (long long)off);
                        const long long ih = (long long)blk.oh0 * s.sh - s.ph + c.r, iw = (long long)blk.ow0 * s.sw - s.pw + c.col + t;
                        if (ih < 0 || ih >= s.H || iw < 0 || iw >= s.W || off != (p * s.H + ih) * s.W + iw) FAIL("cell %d reads x[%lld]", wq, (long long)off);
                        code = qx[(size_t)off];
                        src[t] = off + 1;
                        ++xread[(size_t)off];
                        ++reads;
                    }
                    word |= (uint32_t)(code & 0xFF) << (8 * t);
                    keep |= on ? 0xFFu << (8 * t) : 0u;
                }
                word &= keep;
                if (!active) continue;
                const int32_t at = dwc_lds_byte(g, c.pl, c.r, c.col);
                if (at < 0 || at % 4 || at + 4 > kDwCodeBytes) FAIL("LDS word at %d", at);
                for (int t = 0; t < 4; ++t) {
                    if (ldsw[(size_t)(at + t)]++) FAIL("LDS byte %d written twice", at + t);
                    lds[(size_t)(at + t)] = (uint8_t)(word >> (8 * t));
                    ldssrc[(size_t)(at + t)] = src[t];
                }
                ++cells;
            }
        const int32_t nquads = dwc_quads(g);
        for (int32_t m0 = 0; m0 < g.mult; m0 += g.mc) {
            const int32_t mcn = g.mult - m0 < g.mc ? g.mult - m0 : g.mc;
            std::fill(wtsw.begin(), wtsw.end(), 0);
            // 2. the weights
            for (int32_t t = 0; t < g.pp * mcn * g.words; ++t) {
                const int32_t w = t % g.words, pm = t / g.words, m = pm % mcn, pl = pm / mcn;
                const int64_t p = blk.p0 + pl;
                uint32_t raw = 0;
                if (p < g.planes) {
                    const int64_t n = (p % g.C) * g.mult + m0 + m;
                    for (int e = 0; e < 4; ++e)
                        if (4 * w + e < g.K) {
                            const uint32_t code = dwc_b_code(bbytes.data(), n, 4 * w + e, g.K, packed, b_signed);
                            if ((int)(b_signed ? (int8_t)code : (int)code) != qb[(size_t)(n * K + 4 * w + e)]) FAIL("B's code (%lld, %d)", (long long)n, 4 * w + e);
                            raw |= code << (8 * e);
                        }
                }
                const int32_t at = dwc_w_index(g, pl, m, w);
                if (at < 0 || at >= kDwWeightWords || wtsw[(size_t)at]++) FAIL("weight word %d", at);
                wts[(size_t)at] = dwc_operand_word(raw, xb, full, w);
            }
            // 3. the outputs
            for (int32_t q = 0; q < nquads; ++q) {
                const DwcQuad d = dwc_quad(g, q);
                if (d.pl < 0 || d.pl >= g.pp || d.r < 0 || d.r >= g.th || d.c0 < 0 || d.c0 >= g.tw) FAIL("quad %d", q);
                const int64_t p = blk.p0 + d.pl;
                const int32_t oh = blk.oh0 + d.r;
                if (p >= g.planes || oh >= g.OH || !dwc_out_on(g, blk, d, 0)) continue;
                const long long b = p / s.C, c = p % s.C;
                const uint64_t row_bits = g.masked ? dwc_axis_bits(oh * g.sh - g.ph, g.H, g.KH, g.dh) : 0;
                bool on[kDwQuad];
                uint64_t vm[kDwQuad];
                int32_t T[kDwQuad], at[kDwQuad];
                for (int e = 0; e < kDwQuad; ++e) {
                    on[e] = dwc_out_on(g, blk, d, e);
                    const int32_t ow = blk.ow0 + d.c0 + e;
                    vm[e] = !on[e] ? 0 : !g.masked ? full : dwc_tap_mask(g, row_bits, dwc_axis_bits(ow * g.sw - g.pw, g.W, g.KW, g.dw));
                    T[e] = !on[e] ? 0 : g.masked ? dwc_taps(g, oh, ow) : g.K;
                    at[e] = dwc_tap_byte(g, d.pl, d.r, on[e] ? d.c0 + e : d.c0, dwc_tap0());
                    if (on[e] && T[e] != __builtin_popcountll(vm[e])) FAIL("T of (%d, %d): %d, the mask holds %d", oh, ow, T[e], __builtin_popcountll(vm[e]));
                }
                if (!on[0]) FAIL("a quad without a first output");
                for (int32_t m = 0; m < mcn; ++m) {
                    int32_t acc[kDwQuad] = {0, 0, 0, 0}, ra[kDwQuad] = {0, 0, 0, 0}, rb[kDwQuad] = {0, 0, 0, 0};
                    DwcTap tap = dwc_tap0();
                    const int64_t n = c * s.mult + m0 + m;
                    for (int32_t w = 0; w < g.words; ++w) {
                        uint32_t raw[kDwQuad] = {0, 0, 0, 0};
                        for (int t = 0; t < 4; ++t) {
                            const int k = 4 * w + t;
                            if (k < g.K) {
                                if (tap.i != k / g.KW || tap.j != k % g.KW) FAIL("tap %d walks to (%d, %d)", k, tap.i, tap.j);
                                for (int e = 0; e < kDwQuad; ++e) {
                                    const int32_t a = at[e] + tap.off;
                                    if (a < 0 || a >= kDwCodeBytes || ldsw[(size_t)a] != 1) FAIL("LDS byte %d read, never written", a);
                                    raw[e] |= (uint32_t)lds[(size_t)a] << (8 * t);
                                    if (!on[e]) continue;
                                    const long long want = definition(s, b, c, oh, blk.ow0 + d.c0 + e, tap.i, tap.j);
                                    if (ldssrc[(size_t)a] != want + 1) FAIL("output (%lld, %d, %d) tap %d holds x[%lld], the definition reads x[%lld]",
                                                                            (long long)p, oh, blk.ow0 + d.c0 + e, k, ldssrc[(size_t)a] - 1, want);
                                    if (((vm[e] >> k) & 1u) != (uint64_t)(want >= 0)) FAIL("mask bit %d of output (%d, %d)", k, oh, blk.ow0 + d.c0 + e);
                                    if (want < 0 && lds[(size_t)a] != 0) FAIL("a padding byte that is not 0");
                                    if (m == 0 && m0 == 0) taps += want >= 0;
                                }
                            }
                            dwc_tap_next(g, tap);
                        }
                        const int32_t wa = dwc_w_index(g, d.pl, m, w);
                        if (!wtsw[(size_t)wa]) FAIL("weight word %d read, never written", wa);
                        const uint32_t bw = wts[(size_t)wa];
                        for (int e = 0; e < kDwQuad; ++e) {
                            const uint32_t aw = dwc_operand_word(raw[e], xa, vm[e], w), ones = dwc_ones_word(vm[e], w);
                            acc[e] = dwc_dot4(aw, bw, acc[e]);
                            ra[e] = dwc_dot4(aw, 0x01010101u, ra[e]);
                            rb[e] = dwc_dot4(ones, bw, rb[e]);
                        }
                    }
                    const int64_t o = dwc_out_offset(g, p, m0 + m, oh, blk.ow0 + d.c0);
                    const bool all = on[0] && on[1] && on[2] && on[3];
                    for (int e = 0; e < kDwQuad; ++e) {
                        if (!on[e]) continue;
                        const long long ow = blk.ow0 + d.c0 + e;
                        long long P = 0, Sa = 0, Sb = 0, Tn = 0;
                        for (long long i = 0; i < s.KH; ++i)
                            for (long long j = 0; j < s.KW; ++j) {
                                const long long off = definition(s, b, c, oh, ow, i, j);
                                if (off < 0) continue;
                                const long long a = qx[(size_t)off], bq = qb[(size_t)(n * K + i * s.KW + j)];
                                P += a * bq;
                                Sa += a;
                                Sb += bq;
                                ++Tn;
                            }
                        if (Tn != T[e]) FAIL("T of (%d, %lld)", oh, ow);
                        if (ig_fold_p(acc[e], ra[e], rb[e], oa, ob, T[e]) != P) FAIL("P of (%lld, %lld, %d, %lld)", b, (long long)n, oh, ow);
                        if (ig_fold_s(ra[e], oa, T[e]) != Sa) FAIL("Sa of (%lld, %lld, %d, %lld)", b, c, oh, ow);
                        if (ig_fold_s(rb[e], ob, T[e]) != Sb) FAIL("Sb of (%lld, %d, %lld)", (long long)n, oh, ow);
                        const long long want = ((b * N + n) * g.OH + oh) * g.OW + ow;
                        if (o + e != want || want < 0 || want >= osize) FAIL("store of (%lld, %lld, %d, %lld) at %lld", b, (long long)n, oh, ow, (long long)(o + e));
                        ++stored[(size_t)want];
                        ++stores;
                    }
                    quads16 += all;
                }
            }
        }
    }
    for (size_t i = 0; i < stored.size(); ++i)
        if (stored[i] != 1) FAIL("output element %lld stored %d times", (long long)i, stored[i]);
    long long distinct = 0;
    for (int r : xread) distinct += r > 0;
    printf("ok %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld xs %d bs %d packed %d K %lld OH %d OW %d th %d tw %d pp %d mc %d grid %lld "
           "cells %lld reads %lld distinct %lld taps %lld stores %lld quads %lld\n",
           s.B, s.C, s.H, s.W, s.mult, s.KH, s.KW, s.sh, s.sw, s.ph, s.pw, s.dh, s.dw, (int)x_sym, (int)b_signed, (int)packed, K, g.OH, g.OW,
           g.th, g.tw, g.pp, g.mc, (long long)grid, cells, reads, distinct, taps, stores, quads16);
    return true;
}

bool check(const Shape& s) {
    dfq_int_dwconv2d_desc d{};
    d.x = reinterpret_cast<const float*>((uintptr_t)0x10004);
    d.b_codes = reinterpret_cast<const void*>((uintptr_t)0x20010);
    d.b_scale = reinterpret_cast<const float*>((uintptr_t)0x30004);
    d.out = reinterpret_cast<float*>((uintptr_t)0x40004);
    d.B = s.B; d.C = s.C; d.H = s.H; d.W = s.W; d.mult = s.mult; d.KH = s.KH; d.KW = s.KW;
    d.stride_h = s.sh; d.stride_w = s.sw; d.pad_h = s.ph; d.pad_w = s.pw; d.dil_h = s.dh; d.dil_w = s.dw;
    d.x_bits = 8;
    DwcGeom g;
    int64_t grid = 0;
    if (dwc_check(&d, g, grid) != DFQ_OK || grid < 1) FAIL("dwc_check refuses a good descriptor");
    if (g.planes != s.B * s.C || g.masked != (s.ph != 0 || s.pw != 0)) FAIL("planes or masked");
    const bool even = (s.KH * s.KW) % 2 == 0;
    for (int mode = 0; mode < (even ? 8 : 4); ++mode)
        if (!walk(s, g, grid, (mode & 1) != 0, (mode & 2) != 0, (mode & 4) != 0)) return false;
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return fprintf(stderr, "usage: %s shapes.txt\n", argv[0]), 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return perror(argv[1]), 2;
    Shape s;
    while (fscanf(f, "%lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld", &s.B, &s.C, &s.H, &s.W, &s.mult, &s.KH, &s.KW, &s.sh,
                  &s.sw, &s.ph, &s.pw, &s.dh, &s.dw) == 13)
        if (!check(s)) {
            fprintf(stderr, "geometry %lld %lld %lld %lld x%lld, %lldx%lld\n", s.B, s.C, s.H, s.W, s.mult, s.KH, s.KW);
            fclose(f);
            return 1;
        }
    fclose(f);
    return 0;
}
