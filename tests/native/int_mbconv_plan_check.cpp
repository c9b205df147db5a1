// Host walk of dfq_int_mbconv_q's planner (dfq_int_mbconv_plan.h), built with the plan file alone under sanitizers: for each
// shape of the file (B Cin H W Ch Cout stride pad a line) every block, wave and lane is walked with the kernel's helpers; every
// LDS byte read was written and lies in its region, every global read in its tensor, every output is stored once.  Silent when so.
#include <cstdio>
#include <vector>

#include "dfq_int_mbconv_plan.h"

using namespace dfq;

namespace {

int failures = 0;
void fail(const char* what, long a, long b) { if (failures++ < 20) std::printf("%s: %ld %ld\n", what, a, b); }

struct Lds {
    std::vector<char> written;
    explicit Lds(int n) : written(n, 0) {}
    void touch(int at, int n, int lo, int hi, bool wr) {
        if (at < lo || at + n > hi || at + n > (int)written.size()) return fail("LDS access outside its region", at, hi);
        for (int i = 0; i < n; ++i) {
            if (!wr && !written[at + i]) return fail("LDS byte read before it was written", at + i, lo);
            written[at + i] = 1;
        }
    }
    void write(int at, int n, int lo, int hi) { touch(at, n, lo, hi, true); }
    void read(int at, int n, int lo, int hi) { touch(at, n, lo, hi, false); }
};

void b_frag(int64_t row, int64_t rows, int64_t K, int64_t step, int lane) {   // the bytes ig_load_bytes reads of codes[rows][K]
    const int64_t k0 = ig_lane_k0(step, lane);
    const int nv = ig_lane_valid(row, rows, k0, K);
    if (nv && (ig_byte_offset(row, k0, K) < 0 || ig_byte_offset(row, k0, K) + (ig_wide(K) ? kIgLaneK : nv) > rows * K)) fail("weight read outside", row, k0);
}

void walk(const dfq_int_mbconv_desc& d) {
    MbGeom g;
    int64_t grid = 0;
    if (mb_check(&d, g, grid) != DFQ_OK) return fail("mb_check refuses", d.Cin, d.Ch);
    if (g.lds_bytes > kMbLdsBytes || g.frt > kMbMaxRowTiles || g.ksteps > kMbMaxKSteps || g.nt > 5 * kMbWaves) fail("limits", g.lds_bytes, g.frt);
    const int64_t x_size = d.B * d.Cin * g.HW;
    std::vector<int> stored((size_t)(d.B * d.Cout * g.OHW), 0);
    for (int64_t block = 0; block < grid; ++block) {
        const MbBlock blk = mb_block(g, (uint32_t)block);
        Lds lds(g.lds_bytes);
        for (int32_t cell = 0; cell < mb_cells(g); ++cell) {
            const int32_t k0 = mb_cell_k(g, cell), fr = mb_cell_fr(g, cell);
            const MbPixel q = mb_pixel(g, blk, fr);
            for (int t = 0; t < 4; ++t)
                if (q.inside && k0 + t < g.Cin) {
                    const int64_t o = mb_x_offset(g, blk.b, k0 + t, q.ih, q.iw);
                    if (o < 0 || o >= x_size) fail("x read outside", o, x_size);
                }
            lds.write(mb_xs_byte(g, fr, k0), 4, 0, g.xsum_off);
        }
        for (int32_t i = 0; i < g.frt; ++i)
            for (int lane = 0; lane < 64; ++lane) {
                for (int32_t s = 0; s < g.ksteps; ++s) lds.read(mb_xs_frag(g, i, s, lane), 16, 0, g.xsum_off);
                if ((lane & 15) == 0) lds.write(mb_xsum_byte(g, mb_acc_row(i, lane)), 16, g.xsum_off, g.hid_off);
            }
        for (int32_t c = 0; c < g.chunks; ++c) {
            const int32_t ch0 = c * kMbChunk;
            for (int tid = 0; tid < kMbChunk * 3; ++tid) lds.write(mb_wts_byte(g, tid / 3, tid % 3), 4, g.wts_off, g.pa_off);
            for (int wave = 0; wave < kMbWaves; ++wave)
                for (int lane = 0; lane < 64; ++lane) {
                    const int32_t nl = wave * 16 + (lane & 15);
                    for (int32_t s = 0; s < g.ksteps; ++s) b_frag(ch0 + nl, g.Ch, g.Cin, s, lane);
                    for (int32_t i = 0; i < g.frt; ++i) {
                        lds.read(mb_xsum_byte(g, mb_acc_row(i, lane)), 16, g.xsum_off, g.hid_off);
                        lds.write(mb_hid_byte(g, nl, mb_acc_row(i, lane)), 4, g.hid_off, g.wts_off);
                    }
                }
            for (int32_t u = 0; u < mb_units(g); ++u) {
                const MbUnit q = mb_unit(g, blk, u);
                for (int e = 0; e < 4; ++e) {
                    for (int k = 0; k < 9; ++k) lds.read(mb_hid_byte(g, q.cq * 4 + e, q.at) + mb_tap(g, k), 1, g.hid_off, g.wts_off);
                    for (int w = 0; w < 3; ++w) lds.read(mb_wts_byte(g, q.cq * 4 + e, w), 4, g.wts_off, g.pa_off);
                }
                if (q.on && q.at + mb_tap(g, 8) >= g.fr) fail("a tap past the footprint", q.at, g.fr);
                lds.write(mb_pa_byte(g, q.tp, q.cq * 4), 4, g.pa_off, g.lds_bytes);
            }
            for (int wave = 0; wave < kMbWaves; ++wave)
                for (int lane = 0; lane < 64; ++lane) {
                    for (int32_t i = 0; i < g.rt; ++i) lds.read(mb_pa_frag(g, i, lane), 16, g.pa_off, g.lds_bytes);
                    for (int32_t tile = wave; tile < g.nt; tile += kMbWaves) b_frag(tile * 16 + (lane & 15), g.Cout, g.Ch, c, lane);
                }
        }
        for (int32_t tile = 0; tile < g.nt; ++tile)
            for (int lane = 0; lane < 64; ++lane)
                for (int32_t i = 0; i < g.rt; ++i) {
                    const int64_t n = tile * 16 + (lane & 15);
                    const int32_t tp0 = mb_acc_row(i, lane);
                    for (int r = 0; r < 4; ++r)
                        if (n < g.Cout && mb_tp_on(g, blk, tp0 + r)) {
                            const int64_t o = mb_out_offset(g, blk.b, n, blk.oh0 + (tp0 >> 3), blk.ow0 + (tp0 & 7)) + r;
                            if (o < 0 || o >= (int64_t)stored.size()) fail("store outside", o, (long)stored.size());
                            else ++stored[(size_t)o];
                        }
                }
    }
    for (size_t o = 0; o < stored.size(); ++o)
        if (stored[o] != 1) return fail("an output not stored once", (long)o, stored[o]);
}

}  // namespace

int main(int argc, char** argv) {
    std::FILE* f = argc > 1 ? std::fopen(argv[1], "r") : nullptr;
    if (!f) return 2;
    long v[8];
    while (std::fscanf(f, "%ld %ld %ld %ld %ld %ld %ld %ld", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6], &v[7]) == 8) {
        dfq_int_mbconv_desc d{};   // made-up pointers: nothing is dereferenced
        d.x = d.out = reinterpret_cast<void*>(0x1000);
        for (dfq_int_mbconv_layer* l : {&d.expand, &d.depthwise, &d.project}) l->b_codes = l->b_scale = reinterpret_cast<const float*>(0x3000);
        for (dfq_int_mbconv_quant* q : {&d.x_quant, &d.hidden1, &d.hidden2}) q->bits = 8, q->given_max = 6.0;
        d.B = v[0]; d.Cin = v[1]; d.H = v[2]; d.W = v[3]; d.Ch = v[4]; d.Cout = v[5]; d.stride = v[6]; d.pad = v[7];
        walk(d);
    }
    std::fclose(f);
    return failures ? 1 : 0;
}
