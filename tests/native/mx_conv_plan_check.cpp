// dfq_mx_conv2d's index arithmetic on its own: dfq_mx_conv_plan.h / .cpp linked with this main
// and nothing else, so it runs under AddressSanitizer / UBSan on a machine without a GPU
// (tests/test_mx_conv_host.py builds and runs it).
//
//   mx_conv_plan_check shapes.txt
//
// shapes.txt: lines `B C H W N KH KW sh sw ph pw dh dw`.  For every geometry and each of the four
// activation formats (FP8 walks K in two runs of 16 per lane, the others in one run of 32) --
// and, for a pointwise geometry, both the general gather and the pointwise variant -- x is an
// array of exactly B * C * H * W floats holding its own index + 1, and the program walks every
// (block, wave, K step, instruction tile, lane) through the header's helpers exactly as the
// kernel does (MxmConvA::fetch, MxmNchwStore::store) and checks that
//   - every read lies inside x,
//   - the element a lane gathers for (m, k) is the im2col definition's -- found here from m and
//     k with plain divisions, sharing nothing with the helpers -- and +0 for a padding tap, a
//     column >= K or a row >= M; every (m, k) is gathered once per wave tile in N,
//   - every output element is stored exactly once, at its NCHW offset (found here from (m, n)),
//     the 16-B groups only where mxc_out_quad allows and all four offsets are consecutive.
// Output per (geometry, format, variant):
//   `ok <13 numbers> fmt <f> pw <0|1> M <M> K <K> reads <n> zeros <n> stores <n> quads <n> grid <n>`.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dfq_mx_conv_plan.h"

using namespace dfq;

namespace {

const int32_t kFormats[4] = {DFQ_MX_FP4_E2M1, DFQ_MX_FP6_E2M3, DFQ_MX_FP6_E3M2, DFQ_MX_FP8_E4M3};

#define FAIL(...) return fprintf(stderr, __VA_ARGS__), fprintf(stderr, "\n"), false

struct Shape {
    long long B, C, H, W, N, KH, KW, sh, sw, ph, pw, dh, dw;
};

// the im2col definition: the offset into x of A[m][k], or -1 for +0
long long definition(const Shape& s, long long OH, long long OW, long long m, long long k) {
    const long long ow = m % OW, oh = m / OW % OH, b = m / (OW * OH);
    const long long j = k % s.KW, i = k / s.KW % s.KH, c = k / (s.KW * s.KH);
    const long long ih = oh * s.sh - s.ph + i * s.dh, iw = ow * s.sw - s.pw + j * s.dw;
    if (ih < 0 || ih >= s.H || iw < 0 || iw >= s.W) return -1;
    return ((b * s.C + c) * s.H + ih) * s.W + iw;
}

template <bool PW>
bool walk(const Shape& s, int32_t fx, const MxcGeom& g, int64_t M, int64_t K, int64_t grid) {
    const int hw = mxg_hw_format(fx);
    const int n = mxl_part_len(hw);
    const long long xsize = s.B * s.C * s.H * s.W, osize = s.B * s.N * g.OH * g.OW;
    std::vector<float> x((size_t)xsize);
    for (long long i = 0; i < xsize; ++i) x[(size_t)i] = (float)(i + 1);
    std::vector<int> gathered((size_t)(M * K), 0), stored((size_t)osize, 0);
    long long reads = 0, zeros = 0, stores = 0, quads = 0;
    const int64_t steps = mxg_steps(mxg_blocks(K));
    for (int64_t block = 0; block < grid; ++block)
        for (int wave = 0; wave < kMxgWaves; ++wave) {
            const int64_t m0 = mxg_wave_m0(block, wave, s.N), n0 = mxg_wave_n0(block, wave, s.N);
            if (!mxg_wave_works(m0, n0, M, s.N)) continue;
            for (int lane = 0; lane < 64; ++lane)
                for (int sub = 0; sub < kMxgSub; ++sub) {
                    const int64_t m = mxg_lane_row(m0, sub, lane);
                    const MxcRow row = mxc_row(g, m, M);   // once, before the K loop
                    if (row.m != m || row.on != (m < M)) FAIL("row %lld", (long long)m);
                    for (int64_t step = 0; step < steps; ++step)
                        for (int part = 0; part < mxl_parts(hw); ++part) {
                            const int64_t k0 = mxl_part_k(hw, step, lane, part);
                            MxcTap t = mxc_tap<PW>(g, k0);
                            for (int e = 0; e < n; ++e) {
                                const int64_t k = k0 + e;
                                float v = 0.f;
                                if (mxc_reads<PW>(g, row, t, k, K)) {
                                    const int64_t off = mxc_x_offset(row, t);
                                    if (off < 0 || off >= xsize) FAIL("read of x at %lld for (m, k) = (%lld, %lld)", (long long)off, (long long)m, (long long)k);
                                    v = x[(size_t)off];
                                    ++reads;
                                } else {
                                    ++zeros;
                                }
                                const long long want = m < M && k < K ? definition(s, g.OH, g.OW, m, k) : -1;
                                if (v != (want < 0 ? 0.f : (float)(want + 1)))
                                    FAIL("(m, k) = (%lld, %lld): gathered %g, the definition reads x[%lld]", (long long)m, (long long)k, v, want);
                                if (m < M && k < K) ++gathered[(size_t)(m * K + k)];
                                mxc_next<PW>(g, t);
                            }
                        }
                }
            // MxmNchwStore::store
            for (int lane = 0; lane < 64; ++lane)
                for (int i = 0; i < kMxgSub; ++i) {
                    const int64_t m = mxg_out_row(m0, i, lane, 0);
                    const bool quad = mxc_out_quad(g, m, M);
                    for (int j = 0; j < kMxgSub; ++j) {
                        const int64_t col = mxg_out_col(n0, j, lane);
                        if (col >= s.N) continue;
                        for (int r = 0; r < 4; ++r) {
                            int64_t o;
                            if (quad) o = mxc_out_offset(g, m, col) + r;
                            else if (mxg_stores(m + r, col, M, s.N)) o = mxc_out_offset(g, m + r, col);
                            else continue;
                            const long long mm = m + r, b = mm / g.OHW, p = mm % g.OHW;
                            if (mm >= M || o != (b * s.N + col) * g.OHW + p || o < 0 || o >= osize)
                                FAIL("store of (m, n) = (%lld, %lld) at %lld", mm, (long long)col, (long long)o);
                            ++stored[(size_t)o];
                            ++stores;
                        }
                        quads += quad;
                    }
                }
        }
    const int tiles_n = (int)ceil_div(s.N, kMxgWaveTile);
    for (size_t i = 0; i < gathered.size(); ++i)
        if (gathered[i] != tiles_n) FAIL("(m, k) = (%lld, %lld) gathered %d times", (long long)(i / K), (long long)(i % K), gathered[i]);
    for (size_t i = 0; i < stored.size(); ++i)
        if (stored[i] != 1) FAIL("output element %lld stored %d times", (long long)i, stored[i]);
    printf("ok %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld fmt %d pw %d M %lld K %lld reads %lld zeros %lld stores %lld quads %lld grid %lld\n",
           s.B, s.C, s.H, s.W, s.N, s.KH, s.KW, s.sh, s.sw, s.ph, s.pw, s.dh, s.dw, fx, (int)PW, (long long)M, (long long)K, reads, zeros,
           stores, quads, (long long)grid);
    return true;
}

bool check(const Shape& s, int32_t fx) {
    dfq_mx_conv2d_desc d{};
    d.x = reinterpret_cast<const float*>((uintptr_t)0x10004);
    d.b_codes = reinterpret_cast<const void*>((uintptr_t)0x20010);
    d.b_scales = reinterpret_cast<const void*>((uintptr_t)0x30001);
    d.out = reinterpret_cast<float*>((uintptr_t)0x40004);
    d.B = s.B; d.C = s.C; d.H = s.H; d.W = s.W; d.N = s.N; d.KH = s.KH; d.KW = s.KW;
    d.stride_h = s.sh; d.stride_w = s.sw; d.pad_h = s.ph; d.pad_w = s.pw; d.dil_h = s.dh; d.dil_w = s.dw;
    d.x_format = fx; d.b_format = DFQ_MX_FP4_E2M1;
    MxcGeom g;
    int64_t M = 0, K = 0, grid = 0;
    if (mxc_check(&d, g, M, K, grid) != DFQ_OK) FAIL("mxc_check refuses a good descriptor");
    if (K != s.C * s.KH * s.KW || M != s.B * g.OH * g.OW || grid != mxg_grid(M, s.N) || grid < 1) FAIL("M, K or the grid");
    if (mxc_pointwise(g) != (s.KH == 1 && s.KW == 1 && s.ph == 0 && s.pw == 0 && s.dh == 1 && s.dw == 1)) FAIL("pointwise");
    if (!walk<false>(s, fx, g, M, K, grid)) return false;
    return !mxc_pointwise(g) || walk<true>(s, fx, g, M, K, grid);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return fprintf(stderr, "usage: %s shapes.txt\n", argv[0]), 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return perror(argv[1]), 2;
    Shape s;
    while (fscanf(f, "%lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld", &s.B, &s.C, &s.H, &s.W, &s.N, &s.KH, &s.KW, &s.sh,
                  &s.sw, &s.ph, &s.pw, &s.dh, &s.dw) == 13)
        for (int32_t fx : kFormats)
            if (!check(s, fx)) {
                fprintf(stderr, "geometry %lld %lld %lld %lld -> %lld, %lldx%lld, format %d\n", s.B, s.C, s.H, s.W, s.N, s.KH, s.KW, fx);
                fclose(f);
                return 1;
            }
    fclose(f);
    return 0;
}
