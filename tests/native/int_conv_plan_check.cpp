// dfq_int_conv2d's index arithmetic on its own: dfq_int_conv_plan.h / .cpp (with the headers it
// builds on and dfq_mx_conv_plan.cpp) linked with this main and nothing else, so it runs under
// AddressSanitizer / UBSan on a machine without a GPU (tests/test_int_conv_host.py builds and
// runs it).
//
//   int_conv_plan_check shapes.txt
//
// shapes.txt: lines `B C H W N KH KW sh sw ph pw dh dw`.  For every geometry, each kernel variant
// that may run it -- the general gather with the mask operand; without it where the geometry has
// no padding; the pointwise variant where it is pointwise -- and each (x_symmetric, b_signed),
// x is an array of exactly B * C * H * W floats holding its own index + 1, the codes of both
// operands are random over the full byte range, and the program walks every (block, wave, K
// step, instruction tile, lane) through the headers' helpers exactly as the kernel does
// (IgConvA::fetch / operand / mask, the epilogue, IgNchwStore::store) and checks that
//   - every read lies inside x,
//   - the element a lane gathers for (m, k) and its mask bit are the im2col definition's -- found
//     here from m and k with plain divisions, sharing nothing with the helpers -- and +0 / a clear
//     bit for a padding tap, a column >= K or a row >= M; every (m, k) is gathered once per wave
//     tile in N,
//   - a host emulation of the instruction over the fragments as the helpers build them (an
//     element whose bit is clear carries a junk code before igc_operand_word, so only the mask can
//     remove it), with int32 accumulators for the four products, the two a' row sums and the
//     four mask x b' (or two ones x b') sums, folded by igc_fold_p / igc_fold_s with T =
//     igc_taps(row) (K without the mask), equals the contract's P, Sa, Sb and T computed directly
//     from the codes and the definition's v in int64,
//   - every output element is stored exactly once, at its NCHW offset (found here from (m, n)),
//     the 16-B groups only where mxc_out_quad allows and all four offsets are consecutive.
// Output per (geometry, variant, signs):
//   `ok <13 numbers> pw <0|1> mask <0|1> xs <0|1> bs <0|1> M <M> K <K> reads <n> zeros <n> taps <n> stores <n> quads <n> grid <n>`.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dfq_int_conv_plan.h"

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
    long long B, C, H, W, N, KH, KW, sh, sw, ph, pw, dh, dw;
};

// the im2col definition: the offset into x of A[m][k], or -1 for a padding tap
long long definition(const Shape& s, long long OH, long long OW, long long m, long long k) {
    const long long ow = m % OW, oh = m / OW % OH, b = m / (OW * OH);
    const long long j = k % s.KW, i = k / s.KW % s.KH, c = k / (s.KW * s.KH);
    const long long ih = oh * s.sh - s.ph + i * s.dh, iw = ow * s.sw - s.pw + j * s.dw;
    if (ih < 0 || ih >= s.H || iw < 0 || iw >= s.W) return -1;
    return ((b * s.C + c) * s.H + ih) * s.W + iw;
}

int slot(const uint32_t (&word)[4], int e) { return (int)(int8_t)((word[e >> 2] >> (8 * (e & 3))) & 0xFF); }

template <bool PW, bool MASK>
bool walk(const Shape& s, const MxcGeom& g, int64_t M, int64_t K, int64_t grid, bool x_sym, bool b_signed) {
    const long long xsize = s.B * s.C * s.H * s.W, osize = s.B * s.N * g.OH * g.OW;
    std::vector<float> x((size_t)xsize);
    for (long long i = 0; i < xsize; ++i) x[(size_t)i] = (float)(i + 1);
    // codes over the full byte range; v and the contract's integers straight from the definition
    std::vector<int> qa((size_t)(M * K)), qb((size_t)(s.N * K)), v((size_t)(M * K));
    const int alo = x_sym ? -128 : 0, blo = b_signed ? -128 : 0;
    for (auto& q : qa) q = alo + (int)(rnd() % 256u);
    for (auto& q : qb) q = blo + (int)(rnd() % 256u);
    for (int64_t k = 0; k < K && M > 0; ++k) qa[(size_t)k] = alo + 255;          // row 0: the largest code
    for (int64_t k = 0; k < K; ++k) qb[(size_t)k] = s.N > 1 ? blo : blo + 255;  // B's row 0: the smallest (or largest)
    std::vector<int64_t> Sa((size_t)M, 0), T((size_t)M, 0);
    long long taps = 0;
    for (int64_t m = 0; m < M; ++m)
        for (int64_t k = 0; k < K; ++k) {
            const int on = definition(s, g.OH, g.OW, m, k) >= 0;
            v[(size_t)(m * K + k)] = on;
            Sa[(size_t)m] += on * qa[(size_t)(m * K + k)];
            T[(size_t)m] += on;
            taps += on;
        }
    if (!MASK && taps != M * K) FAIL("the unmasked variant on a geometry with padding taps");
    const int oa = ig_offset(x_sym), ob = ig_offset(b_signed);
    const uint32_t xa = ig_xor_mask(x_sym), xb = ig_xor_mask(b_signed);
    std::vector<int> gathered((size_t)(M * K), 0), stored((size_t)osize, 0);
    long long reads = 0, zeros = 0, stores = 0, quads = 0;
    const int64_t steps = ig_steps(K);
    for (int64_t block = 0; block < grid; ++block)
        for (int wave = 0; wave < kMxgWaves; ++wave) {
            const int64_t m0 = mxg_wave_m0(block, wave, s.N), n0 = mxg_wave_n0(block, wave, s.N);
            if (!mxg_wave_works(m0, n0, M, s.N)) continue;
            static int32_t acc[kMxgWaveTile][kMxgWaveTile], ra[kMxgWaveTile], rb[kMxgWaveTile], rbm[kMxgWaveTile][kMxgWaveTile];
            std::memset(acc, 0, sizeof acc);
            std::memset(ra, 0, sizeof ra);
            std::memset(rb, 0, sizeof rb);
            std::memset(rbm, 0, sizeof rbm);
            for (int64_t step = 0; step < steps; ++step) {
                // [sub][row of the instruction tile][K position of the step]
                static int8_t fa[kMxgSub][kMxgMfma][kIgStepK], fm[kMxgSub][kMxgMfma][kIgStepK], fb[kMxgSub][kMxgMfma][kIgStepK];
                for (int sub = 0; sub < kMxgSub; ++sub)
                    for (int lane = 0; lane < kWave; ++lane) {
                        // IgConvA::fetch
                        const int64_t m = mxg_lane_row(m0, sub, lane);
                        const MxcRow row = mxc_row(g, m, M);   // the kernel makes it once, before the K loop
                        if (row.m != m || row.on != (m < M)) FAIL("row %lld", (long long)m);
                        const int64_t k0 = ig_lane_k0(step, lane);
                        MxcTap t = mxc_tap<PW>(g, k0);
                        uint32_t mask = 0, raw[4] = {0, 0, 0, 0};
                        for (int e = 0; e < kIgLaneK; ++e) {
                            const int64_t k = k0 + e;
                            const uint32_t bit = igc_mask_bit<PW>(g, row, t, k, K, e);
                            float val = 0.f;
                            if (bit) {
                                const int64_t off = mxc_x_offset(row, t);
                                if (off < 0 || off >= xsize) FAIL("read of x at %lld for (m, k) = (%lld, %lld)", (long long)off, (long long)m, (long long)k);
                                val = x[(size_t)off];
                                ++reads;
                            } else {
                                ++zeros;
                            }
                            if (bit != 0 && bit != 1u << e) FAIL("mask bit %d", e);
                            mask |= bit;
                            const long long want = m < M && k < K ? definition(s, g.OH, g.OW, m, k) : -1;
                            if (val != (want < 0 ? 0.f : (float)(want + 1)) || (bit != 0) != (want >= 0))
                                FAIL("(m, k) = (%lld, %lld): gathered %g, bit %u, the definition reads x[%lld]", (long long)m, (long long)k, val, bit, want);
                            if (m < M && k < K) ++gathered[(size_t)(m * K + k)];
                            // the code of the element; where there is none, a junk byte that only the mask removes
                            const int code = want >= 0 ? qa[(size_t)(m * K + k)] : 0x5A;
                            raw[e >> 2] |= (uint32_t)(code & 0xFF) << (8 * (e & 3));
                            mxc_next<PW>(g, t);
                        }
                        // IgConvA::operand / mask
                        uint32_t wa[4], wm[4], wb[4];
                        for (int j = 0; j < 4; ++j) {
                            wa[j] = igc_operand_word(raw[j], xa, mask, j);
                            wm[j] = igc_ones_word(mask, j);
                        }
                        // B: the stored bytes of row n, IgBytesB's
                        const int64_t n = mxg_lane_row(n0, sub, lane);
                        const int nv = ig_lane_valid(n, s.N, k0, K);
                        uint32_t rawb[4] = {0, 0, 0, 0};
                        for (int e = 0; e < nv; ++e) rawb[e >> 2] |= (uint32_t)(qb[(size_t)(ig_byte_offset(n, k0 + e, K))] & 0xFF) << (8 * (e & 3));
                        for (int j = 0; j < 4; ++j) wb[j] = ig_operand_word(rawb[j], xb, nv, j);
                        for (int e = 0; e < kIgLaneK; ++e) {
                            const int kk = kIgLaneK * (lane >> 4) + e;
                            fa[sub][lane & 15][kk] = (int8_t)slot(wa, e);
                            fm[sub][lane & 15][kk] = (int8_t)slot(wm, e);
                            fb[sub][lane & 15][kk] = (int8_t)slot(wb, e);
                            if (slot(wm, e) != (int)((mask >> e) & 1u)) FAIL("mask byte %d", e);
                        }
                    }
                // the step's instructions: a x b, a x ones, and mask x b (MASK) or ones x b
                for (int i = 0; i < kMxgWaveTile; ++i) {
                    const int8_t *a = fa[i / kMxgMfma][i % kMxgMfma], *mk = fm[i / kMxgMfma][i % kMxgMfma];
                    for (int k = 0; k < kIgStepK; ++k) ra[i] += a[k];
                    for (int j = 0; j < kMxgWaveTile; ++j) {
                        const int8_t* b = fb[j / kMxgMfma][j % kMxgMfma];
                        int32_t p = 0, q = 0;
                        for (int k = 0; k < kIgStepK; ++k) {
                            p += (int32_t)a[k] * (int32_t)b[k];
                            q += (int32_t)mk[k] * (int32_t)b[k];
                        }
                        acc[i][j] += p;
                        rbm[i][j] += q;
                    }
                }
                for (int j = 0; j < kMxgWaveTile; ++j) {
                    const int8_t* b = fb[j / kMxgMfma][j % kMxgMfma];
                    for (int k = 0; k < kIgStepK; ++k) rb[j] += b[k];
                }
            }
            // the epilogue and IgNchwStore::store
            for (int lane = 0; lane < kWave; ++lane)
                for (int i = 0; i < kMxgSub; ++i) {
                    const int64_t m = mxg_out_row(m0, i, lane, 0);
                    const bool quad = mxc_out_quad(g, m, M);
                    for (int j = 0; j < kMxgSub; ++j) {
                        const int64_t col = mxg_out_col(n0, j, lane);
                        if (col >= s.N) continue;
                        for (int r = 0; r < 4; ++r) {
                            const int64_t row = mxg_out_row(m0, i, lane, r);
                            if (row != m + r) FAIL("a lane's four rows are not consecutive");
                            if (mxg_stores(row, col, M, s.N)) {
                                const int64_t Tr = MASK ? igc_taps(g, mxc_row(g, row, M)) : K;
                                if (Tr != T[(size_t)row]) FAIL("T of row %lld: %lld, the mask's row sum is %lld", (long long)row, (long long)Tr, (long long)T[(size_t)row]);
                                const int ti = (int)(row - m0), tj = (int)(col - n0);
                                const int32_t rbv = MASK ? rbm[ti][tj] : rb[tj];
                                int64_t P = 0, Sb = 0;
                                for (int64_t k = 0; k < K; ++k) {
                                    const int64_t on = v[(size_t)(row * K + k)], b = qb[(size_t)(col * K + k)];
                                    P += on * qa[(size_t)(row * K + k)] * b;
                                    Sb += on * b;
                                }
                                if (igc_fold_p(acc[ti][tj], ra[ti], rbv, oa, ob, Tr) != P) FAIL("P of (%lld, %lld)", (long long)row, (long long)col);
                                if (igc_fold_s(ra[ti], oa, Tr) != Sa[(size_t)row]) FAIL("Sa of row %lld", (long long)row);
                                if (igc_fold_s(rbv, ob, Tr) != Sb) FAIL("Sb of (%lld, %lld)", (long long)row, (long long)col);
                                if (P < INT32_MIN || P > INT32_MAX) FAIL("P leaves int32");
                            }
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
    printf("ok %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld pw %d mask %d xs %d bs %d M %lld K %lld reads %lld zeros %lld taps %lld stores %lld quads %lld grid %lld\n",
           s.B, s.C, s.H, s.W, s.N, s.KH, s.KW, s.sh, s.sw, s.ph, s.pw, s.dh, s.dw, (int)PW, (int)MASK, (int)x_sym, (int)b_signed,
           (long long)M, (long long)K, reads, zeros, taps, stores, quads, (long long)grid);
    return true;
}

bool check(const Shape& s) {
    dfq_int_conv2d_desc d{};
    d.x = reinterpret_cast<const float*>((uintptr_t)0x10004);
    d.b_codes = reinterpret_cast<const void*>((uintptr_t)0x20010);
    d.b_scale = reinterpret_cast<const float*>((uintptr_t)0x30004);
    d.out = reinterpret_cast<float*>((uintptr_t)0x40004);
    d.B = s.B; d.C = s.C; d.H = s.H; d.W = s.W; d.N = s.N; d.KH = s.KH; d.KW = s.KW;
    d.stride_h = s.sh; d.stride_w = s.sw; d.pad_h = s.ph; d.pad_w = s.pw; d.dil_h = s.dh; d.dil_w = s.dw;
    d.x_bits = 8;
    MxcGeom g;
    int64_t M = 0, K = 0, grid = 0;
    if (igc_check(&d, g, M, K, grid) != DFQ_OK) FAIL("igc_check refuses a good descriptor");
    if (K != s.C * s.KH * s.KW || M != s.B * g.OH * g.OW || grid != mxg_grid(M, s.N) || grid < 1) FAIL("M, K or the grid");
    if (igc_masked(g) != (s.ph != 0 || s.pw != 0)) FAIL("igc_masked");
    // the geometry is the MX convolution's: one shared check
    dfq_mx_conv2d_desc dm{};
    dm.x = d.x; dm.b_codes = d.b_codes; dm.b_scales = d.b_codes; dm.out = d.out;
    dm.B = s.B; dm.C = s.C; dm.H = s.H; dm.W = s.W; dm.N = s.N; dm.KH = s.KH; dm.KW = s.KW;
    dm.stride_h = s.sh; dm.stride_w = s.sw; dm.pad_h = s.ph; dm.pad_w = s.pw; dm.dil_h = s.dh; dm.dil_w = s.dw;
    dm.x_format = DFQ_MX_FP8_E4M3; dm.b_format = DFQ_MX_FP4_E2M1;
    MxcGeom gm;
    int64_t Mm = 0, Km = 0, gridm = 0;
    if (mxc_check(&dm, gm, Mm, Km, gridm) != DFQ_OK || Mm != M || Km != K || gridm != grid || std::memcmp(&gm, &g, sizeof g) != 0)
        FAIL("mxc_check and igc_check disagree on the geometry");
    for (int mode = 0; mode < 4; ++mode) {
        const bool xs = (mode & 1) != 0, bs = (mode & 2) != 0;
        if (!walk<false, true>(s, g, M, K, grid, xs, bs)) return false;
        if (!igc_masked(g) && !walk<false, false>(s, g, M, K, grid, xs, bs)) return false;
        if (mxc_pointwise(g) && !walk<true, false>(s, g, M, K, grid, xs, bs)) return false;
    }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return fprintf(stderr, "usage: %s shapes.txt\n", argv[0]), 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return perror(argv[1]), 2;
    Shape s;
    while (fscanf(f, "%lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld", &s.B, &s.C, &s.H, &s.W, &s.N, &s.KH, &s.KW, &s.sh,
                  &s.sw, &s.ph, &s.pw, &s.dh, &s.dw) == 13)
        if (!check(s)) {
            fprintf(stderr, "geometry %lld %lld %lld %lld -> %lld, %lldx%lld\n", s.B, s.C, s.H, s.W, s.N, s.KH, s.KW);
            fclose(f);
            return 1;
        }
    fclose(f);
    return 0;
}
