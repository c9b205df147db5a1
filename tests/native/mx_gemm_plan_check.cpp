// dfq_mx_gemm's index arithmetic on its own: dfq_mx_gemm_plan.h / .cpp linked with this
// main and nothing else, so it runs under AddressSanitizer / UBSan on a machine without a
// GPU (tests/test_mx_gemm_host.py builds and runs it).
// Input: a text file of lines `M N K`.  For every shape and each of the 16 format pairs it
// fills both operands with random valid codes (scale bytes 126..128, some all-zero blocks
// with scale byte 0, +0 codes past K), then walks every (block, wave, K step, lane) through
// the header's helpers exactly as the kernel does and checks that
//   - every byte range a lane reads lies inside its array (the arrays here are exactly
//     [rows][nb][cb] and [rows][nb], so the sanitizer sees any overrun too),
//   - every output element is stored exactly once, inside [M][ldo], never past column N,
//   - a host emulation of the instruction -- operands gathered through the helpers,
//     decoded with explicit tables, accumulated by the documented lane map (A and B: row
//     lane & 15, MX block lane >> 4; D: column lane & 15, row 4 * (lane >> 4) + reg; an
//     FP8 operand's elements in two passes of 64 as measured on the hardware,
//     dfq_mx_gemm_plan.h) --
//     equals the direct double-precision product of the directly decoded operands.  All
//     values are multiples of 2^-20 below 2^31, so both sums are exact and must be equal.
// Output per (shape, pair): `ok M N K a_format b_format reads <bytes> stores <n> grid <n>`.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dfq_mx_gemm_plan.h"

using namespace dfq;

namespace {

const int32_t kFormats[4] = {DFQ_MX_FP4_E2M1, DFQ_MX_FP6_E2M3, DFQ_MX_FP6_E3M2, DFQ_MX_FP8_E4M3};

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 32);
}

int elem_bits(int32_t f) { return f == DFQ_MX_FP4_E2M1 ? 4 : f == DFQ_MX_FP8_E4M3 ? 8 : 6; }

// the value of one code, from the formats' definitions
double decode(int32_t f, uint32_t c) {
    double mag;
    uint32_t sign;
    if (f == DFQ_MX_FP4_E2M1) {
        const uint32_t e = (c >> 1) & 3, m = c & 1;
        mag = e == 0 ? m * 0.5 : (2 + m) * (double)(1 << e) / 4.0;
        sign = c & 0x8;
    } else if (f == DFQ_MX_FP6_E2M3) {
        const uint32_t e = (c >> 3) & 3, m = c & 7;
        mag = e == 0 ? m / 8.0 : (8 + m) * (double)(1 << e) / 16.0;
        sign = c & 0x20;
    } else if (f == DFQ_MX_FP6_E3M2) {
        const uint32_t e = (c >> 2) & 7, m = c & 3;
        mag = e == 0 ? m / 16.0 : (4 + m) * (double)(1 << e) / 32.0;
        sign = c & 0x20;
    } else {
        const uint32_t e = (c >> 3) & 15, m = c & 7;
        mag = e == 0 ? m / 512.0 : (8 + m) * (double)(1 << e) / 1024.0;
        sign = c & 0x80;
    }
    return sign ? -mag : mag;
}
double scale_value(uint8_t s) { return s == 0 ? 0.0 : s == 126 ? 0.5 : s == 127 ? 1.0 : 2.0; }   // byte 0: only over zero codes

// element e (0..31) of one block's code bytes, as include/dfq_hip.h lays them out
uint32_t block_elem(int32_t f, const uint8_t* blk, int e) {
    if (f == DFQ_MX_FP4_E2M1) return (blk[e >> 1] >> (4 * (e & 1))) & 0xF;
    if (f == DFQ_MX_FP8_E4M3) return blk[e];
    const int bit = 6 * e;   // dense little-endian string
    const uint32_t w = blk[bit >> 3] | ((bit >> 3) + 1 < 24 ? (uint32_t)blk[(bit >> 3) + 1] << 8 : 0u);
    return (w >> (bit & 7)) & 0x3F;
}
void put_elem(int32_t f, uint8_t* blk, int e, uint32_t c) {
    if (f == DFQ_MX_FP4_E2M1) blk[e >> 1] |= (uint8_t)(c << (4 * (e & 1)));
    else if (f == DFQ_MX_FP8_E4M3) blk[e] = (uint8_t)c;
    else {
        const int bit = 6 * e;
        const uint32_t w = c << (bit & 7);
        blk[bit >> 3] |= (uint8_t)w;
        if (w >> 8) blk[(bit >> 3) + 1] |= (uint8_t)(w >> 8);
    }
}

struct Operand {
    int32_t format;
    int64_t rows, nb;
    int cb;
    std::vector<uint8_t> codes, scales;
    std::vector<double> direct;   // [rows][nb * 32], decoded without the helpers
};

Operand make_operand(int32_t f, int64_t rows, int64_t K) {
    Operand o;
    o.format = f;
    o.rows = rows;
    o.nb = mxg_blocks(K);
    o.cb = mxg_code_bytes(f);
    o.codes.assign((size_t)(rows * o.nb * o.cb), 0);
    o.scales.assign((size_t)(rows * o.nb), 0);
    o.direct.assign((size_t)(rows * o.nb * 32), 0.0);
    const uint32_t mask = (1u << elem_bits(f)) - 1;
    for (int64_t r = 0; r < rows; ++r)
        for (int64_t b = 0; b < o.nb; ++b) {
            uint8_t* blk = &o.codes[(size_t)((r * o.nb + b) * o.cb)];
            if (rnd() % 16 == 0) continue;   // an all-zero block: +0 codes, scale byte 0
            const uint8_t s = (uint8_t)(126 + rnd() % 3);
            o.scales[(size_t)(r * o.nb + b)] = s;
            for (int e = 0; e < 32; ++e) {
                if (b * 32 + e >= K) break;   // +0 padding
                uint32_t c = rnd() & mask;
                if (f == DFQ_MX_FP8_E4M3 && (c & 0x7F) == 0x7F) c ^= 1;   // no NaN code
                put_elem(f, blk, e, c);
                o.direct[(size_t)((r * o.nb + b) * 32 + e)] = decode(f, c) * scale_value(s);
            }
        }
    return o;
}

// One lane's operand of one instruction as the hardware sees it: 32 element slots (slot e
// is bits [w * e, w * e + w) of the registers, w the element width) and the scale register.
struct Fragment {
    double v[32];
    double scale;
};

#define FAIL(...) return fprintf(stderr, __VA_ARGS__), fprintf(stderr, "\n"), false

bool read_ok(const Operand& o, int64_t co, int nbytes) {
    if (co < 0 || co + nbytes > (int64_t)o.codes.size()) FAIL("code read [%lld, +%d) outside %zu", (long long)co, nbytes, o.codes.size());
    if (co % mxg_code_align(o.format)) FAIL("code read at %lld breaks the alignment", (long long)co);
    return true;
}

// The lane's fragment of K step `step` for instruction tile `sub`, loaded as the kernel loads it.
bool gather(const Operand& o, int64_t t0, int sub, int64_t step, int lane, Fragment& f, long long& reads) {
    const int64_t row = mxg_lane_row(t0, sub, lane), kb = mxg_lane_kblock(step, lane);
    uint8_t bytes[32] = {0};
    uint8_t s = 127;
    const bool on = mxg_lane_loads(row, o.rows, kb, o.nb);
    if (on) {
        const int64_t so = mxg_scale_offset(row, kb, o.nb);
        if (so < 0 || so >= (int64_t)o.scales.size()) FAIL("scale read %lld outside %zu", (long long)so, o.scales.size());
        s = o.scales[(size_t)so];
        reads += 1;
    }
    if (!mxg_hw_split(mxg_hw_format(o.format))) {
        if (on) {
            const int64_t co = mxg_code_offset(row, kb, o.nb, o.cb);
            if (!read_ok(o, co, o.cb)) return false;
            std::memcpy(bytes, &o.codes[(size_t)co], (size_t)o.cb);
            reads += o.cb;
        }
    } else {
        for (int h = 0; h < 2; ++h) {
            const int64_t kh = mxg_split_kblock(step, lane, h);
            if (!mxg_lane_loads(row, o.rows, kh, o.nb)) continue;
            const int64_t co = mxg_split_code_offset(row, kh, o.nb, lane);
            if (!read_ok(o, co, kMxgHalfBytes)) return false;
            std::memcpy(bytes + kMxgHalfBytes * h, &o.codes[(size_t)co], (size_t)kMxgHalfBytes);
            reads += kMxgHalfBytes;
        }
    }
    for (int e = 0; e < 32; ++e) f.v[e] = decode(o.format, block_elem(o.format, bytes, e));
    f.scale = scale_value(s);
    return true;
}

// The instruction on one tile: acc[lane][reg] += its 128 products.  K position k of an operand
// is the slot mxg_hw_slot of lane group mxg_hw_group (as measured on the hardware: FP8 in
// two passes of 64, FP6 / FP4 block by block) under lane group k / 32's scale.
void mfma(const Fragment* A, const Fragment* B, bool a8, bool b8, double (*acc)[4]) {
    for (int lane = 0; lane < 64; ++lane)
        for (int reg = 0; reg < 4; ++reg) {
            const int r = 4 * (lane >> 4) + reg, c = lane & 15;
            double sum = 0.0;
            for (int k = 0; k < 32 * kMxgStepBlocks; ++k) {
                const double a = A[r + 16 * mxg_hw_group(a8, k)].v[mxg_hw_slot(a8, k)] * A[r + 16 * (k / 32)].scale;
                const double b = B[c + 16 * mxg_hw_group(b8, k)].v[mxg_hw_slot(b8, k)] * B[c + 16 * (k / 32)].scale;
                sum += a * b;
            }
            acc[lane][reg] += sum;
        }
}

bool check(int64_t M, int64_t N, int64_t K, int32_t fa, int32_t fb) {
    const Operand A = make_operand(fa, M, K), B = make_operand(fb, N, K);
    const int64_t ldo = N + 3;
    dfq_mx_gemm_desc d{};
    d.a_codes = reinterpret_cast<const void*>((uintptr_t)0x10000);
    d.a_scales = d.b_scales = reinterpret_cast<const void*>((uintptr_t)0x30001);
    d.b_codes = reinterpret_cast<const void*>((uintptr_t)0x20008 + (mxg_code_align(fb) == 8 ? 0 : 8));
    d.out = reinterpret_cast<float*>((uintptr_t)0x40004);
    d.ldo = ldo;
    d.M = M; d.N = N; d.K = K;
    d.a_format = fa; d.b_format = fb;
    int64_t grid = 0;
    if (mxg_check(&d, grid) != DFQ_OK) FAIL("mxg_check refuses a good descriptor");
    if (grid != mxg_grid(M, N) || grid < 1) FAIL("grid");
    std::vector<double> out((size_t)(M * ldo), 0.0);
    std::vector<int> stored((size_t)(M * ldo), 0);
    const int64_t nb = A.nb, steps = mxg_steps(nb);
    long long reads = 0, stores = 0;
    const int hwa = mxg_hw_format(fa), hwb = mxg_hw_format(fb);
    const bool a8 = mxg_hw_split(hwa), b8 = mxg_hw_split(hwb);
    std::vector<Fragment> fa_(kMxgSub * 64), fb_(kMxgSub * 64);   // [instruction tile][lane]
    for (int64_t block = 0; block < grid; ++block)
        for (int wave = 0; wave < kMxgWaves; ++wave) {
            const int64_t m0 = mxg_wave_m0(block, wave, N), n0 = mxg_wave_n0(block, wave, N);
            if (m0 % kMxgWaveTile || n0 % kMxgWaveTile) FAIL("tile origin");
            if (!mxg_wave_works(m0, n0, M, N)) continue;
            double acc[kMxgSub][kMxgSub][64][4] = {};
            for (int64_t s = 0; s < steps; ++s) {
                for (int i = 0; i < kMxgSub; ++i)
                    for (int lane = 0; lane < 64; ++lane)
                        if (!gather(A, m0, i, s, lane, fa_[i * 64 + lane], reads) ||
                            !gather(B, n0, i, s, lane, fb_[i * 64 + lane], reads))
                            return false;
                for (int i = 0; i < kMxgSub; ++i)
                    for (int j = 0; j < kMxgSub; ++j) mfma(&fa_[i * 64], &fb_[j * 64], a8, b8, acc[i][j]);
            }
            for (int i = 0; i < kMxgSub; ++i)
                for (int j = 0; j < kMxgSub; ++j)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int reg = 0; reg < 4; ++reg) {
                            const int64_t row = mxg_out_row(m0, i, lane, reg), col = mxg_out_col(n0, j, lane);
                            if (!mxg_stores(row, col, M, N)) continue;
                            const int64_t o = mxg_out_offset(row, col, ldo);
                            if (o < 0 || o >= (int64_t)out.size() || o % ldo >= N) FAIL("store at %lld", (long long)o);
                            out[(size_t)o] = acc[i][j][lane][reg];
                            ++stored[(size_t)o];
                            ++stores;
                        }
        }
    for (int64_t m = 0; m < M; ++m)
        for (int64_t n = 0; n < ldo; ++n) {
            const int want = n < N ? 1 : 0;
            if (stored[(size_t)(m * ldo + n)] != want) FAIL("element (%lld, %lld) stored %d times", (long long)m, (long long)n, stored[(size_t)(m * ldo + n)]);
            if (n >= N) continue;
            double sum = 0.0;
            const double* a = &A.direct[(size_t)(m * nb * 32)];
            const double* b = &B.direct[(size_t)(n * nb * 32)];
            for (int64_t k = 0; k < nb * 32; ++k) sum += a[k] * b[k];
            if (sum != out[(size_t)(m * ldo + n)])
                FAIL("element (%lld, %lld): emulation %.17g, direct %.17g", (long long)m, (long long)n, out[(size_t)(m * ldo + n)], sum);
        }
    printf("ok %lld %lld %lld %d %d reads %lld stores %lld grid %lld\n", (long long)M, (long long)N, (long long)K, fa, fb, reads,
           stores, (long long)grid);
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return fprintf(stderr, "usage: %s shapes.txt\n", argv[0]), 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return perror(argv[1]), 2;
    long long M, N, K;
    while (fscanf(f, "%lld %lld %lld", &M, &N, &K) == 3)
        for (int32_t fa : kFormats)
            for (int32_t fb : kFormats)
                if (!check(M, N, K, fa, fb)) {
                    fprintf(stderr, "shape %lld %lld %lld formats %d %d\n", M, N, K, fa, fb);
                    fclose(f);
                    return 1;
                }
    fclose(f);
    return 0;
}
