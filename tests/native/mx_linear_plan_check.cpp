// dfq_mx_linear's index arithmetic and per-lane quantizer on their own: dfq_mx_linear_plan.h /
// .cpp (with dfq_mx_encode.h compiled for the host) linked with this main and nothing else, so
// it runs under AddressSanitizer / UBSan on a machine without a GPU
// (tests/test_mx_linear_host.py builds and runs it).
//
//   mx_linear_plan_check shapes.txt [cases.bin out.bin]
//
// shapes.txt: lines `M N K`.  For every shape, each of the 16 (x_format, b_format) pairs and two
// placements of x (rows 16-B aligned with ldx = K rounded up to 4: the 16-B path when K % 4 == 0;
// a base one float past a 16-B boundary with ldx = K + 3: the 4-B path) it fills x -- an array of
// exactly (M - 1) * ldx + K floats, so the sanitizer sees any overrun too -- with blocks of
// random magnitude (exponents -30..30, all-zero blocks, -0, grid values that tie, values that
// saturate), quantizes it plainly on the host into the stored layout [M][nb][cb] / [M][nb]
// (host_quantize: block by block, element by element, dfq_mx_encode.h's encoder, the packing
// written from include/dfq_hip.h), then walks every (block, wave, K step, instruction tile,
// lane) through the header's helpers exactly as the kernel does and checks that
//   - every fp32 read lies inside [row * ldx, row * ldx + K) of a row < M, and a 16-B read is
//     16-B aligned,
//   - the lane's operand registers and scale byte -- its elements encoded by the header's
//     per-lane quantizer, the FP8 exchanges emulated by indexing the wave's lanes with
//     mxl_split_partner / mxl_split_scale_lane / mxl_split_scale_byte -- equal, byte for byte,
//     what dfq_mx_gemm's helpers (mxg_*) gather for that lane from the stored arrays,
//   - every output element is stored exactly once, inside [M][ldo], never past column N.
// Output per (shape, pair): `ok M N K x_format b_format reads <floats> frags <n> stores <n> grid <n>`.
//
// cases.bin: records {int32 format, int32 rows, int32 row_len, float x[rows * row_len]}; out.bin
// receives, per record, host_quantize's codes [rows][nb][cb] then scales [rows][nb]: the pytest
// compares them with the contract's statement, which ties the shared encoder to it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dfq_mx_linear_plan.h"

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

#define FAIL(...) return fprintf(stderr, __VA_ARGS__), fprintf(stderr, "\n"), false

// element e (0..31) of one stored block takes code c, as include/dfq_hip.h lays the codes out
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

template <int FMT>
void host_quantize_block(const float* x, int n, uint8_t* blk, uint8_t* scale) {
    float v[DFQ_MX_BLOCK] = {0};   // a partial block is padded with +0
    for (int e = 0; e < n; ++e) v[e] = x[e];
    uint32_t amax = 0;
    for (int e = 0; e < DFQ_MX_BLOCK; ++e) {
        const uint32_t b = mx_bits(v[e]) & 0x7fffffffu;
        if (b > amax) amax = b;
    }
    const int X = mx_exponent<FMT>(amax);
    *scale = (uint8_t)(X + 127);
    for (int e = 0; e < DFQ_MX_BLOCK; ++e) {
        float y;
        put_elem(FMT, blk, e, mx_encode<FMT>(v[e], pow2f(-X), pow2f(X), y));
    }
}

// x [rows][ldx] (row_len used) -> codes [rows][nb][cb], scales [rows][nb]
void host_quantize(int32_t f, const float* x, int64_t rows, int64_t row_len, int64_t ldx, std::vector<uint8_t>& codes,
                   std::vector<uint8_t>& scales) {
    const int64_t nb = mxg_blocks(row_len);
    const int cb = mxg_code_bytes(f);
    codes.assign((size_t)(rows * nb * cb), 0);
    scales.assign((size_t)(rows * nb), 0);
    for (int64_t r = 0; r < rows; ++r)
        for (int64_t b = 0; b < nb; ++b) {
            const float* src = x + r * ldx + b * DFQ_MX_BLOCK;
            const int n = (int)(row_len - b * DFQ_MX_BLOCK < DFQ_MX_BLOCK ? row_len - b * DFQ_MX_BLOCK : DFQ_MX_BLOCK);
            uint8_t* blk = &codes[(size_t)((r * nb + b) * cb)];
            uint8_t* sc = &scales[(size_t)(r * nb + b)];
            switch (f) {
                case DFQ_MX_FP4_E2M1: host_quantize_block<DFQ_MX_FP4_E2M1>(src, n, blk, sc); break;
                case DFQ_MX_FP6_E2M3: host_quantize_block<DFQ_MX_FP6_E2M3>(src, n, blk, sc); break;
                case DFQ_MX_FP6_E3M2: host_quantize_block<DFQ_MX_FP6_E3M2>(src, n, blk, sc); break;
                default: host_quantize_block<DFQ_MX_FP8_E4M3>(src, n, blk, sc); break;
            }
        }
}

// blocks of one magnitude each, with the values a quantizer can get wrong
void fill(std::vector<float>& x, int64_t M, int64_t K, int64_t ldx) {
    static const float grid[8] = {0.25f, 0.75f, 1.25f, 2.5f, 5.0f, 1.0625f, 1.99f, 7.99f};   // midpoints, near-saturating
    for (int64_t r = 0; r < M; ++r)
        for (int64_t b = 0; b * DFQ_MX_BLOCK < K; ++b) {
            const int kind = (int)(rnd() % 8);
            const float scale = pow2f((int)(rnd() % 61) - 30);
            for (int64_t k = b * DFQ_MX_BLOCK; k < K && k < (b + 1) * DFQ_MX_BLOCK; ++k) {
                float v;
                if (kind == 0) v = 0.f;
                else if (kind == 1) v = grid[rnd() % 8] * scale;
                else if (kind == 2) v = (k % DFQ_MX_BLOCK == (int64_t)(rnd() % 32)) ? scale : 0.f;
                else v = (float)((int)(rnd() % 2001) - 1000) * 1e-3f * scale;
                if (rnd() % 2) v = -v;   // -0 included
                x[(size_t)(r * ldx + k)] = v;
            }
        }
}

struct Stored {
    int32_t format;
    int64_t rows, nb;
    int cb;
    std::vector<uint8_t> codes, scales;
};

// what dfq_mx_gemm loads for the lane from the stored arrays (mx_gemm_plan_check's gather)
bool gather(const Stored& o, int64_t t0, int sub, int64_t step, int lane, uint8_t (&bytes)[32], int& s) {
    const int64_t row = mxg_lane_row(t0, sub, lane), kb = mxg_lane_kblock(step, lane);
    std::memset(bytes, 0, sizeof bytes);
    s = 127;
    const bool on = mxg_lane_loads(row, o.rows, kb, o.nb);
    if (on) s = o.scales[(size_t)mxg_scale_offset(row, kb, o.nb)];
    if (!mxg_hw_split(mxg_hw_format(o.format))) {
        if (on) std::memcpy(bytes, &o.codes[(size_t)mxg_code_offset(row, kb, o.nb, o.cb)], (size_t)o.cb);
    } else {
        for (int h = 0; h < 2; ++h) {
            const int64_t kh = mxg_split_kblock(step, lane, h);
            if (!mxg_lane_loads(row, o.rows, kh, o.nb)) continue;
            std::memcpy(bytes + kMxgHalfBytes * h, &o.codes[(size_t)mxg_split_code_offset(row, kh, o.nb, lane)], (size_t)kMxgHalfBytes);
        }
    }
    return true;
}

struct XView {
    const float* base;   // the array: exactly (M - 1) * ldx + K floats
    uintptr_t addr;      // the device address it stands for (alignment only)
    int64_t ldx, M, K;
    bool vec;
};

// the lane's 32 elements, read as the kernel reads them (mxl_load_x)
template <int HW>
bool load_x(const XView& x, int64_t row, int64_t step, int lane, float (&v)[DFQ_MX_BLOCK], long long& reads) {
    constexpr int n = mxl_part_len(HW);
    const int64_t size = (x.M - 1) * x.ldx + x.K;
    for (int part = 0; part < mxl_parts(HW); ++part) {
        const int64_t k0 = mxl_part_k(HW, step, lane, part);
        if (k0 % n) FAIL("run start %lld", (long long)k0);
        for (int q = 0; q < n; q += 4)
            for (int j = 0; j < 4; ++j) {
                const int64_t k = k0 + q + j;
                // 16-B path: the quad's first element decides for all four
                const bool reads_it = x.vec ? mxl_reads(row, x.M, k0 + q, x.K) : mxl_reads(row, x.M, k, x.K);
                float& o = v[n * part + q + j];
                o = 0.f;
                if (!reads_it) continue;
                const int64_t off = mxl_x_offset(row, k, x.ldx);
                if (row < 0 || row >= x.M || k < 0 || k >= x.K || off < row * x.ldx || off >= row * x.ldx + x.K || off >= size)
                    FAIL("read of x[%lld][%lld] (ldx %lld)", (long long)row, (long long)k, (long long)x.ldx);
                if (x.vec && j == 0 && (x.addr + 4 * (uintptr_t)off) % 16) FAIL("16-B read at float %lld is misaligned", (long long)off);
                o = x.base[off];
                ++reads;
            }
    }
    return true;
}

// One instruction tile's A operand of a wave, as the kernel builds it (mxl_quantize), against the stored codes.
template <int HW>
bool check_fragment(const XView& x, const Stored& st, int64_t m0, int sub, int64_t step, long long& reads) {
    static float v[64][DFQ_MX_BLOCK];
    uint32_t regs[64][8];
    int byte[64], b[64][2];
    uint32_t mine[64][2];
    for (int lane = 0; lane < 64; ++lane)
        if (!load_x<HW>(x, mxg_lane_row(m0, sub, lane), step, lane, v[lane], reads)) return false;
    std::memset(regs, 0, sizeof regs);
    if (!mxg_hw_split(HW)) {
        for (int lane = 0; lane < 64; ++lane) {
            byte[lane] = mxl_scale_byte<HW>(mxl_part_amax<HW>(v[lane], 0));
            mxl_encode_part<HW>(regs[lane], v[lane], 0, byte[lane]);
        }
    } else {
        for (int lane = 0; lane < 64; ++lane)
            for (int h = 0; h < 2; ++h) mine[lane][h] = mxl_part_amax<HW>(v[lane], h);
        for (int lane = 0; lane < 64; ++lane)
            for (int h = 0; h < 2; ++h) {
                const int p = mxl_split_partner(lane);
                if (p < 0 || p >= 64) FAIL("partner lane %d", p);
                const uint32_t other = mine[p][h];
                b[lane][h] = mxl_scale_byte<HW>(mine[lane][h] > other ? mine[lane][h] : other);
                mxl_encode_part<HW>(regs[lane], v[lane], h, b[lane][h]);
            }
        for (int lane = 0; lane < 64; ++lane) {
            const int src = mxl_split_scale_lane(lane), which = mxl_split_scale_byte(lane);
            if (src < 0 || src >= 64 || which < 0 || which > 1) FAIL("scale source lane %d byte %d", src, which);
            const uint32_t w = (uint32_t)b[src][0] | ((uint32_t)b[src][1] << 8);
            byte[lane] = (int)((w >> (8 * which)) & 0xFFu);
        }
    }
    for (int lane = 0; lane < 64; ++lane) {
        const int64_t row = mxg_lane_row(m0, sub, lane);
        const int s = mxg_lane_loads(row, x.M, mxg_lane_kblock(step, lane), st.nb) ? byte[lane] : 127;
        uint8_t want[32], got[32];
        int ws;
        gather(st, m0, sub, step, lane, want, ws);
        for (int i = 0; i < 8; ++i)
            for (int k = 0; k < 4; ++k) got[4 * i + k] = (uint8_t)(regs[lane][i] >> (8 * k));
        if (std::memcmp(want, got, 32) != 0 || ws != s) {
            int at = 0;
            while (at < 31 && want[at] == got[at]) ++at;
            FAIL("tile row %lld step %lld lane %d: scale byte %d (stored %d), first differing code byte %d: %02x (stored %02x)",
                 (long long)m0 + 16 * sub, (long long)step, lane, s, ws, at, got[at], want[at]);
        }
    }
    return true;
}

bool check_fragment_hw(int hw, const XView& x, const Stored& st, int64_t m0, int sub, int64_t step, long long& reads) {
    switch (hw) {
        case 0: return check_fragment<0>(x, st, m0, sub, step, reads);
        case 2: return check_fragment<2>(x, st, m0, sub, step, reads);
        case 3: return check_fragment<3>(x, st, m0, sub, step, reads);
        default: return check_fragment<4>(x, st, m0, sub, step, reads);
    }
}

bool check(int64_t M, int64_t N, int64_t K, int32_t fx, int32_t fb) {
    long long reads = 0, frags = 0, stores = 0;
    int64_t grid = 0;
    const int64_t ldo = N + 3;
    for (int placement = 0; placement < 2; ++placement) {
        const int64_t ldx = placement == 0 ? (K + 3) / 4 * 4 : K + 3;
        const uintptr_t addr = placement == 0 ? 0x10000 : 0x10004;
        std::vector<float> xdata((size_t)((M - 1) * ldx + K), 12345.f);
        fill(xdata, M, K, ldx);
        dfq_mx_linear_desc d{};
        d.x = reinterpret_cast<const float*>(addr);
        d.b_codes = reinterpret_cast<const void*>((uintptr_t)0x20008 + (mxg_code_align(fb) == 8 ? 0 : 8));
        d.b_scales = reinterpret_cast<const void*>((uintptr_t)0x30001);
        d.out = reinterpret_cast<float*>((uintptr_t)0x40004);
        d.ldx = ldx; d.ldo = ldo;
        d.M = M; d.N = N; d.K = K;
        d.x_format = fx; d.b_format = fb;
        if (mxl_check(&d, grid) != DFQ_OK) FAIL("mxl_check refuses a good descriptor");
        if (grid != mxg_grid(M, N) || grid < 1) FAIL("grid");
        XView x{xdata.data(), addr, ldx, M, K, mxl_vec(addr, ldx, K)};
        if (x.vec != (placement == 0 && K % 4 == 0)) FAIL("path choice");
        Stored st;
        st.format = fx;
        st.rows = M;
        st.nb = mxg_blocks(K);
        st.cb = mxg_code_bytes(fx);
        host_quantize(fx, xdata.data(), M, K, ldx, st.codes, st.scales);
        std::vector<int> stored((size_t)(M * ldo), 0);
        const int64_t steps = mxg_steps(st.nb);
        const int hw = mxg_hw_format(fx);
        for (int64_t block = 0; block < grid; ++block)
            for (int wave = 0; wave < kMxgWaves; ++wave) {
                const int64_t m0 = mxg_wave_m0(block, wave, N), n0 = mxg_wave_n0(block, wave, N);
                if (m0 % kMxgWaveTile || n0 % kMxgWaveTile) FAIL("tile origin");
                if (!mxg_wave_works(m0, n0, M, N)) continue;
                for (int64_t s = 0; s < steps; ++s)
                    for (int i = 0; i < kMxgSub; ++i) {
                        if (!check_fragment_hw(hw, x, st, m0, i, s, reads)) return false;
                        ++frags;
                    }
                if (placement) continue;
                for (int i = 0; i < kMxgSub; ++i)
                    for (int j = 0; j < kMxgSub; ++j)
                        for (int lane = 0; lane < 64; ++lane)
                            for (int reg = 0; reg < 4; ++reg) {
                                const int64_t row = mxg_out_row(m0, i, lane, reg), col = mxg_out_col(n0, j, lane);
                                if (!mxg_stores(row, col, M, N)) continue;
                                const int64_t o = mxg_out_offset(row, col, ldo);
                                if (o < 0 || o >= (int64_t)stored.size() || o % ldo >= N) FAIL("store at %lld", (long long)o);
                                ++stored[(size_t)o];
                                ++stores;
                            }
            }
        if (placement) continue;
        for (int64_t m = 0; m < M; ++m)
            for (int64_t n = 0; n < ldo; ++n)
                if (stored[(size_t)(m * ldo + n)] != (n < N ? 1 : 0))
                    FAIL("element (%lld, %lld) stored %d times", (long long)m, (long long)n, stored[(size_t)(m * ldo + n)]);
    }
    printf("ok %lld %lld %lld %d %d reads %lld frags %lld stores %lld grid %lld\n", (long long)M, (long long)N, (long long)K, fx, fb,
           reads, frags, stores, (long long)grid);
    return true;
}

bool encode_cases(const char* in, const char* out) {
    FILE* f = fopen(in, "rb");
    FILE* o = fopen(out, "wb");
    if (!f || !o) FAIL("cannot open %s / %s", in, out);
    int32_t head[3];
    long long n = 0;
    while (fread(head, sizeof head, 1, f) == 1) {
        if (mxg_hw_format(head[0]) < 0 || head[1] < 1 || head[2] < 1) FAIL("bad case header");
        std::vector<float> x((size_t)head[1] * (size_t)head[2]);
        if (fread(x.data(), sizeof(float), x.size(), f) != x.size()) FAIL("short case");
        std::vector<uint8_t> codes, scales;
        host_quantize(head[0], x.data(), head[1], head[2], head[2], codes, scales);
        fwrite(codes.data(), 1, codes.size(), o);
        fwrite(scales.data(), 1, scales.size(), o);
        ++n;
    }
    fclose(f);
    fclose(o);
    printf("cases %lld\n", n);
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2 && argc != 4) return fprintf(stderr, "usage: %s shapes.txt [cases.bin out.bin]\n", argv[0]), 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return perror(argv[1]), 2;
    long long M, N, K;
    while (fscanf(f, "%lld %lld %lld", &M, &N, &K) == 3)
        for (int32_t fx : kFormats)
            for (int32_t fb : kFormats)
                if (!check(M, N, K, fx, fb)) {
                    fprintf(stderr, "shape %lld %lld %lld formats %d %d\n", M, N, K, fx, fb);
                    fclose(f);
                    return 1;
                }
    fclose(f);
    if (argc == 4 && !encode_cases(argv[2], argv[3])) return 1;
    return 0;
}
