// dfq_int_gemm's index arithmetic on its own: dfq_int_gemm_plan.h / .cpp linked with this
// main and nothing else, so it runs under AddressSanitizer / UBSan on a machine without a
// GPU (tests/test_int_gemm_host.py builds and runs it).
// Input: a text file of lines `M N K`.  For every shape and each (a_signed, b_signed, packed)
// mode (packed skips odd K) it fills both operands with random codes over the full byte or
// nibble range (row 0 all the largest code, row 1 all the smallest), then walks every
// (block, wave, K step, lane) through the header's helpers exactly as the kernel does -- the
// wide path where ig_wide(K), else the byte path -- and checks that
//   - every byte a lane reads lies inside its array (the arrays here are exactly [rows][K]
//     or [rows][K / 2], so the sanitizer sees any overrun too), and every fp32 element the
//     quantizing A source would read lies inside x[M][ldx] up to its last row's K-th element,
//   - every output element is stored exactly once, inside [M][ldo], never past column N,
//   - a host emulation of the instruction -- fragments gathered and moved to the signed
//     domain through the helpers, multiplied as signed bytes by the documented lane map (A and
//     B: row lane & 15, byte slot e of lane group lane >> 4 against the same slot of the same
//     group; D: column lane & 15, row 4 * (lane >> 4) + reg), the row sums against an
//     all-ones operand, int32 accumulators -- folded by ig_fold_p / ig_fold_s equals the
//     contract's integers P, Sa and Sb computed directly from the codes in int64.
// Output per (shape, mode): `ok M N K a_signed b_signed packed reads <bytes> stores <n> grid <n>`.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dfq_int_gemm_plan.h"

using namespace dfq;

namespace {

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 32);
}

int fail(const char* what, int64_t a = 0, int64_t b = 0, int64_t c = 0) {
    std::printf("FAIL %s %lld %lld %lld\n", what, (long long)a, (long long)b, (long long)c);
    return 1;
}

// rows x K integers over the code range, edge rows first
std::vector<int> make_codes(int64_t rows, int64_t K, bool is_signed, bool nibbles) {
    const int bits = nibbles ? 4 : 8;
    const int lo = is_signed ? -(1 << (bits - 1)) : 0, hi = is_signed ? (1 << (bits - 1)) - 1 : (1 << bits) - 1;
    std::vector<int> q((size_t)(rows * K));
    for (int64_t r = 0; r < rows; ++r)
        for (int64_t k = 0; k < K; ++k) q[(size_t)(r * K + k)] = r == 0 ? hi : r == 1 ? lo : lo + (int)(rnd() % (uint32_t)(hi - lo + 1));
    return q;
}
std::vector<uint8_t> to_bytes(const std::vector<int>& q, bool packed) {
    std::vector<uint8_t> b(packed ? q.size() / 2 : q.size());
    for (size_t i = 0; i < q.size(); ++i) {
        if (packed) b[i / 2] = (uint8_t)(b[i / 2] | ((q[i] & 0xF) << (4 * (i & 1))));
        else b[i] = (uint8_t)q[i];
    }
    return b;
}

struct Operand {
    const std::vector<uint8_t>* bytes;
    int64_t rows;
    bool is_signed, packed;
};

// A lane's fragment as the kernel's loaders build it; false on a read outside the array.
bool gather(const Operand& o, int64_t row, int64_t K, int64_t step, int lane, uint32_t (&word)[4], int64_t& reads) {
    const int64_t k0 = ig_lane_k0(step, lane);
    const int nv = ig_lane_valid(row, o.rows, k0, K);
    const int64_t size = (int64_t)o.bytes->size();
    uint32_t raw[4] = {0, 0, 0, 0};
    if (nv != 0) {
        const int64_t off = o.packed ? ig_packed_offset(row, k0, K) : ig_byte_offset(row, k0, K);
        const int n = ig_wide(K) ? (o.packed ? kIgLaneK / 2 : kIgLaneK) : (o.packed ? ig_packed_bytes(nv) : nv);
        if (ig_wide(K) && nv != kIgLaneK) return false;                     // the wide path holds all or none
        if (ig_wide(K) && off % (o.packed ? 8 : 16) != 0) return false;     // and its loads are aligned
        if (o.packed && (nv % 2 != 0 || k0 % 2 != 0)) return false;
        if (off < 0 || off + n > size) return false;
        for (int e = 0; e < n; ++e) raw[e >> 2] |= (uint32_t)(*o.bytes)[(size_t)(off + e)] << (8 * (e & 3));
        reads += n;
    }
    const uint32_t xm = ig_xor_mask(o.is_signed);
    for (int j = 0; j < 4; ++j) {
        uint32_t w = raw[j];
        if (o.packed) {
            const uint32_t pw[2] = {raw[0], raw[1]};
            w = ig_unpack4(pw, j, o.is_signed);
        }
        word[j] = ig_operand_word(w, xm, nv, j);
    }
    return true;
}

int slot(const uint32_t (&word)[4], int e) { return (int)(int8_t)((word[e >> 2] >> (8 * (e & 3))) & 0xFF); }

int run(int64_t M, int64_t N, int64_t K, bool a_signed, bool b_signed, bool packed) {
    const std::vector<int> qa = make_codes(M, K, a_signed, false), qb = make_codes(N, K, b_signed, packed);
    const std::vector<uint8_t> ab = to_bytes(qa, false), bb = to_bytes(qb, packed);
    const Operand A{&ab, M, a_signed, false}, B{&bb, N, b_signed, packed};
    const int64_t ldo = N + 3, ldx = K + 5;
    std::vector<uint8_t> stored((size_t)(M * ldo), 0);
    std::vector<int64_t> Sa((size_t)M, 0), Sb((size_t)N, 0);
    for (int64_t m = 0; m < M; ++m)
        for (int64_t k = 0; k < K; ++k) Sa[(size_t)m] += qa[(size_t)(m * K + k)];
    for (int64_t n = 0; n < N; ++n)
        for (int64_t k = 0; k < K; ++k) Sb[(size_t)n] += qb[(size_t)(n * K + k)];
    const int oa = ig_offset(a_signed), ob = ig_offset(b_signed);
    const int64_t grid = mxg_grid(M, N), steps = ig_steps(K), x_size = (M - 1) * ldx + K;
    int64_t reads = 0, stores = 0;
    for (int64_t block = 0; block < grid; ++block)
        for (int wave = 0; wave < kMxgWaves; ++wave) {
            const int64_t m0 = mxg_wave_m0(block, wave, N), n0 = mxg_wave_n0(block, wave, N);
            if (!mxg_wave_works(m0, n0, M, N)) continue;
            // accumulators of the wave tile by (row, column) of the tile; the row sums likewise
            static int32_t acc[kMxgWaveTile][kMxgWaveTile], ra[kMxgWaveTile], rb[kMxgWaveTile];
            std::memset(acc, 0, sizeof acc);
            std::memset(ra, 0, sizeof ra);
            std::memset(rb, 0, sizeof rb);
            for (int64_t s = 0; s < steps; ++s) {
                // [sub][row of the instruction tile][K position of the step]
                static int8_t fa[kMxgSub][kMxgMfma][kIgStepK], fb[kMxgSub][kMxgMfma][kIgStepK];
                for (int sub = 0; sub < kMxgSub; ++sub)
                    for (int lane = 0; lane < kWave; ++lane) {
                        uint32_t wa[4], wb[4];
                        const int64_t arow = mxg_lane_row(m0, sub, lane), brow = mxg_lane_row(n0, sub, lane);
                        if (!gather(A, arow, K, s, lane, wa, reads)) return fail("A read", arow, s, lane);
                        if (!gather(B, brow, K, s, lane, wb, reads)) return fail("B read", brow, s, lane);
                        // the fp32 A source's reads of the same lane
                        const int64_t k0 = ig_lane_k0(s, lane);
                        const int nv = ig_lane_valid(arow, M, k0, K);
                        for (int e = 0; e < nv; ++e) {
                            const int64_t off = ig_x_offset(arow, k0 + e, ldx);
                            if (off < 0 || off >= x_size) return fail("x read", arow, k0 + e, off);
                        }
                        for (int e = 0; e < kIgLaneK; ++e) {
                            fa[sub][lane & 15][kIgLaneK * (lane >> 4) + e] = (int8_t)slot(wa, e);
                            fb[sub][lane & 15][kIgLaneK * (lane >> 4) + e] = (int8_t)slot(wb, e);
                        }
                    }
                for (int i = 0; i < kMxgWaveTile; ++i) {
                    const int8_t* a = fa[i / kMxgMfma][i % kMxgMfma];
                    for (int k = 0; k < kIgStepK; ++k) ra[i] += a[k];
                    for (int j = 0; j < kMxgWaveTile; ++j) {
                        const int8_t* b = fb[j / kMxgMfma][j % kMxgMfma];
                        int32_t t = 0;
                        for (int k = 0; k < kIgStepK; ++k) t += (int32_t)a[k] * (int32_t)b[k];
                        acc[i][j] += t;
                    }
                }
                for (int j = 0; j < kMxgWaveTile; ++j) {
                    const int8_t* b = fb[j / kMxgMfma][j % kMxgMfma];
                    for (int k = 0; k < kIgStepK; ++k) rb[j] += b[k];
                }
            }
            for (int sub_n = 0; sub_n < kMxgSub; ++sub_n)
                for (int sub_m = 0; sub_m < kMxgSub; ++sub_m)
                    for (int lane = 0; lane < kWave; ++lane)
                        for (int reg = 0; reg < 4; ++reg) {
                            const int64_t row = mxg_out_row(m0, sub_m, lane, reg), col = mxg_out_col(n0, sub_n, lane);
                            if (!mxg_stores(row, col, M, N)) continue;
                            const int64_t off = mxg_out_offset(row, col, ldo);
                            if (off < 0 || off >= M * ldo || col >= N) return fail("store", row, col, off);
                            if (stored[(size_t)off]++) return fail("stored twice", row, col, off);
                            ++stores;
                            const int ti = (int)(row - m0), tj = (int)(col - n0);
                            int64_t P = 0;
                            for (int64_t k = 0; k < K; ++k) P += (int64_t)qa[(size_t)(row * K + k)] * qb[(size_t)(col * K + k)];
                            if (ig_fold_p(acc[ti][tj], ra[ti], rb[tj], oa, ob, K) != P) return fail("P", row, col, P);
                            if (ig_fold_s(ra[ti], oa, K) != Sa[(size_t)row]) return fail("Sa", row, col, Sa[(size_t)row]);
                            if (ig_fold_s(rb[tj], ob, K) != Sb[(size_t)col]) return fail("Sb", row, col, Sb[(size_t)col]);
                            if (P < INT32_MIN || P > INT32_MAX) return fail("P leaves int32", row, col, P);
                        }
        }
    for (int64_t m = 0; m < M; ++m)
        for (int64_t n = 0; n < ldo; ++n)
            if (stored[(size_t)(m * ldo + n)] != (n < N ? 1 : 0)) return fail("store count", m, n);
    std::printf("ok %lld %lld %lld %d %d %d reads %lld stores %lld grid %lld\n", (long long)M, (long long)N, (long long)K, (int)a_signed,
                (int)b_signed, (int)packed, (long long)reads, (long long)stores, (long long)grid);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    long long M, N, K;
    int rc = 0;
    while (rc == 0 && std::fscanf(f, "%lld %lld %lld", &M, &N, &K) == 3) {
        // the argument checks agree with the shape
        dfq_int_gemm_desc d{};
        d.a_codes = d.b_codes = reinterpret_cast<const void*>(0x1000);
        d.a_scale = d.b_scale = reinterpret_cast<const float*>(0x2000);
        d.out = reinterpret_cast<float*>(0x3000);
        d.M = M; d.N = N; d.K = K; d.ldo = N + 3;
        int64_t grid = 0;
        if (ig_check(&d, grid) != DFQ_OK || grid != mxg_grid(M, N)) rc = fail("ig_check", M, N, K);
        for (int mode = 0; mode < 8 && rc == 0; ++mode) {
            if ((mode & 4) && K % 2) continue;
            rc = run(M, N, K, (mode & 1) != 0, (mode & 2) != 0, (mode & 4) != 0);
        }
    }
    std::fclose(f);
    return rc;
}
