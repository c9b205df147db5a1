// dfq_int_gemm, dfq_int_linear and dfq_int_conv2d: out[m][n] = sum_k A[m][k] * B[n][k] (+ bias[n])
// of the affine values A = qa * sa + za, B = qb * sb[n] + zb[n] that the sweep's integer codes
// stand for, on the integer matrix instruction v_mfma_i32_16x16x64_i8 (include/dfq_hip.h;
// DESIGN.md 3.9).  One kernel template over how a lane obtains the 16 bytes of its A fragment --
// stored codes (dfq_int_gemm), fp32 x quantized on the way (dfq_int_linear: dfq_fake_quant_given's
// quantizer, the code being its q), or the im2col rows of an NCHW x gathered and quantized on the
// way (dfq_int_conv2d) -- of its B fragment: 16 stored bytes, or 8 packed bytes widened -- and
// over where the result goes: row-major, or NCHW.
//
// The convolution pads with the real value 0: a padding tap is absent from every sum (0 in the
// signed domain), so sum_k b' over the taps inside the image depends on the output row.  Where
// the geometry has padding the two ones x B-fragment instructions become four mask x B-fragment
// instructions (the mask operand holds 0x01 where the tap is inside), ten a step, and the folds
// take T[m] = sum_k v, a closed form of the row's position, where they had K
// (dfq_int_conv_plan.h).
//
// All addressing and every bit operation on a fragment is dfq_int_gemm_plan.h's (the convolution's:
// dfq_mx_conv_plan.h's and dfq_int_conv_plan.h's); the tiling is
// dfq_mx_gemm's: a wave owns a 32 x 32 output tile, so each of its two A and two B fragments of a
// K step (64 elements) feeds two product instructions, and four waves make a 64 x 64 block.  The
// instruction multiplies signed bytes.  An unsigned code q enters as q - 128 (xor 0x80); elements
// at k >= K and rows past M / N enter as 0 in that domain.  Next to the four products a step
// issues four more instructions against an all-ones operand: A-fragment x ones leaves sum_k a' in
// every column of C -- already in the lane and register that stores that row -- and ones x
// B-fragment leaves sum_k b' in every row.  The epilogue folds the two offsets back in integers
// (ig_fold_p / ig_fold_s: the contract's P, Sa and Sb, exact) and then runs the contract's fp64
// steps in its order; the library builds with -ffp-contract=off.  No LDS, no workspace, no
// atomics, no split of K: an output element is one accumulator of one lane, K steps in order.
//
// K % 16 == 0: a lane's bytes are one aligned 16-B (packed: 8-B) load and all exist or none do.
// Otherwise: guarded byte loads into the same words.  fp32 A: 16-B loads where x's rows allow
// (ig_x_vec), else 4-B loads.  The A fragment of dfq_int_linear is re-quantized by every wave that
// needs it (once per 32 output columns): the kernel is aimed at layer-sized calls.
//
// A K step: turn what was fetched for step s into operand registers, issue the loads of step
// s + 1, then the step's eight instructions.
#include "dfq_common.h"

#include "dfq_int_conv_plan.h"
#include "dfq_int_gemm_plan.h"
#include "dfq_int_quant.h"

namespace dfq {
namespace {

typedef int ig_v4i __attribute__((ext_vector_type(4)));
typedef int ig_v2i __attribute__((ext_vector_type(2)));

struct IgArgs {
    const void* a;            // stored A: its codes; fp32 A: x
    const uint8_t* b;
    const float* a_scale;     // stored A only
    const float* a_zero;      // stored A only; may be null
    const float* b_scale;
    const float* b_zero;      // may be null
    const float* bias;        // may be null
    float* out;
    int64_t lda;              // fp32 A only: x's row stride in elements
    int64_t ldo, M, N, K;
    int a_signed;             // stored A only (fp32 A: x_symmetric)
    int b_signed, per_row;
    // fp32 A only: the quantizer's arguments, dfq_fake_quant_given's
    const float* min_dev;
    const float* max_dev;
    double gmin, gmax;
    int x_bits, x_symmetric, x_flags;
};
// dfq_int_conv2d's: M and K are the im2col matrix's, a is the NCHW x.
struct IgcArgs : IgArgs {
    MxcGeom c;
};

// A lane's 16 stored bytes as four words, zero where they do not exist.
template <bool WIDE>
__device__ __forceinline__ ig_v4i ig_load_bytes(const uint8_t* base_, int64_t row, int64_t rows, int64_t K, int64_t step, int lane) {
    const DFQ_GLOBAL uint8_t* base = (const DFQ_GLOBAL uint8_t*)base_;
    const int64_t k0 = ig_lane_k0(step, lane);
    const int nv = ig_lane_valid(row, rows, k0, K);
    ig_v4i v = {0, 0, 0, 0};
    if (nv == 0) return v;
    const DFQ_GLOBAL uint8_t* p = base + ig_byte_offset(row, k0, K);
    if (WIDE) {
        v = *(const DFQ_GLOBAL ig_v4i*)p;
    } else {
        uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
        for (int e = 0; e < kIgLaneK; ++e)
            if (e < nv) w[e >> 2] |= (uint32_t)p[e] << (8 * (e & 3));
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (int)w[j];
    }
    return v;
}
// A lane's 8 packed bytes as two words.
template <bool WIDE>
__device__ __forceinline__ ig_v2i ig_load_packed(const uint8_t* base_, int64_t row, int64_t rows, int64_t K, int64_t step, int lane) {
    const DFQ_GLOBAL uint8_t* base = (const DFQ_GLOBAL uint8_t*)base_;
    const int64_t k0 = ig_lane_k0(step, lane);
    const int nv = ig_lane_valid(row, rows, k0, K);
    ig_v2i v = {0, 0};
    if (nv == 0) return v;
    const DFQ_GLOBAL uint8_t* p = base + ig_packed_offset(row, k0, K);
    if (WIDE) {
        v = *(const DFQ_GLOBAL ig_v2i*)p;
    } else {
        uint32_t w[2] = {0, 0};
#pragma unroll
        for (int e = 0; e < kIgLaneK / 2; ++e)
            if (e < ig_packed_bytes(nv)) w[e >> 2] |= (uint32_t)p[e] << (8 * (e & 3));
        v[0] = (int)w[0];
        v[1] = (int)w[1];
    }
    return v;
}

// Where a fragment comes from.  Fetched: what a lane holds of its row between the loads of a K
// step and the top of that step; fetch() issues the loads, operand() turns them into the
// instruction's four registers (signed domain, absent elements zero).  A sources also carry the
// contract's sa, za and offset (Params, made once before the loop).
template <bool WIDE>
struct IgBytesB {
    typedef ig_v4i Fetched;
    static __device__ __forceinline__ void fetch(Fetched& f, const IgArgs& g, int64_t row, int64_t step, int lane) {
        f = ig_load_bytes<WIDE>(g.b, row, g.N, g.K, step, lane);
    }
    static __device__ __forceinline__ ig_v4i operand(const Fetched& f, uint32_t xm, int nv) {
        ig_v4i v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (int)ig_operand_word((uint32_t)f[j], xm, nv, j);
        return v;
    }
};
template <bool WIDE>
struct IgPackedB {
    typedef ig_v2i Fetched;
    static __device__ __forceinline__ void fetch(Fetched& f, const IgArgs& g, int64_t row, int64_t step, int lane) {
        f = ig_load_packed<WIDE>(g.b, row, g.N, g.K, step, lane);
    }
    static __device__ __forceinline__ ig_v4i operand(const Fetched& f, uint32_t xm, int nv) {
        const uint32_t w[2] = {(uint32_t)f[0], (uint32_t)f[1]};
        ig_v4i v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (int)ig_operand_word(ig_unpack4(w, j, xm == 0), xm, nv, j);
        return v;
    }
};

// Rows: the lane's rows of A, one per instruction tile of its wave tile, made once before the K
// loop; at(i) is what fetch() takes for tile i and m(i) the row's index.  kMask: sum_k b' depends
// on the row (a mask operand, mask()); taps(): the contract's T of an output row.
struct IgRowIndex {
    int64_t m0;
    int lane;
    __device__ __forceinline__ IgRowIndex(const IgArgs&, int64_t m0_, int lane_) : m0(m0_), lane(lane_) {}
    __device__ __forceinline__ int64_t at(int i) const { return mxg_lane_row(m0, i, lane); }
    __device__ __forceinline__ int64_t m(int i) const { return mxg_lane_row(m0, i, lane); }
};

template <bool WIDE>
struct IgStoredA {
    typedef IgArgs Args;
    typedef IgRowIndex Rows;
    static constexpr bool kMask = false;
    static __device__ __forceinline__ int64_t taps(const IgArgs& g, int64_t) { return g.K; }
    typedef ig_v4i Fetched;
    static __device__ __forceinline__ IgAParams params(const IgArgs& g) {
        IgAParams p;
        p.s = ((const DFQ_GLOBAL float*)g.a_scale)[0];
        p.has_z = g.a_zero != nullptr;
        p.z = p.has_z ? ((const DFQ_GLOBAL float*)g.a_zero)[0] : 0.f;
        p.xm = ig_xor_mask(g.a_signed != 0);
        p.off = ig_offset(g.a_signed != 0);
        return p;
    }
    static __device__ __forceinline__ void fetch(Fetched& f, const IgArgs& g, int64_t row, int64_t step, int lane) {
        f = ig_load_bytes<WIDE>(static_cast<const uint8_t*>(g.a), row, g.M, g.K, step, lane);
    }
    static __device__ __forceinline__ ig_v4i operand(const Fetched& f, const IgAParams& p, int nv) {
        return IgBytesB<WIDE>::operand(f, p.xm, nv);
    }
};

// VEC: x on the 16-B path (ig_x_vec).
template <bool VEC>
struct IgFp32A {
    typedef IgArgs Args;
    typedef IgRowIndex Rows;
    static constexpr bool kMask = false;
    static __device__ __forceinline__ int64_t taps(const IgArgs& g, int64_t) { return g.K; }
    typedef float Fetched[kIgLaneK];
    // the parameters as fq_given_kernel builds them (dfq_int_quant.h)
    static __device__ __forceinline__ IgAParams params(const IgArgs& g) {
        return ig_quant_params(g.min_dev, g.max_dev, g.gmin, g.gmax, g.x_bits, g.x_symmetric, g.x_flags);
    }
    static __device__ __forceinline__ void fetch(Fetched& v, const IgArgs& g, int64_t row, int64_t step, int lane) {
        const DFQ_GLOBAL float* x = (const DFQ_GLOBAL float*)g.a;
        const int64_t k0 = ig_lane_k0(step, lane);
        const int nv = ig_lane_valid(row, g.M, k0, g.K);
        const DFQ_GLOBAL float* p = x + ig_x_offset(nv ? row : 0, nv ? k0 : 0, g.lda);   // never past the array
#pragma unroll
        for (int q = 0; q < kIgLaneK; q += 4) {
            if (VEC) {
                f32x4 t = {0.f, 0.f, 0.f, 0.f};
                if (q < nv) t = *(const DFQ_GLOBAL f32x4*)(p + q);   // K % 4 == 0: all four exist
                v[q] = t.x; v[q + 1] = t.y; v[q + 2] = t.z; v[q + 3] = t.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) v[q + j] = q + j < nv ? p[q + j] : 0.f;
            }
        }
    }
    // qdq's q of elements 4 j .. 4 j + 3 as a word of code bytes (ig_codes4: the screened quotient,
    // the ballot in wave-uniform control flow -- every lane of a working wave gets here).
    static __device__ __forceinline__ uint32_t codes(const float (&x)[kIgLaneK], const IgAParams& p, int j) {
        return ig_codes4(&x[4 * j], p);
    }
    static __device__ __forceinline__ ig_v4i operand(const Fetched& x, const IgAParams& p, int nv) {
        ig_v4i v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (int)ig_operand_word(codes(x, p, j), p.xm, nv, j);
        return v;
    }
};

// A = Q(im2col(x)), x the NCHW activation (dfq_mx_conv_plan.h, dfq_int_conv_plan.h): the lane's
// run of 16 consecutive k gathered with 4-B loads -- the run's first tap decomposed once, then
// walked with carries; taps outside the image, columns >= K and rows >= M are loads not issued
// and clear bits of the run's mask, never an exit, so every lane reaches operand()'s ballot.
// operand() is the fp32 A's quantizer; an element whose mask bit is clear enters as 0 in the
// signed domain: a padding tap has the real value 0, not the code of 0.0.  PW: the pointwise
// variant.  MASK: some tap of the geometry can fall in padding (igc_masked).
template <bool PW, bool MASK>
struct IgConvA {
    typedef IgcArgs Args;
    typedef MxcRow Row;
    static constexpr bool kMask = MASK;
    struct Rows {   // a lane's row keeps its (b, oh, ow) for the whole K loop: decomposed here, once
        Row r[kMxgSub];
        __device__ __forceinline__ Rows(const Args& g, int64_t m0, int lane) {
#pragma unroll
            for (int i = 0; i < kMxgSub; ++i) r[i] = mxc_row(g.c, mxg_lane_row(m0, i, lane), g.M);
        }
        __device__ __forceinline__ const Row& at(int i) const { return r[i]; }
        __device__ __forceinline__ int64_t m(int i) const { return r[i].m; }
    };
    struct Fetched {
        float v[kIgLaneK];
        uint32_t mask;   // bit e: element e of the run is read (the contract's v)
    };
    static __device__ __forceinline__ int64_t taps(const Args& g, int64_t row) {
        return MASK ? igc_taps(g.c, mxc_row(g.c, row, g.M)) : g.K;
    }
    static __device__ __forceinline__ IgAParams params(const Args& g) { return IgFp32A<false>::params(g); }
    static __device__ __forceinline__ void fetch(Fetched& f, const Args& g, const Row& row, int64_t step, int lane) {
        const DFQ_GLOBAL float* x = (const DFQ_GLOBAL float*)g.a;
        const int64_t k0 = ig_lane_k0(step, lane);
        MxcTap t = mxc_tap<PW>(g.c, k0);
        uint32_t mask = 0;
#pragma unroll
        for (int e = 0; e < kIgLaneK; ++e) {
            const uint32_t bit = igc_mask_bit<PW>(g.c, row, t, k0 + e, g.K, e);
            f.v[e] = bit ? x[mxc_x_offset(row, t)] : 0.f;
            mask |= bit;
            mxc_next<PW>(g.c, t);
        }
        f.mask = mask;
    }
    static __device__ __forceinline__ ig_v4i operand(const Fetched& f, const IgAParams& p, int) {
        ig_v4i v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (int)igc_operand_word(IgFp32A<false>::codes(f.v, p, j), p.xm, f.mask, j);
        return v;
    }
    static __device__ __forceinline__ ig_v4i mask(const Fetched& f) {
        ig_v4i v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (int)igc_ones_word(f.mask, j);
        return v;
    }
};

// Where the result goes.  kGroups: the epilogue hands over a lane's four rows of a column at once
// (rows that are not stored hold 0), else every stored element as it is made.  Row-major [M][ldo]:
// dfq_int_gemm's and dfq_int_linear's.
struct IgRowMajorStore {
    static constexpr bool kGroups = false;
    static __device__ __forceinline__ void store(float v, const IgArgs& g, int64_t row, int64_t col) {
        ((DFQ_GLOBAL float*)g.out)[mxg_out_offset(row, col, g.ldo)] = v;
    }
};
// NCHW [B][N][OH][OW], row m = (b, oh, ow): a lane's four accumulator registers are rows m .. m + 3
// of one column n -- one 16-B store (4-B aligned) where they lie in one image (mxc_out_quad), else
// element by element.
typedef float ig_v4f_a4 __attribute__((ext_vector_type(4), aligned(4)));
struct IgNchwStore {
    static constexpr bool kGroups = true;
    static __device__ __forceinline__ void store(const float (&v)[4], const IgcArgs& g, int64_t m, int64_t col) {
        DFQ_GLOBAL float* out = (DFQ_GLOBAL float*)g.out;
        if (mxc_out_quad(g.c, m, g.M)) {
            const ig_v4f_a4 q = {v[0], v[1], v[2], v[3]};
            *(DFQ_GLOBAL ig_v4f_a4*)(out + mxc_out_offset(g.c, m, col)) = q;
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (mxg_stores(m + r, col, g.M, g.N)) out[mxc_out_offset(g.c, m + r, col)] = v[r];
        }
    }
};

// A: IgStoredA, IgFp32A or IgConvA.  B: IgBytesB or IgPackedB.  Store: IgRowMajorStore or IgNchwStore.
template <class A, class B, class Store>
__global__ __launch_bounds__(kThreads) void int_mm_kernel(const typename A::Args g) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int64_t m0 = mxg_wave_m0(blockIdx.x, wave, g.N), n0 = mxg_wave_n0(blockIdx.x, wave, g.N);
    if (!mxg_wave_works(m0, n0, g.M, g.N)) return;   // wave-uniform; the kernel has no barrier
    const IgAParams pa = A::params(g);
    const uint32_t xb = ig_xor_mask(g.b_signed != 0);
    const ig_v4i zero4 = {0, 0, 0, 0}, ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101};
    // rb: sum_k b' of C's columns -- one per column tile, or, under a mask, one per tile: sum_k v b'
    constexpr int kRb = A::kMask ? kMxgSub : 1;
    ig_v4i acc[kMxgSub][kMxgSub], ra[kMxgSub], rb[kRb][kMxgSub];
    const typename A::Rows rows(g, m0, lane);
    int64_t brow[kMxgSub];
#pragma unroll
    for (int i = 0; i < kMxgSub; ++i) {
        ra[i] = zero4;
        brow[i] = mxg_lane_row(n0, i, lane);
#pragma unroll
        for (int j = 0; j < kMxgSub; ++j) acc[i][j] = zero4;
#pragma unroll
        for (int t = 0; t < kRb; ++t) rb[t][i] = zero4;
    }
    const int64_t steps = ig_steps(g.K);
    typename A::Fetched fa[kMxgSub];
    typename B::Fetched fb[kMxgSub];
#pragma unroll
    for (int i = 0; i < kMxgSub; ++i) {
        A::fetch(fa[i], g, rows.at(i), 0, lane);
        B::fetch(fb[i], g, brow[i], 0, lane);
    }
    for (int64_t s = 0; s < steps; ++s) {
        const int64_t k0 = ig_lane_k0(s, lane);
        ig_v4i a[kMxgSub], b[kMxgSub], am[kMxgSub];
#pragma unroll
        for (int i = 0; i < kMxgSub; ++i) {
            a[i] = A::operand(fa[i], pa, ig_lane_valid(rows.m(i), g.M, k0, g.K));
            b[i] = B::operand(fb[i], xb, ig_lane_valid(brow[i], g.N, k0, g.K));
            if constexpr (A::kMask) am[i] = A::mask(fa[i]);
        }
        if (s + 1 < steps) {
#pragma unroll
            for (int i = 0; i < kMxgSub; ++i) {
                A::fetch(fa[i], g, rows.at(i), s + 1, lane);
                B::fetch(fb[i], g, brow[i], s + 1, lane);
            }
        }
#pragma unroll
        for (int i = 0; i < kMxgSub; ++i) {
#pragma unroll
            for (int j = 0; j < kMxgSub; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[i], b[j], acc[i][j], 0, 0, 0);
            ra[i] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[i], ones, ra[i], 0, 0, 0);   // sum_k a' of C's rows
            if constexpr (A::kMask) {
#pragma unroll
                for (int j = 0; j < kMxgSub; ++j) rb[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(am[i], b[j], rb[i][j], 0, 0, 0);
            } else {
                rb[0][i] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, b[i], rb[0][i], 0, 0, 0);   // sum_k b' of C's columns
            }
        }
    }
    // the contract's integers, then its fp64 steps in its order
    const DFQ_GLOBAL float* bias = (const DFQ_GLOBAL float*)g.bias;
    const DFQ_GLOBAL float* b_scale = (const DFQ_GLOBAL float*)g.b_scale;
    const DFQ_GLOBAL float* b_zero = (const DFQ_GLOBAL float*)g.b_zero;
    const int ob = ig_offset(g.b_signed != 0);
    const bool has_zb = b_zero != nullptr;
    const double sa = (double)pa.s, za = (double)pa.z;
    int64_t T[kMxgSub][4];   // the contract's T of the lane's output rows: K unless a mask is on
#pragma unroll
    for (int i = 0; i < kMxgSub; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) T[i][r] = A::taps(g, mxg_out_row(m0, i, lane, r));
#pragma unroll
    for (int j = 0; j < kMxgSub; ++j) {
        const int64_t col = mxg_out_col(n0, j, lane);
        if (col >= g.N) continue;
        const int64_t pc = g.per_row ? col : 0;
        const double sb = (double)b_scale[pc], zb = has_zb ? (double)b_zero[pc] : 0.0;
        const double ss = sa * sb, sz = sa * zb, zs = za * sb, zz = za * zb;
        const double bv = bias != nullptr ? (double)bias[col] : 0.0;
#pragma unroll
        for (int i = 0; i < kMxgSub; ++i) {
            float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t row = mxg_out_row(m0, i, lane, r);
                if (!mxg_stores(row, col, g.M, g.N)) continue;
                const int rbv = rb[A::kMask ? i : 0][j][r];
                const int64_t P = igc_fold_p(acc[i][j][r], ra[i][r], rbv, pa.off, ob, T[i][r]);
                double t = ss * (double)P;
                if (has_zb) t += sz * (double)igc_fold_s(ra[i][r], pa.off, T[i][r]);
                if (pa.has_z) t += zs * (double)igc_fold_s(rbv, ob, T[i][r]);
                if (has_zb && pa.has_z) t += zz * (double)T[i][r];
                if (bias != nullptr) t += bv;
                v[r] = (float)t;
                if constexpr (!Store::kGroups) Store::store(v[r], g, row, col);
            }
            if constexpr (Store::kGroups) Store::store(v, g, mxg_out_row(m0, i, lane, 0), col);
        }
    }
}

template <class A, class Store, class G>
void ig_launch_b(const G& g, bool packed, bool wide, int64_t grid, hipStream_t s) {
    const dim3 blocks((unsigned)grid), threads(kThreads);
    if (packed) {
        if (wide) hipLaunchKernelGGL((int_mm_kernel<A, IgPackedB<true>, Store>), blocks, threads, 0, s, g);
        else hipLaunchKernelGGL((int_mm_kernel<A, IgPackedB<false>, Store>), blocks, threads, 0, s, g);
    } else {
        if (wide) hipLaunchKernelGGL((int_mm_kernel<A, IgBytesB<true>, Store>), blocks, threads, 0, s, g);
        else hipLaunchKernelGGL((int_mm_kernel<A, IgBytesB<false>, Store>), blocks, threads, 0, s, g);
    }
}

}  // namespace
}  // namespace dfq

using namespace dfq;

extern "C" int dfq_int_gemm(const dfq_int_gemm_desc* d, void* stream) {
    static_assert(kMxgWaves * kWave == kThreads, "four waves per block");
    int64_t grid = 0;
    const int rc = ig_check(d, grid);
    if (rc != DFQ_OK) return rc;
    IgArgs g{};
    g.a = d->a_codes;
    g.b = static_cast<const uint8_t*>(d->b_codes);
    g.a_scale = d->a_scale;
    g.a_zero = d->a_zero;
    g.b_scale = d->b_scale;
    g.b_zero = d->b_zero;
    g.bias = d->bias;
    g.out = d->out;
    g.ldo = d->ldo; g.M = d->M; g.N = d->N; g.K = d->K;
    g.a_signed = d->a_signed;
    g.b_signed = d->b_signed;
    g.per_row = (d->flags & DFQ_INT_B_PER_ROW) != 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool packed = (d->flags & DFQ_INT_B_PACK4) != 0, wide = ig_wide(d->K);
    if (wide) ig_launch_b<IgStoredA<true>, IgRowMajorStore>(g, packed, wide, grid, s);
    else ig_launch_b<IgStoredA<false>, IgRowMajorStore>(g, packed, wide, grid, s);
    DFQ_LAUNCH_CHECK();
    return DFQ_OK;
}

extern "C" int dfq_int_linear(const dfq_int_linear_desc* d, void* stream) {
    int64_t grid = 0;
    const int rc = igl_check(d, grid);
    if (rc != DFQ_OK) return rc;
    IgArgs g{};
    g.a = d->x;
    g.b = static_cast<const uint8_t*>(d->b_codes);
    g.b_scale = d->b_scale;
    g.b_zero = d->b_zero;
    g.bias = d->bias;
    g.out = d->out;
    g.lda = d->ldx; g.ldo = d->ldo; g.M = d->M; g.N = d->N; g.K = d->K;
    g.b_signed = d->b_signed;
    g.per_row = (d->flags & DFQ_INT_B_PER_ROW) != 0;
    g.min_dev = d->min_dev;
    g.max_dev = d->max_dev;
    g.gmin = d->given_min;
    g.gmax = d->given_max;
    g.x_bits = d->x_bits;
    g.x_symmetric = d->x_symmetric;
    g.x_flags = d->flags & DFQ_SCALE_F32;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool packed = (d->flags & DFQ_INT_B_PACK4) != 0, wide = ig_wide(d->K);
    if (ig_x_vec(reinterpret_cast<uintptr_t>(d->x), d->ldx, d->K)) ig_launch_b<IgFp32A<true>, IgRowMajorStore>(g, packed, wide, grid, s);
    else ig_launch_b<IgFp32A<false>, IgRowMajorStore>(g, packed, wide, grid, s);
    DFQ_LAUNCH_CHECK();
    return DFQ_OK;
}

extern "C" int dfq_int_conv2d(const dfq_int_conv2d_desc* d, void* stream) {
    IgcArgs g{};
    int64_t grid = 0;
    const int rc = igc_check(d, g.c, g.M, g.K, grid);
    if (rc != DFQ_OK) return rc;
    g.a = d->x;
    g.b = static_cast<const uint8_t*>(d->b_codes);
    g.b_scale = d->b_scale;
    g.b_zero = d->b_zero;
    g.bias = d->bias;
    g.out = d->out;
    g.N = d->N;
    g.b_signed = d->b_signed;
    g.per_row = (d->flags & DFQ_INT_B_PER_ROW) != 0;
    g.min_dev = d->min_dev;
    g.max_dev = d->max_dev;
    g.gmin = d->given_min;
    g.gmax = d->given_max;
    g.x_bits = d->x_bits;
    g.x_symmetric = d->x_symmetric;
    g.x_flags = d->flags & DFQ_SCALE_F32;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool packed = (d->flags & DFQ_INT_B_PACK4) != 0, wide = ig_wide(g.K);
    if (igc_masked(g.c)) ig_launch_b<IgConvA<false, true>, IgNchwStore>(g, packed, wide, grid, s);
    else if (mxc_pointwise(g.c)) ig_launch_b<IgConvA<true, false>, IgNchwStore>(g, packed, wide, grid, s);
    else ig_launch_b<IgConvA<false, false>, IgNchwStore>(g, packed, wide, grid, s);
    DFQ_LAUNCH_CHECK();
    return DFQ_OK;
}
