// The fragment sources and stores of the integer matrix multiply kernels (dfq_int_gemm.hip:
// int_mm_kernel; dfq_int_group.hip: int_mm_group_kernel): how a lane obtains the 16 bytes of its A
// fragment (stored codes, fp32 x quantized on the way, im2col rows gathered and quantized on the
// way, im2col rows gathered from stored codes), of its B fragment (stored bytes, packed nibbles),
// and where a result goes (row-major or NCHW, as fp32 or as the next layer's code bytes).  Device
// code: included by the kernel files (dfq_int_mm_kernel.h, dfq_int_group.hip) and nothing else.
#pragma once
#include "dfq_common.h"

#include "dfq_int_conv_plan.h"
#include "dfq_int_gemm_plan.h"
#include "dfq_int_io_plan.h"
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

// A = the stored codes of an NCHW activation (dfq_int_conv2d_q with x_codes): IgConvA's rows, tap
// walker and mask, the lane's run of 16 consecutive k gathered as byte loads straight into the
// fragment's four words.  No quantizer and no ballot: the range of the descriptor only names the
// grid (params(): sa, za, the xor mask).  A padding tap, a column >= K and a row >= M are loads
// not issued and clear mask bits, 0 in the signed domain.  Where IgConvA holds 16 floats between
// the loads and the top of the step, this holds 16 bytes.
template <bool PW, bool MASK>
struct IgConvCodesA : IgConvA<PW, MASK> {
    typedef IgcArgs Args;
    typedef MxcRow Row;
    struct Fetched {
        uint32_t w[4];
        uint32_t mask;
    };
    static __device__ __forceinline__ void fetch(Fetched& f, const Args& g, const Row& row, int64_t step, int lane) {
        const DFQ_GLOBAL uint8_t* x = (const DFQ_GLOBAL uint8_t*)g.a;
        const int64_t k0 = ig_lane_k0(step, lane);
        MxcTap t = mxc_tap<PW>(g.c, k0);
        uint32_t mask = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) f.w[j] = 0;
#pragma unroll
        for (int e = 0; e < kIgLaneK; ++e) {
            const uint32_t bit = igc_mask_bit<PW>(g.c, row, t, k0 + e, g.K, e);
            const uint32_t code = bit ? x[mxc_x_offset(row, t)] : 0u;
            f.w[e >> 2] |= code << (8 * (e & 3));
            mask |= bit;
            mxc_next<PW>(g.c, t);
        }
        f.mask = mask;
    }
    static __device__ __forceinline__ ig_v4i operand(const Fetched& f, const IgAParams& p, int) {
        ig_v4i v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (int)igc_operand_word(f.w[j], p.xm, f.mask, j);
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
    static constexpr bool kGroups = false, kCodes = false;
    static __device__ __forceinline__ void store(float v, const IgArgs& g, int64_t row, int64_t col) {
        ((DFQ_GLOBAL float*)g.out)[mxg_out_offset(row, col, g.ldo)] = v;
    }
};
// NCHW [B][N][OH][OW], row m = (b, oh, ow): a lane's four accumulator registers are rows m .. m + 3
// of one column n -- one 16-B store (4-B aligned) where they lie in one image (mxc_out_quad), else
// element by element.
typedef float ig_v4f_a4 __attribute__((ext_vector_type(4), aligned(4)));
struct IgNchwStore {
    static constexpr bool kGroups = true, kCodes = false;
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

// The code stores (dfq_int_*_q with out_bits): the epilogue quantizes a lane's four rows of a
// column with one ig_codes4 call -- every lane of a working wave, rows and columns that are not
// stored carrying 0 -- and hands over the word of four code bytes; only the store is guarded.
// IgOutQ: the output quantizer's arguments, dfq_fake_quant_given's.
struct IgOutQ {
    const float* min_dev;
    const float* max_dev;
    double gmin, gmax;
    int bits, symmetric, flags;
};
inline IgOutQ ig_out_q(const dfq_int_io* io) {
    return IgOutQ{io->out_min_dev, io->out_max_dev, io->out_given_min, io->out_given_max, io->out_bits, io->out_symmetric, io->out_flags};
}
__device__ __forceinline__ IgAParams ig_out_params(const IgOutQ& o) {
    return ig_quant_params(o.min_dev, o.max_dev, o.gmin, o.gmax, o.bits, o.symmetric, o.flags);
}
// Row-major bytes [M][ldo]: byte stores.
struct IgRowMajorCodeStore {
    static constexpr bool kGroups = true, kCodes = true;
    static __device__ __forceinline__ void store(uint32_t w, const IgArgs& g, int64_t m, int64_t col) {
        DFQ_GLOBAL uint8_t* out = (DFQ_GLOBAL uint8_t*)g.out;
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (mxg_stores(m + r, col, g.M, g.N)) out[mxg_out_offset(m + r, col, g.ldo)] = (uint8_t)(w >> (8 * r));
    }
};
// NCHW bytes: one 4-B store where the four rows lie in one image and the address allows
// (igio_out_word), else byte stores.
struct IgNchwCodeStore {
    static constexpr bool kGroups = true, kCodes = true;
    static __device__ __forceinline__ void store(uint32_t w, const IgcArgs& g, int64_t m, int64_t col) {
        DFQ_GLOBAL uint8_t* out = (DFQ_GLOBAL uint8_t*)g.out;
        if (col < g.N && igio_out_word(g.c, m, g.M, col, reinterpret_cast<uintptr_t>(g.out))) {
            *(DFQ_GLOBAL uint32_t*)(out + mxc_out_offset(g.c, m, col)) = w;
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (mxg_stores(m + r, col, g.M, g.N)) out[mxc_out_offset(g.c, m + r, col)] = (uint8_t)(w >> (8 * r));
        }
    }
};

// A descriptor's fields as the kernels take them (the checks have passed).
inline void ig_fill_b(IgArgs& g, const void* b_codes, const float* b_scale, const float* b_zero, const float* bias, float* out,
                      int32_t b_signed, int32_t flags) {
    g.b = static_cast<const uint8_t*>(b_codes);
    g.b_scale = b_scale;
    g.b_zero = b_zero;
    g.bias = bias;
    g.out = out;
    g.b_signed = b_signed;
    g.per_row = (flags & DFQ_INT_B_PER_ROW) != 0;
}
template <class Desc>   // dfq_int_linear's and dfq_int_conv2d's quantizer
inline void ig_fill_quant(IgArgs& g, const Desc* d) {
    g.a = d->x;
    g.min_dev = d->min_dev;
    g.max_dev = d->max_dev;
    g.gmin = d->given_min;
    g.gmax = d->given_max;
    g.x_bits = d->x_bits;
    g.x_symmetric = d->x_symmetric;
    g.x_flags = d->flags & DFQ_SCALE_F32;
}
inline IgArgs ig_args(const dfq_int_gemm_desc* d) {
    IgArgs g{};
    ig_fill_b(g, d->b_codes, d->b_scale, d->b_zero, d->bias, d->out, d->b_signed, d->flags);
    g.a = d->a_codes;
    g.a_scale = d->a_scale;
    g.a_zero = d->a_zero;
    g.ldo = d->ldo; g.M = d->M; g.N = d->N; g.K = d->K;
    g.a_signed = d->a_signed;
    return g;
}
inline IgArgs ig_args(const dfq_int_linear_desc* d) {
    IgArgs g{};
    ig_fill_b(g, d->b_codes, d->b_scale, d->b_zero, d->bias, d->out, d->b_signed, d->flags);
    ig_fill_quant(g, d);
    g.lda = d->ldx; g.ldo = d->ldo; g.M = d->M; g.N = d->N; g.K = d->K;
    return g;
}
// g.c, g.M and g.K are igc_check's
inline void ig_fill(IgcArgs& g, const dfq_int_conv2d_desc* d) {
    ig_fill_b(g, d->b_codes, d->b_scale, d->b_zero, d->bias, d->out, d->b_signed, d->flags);
    ig_fill_quant(g, d);
    g.N = d->N;
}

}  // namespace
}  // namespace dfq
