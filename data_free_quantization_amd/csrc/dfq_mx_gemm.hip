// dfq_mx_gemm, dfq_mx_linear and dfq_mx_conv2d: out[m][n] = sum_k A[m][k] * B[n][k] (+ bias[n]) on the scaled
// matrix instruction v_mfma_scale_f32_16x16x128_f8f6f4 (include/dfq_hip.h).  One
// kernel template over where the A operand comes from: dfq_mx_gemm reads both operands as the
// MX codes and E8M0 scale bytes dfq_mx_quantize_batch writes ("stored" A); dfq_mx_linear builds
// A in the kernel from the fp32 activation x ("fp32" A, A = Q(x)) and is otherwise the same
// multiply in one launch; dfq_mx_conv2d builds A from the im2col rows of an fp32 NCHW activation
// ("conv" A: the fp32 A's quantizer behind a gather, dfq_mx_conv_plan.h) and stores to NCHW.
//
// For FP4 and FP6 a lane's operand of the instruction is 32 consecutive K elements of one
// row and one scale byte: exactly one stored MX block, codes[row][blk][0 .. cb) and
// scales[row][blk].  So every lane loads its block straight from global memory into the
// operand registers -- 16 B (FP4) or 24 B (FP6) -- and nothing is unpacked, permuted or
// dequantized on the way: the bit order inside a block is the instruction's.  For FP8 the
// instruction walks K in two passes of 64, measured on the hardware: a lane holds 16
// consecutive elements of each pass, so it loads two stored 16-byte halves (of two MX
// blocks of its row) where the others load one block, and its scale byte is still the
// lane group's block's.  The bytes are the stored ones, placed by address alone
// (dfq_mx_gemm_plan.h, "split"; tests/test_gpu_mx_gemm.py proves all of it with exact
// integer data on the 16 format pairs).
// All addressing is dfq_mx_gemm_plan.h's: a wave owns a 32 x 32 output tile, so each of
// its two A and two B fragments per K step (128 elements) feeds two instructions; four
// waves make a 64 x 64 block tile.  Lanes of rows past M / N and of MX blocks past nb issue
// no load and hold zero codes with scale byte 127; such rows are not stored.  No LDS, no
// workspace, no atomics, no split of K: an output element is one accumulator of one lane,
// added up in K-step order, then one fp32 add of the bias.
//
// fp32 A: a lane reads the fp32 elements its operand stands for -- one MX block of one row for
// FP4 / FP6, two 16-element halves of two blocks for FP8 -- as 16-B loads where the rows of x
// start 16-B aligned and K % 4 == 0 (a kernel instantiation of its own) and as 4-B loads
// otherwise, takes the amax of the magnitudes' bit patterns, derives the floor rule's exponent
// and encodes (dfq_mx_encode.h, the quantizer's own encoder) straight into the operand
// registers in the stored blocks' bit order (dfq_mx_linear_plan.h).  An FP8 lane exchanges its
// two halves' amax with lane ^ 16 and gathers its lane group's block's scale byte from the lane
// group that knows it: three ds_bpermute per fragment, no LDS memory, no barrier.  Every lane
// of a working wave takes part in the exchanges: the only early return is wave-uniform and
// lies before the loop.  Elements at k >= K and rows >= M are never read and count as +0.  So
// the operand registers are bit for bit the ones a stored A holds after
// dfq_mx_quantize_batch of x, and so is the result.  The A fragment is re-quantized by every
// wave that needs it (once per 32 output columns): the kernel is aimed at layer-sized calls.
//
// A K step, for either A: turn what was fetched for step s into A's operand registers (a
// copy for a stored A, the quantizer for an fp32 A), issue the loads of step s + 1 -- A's
// codes or fp32 elements, and B's fragments -- then the step's four instructions.
#include "dfq_common.h"
#include <type_traits>

#include "dfq_mx_conv_plan.h"

namespace dfq {
namespace {

typedef int mxg_v8i __attribute__((ext_vector_type(8)));
typedef int mxg_v4i __attribute__((ext_vector_type(4)));
typedef int mxg_v2i __attribute__((ext_vector_type(2)));
typedef float mxg_v4f __attribute__((ext_vector_type(4)));

// One MX block's code bytes as the operand registers (the registers past the format's
// size stay zero and are not read by the instruction).
template <int CB>
__device__ __forceinline__ mxg_v8i mxg_load_codes(const DFQ_GLOBAL uint8_t* p, bool on) {
    mxg_v8i v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (on) {
        if (CB == 24) {   // 8-B aligned
            const mxg_v2i q0 = *(const DFQ_GLOBAL mxg_v2i*)p, q1 = *(const DFQ_GLOBAL mxg_v2i*)(p + 8),
                          q2 = *(const DFQ_GLOBAL mxg_v2i*)(p + 16);
            v[0] = q0.x; v[1] = q0.y; v[2] = q1.x; v[3] = q1.y; v[4] = q2.x; v[5] = q2.y;
        } else {
            const mxg_v4i q0 = *(const DFQ_GLOBAL mxg_v4i*)p;
            v[0] = q0.x; v[1] = q0.y; v[2] = q0.z; v[3] = q0.w;
            if (CB == 32) {
                const mxg_v4i q1 = *(const DFQ_GLOBAL mxg_v4i*)(p + 16);
                v[4] = q1.x; v[5] = q1.y; v[6] = q1.z; v[7] = q1.w;
            }
        }
    }
    return v;
}

// One operand's fragment of a lane: F its format field.  FP6 / FP4: the lane's MX block as
// stored.  FP8: the 16-byte halves of two MX blocks the instruction expects in the lane
// (dfq_mx_gemm_plan.h, "split").  The scale byte is the lane group's block's either way.
template <int F>
__device__ __forceinline__ void mxg_load_operand(mxg_v8i& v, int& s, const uint8_t* codes_, const uint8_t* scales_,
                                                 int64_t row, int64_t rows, int64_t nb, int64_t step, int lane) {
    const DFQ_GLOBAL uint8_t* codes = (const DFQ_GLOBAL uint8_t*)codes_;
    const DFQ_GLOBAL uint8_t* scales = (const DFQ_GLOBAL uint8_t*)scales_;
    const int64_t kb = mxg_lane_kblock(step, lane);
    const bool on = mxg_lane_loads(row, rows, kb, nb);
    s = on ? (int)scales[mxg_scale_offset(row, kb, nb)] : 127;
    if (!mxg_hw_split(F)) {
        constexpr int cb = mxg_hw_code_bytes(F);
        v = mxg_load_codes<cb>(codes + mxg_code_offset(row, kb, nb, cb), on);
    } else {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int64_t kh = mxg_split_kblock(step, lane, h);
            const mxg_v8i q = mxg_load_codes<kMxgHalfBytes>(codes + mxg_split_code_offset(row, kh, nb, lane),
                                                            mxg_lane_loads(row, rows, kh, nb));
            v[4 * h] = q[0]; v[4 * h + 1] = q[1]; v[4 * h + 2] = q[2]; v[4 * h + 3] = q[3];
        }
    }
}

// A wave's 2 x 2 accumulator tiles to out (+ bias[n], one fp32 add), rows past M and columns
// past N not stored: row-major [M][ldo].
__device__ __forceinline__ void mxg_store_tile(const mxg_v4f (&acc)[kMxgSub][kMxgSub], float* out_, const float* bias_,
                                               int64_t ldo, int64_t M, int64_t N, int64_t m0, int64_t n0, int lane) {
    DFQ_GLOBAL float* out = (DFQ_GLOBAL float*)out_;
    const DFQ_GLOBAL float* bias = (const DFQ_GLOBAL float*)bias_;
#pragma unroll
    for (int j = 0; j < kMxgSub; ++j) {
        const int64_t col = mxg_out_col(n0, j, lane);
        const float bv = bias != nullptr && col < N ? bias[col] : 0.f;
#pragma unroll
        for (int i = 0; i < kMxgSub; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t row = mxg_out_row(m0, i, lane, r);
                if (!mxg_stores(row, col, M, N)) continue;
                const float v = acc[i][j][r];
                out[mxg_out_offset(row, col, ldo)] = bias != nullptr ? v + bv : v;
            }
    }
}

// a_scales comes last so that an fp32 A's fields lie where dfq_mx_linear's kernel always had them.
struct MxmArgs {
    const void* a;             // stored A: its codes; fp32 A and conv A: x
    const uint8_t* b_codes;
    const uint8_t* b_scales;
    const float* bias;
    float* out;
    int64_t lda;               // fp32 A only: x's row stride in elements
    int64_t ldo, M, N, K, nb;  // ldo: the row-major store only
    const uint8_t* a_scales;   // stored A only
};
// dfq_mx_conv2d's: M and K are the im2col matrix's.
struct MxcArgs : MxmArgs {
    MxcGeom c;
};

// Where the result goes.  Row-major [M][ldo]: dfq_mx_gemm's and dfq_mx_linear's.
struct MxmRowMajorStore {
    static __device__ __forceinline__ void store(const mxg_v4f (&acc)[kMxgSub][kMxgSub], const MxmArgs& g, int64_t m0, int64_t n0,
                                                 int lane) {
        mxg_store_tile(acc, g.out, g.bias, g.ldo, g.M, g.N, m0, n0, lane);
    }
};
// NCHW [B][N][OH][OW], row m = (b, oh, ow): a lane's four accumulator registers are rows m .. m + 3
// of one column n -- four consecutive floats where they lie in one image (mxc_out_quad), one
// 16-B store (4-B aligned: OH * OW need not be a multiple of 4); the groups that straddle two
// images or the end of M go element by element.
typedef mxg_v4f mxc_v4f_a4 __attribute__((aligned(4)));
struct MxmNchwStore {
    static __device__ __forceinline__ void store(const mxg_v4f (&acc)[kMxgSub][kMxgSub], const MxcArgs& g, int64_t m0, int64_t n0,
                                                 int lane) {
        DFQ_GLOBAL float* out = (DFQ_GLOBAL float*)g.out;
        const DFQ_GLOBAL float* bias = (const DFQ_GLOBAL float*)g.bias;
#pragma unroll
        for (int i = 0; i < kMxgSub; ++i) {
            const int64_t m = mxg_out_row(m0, i, lane, 0);
            const bool quad = mxc_out_quad(g.c, m, g.M);
#pragma unroll
            for (int j = 0; j < kMxgSub; ++j) {
                const int64_t col = mxg_out_col(n0, j, lane);
                if (col >= g.N) continue;
                mxg_v4f v = acc[i][j];
                if (bias != nullptr) {
                    const float bv = bias[col];
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = v[r] + bv;
                }
                if (quad) {
                    *(DFQ_GLOBAL mxc_v4f_a4*)(out + mxc_out_offset(g.c, m, col)) = v;
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (mxg_stores(m + r, col, g.M, g.N)) out[mxc_out_offset(g.c, m + r, col)] = v[r];
                }
            }
        }
    }
};

__device__ __forceinline__ uint32_t mxl_from_lane(int src_lane, uint32_t v) {
    return (uint32_t)__builtin_amdgcn_ds_bpermute(4 * src_lane, (int)v);
}

// Where A comes from.  Args: the kernel's arguments.  Rows: the lane's rows of A, one per
// instruction tile of its wave tile, made once before the K loop; at(i) is what fetch() and
// operand() take for tile i (MxmRowIndex: the row's index).  Fetched: what a lane holds of that row between the
// loads of a K step and the top of that step; fetch() issues those loads, operand() turns them
// into the instruction's registers and scale byte (bits [0, 8), opsel 0).  F: the instruction's
// format field (cbsz).  kAfterB: a step's loads of A are issued after both of B's fragments'
// instead of fragment by fragment before B's -- the order each source measured faster with
// (DESIGN.md 3.8).
struct MxmRowIndex {
    int64_t m0;
    int lane;
    __device__ __forceinline__ MxmRowIndex(const MxmArgs&, int64_t m0_, int lane_) : m0(m0_), lane(lane_) {}
    __device__ __forceinline__ int64_t at(int i) const { return mxg_lane_row(m0, i, lane); }
};

template <int FA>
struct MxmStoredA {
    static constexpr int F = FA;
    static constexpr bool kAfterB = true;
    typedef MxmArgs Args;
    typedef MxmRowIndex Rows;
    struct Fetched {
        mxg_v8i a;
        int sa;
    };
    static __device__ __forceinline__ void fetch(Fetched& f, const MxmArgs& g, int64_t row, int64_t step, int lane) {
        mxg_load_operand<FA>(f.a, f.sa, static_cast<const uint8_t*>(g.a), g.a_scales, row, g.M, g.nb, step, lane);
    }
    static __device__ __forceinline__ void operand(mxg_v8i& a, int& s, const Fetched& f, const MxmArgs&, int64_t, int64_t, int) {
        a = f.a;
        s = f.sa;
    }
};

// VEC: x on the 16-B path (mxl_vec).
template <int FA, bool VEC>
struct MxmFp32A {
    static constexpr int F = FA;
    static constexpr bool kAfterB = false;
    typedef MxmArgs Args;
    typedef MxmRowIndex Rows;
    typedef float Fetched[DFQ_MX_BLOCK];   // the lane's 32 fp32 elements, in slot order

    static __device__ __forceinline__ void fetch(Fetched& v, const MxmArgs& g, int64_t row, int64_t step, int lane) {
        const DFQ_GLOBAL float* x = (const DFQ_GLOBAL float*)g.a;
        constexpr int n = mxl_part_len(FA);
#pragma unroll
        for (int part = 0; part < mxl_parts(FA); ++part) {
            const int64_t k0 = mxl_part_k(FA, step, lane, part);
            const DFQ_GLOBAL float* p = x + mxl_x_offset(row < g.M ? row : 0, k0 < g.K ? k0 : 0, g.lda);   // never past the array
#pragma unroll
            for (int q = 0; q < n; q += 4) {
                float* o = &v[n * part + q];
                if (VEC) {
                    f32x4 t = {0.f, 0.f, 0.f, 0.f};
                    if (mxl_reads(row, g.M, k0 + q, g.K)) t = *(const DFQ_GLOBAL f32x4*)(p + q);   // K % 4 == 0: all four exist
                    o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = t.w;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) o[j] = mxl_reads(row, g.M, k0 + q + j, g.K) ? p[q + j] : 0.f;
                }
            }
        }
    }

    static __device__ __forceinline__ void operand(mxg_v8i& a, int& s, const Fetched& v, const MxmArgs& g, int64_t row, int64_t step,
                                                   int lane) {
        uint32_t r[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        int byte;
        if (!mxg_hw_split(FA)) {
            byte = mxl_scale_byte<FA>(mxl_part_amax<FA>(v, 0));
            mxl_encode_part<FA>(r, v, 0, byte);
        } else {
            int b[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const uint32_t mine = mxl_part_amax<FA>(v, h), other = mxl_from_lane(mxl_split_partner(lane), mine);
                b[h] = mxl_scale_byte<FA>(mine > other ? mine : other);
                mxl_encode_part<FA>(r, v, h, b[h]);
            }
            const uint32_t w = mxl_from_lane(mxl_split_scale_lane(lane), (uint32_t)b[0] | ((uint32_t)b[1] << 8));
            byte = (int)((w >> (8 * mxl_split_scale_byte(lane))) & 0xFFu);
        }
        s = mxg_lane_loads(row, g.M, mxg_lane_kblock(step, lane), g.nb) ? byte : 127;
#pragma unroll
        for (int i = 0; i < 8; ++i) a[i] = (int)r[i];
    }
};

// A = Q(im2col(x)), x the NCHW activation (dfq_mx_conv_plan.h): the lane's runs of consecutive k
// gathered with 4-B loads -- the run's first tap decomposed once, then walked with carries; taps
// outside the image, columns >= K and rows >= M are loads not issued (+0), never an exit, so every
// lane reaches operand()'s exchanges.  operand() is the fp32 A's.  PW: the pointwise variant.
template <int FA, bool PW>
struct MxmConvA {
    static constexpr int F = FA;
    static constexpr bool kAfterB = false;
    typedef MxcArgs Args;
    typedef MxcRow Row;
    struct Rows {   // a lane's row keeps its (b, oh, ow) for the whole K loop: decomposed here, once
        Row r[kMxgSub];
        __device__ __forceinline__ Rows(const Args& g, int64_t m0, int lane) {
#pragma unroll
            for (int i = 0; i < kMxgSub; ++i) r[i] = mxc_row(g.c, mxg_lane_row(m0, i, lane), g.M);
        }
        __device__ __forceinline__ const Row& at(int i) const { return r[i]; }
    };
    typedef float Fetched[DFQ_MX_BLOCK];

    static __device__ __forceinline__ void fetch(Fetched& v, const Args& g, const Row& row, int64_t step, int lane) {
        const DFQ_GLOBAL float* x = (const DFQ_GLOBAL float*)g.a;
        constexpr int n = mxl_part_len(FA);
#pragma unroll
        for (int part = 0; part < mxl_parts(FA); ++part) {
            const int64_t k0 = mxl_part_k(FA, step, lane, part);
            MxcTap t = mxc_tap<PW>(g.c, k0);
#pragma unroll
            for (int e = 0; e < n; ++e) {
                v[n * part + e] = mxc_reads<PW>(g.c, row, t, k0 + e, g.K) ? x[mxc_x_offset(row, t)] : 0.f;
                mxc_next<PW>(g.c, t);
            }
        }
    }

    static __device__ __forceinline__ void operand(mxg_v8i& a, int& s, const Fetched& v, const Args& g, const Row& row, int64_t step,
                                                   int lane) {
        MxmFp32A<FA, false>::operand(a, s, v, g, row.m, step, lane);
    }
};

// B's fragments of one K step: fragment j is instruction tile column j's.
struct MxmB {
    mxg_v8i b[kMxgSub];
    int sb[kMxgSub];
};

template <class A, int FB>
__device__ __forceinline__ void mxm_fetch(typename A::Fetched (&fa)[kMxgSub], MxmB& fb, const typename A::Args& g,
                                          const typename A::Rows& rows, int64_t n0, int64_t step, int lane) {
#pragma unroll
    for (int i = 0; i < kMxgSub; ++i) {
        if (!A::kAfterB) A::fetch(fa[i], g, rows.at(i), step, lane);
        mxg_load_operand<FB>(fb.b[i], fb.sb[i], g.b_codes, g.b_scales, mxg_lane_row(n0, i, lane), g.N, g.nb, step, lane);
    }
    if (A::kAfterB) {
#pragma unroll
        for (int i = 0; i < kMxgSub; ++i) A::fetch(fa[i], g, rows.at(i), step, lane);
    }
}

// A: MxmStoredA, MxmFp32A or MxmConvA.  A::F / FB: the instruction's format fields (cbsz / blgp) of
// A and B.  Store: MxmRowMajorStore or MxmNchwStore.
template <class A, int FB, class Store>
__global__ __launch_bounds__(kThreads) void mx_mm_kernel(const typename A::Args g) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int64_t m0 = mxg_wave_m0(blockIdx.x, wave, g.N), n0 = mxg_wave_n0(blockIdx.x, wave, g.N);
    if (!mxg_wave_works(m0, n0, g.M, g.N)) return;   // wave-uniform; the kernel has no barrier
    mxg_v4f acc[kMxgSub][kMxgSub];
#pragma unroll
    for (int i = 0; i < kMxgSub; ++i)
#pragma unroll
        for (int j = 0; j < kMxgSub; ++j) acc[i][j] = mxg_v4f{0.f, 0.f, 0.f, 0.f};
    const int64_t steps = mxg_steps(g.nb);
    const typename A::Rows rows(g, m0, lane);
    typename A::Fetched fa[kMxgSub];
    MxmB cur, nxt;
    mxg_v8i a[kMxgSub];
    int sa[kMxgSub];
    mxm_fetch<A, FB>(fa, cur, g, rows, n0, 0, lane);
    for (int64_t s = 0; s < steps; ++s) {
#pragma unroll
        for (int i = 0; i < kMxgSub; ++i) A::operand(a[i], sa[i], fa[i], g, rows.at(i), s, lane);
        if (s + 1 < steps) mxm_fetch<A, FB>(fa, nxt, g, rows, n0, s + 1, lane);
#pragma unroll
        for (int i = 0; i < kMxgSub; ++i)
#pragma unroll
            for (int j = 0; j < kMxgSub; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a[i], cur.b[j], acc[i][j], A::F, FB, 0, sa[i], 0,
                                                                             cur.sb[j]);
        cur = nxt;
    }
    Store::store(acc, g, m0, n0, lane);
}

// Which A an entry point launches: stored codes, x (on the 4-B or the 16-B path), or the
// im2col rows of an NCHW x (the general gather or the pointwise variant).
enum MxmSource { kMxmStored, kMxmFp32, kMxmFp32Vec, kMxmConv, kMxmConvPointwise };

// The launch of the three entry points.  G: MxmArgs (row-major result) or MxcArgs (NCHW).
template <int FA, int FB, class G>
void mxm_launch(const G& g, MxmSource src, int64_t grid, hipStream_t s) {
    const dim3 blocks((unsigned)grid), threads(kThreads);
    if constexpr (std::is_same<G, MxcArgs>::value) {
        if (src == kMxmConvPointwise) hipLaunchKernelGGL((mx_mm_kernel<MxmConvA<FA, true>, FB, MxmNchwStore>), blocks, threads, 0, s, g);
        else hipLaunchKernelGGL((mx_mm_kernel<MxmConvA<FA, false>, FB, MxmNchwStore>), blocks, threads, 0, s, g);
    } else {
        if (src == kMxmStored) hipLaunchKernelGGL((mx_mm_kernel<MxmStoredA<FA>, FB, MxmRowMajorStore>), blocks, threads, 0, s, g);
        else if (src == kMxmFp32Vec) hipLaunchKernelGGL((mx_mm_kernel<MxmFp32A<FA, true>, FB, MxmRowMajorStore>), blocks, threads, 0, s, g);
        else hipLaunchKernelGGL((mx_mm_kernel<MxmFp32A<FA, false>, FB, MxmRowMajorStore>), blocks, threads, 0, s, g);
    }
}
template <int FA, class G>
void mxm_launch_b(int fb, const G& g, MxmSource src, int64_t grid, hipStream_t s) {
    switch (fb) {
        case 0: return mxm_launch<FA, 0>(g, src, grid, s);
        case 2: return mxm_launch<FA, 2>(g, src, grid, s);
        case 3: return mxm_launch<FA, 3>(g, src, grid, s);
        default: return mxm_launch<FA, 4>(g, src, grid, s);
    }
}
// fa / fb: mxg_hw_format of the two DFQ_MX_* formats (checked).
template <class G>
int mxm_run(int fa, int fb, const G& g, MxmSource src, int64_t grid, void* stream) {
    static_assert(kMxgWaves * kWave == kThreads, "four waves per block");
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (fa) {
        case 0: mxm_launch_b<0>(fb, g, src, grid, s); break;
        case 2: mxm_launch_b<2>(fb, g, src, grid, s); break;
        case 3: mxm_launch_b<3>(fb, g, src, grid, s); break;
        default: mxm_launch_b<4>(fb, g, src, grid, s); break;
    }
    DFQ_LAUNCH_CHECK();
    return DFQ_OK;
}

}  // namespace
}  // namespace dfq

using namespace dfq;

extern "C" int dfq_mx_gemm(const dfq_mx_gemm_desc* d, void* stream) {
    int64_t grid = 0;
    const int rc = mxg_check(d, grid);
    if (rc != DFQ_OK) return rc;
    const MxmArgs g{d->a_codes, static_cast<const uint8_t*>(d->b_codes), static_cast<const uint8_t*>(d->b_scales), d->bias, d->out,
                    0, d->ldo, d->M, d->N, d->K, mxg_blocks(d->K), static_cast<const uint8_t*>(d->a_scales)};
    return mxm_run(mxg_hw_format(d->a_format), mxg_hw_format(d->b_format), g, kMxmStored, grid, stream);
}

extern "C" int dfq_mx_linear(const dfq_mx_linear_desc* d, void* stream) {
    int64_t grid = 0;
    const int rc = mxl_check(d, grid);
    if (rc != DFQ_OK) return rc;
    const MxmArgs g{d->x, static_cast<const uint8_t*>(d->b_codes), static_cast<const uint8_t*>(d->b_scales), d->bias, d->out,
                    d->ldx, d->ldo, d->M, d->N, d->K, mxg_blocks(d->K), nullptr};
    const bool vec = mxl_vec(reinterpret_cast<uintptr_t>(d->x), d->ldx, d->K);
    return mxm_run(mxg_hw_format(d->x_format), mxg_hw_format(d->b_format), g, vec ? kMxmFp32Vec : kMxmFp32, grid, stream);
}

extern "C" int dfq_mx_conv2d(const dfq_mx_conv2d_desc* d, void* stream) {
    MxcArgs g{};
    int64_t grid = 0;
    const int rc = mxc_check(d, g.c, g.M, g.K, grid);
    if (rc != DFQ_OK) return rc;
    g.a = d->x;
    g.b_codes = static_cast<const uint8_t*>(d->b_codes);
    g.b_scales = static_cast<const uint8_t*>(d->b_scales);
    g.bias = d->bias;
    g.out = d->out;
    g.N = d->N;
    g.nb = mxg_blocks(g.K);
    // the diagnostics build's switch: scripts/mx_conv_time.py's A/B of the pointwise variant
    const bool pointwise = mxc_pointwise(g.c) && !ab_env("DFQ_MX_CONV_GENERAL");
    return mxm_run(mxg_hw_format(d->x_format), mxg_hw_format(d->b_format), g, pointwise ? kMxmConvPointwise : kMxmConv, grid, stream);
}
