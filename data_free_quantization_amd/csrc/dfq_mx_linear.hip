// dfq_mx_linear: out[m][n] = sum_k Q(x)[m][k] * B[n][k] (+ bias[n]) in one launch -- dfq_mx_gemm
// (dfq_mx_gemm.hip) whose A operand is built in the kernel from the fp32 activation x instead
// of loaded as stored codes (include/dfq_hip.h).
//
// Tiling, the B operand, the accumulators, the K-step order and the stores are dfq_mx_gemm's:
// a wave owns a 32 x 32 output tile, four waves a 64 x 64 block tile, and B's fragments come
// from the stored codes through the same loader.  For A, a lane reads the fp32 elements its
// operand of v_mfma_scale_f32_16x16x128_f8f6f4 stands for -- one MX block of one row for FP4 /
// FP6, two 16-element halves of two blocks for FP8 -- as 16-B loads where the rows of x start
// 16-B aligned and K % 4 == 0 (a kernel instantiation of its own) and as 4-B loads otherwise,
// takes the amax of the magnitudes' bit patterns, derives the floor rule's exponent and encodes (dfq_mx_encode.h, the quantizer's own encoder)
// straight into the operand registers in the stored blocks' bit order
// (dfq_mx_linear_plan.h).  An FP8 lane exchanges its two halves' amax with lane ^ 16 and
// gathers its lane group's block's scale byte from the lane group that knows it: three
// ds_bpermute per fragment, no LDS memory, no barrier.  Every lane of a working wave takes
// part in the exchanges: the only early return is wave-uniform and lies before the loop.
// Elements at k >= K and rows >= M are never read and count as +0; lanes of rows past M and of
// MX blocks past nb hold zero codes with scale byte 127, as in dfq_mx_gemm.  So the operand
// registers are bit for bit the ones dfq_mx_gemm loads from dfq_mx_quantize_batch's codes of
// x, and with one accumulator per output element and the K steps in order so is the result.
// The fp32 elements and B's fragments of step s + 1 are loaded before step s's four
// instructions issue; the encode of step s + 1 follows them.  The A fragment is re-quantized
// by every wave that needs it (once per 32 output columns): the kernel is aimed at
// layer-sized calls.
#include "dfq_mx_gemm_frag.h"
#include "dfq_mx_linear_plan.h"

namespace dfq {
namespace {

struct MxlArgs {
    const float* x;
    const uint8_t* b_codes;
    const uint8_t* b_scales;
    const float* bias;
    float* out;
    int64_t ldx, ldo, M, N, K, nb;
};

// The lane's 32 fp32 elements of instruction tile row `row` in K step `step`, in slot order.
// VEC: the 16-B path (mxl_vec).
template <int FA, bool VEC>
__device__ __forceinline__ void mxl_load_x(float (&v)[DFQ_MX_BLOCK], const MxlArgs& g, int64_t row, int64_t step, int lane) {
    const DFQ_GLOBAL float* x = (const DFQ_GLOBAL float*)g.x;
    constexpr int n = mxl_part_len(FA);
#pragma unroll
    for (int part = 0; part < mxl_parts(FA); ++part) {
        const int64_t k0 = mxl_part_k(FA, step, lane, part);
        const DFQ_GLOBAL float* p = x + mxl_x_offset(row < g.M ? row : 0, k0 < g.K ? k0 : 0, g.ldx);   // never past the array
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

__device__ __forceinline__ uint32_t mxl_from_lane(int src_lane, uint32_t v) {
    return (uint32_t)__builtin_amdgcn_ds_bpermute(4 * src_lane, (int)v);
}

// The lane's fp32 elements as the instruction's A operand: registers and scale byte.
template <int FA>
__device__ __forceinline__ void mxl_quantize(mxg_v8i& a, int& s, const float (&v)[DFQ_MX_BLOCK], const MxlArgs& g, int64_t row,
                                             int64_t step, int lane) {
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

struct MxlB {
    mxg_v8i b[kMxgSub];
    int sb[kMxgSub];
};
struct MxlX {
    float v[kMxgSub][DFQ_MX_BLOCK];
};

template <int FA, int FB, bool VEC>
__device__ __forceinline__ void mxl_load(MxlX& xs, MxlB& f, const MxlArgs& g, int64_t m0, int64_t n0, int64_t step, int lane) {
#pragma unroll
    for (int i = 0; i < kMxgSub; ++i) {
        mxl_load_x<FA, VEC>(xs.v[i], g, mxg_lane_row(m0, i, lane), step, lane);
        mxg_load_operand<FB>(f.b[i], f.sb[i], g.b_codes, g.b_scales, mxg_lane_row(n0, i, lane), g.N, g.nb, step, lane);
    }
}

// FA / FB: the instruction's format fields (cbsz / blgp) of Q(x) and B.  VEC: x on the 16-B path.
template <int FA, int FB, bool VEC>
__global__ __launch_bounds__(kThreads) void mx_linear_kernel(const MxlArgs g) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int64_t m0 = mxg_wave_m0(blockIdx.x, wave, g.N), n0 = mxg_wave_n0(blockIdx.x, wave, g.N);
    if (!mxg_wave_works(m0, n0, g.M, g.N)) return;   // wave-uniform; the kernel has no barrier
    mxg_v4f acc[kMxgSub][kMxgSub];
#pragma unroll
    for (int i = 0; i < kMxgSub; ++i)
#pragma unroll
        for (int j = 0; j < kMxgSub; ++j) acc[i][j] = mxg_v4f{0.f, 0.f, 0.f, 0.f};
    const int64_t steps = mxg_steps(g.nb);
    MxlX xs;
    MxlB cur, nxt;
    mxg_v8i a[kMxgSub];
    int sa[kMxgSub];
    mxl_load<FA, FB, VEC>(xs, cur, g, m0, n0, 0, lane);
    for (int64_t s = 0; s < steps; ++s) {
#pragma unroll
        for (int i = 0; i < kMxgSub; ++i) mxl_quantize<FA>(a[i], sa[i], xs.v[i], g, mxg_lane_row(m0, i, lane), s, lane);
        if (s + 1 < steps) mxl_load<FA, FB, VEC>(xs, nxt, g, m0, n0, s + 1, lane);
#pragma unroll
        for (int i = 0; i < kMxgSub; ++i)
#pragma unroll
            for (int j = 0; j < kMxgSub; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a[i], cur.b[j], acc[i][j], FA, FB, 0, sa[i], 0,
                                                                             cur.sb[j]);
        cur = nxt;
    }
    mxg_store_tile(acc, g.out, g.bias, g.ldo, g.M, g.N, m0, n0, lane);
}

template <int FA, int FB>
void mxl_launch(const MxlArgs& g, bool vec, int64_t grid, hipStream_t s) {
    if (vec) hipLaunchKernelGGL((mx_linear_kernel<FA, FB, true>), dim3((unsigned)grid), dim3(kThreads), 0, s, g);
    else hipLaunchKernelGGL((mx_linear_kernel<FA, FB, false>), dim3((unsigned)grid), dim3(kThreads), 0, s, g);
}
template <int FA>
void mxl_launch_b(int fb, const MxlArgs& g, bool vec, int64_t grid, hipStream_t s) {
    switch (fb) {
        case 0: return mxl_launch<FA, 0>(g, vec, grid, s);
        case 2: return mxl_launch<FA, 2>(g, vec, grid, s);
        case 3: return mxl_launch<FA, 3>(g, vec, grid, s);
        default: return mxl_launch<FA, 4>(g, vec, grid, s);
    }
}

}  // namespace
}  // namespace dfq

using namespace dfq;

extern "C" int dfq_mx_linear(const dfq_mx_linear_desc* d, void* stream) {
    int64_t grid = 0;
    const int rc = mxl_check(d, grid);
    if (rc != DFQ_OK) return rc;
    static_assert(kMxgWaves * kWave == kThreads, "four waves per block");
    const MxlArgs g{d->x, static_cast<const uint8_t*>(d->b_codes), static_cast<const uint8_t*>(d->b_scales), d->bias, d->out,
                    d->ldx, d->ldo, d->M, d->N, d->K, mxg_blocks(d->K)};
    const bool vec = mxl_vec(reinterpret_cast<uintptr_t>(d->x), d->ldx, d->K);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int fb = mxg_hw_format(d->b_format);
    switch (mxg_hw_format(d->x_format)) {
        case 0: mxl_launch_b<0>(fb, g, vec, grid, s); break;
        case 2: mxl_launch_b<2>(fb, g, vec, grid, s); break;
        case 3: mxl_launch_b<3>(fb, g, vec, grid, s); break;
        default: mxl_launch_b<4>(fb, g, vec, grid, s); break;
    }
    DFQ_LAUNCH_CHECK();
    return DFQ_OK;
}
