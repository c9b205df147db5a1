// dfq_mx_gemm: out[m][n] = sum_k A[m][k] * B[n][k] (+ bias[n]) on the scaled matrix
// instruction v_mfma_scale_f32_16x16x128_f8f6f4, both operands read as the MX codes and
// E8M0 scale bytes dfq_mx_quantize_batch writes (include/dfq_hip.h).
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
// waves make a 64 x 64 block tile.  The next step's fragments are loaded before this
// step's four instructions issue.  Lanes of rows past M / N and of MX blocks past nb issue
// no load and hold zero codes with scale byte 127; such rows are not stored.  No LDS, no
// workspace, no atomics, no split of K: an output element is one accumulator of one lane,
// added up in K-step order, then one fp32 add of the bias.
#include "dfq_mx_gemm_frag.h"

namespace dfq {
namespace {

struct MxgArgs {
    const uint8_t* a_codes;
    const uint8_t* a_scales;
    const uint8_t* b_codes;
    const uint8_t* b_scales;
    const float* bias;
    float* out;
    int64_t ldo, M, N, nb;
};

// A wave's operands of one K step: fragment i of each operand is instruction tile i's;
// s is the lane group's MX block's scale byte in bits [0, 8) (opsel 0).
struct MxgFrags {
    mxg_v8i a[kMxgSub], b[kMxgSub];
    int sa[kMxgSub], sb[kMxgSub];
};

template <int FA, int FB>
__device__ __forceinline__ void mxg_load(MxgFrags& f, const MxgArgs& g, int64_t m0, int64_t n0, int64_t step, int lane) {
#pragma unroll
    for (int i = 0; i < kMxgSub; ++i) {
        mxg_load_operand<FA>(f.a[i], f.sa[i], g.a_codes, g.a_scales, mxg_lane_row(m0, i, lane), g.M, g.nb, step, lane);
        mxg_load_operand<FB>(f.b[i], f.sb[i], g.b_codes, g.b_scales, mxg_lane_row(n0, i, lane), g.N, g.nb, step, lane);
    }
}

// FA / FB: the instruction's format fields (cbsz / blgp) of A and B.
template <int FA, int FB>
__global__ __launch_bounds__(kThreads) void mx_gemm_kernel(const MxgArgs g) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int64_t m0 = mxg_wave_m0(blockIdx.x, wave, g.N), n0 = mxg_wave_n0(blockIdx.x, wave, g.N);
    if (!mxg_wave_works(m0, n0, g.M, g.N)) return;   // wave-uniform; the kernel has no barrier
    mxg_v4f acc[kMxgSub][kMxgSub];
#pragma unroll
    for (int i = 0; i < kMxgSub; ++i)
#pragma unroll
        for (int j = 0; j < kMxgSub; ++j) acc[i][j] = mxg_v4f{0.f, 0.f, 0.f, 0.f};
    const int64_t steps = mxg_steps(g.nb);
    MxgFrags cur, nxt;
    mxg_load<FA, FB>(cur, g, m0, n0, 0, lane);
    for (int64_t s = 0; s < steps; ++s) {
        if (s + 1 < steps) mxg_load<FA, FB>(nxt, g, m0, n0, s + 1, lane);
#pragma unroll
        for (int i = 0; i < kMxgSub; ++i)
#pragma unroll
            for (int j = 0; j < kMxgSub; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(cur.a[i], cur.b[j], acc[i][j], FA, FB, 0,
                                                                             cur.sa[i], 0, cur.sb[j]);
        cur = nxt;
    }
    DFQ_GLOBAL float* out = (DFQ_GLOBAL float*)g.out;
    const DFQ_GLOBAL float* bias = (const DFQ_GLOBAL float*)g.bias;
#pragma unroll
    for (int j = 0; j < kMxgSub; ++j) {
        const int64_t col = mxg_out_col(n0, j, lane);
        const float bv = bias != nullptr && col < g.N ? bias[col] : 0.f;
#pragma unroll
        for (int i = 0; i < kMxgSub; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t row = mxg_out_row(m0, i, lane, r);
                if (!mxg_stores(row, col, g.M, g.N)) continue;
                const float v = acc[i][j][r];
                out[mxg_out_offset(row, col, g.ldo)] = bias != nullptr ? v + bv : v;
            }
    }
}

template <int FA, int FB>
void mxg_launch(const MxgArgs& g, int64_t grid, hipStream_t s) {
    hipLaunchKernelGGL((mx_gemm_kernel<FA, FB>), dim3((unsigned)grid), dim3(kThreads), 0, s, g);
}
template <int FA>
void mxg_launch_b(int fb, const MxgArgs& g, int64_t grid, hipStream_t s) {
    switch (fb) {
        case 0: return mxg_launch<FA, 0>(g, grid, s);
        case 2: return mxg_launch<FA, 2>(g, grid, s);
        case 3: return mxg_launch<FA, 3>(g, grid, s);
        default: return mxg_launch<FA, 4>(g, grid, s);
    }
}

}  // namespace
}  // namespace dfq

using namespace dfq;

extern "C" int dfq_mx_gemm(const dfq_mx_gemm_desc* d, void* stream) {
    int64_t grid = 0;
    const int rc = mxg_check(d, grid);
    if (rc != DFQ_OK) return rc;
    static_assert(kMxgWaves * kWave == kThreads, "four waves per block");
    const MxgArgs g{static_cast<const uint8_t*>(d->a_codes), static_cast<const uint8_t*>(d->a_scales),
                    static_cast<const uint8_t*>(d->b_codes), static_cast<const uint8_t*>(d->b_scales),
                    d->bias, d->out, d->ldo, d->M, d->N, mxg_blocks(d->K)};
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int fb = mxg_hw_format(d->b_format);
    switch (mxg_hw_format(d->a_format)) {
        case 0: mxg_launch_b<0>(fb, g, grid, s); break;
        case 2: mxg_launch_b<2>(fb, g, grid, s); break;
        case 3: mxg_launch_b<3>(fb, g, grid, s); break;
        default: mxg_launch_b<4>(fb, g, grid, s); break;
    }
    DFQ_LAUNCH_CHECK();
    return DFQ_OK;
}
