// Device pieces dfq_mx_gemm.hip and dfq_mx_linear.hip share: the operand register types, the
// load of one operand fragment from stored MX codes and scale bytes, and the store of a wave's
// accumulators (dfq_mx_linear's).  All addressing is dfq_mx_gemm_plan.h's.
#pragma once
#include "dfq_common.h"
#include "dfq_mx_gemm_plan.h"

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
// past N not stored: dfq_mx_gemm's epilogue, which that kernel keeps written out in place so
// that its instruction stream stays what it was.
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

}  // namespace
}  // namespace dfq
