// Bias correction of the DFQ path (gfx950): bias_correction.py:15-106,170-172,
// 206-213.  The per-op kernels (expectation, apply, propagate), the one-launch
// layer kernel for the op groups dfq_bc_chain fuses, and the chain's batched
// copies.  Latency-bound row / column reductions in ATen's summation order: no
// MFMA.  fp32 arithmetic is ordered exactly as the reference's torch CPU ops (one
// rounding per op; -ffp-contract=off, IEEE div/sqrt).  The op checks and the
// grouping are host-only code: dfq_transform_plan.cpp.
#include "dfq_common.h"
#include "dfq_transform_plan.h"

#include <algorithm>

namespace dfq {

// calculate_mean of one BN channel (:33-53): scipy's pdf / cdf in float64 on the
// fp32 argument, the rest in fp32.
__device__ __forceinline__ float bc_expect_value(float wj, float bj, int relu) {
    if (!relu) return bj;
    const float x = (-bj) / wj;               // -bias/weight (fp32)
    const float pdf = std_pdf(x), cdf = std_cdf(x);
    float ex = wj * pdf + bj * (1.0f - cdf);  // torch finishes in fp32
    if (ex < 0.0f) ex = 0.0f;                  // expect[expect < 0] = 0
    return ex;
}

__global__ void bc_expect_kernel(const float* __restrict__ w, const float* __restrict__ b, int64_t n, int relu,
                                 int accumulate, float* __restrict__ out) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
        const float ex = bc_expect_value(w[j], b[j], relu);
        out[j] = accumulate ? out[j] + ex : ex;
    }
}

// Element [r, j] of E (+) expect under torch's broadcasting of [o, i2] + [f]
// (ebc: i2 > 1, xbc: f > 1; bc_bcols columns).
struct BcElem {
    const float* E;
    const float* ex;
    int64_t i2;
    bool ebc, xbc;
    __device__ __forceinline__ float operator()(int64_t r, int64_t j) const {
        return E[r * i2 + (ebc ? j : 0)] + ex[xbc ? j : 0];
    }
};

// A column of view(-1, F) summed over its nrows values `get` in ATen's order:
// the column's cascade (`cascade`: aten_outer_col_is_cascade) or ILP row_sum as a
// wave-parallel tree; one column (F == 1) is no outer reduction but the contiguous
// sum, which the caller supplies.  scratch: this wave's kBcScratch + kBcScratch / 16 floats.
template <typename Get, typename Contig>
__device__ __forceinline__ float bc_col_sum(Get get, Contig contiguous, int64_t nrows, int64_t F, bool cascade,
                                            int lane, float* scratch) {
    float* b1s = scratch + kBcScratch;
    return F == 1    ? contiguous()
           : cascade ? wave_cascade(get, nrows, lane, scratch, b1s, kBcScratch)
                     : wave_row_sum(get, nrows, lane, scratch, b1s, kBcScratch);
}

// APPLY's update: bias[r] += mean of the row's n values (bias.view(O, -1).mean(dim=1)).
__device__ __forceinline__ void bc_add_mean(float* bias, int64_t r, float sum, int64_t n) {
    bias[r] = bias[r] + sum / (float)n;
}
// PROPAGATE's update: fake_b[c] += mean of the negated column (sum(-v) == -sum(v) exactly).
__device__ __forceinline__ void bc_sub_mean(float* fake_b, int64_t c, float sum, int64_t n) {
    fake_b[c] = fake_b[c] + (-sum) / (float)n;
}

// One wave per output row: bias_vec[r, :] = E (+) expect, bias[r] += mean in
// ATen's order (bias.view(O, -1).mean(dim=1)): the 32 (vector lane, ILP) streams
// of the row run on 32 lanes, the combine on lane 0 (wave_inner_sum).
__global__ void __launch_bounds__(kThreads)
bc_apply_kernel(const float* __restrict__ E, int64_t o, int64_t i2, const float* __restrict__ ex, int64_t f,
                int64_t bcols, float* __restrict__ bias, float* __restrict__ bias_vec) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * (kThreads / 64);
    const BcElem elem{E, ex, i2, i2 > 1, f > 1};
    for (int64_t r = wave; r < o; r += nwaves) {
        auto get = [&](int64_t j) { return elem(r, j); };
        if (bias_vec)
            for (int64_t j = lane; j < bcols; j += 64) bias_vec[r * bcols + j] = get(j);
        const float sum = wave_inner_sum(get, bcols, lane);
        if (lane == 0) bc_add_mean(bias, r, sum, bcols);
    }
}

// One wave per BN channel: fake_b[c] += mean_r(-bias_vec[r*f + c]) in ATen's
// order for bias_prev.view(-1, F).mean(0) with `threads` intra-op threads.
__global__ void __launch_bounds__(kThreads)
bc_propagate_kernel(const float* __restrict__ bias_vec, int64_t nrows, int64_t f, int threads,
                    float* __restrict__ fake_b) {
    __shared__ float scratch[kThreads / 64][kBcScratch + kBcScratch / 16];
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int64_t wave = (int64_t)blockIdx.x * (kThreads / 64) + wv;
    const int64_t nwaves = (int64_t)gridDim.x * (kThreads / 64);
    for (int64_t c = wave; c < f; c += nwaves) {
        auto get = [&](int64_t r) { return bias_vec[r * f + c]; };
        const float sum = bc_col_sum(get, [&] { return wave_full_sum(get, nrows, threads, lane, scratch[wv]); }, nrows, f,
                                     aten_outer_col_is_cascade(nrows, f, c, threads), lane, scratch[wv]);
        if (lane == 0) bc_sub_mean(fake_b, c, sum, nrows);
    }
}

// One target layer of the bias-correction walk in ONE launch: the op group
// EXPECT+ -> APPLY (-> PROPAGATE) that dfq_bc_chain records per layer
// (bias_correction.py:170-172,196-213,231-251).  Every block first evaluates the
// layer's expectation vector (the branch's BN terms summed in op order) into
// LDS; blocks [0, apply_blocks) then take the APPLY rows (bias += mean_j
// (E (+) expect)[o, j], bias_vec written), the rest the PROPAGATE columns of
// bias_vec.view(-1, F) -- recomputing each element fl(E + expect) instead of
// reading what the apply blocks store, so the two run in the same launch.
// Same per-element values and the same reduction trees as bc_expect_kernel /
// bc_apply_kernel / bc_propagate_kernel: bit-identical, one dependent launch
// per layer instead of three (MobileNetV2: 173 -> 55 launches).
//
// Rows / columns of at most kBcStage values are first staged into LDS by all 64
// lanes of the wave (independent loads in flight together), then summed in
// ATen's order from LDS: the order's lane-serial parts (cascade tails, the
// 32-stream inner sums) read LDS instead of issuing one dependent global load
// per element (a 96-row propagate column took ~50 us that way, DFQ trace
// profiles/r04/r04i_bc).
__global__ void __launch_bounds__(kThreads) bc_layer_kernel(BcLayerJob J) {
    __shared__ float ex[kBcMaxExpect];
    __shared__ float scratch[kThreads / 64][kBcScratch + kBcScratch / 16];
    __shared__ float stage[kThreads / 64][kBcStage];
    for (int64_t j = threadIdx.x; j < J.f; j += kThreads) {
        float v = bc_expect_value(J.ew[0][j], J.eb[0][j], J.relu[0]);
        for (int t = 1; t < J.nterms; ++t) v = v + bc_expect_value(J.ew[t][j], J.eb[t][j], J.relu[t]);
        ex[j] = v;
        if (blockIdx.x == 0) J.expect_out[j] = v;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const bool ebc = J.i2 > 1, xbc = J.f > 1;
    if ((int64_t)blockIdx.x < J.apply_blocks) {
        const BcElem elem{J.E, ex, J.i2, ebc, xbc};
        const int64_t wave = (int64_t)blockIdx.x * (kThreads / 64) + wv;
        const int64_t nwaves = J.apply_blocks * (kThreads / 64);
        float* rowv = stage[wv];
        for (int64_t r = wave; r < J.o; r += nwaves) {
            for (int64_t j = lane; j < J.bcols; j += 64) {   // bcols <= kBcStage (bc_layer_group)
                const float v = elem(r, j);
                rowv[j] = v;
                if (J.vec) J.vec[r * J.bcols + j] = v;
            }
            wave_lds_sync();
            const float sum = wave_inner_sum([&](int64_t j) { return rowv[j]; }, J.bcols, lane);
            wave_lds_sync();   // rowv is rewritten by the next row
            if (lane == 0) bc_add_mean(J.bias, r, sum, J.bcols);
        }
        return;
    }
    const int64_t wave = ((int64_t)blockIdx.x - J.apply_blocks) * (kThreads / 64) + wv;
    const int64_t nwaves = ((int64_t)gridDim.x - J.apply_blocks) * (kThreads / 64);
    float* colv = stage[wv];
    const BcElem elem{J.E, ex, J.i2, ebc, xbc};
    for (int64_t c = wave; c < J.F; c += nwaves) {
        auto get = [&](int64_t r) {   // 32-bit index math: o * bcols < 2^31 (bc_layer_group)
            const uint32_t idx = (uint32_t)r * (uint32_t)J.F + (uint32_t)c;
            const uint32_t row = idx / (uint32_t)J.bcols, j = idx - row * (uint32_t)J.bcols;
            return elem(row, j);
        };
        const bool cascade = aten_outer_col_is_cascade(J.nrows, J.F, c, J.threads);
        for (int64_t r = lane; r < J.nrows; r += 64) colv[r] = get(r);   // nrows <= kBcStage (bc_layer_group)
        wave_lds_sync();
        auto lds = [&](int64_t r) { return colv[r]; };
        // (one column: the contiguous sum, serial at nrows <= kBcStage < 32768)
        const float sum = bc_col_sum(lds, [&] { return wave_inner_sum(lds, J.nrows, lane); }, J.nrows, J.F, cascade, lane,
                                     scratch[wv]);
        wave_lds_sync();   // colv is rewritten by the next column
        if (lane == 0) bc_sub_mean(J.fake_b, c, sum, J.nrows);
    }
}

__global__ void __launch_bounds__(256) copy_batch_kernel(CopyBatch b) {
    const int k = blockIdx.y;
    const float* __restrict__ src = b.src[k];
    float* __restrict__ dst = b.dst[k];
    const int64_t n = b.n[k];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        dst[i] = src[i];
}

}  // namespace dfq

using namespace dfq;

// ============================================================================
// C ABI
// ============================================================================
extern "C" int dfq_bc_expect(const float* fake_w, const float* fake_b, int64_t n, int32_t relu, int32_t accumulate,
                             float* out, void* stream) {
    const int rc = bc_check_op(dfq_bc_op{DFQ_BC_OP_EXPECT, 0, fake_w, fake_b, out, nullptr, n, 0, 0});
    if (rc != DFQ_OK) return rc;
    if (n == 0) return DFQ_OK;
    hipLaunchKernelGGL(bc_expect_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                       fake_w, fake_b, n, relu, accumulate, out);
    DFQ_LAUNCH_CHECK();
    return DFQ_OK;
}

extern "C" int dfq_bc_apply(const float* E, int64_t o, int64_t i2, const float* expect, int64_t f, float* bias,
                            float* bias_vec, int64_t* bcols_out, void* stream) {
    const int rc = bc_check_op(dfq_bc_op{DFQ_BC_OP_APPLY, 0, E, expect, bias, bias_vec, o, i2, f});
    if (rc == DFQ_ERR_INVALID) return rc;
    const int64_t bcols = bc_bcols(i2, f);
    if (bcols > 0 && bcols_out) *bcols_out = bcols;   // (also where numel == o is then refused)
    if (rc != DFQ_OK) return rc;
    hipLaunchKernelGGL(bc_apply_kernel, dim3((int)std::min<int64_t>(ceil_div(o, (int64_t)4), 2048)), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), E,
                       o, i2, expect, f, bcols, bias, bias_vec);
    DFQ_LAUNCH_CHECK();
    return DFQ_OK;
}

extern "C" int dfq_bc_propagate(const float* bias_vec, int64_t numel, float* fake_b, int64_t f, int32_t ref_threads,
                                void* stream) {
    const int rc = bc_check_op(dfq_bc_op{DFQ_BC_OP_PROPAGATE, ref_threads, bias_vec, nullptr, fake_b, nullptr, numel, 0, f});
    if (rc != DFQ_OK) return rc;
    hipLaunchKernelGGL(bc_propagate_kernel, dim3((int)std::min<int64_t>(ceil_div(f, (int64_t)4), 2048)), dim3(kThreads),
                       0, static_cast<hipStream_t>(stream),
                       bias_vec, numel / f, f, (int)ref_threads, fake_b);
    DFQ_LAUNCH_CHECK();
    return DFQ_OK;
}

extern "C" int dfq_bc_chain(const dfq_bc_op* ops, int32_t n_ops, int32_t* failed_op, void* stream) {
    if (failed_op) *failed_op = -1;
    if (n_ops < 0 || (n_ops > 0 && !ops)) return DFQ_ERR_INVALID;
    auto fail = [&](int32_t k, int rc) {
        if (failed_op) *failed_op = k;
        return rc;
    };
    // validate everything first: a rejected op enqueues nothing
    for (int32_t k = 0; k < n_ops; ++k) {
        const int rc = bc_check_op(ops[k]);
        if (rc != DFQ_OK) return fail(k, rc);
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    auto launch_failed = [&] {   // the chain's own launches (the per-op entry points check theirs)
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) set_last_hip_error(e);
        return e != hipSuccess;
    };
    for (int32_t k = 0; k < n_ops; ++k) {
        const dfq_bc_op& op = ops[k];
        int rc = DFQ_OK;
        if (op.kind == DFQ_BC_OP_EXPECT) {   // a layer's EXPECT+ -> APPLY (-> PROPAGATE) group: one launch
            BcLayerJob J{};
            const int32_t used = bc_layer_group(ops, n_ops, k, J);
            if (used > 0) {
                const int64_t pb = J.fake_b ? std::min<int64_t>(ceil_div(J.F, (int64_t)4), 2048) : 0;
                hipLaunchKernelGGL(bc_layer_kernel, dim3((int)(J.apply_blocks + pb)), dim3(kThreads), 0, s, J);
                if (launch_failed()) return fail(k, DFQ_ERR_HIP);
                k += used - 1;
                continue;
            }
        }
        if (op.kind == DFQ_BC_OP_COPY) {   // this copy and the ones right after it: one launch
            CopyBatch b{};
            int cnt;
            int64_t most;
            const int32_t used = bc_copy_run(ops, n_ops, k, b, cnt, most);
            if (cnt > 0) {
                hipLaunchKernelGGL(copy_batch_kernel, dim3(blocks_for(most), cnt), dim3(256), 0, s, b);
                if (launch_failed()) return fail(k, DFQ_ERR_HIP);
            }
            k += used - 1;
            continue;
        }
        if (op.kind == DFQ_BC_OP_EXPECT)
            rc = dfq_bc_expect(op.a, op.b, op.n, op.flag & 1, (op.flag >> 1) & 1, op.out, stream);
        else if (op.kind == DFQ_BC_OP_APPLY)
            rc = dfq_bc_apply(op.a, op.n, op.i2, op.b, op.f, op.out, op.out2, nullptr, stream);
        else
            rc = dfq_bc_propagate(op.a, op.n, op.out, op.f, op.flag, stream);
        if (rc != DFQ_OK) return fail(k, rc);
    }
    return DFQ_OK;
}
