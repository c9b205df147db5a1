// Graph-transform kernels of the DFQ path (gfx950): BatchNorm folding, weight
// clipping and high-bias absorption (bias correction: dfq_bc.hip; activation
// ranges and fake quant: dfq_act.hip).  All are HBM/latency-bound elementwise or
// row reductions: no MFMA.  fp32 arithmetic is ordered exactly as the reference's
// torch CPU ops (one rounding per op; -ffp-contract=off, IEEE div/sqrt).  The
// batched paths' tables are host-only code: dfq_transform_plan.cpp.
#include "dfq_common.h"
#include "dfq_transform_plan.h"

#include <cstring>

#include <algorithm>
#include <vector>

namespace dfq {

// ---------------------------------------------------------------------------
// BatchNorm folding: utils/layer_transform.py:255-281
// ---------------------------------------------------------------------------
__device__ __forceinline__ float bn_factor(float g, float v, float eps) {
    // bn_weight / torch.sqrt(bn_var + bn_eps)
    return g / sqrtf(v + eps);
}

__global__ void bn_fold_weight_kernel(float* __restrict__ w, const float* __restrict__ g,
                                      const float* __restrict__ v, float eps, int64_t rows, int64_t len) {
    const int64_t n = rows * len;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t o = i / len;
        w[i] = w[i] * bn_factor(g[o], v[o], eps);
    }
}

// Channel o of one fold: the bias / fake-stat update and the BN reset.
__device__ __forceinline__ void bn_fold_channel(const BnFoldJob& J, int64_t o) {
    typedef DFQ_GLOBAL float* G;   // global, not flat
    const G g = (G)J.g, b = (G)J.b, m = (G)J.m, v = (G)J.v, bias = (G)J.bias, fw = (G)J.fake_w, fb = (G)J.fake_b;
    const float go = g[o], bo = b[o], mo = m[o], vo = v[o];
    const float f = bn_factor(go, vo, J.eps);
    // conv_bias.mul(f).add(bn_bias - (bn_weight * bn_mean) / sqrt(bn_var + eps))
    const float shift = bo - (go * mo) / sqrtf(vo + J.eps);
    // a layer without a bias gets torch.zeros first (layer_transform.py:262-263)
    const float b0 = (J.flags & DFQ_BN_FOLD_ZERO_BIAS) ? 0.0f : bias[o];
    bias[o] = b0 * f + shift;
    if (J.fake_w) fw[o] = fabsf(go);
    if (J.fake_b) fb[o] = bo;
    g[o] = 1.0f;
    v[o] = 1.0f;
    b[o] = 0.0f;
    m[o] = 0.0f;
}

__global__ void bn_fold_channel_kernel(float* __restrict__ bias, float* __restrict__ g, float* __restrict__ b,
                                       float* __restrict__ m, float* __restrict__ v, float* __restrict__ fake_w,
                                       float* __restrict__ fake_b, float eps, int64_t rows) {
    const BnFoldJob J{nullptr, bias, g, b, m, v, fake_w, fake_b, eps, 0, rows, 0, nullptr};
    for (int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o < rows; o += (int64_t)gridDim.x * blockDim.x)
        bn_fold_channel(J, o);
}

// The fold factor of row o (bn_factor), without the divide and square root for
// an identity BatchNorm (weight 1, var + eps == 1: the factor is exactly 1).
__device__ __forceinline__ float fold_factor(const BnFoldJob& J, int64_t o) {
    const float go = ((const DFQ_GLOBAL float*)J.g)[o], ve = ((const DFQ_GLOBAL float*)J.v)[o] + J.eps;
    return (go == 1.0f && ve == 1.0f) ? 1.0f : go / sqrtf(ve);
}

// w <- w * factor(row) over one chunk; w * 1 == w, so a factor of exactly 1
// (merge_batchnorm #2, whose BN is the identity the first fold left) rewrites
// nothing.  Row of element i: fold_row (dfq_transform_plan.h).
__device__ __forceinline__ float fold_one(const BnFoldJob& J, int64_t r0, int64_t base, float inv, int64_t i,
                                          float w) {
    int rem;
    const float f = fold_factor(J, fold_row(J.row_len, r0, base, inv, i, &rem));
    return f != 1.0f ? w * f : w;
}

__global__ void __launch_bounds__(kThreads)
bn_fold_weight_batch_kernel(const BnFoldJob* __restrict__ jobs, const BnFoldChunk* __restrict__ chunks,
                            int64_t nchunks) {
    __shared__ float smn[kThreads / kWave], smx[kThreads / kWave];
    for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const BnFoldChunk ch = chunks[c];
        const BnFoldJob J = jobs[ch.job];
        const int64_t r0 = ch.e0 / J.row_len, base = r0 * J.row_len;
        const float inv = 1.0f / (float)J.row_len;
        float a = INFINITY, b = -INFINITY;
        const int64_t n = ch.e1 - ch.e0;
        int64_t done = 0;
        // every row of the chunk with a factor of exactly 1 (merge_batchnorm #2): a
        // read-only stream for the range, 4 x 16 B in flight per thread
        int ident = 1;
        for (int64_t r = r0 + threadIdx.x; r <= (ch.e1 - 1) / J.row_len; r += blockDim.x)
            ident &= fold_factor(J, r) == 1.0f;
        ident = __syncthreads_and(ident);
        if (ident && (reinterpret_cast<uintptr_t>(J.w + ch.e0) & 15) == 0) {
            const DFQ_GLOBAL f32x4* w4 = (const DFQ_GLOBAL f32x4*)(J.w + ch.e0);   // global, not flat
            const int64_t n4 = n >> 2;
            for (int64_t k = threadIdx.x; k < n4; k += 4 * (int64_t)blockDim.x) {
                f32x4 v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (k + u * (int64_t)blockDim.x < n4) v[u] = w4[k + u * blockDim.x];
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (k + u * (int64_t)blockDim.x < n4) {
                        a = fminf(a, fminf(fminf(v[u].x, v[u].y), fminf(v[u].z, v[u].w)));
                        b = fmaxf(b, fmaxf(fmaxf(v[u].x, v[u].y), fmaxf(v[u].z, v[u].w)));
                    }
            }
            done = 4 * n4;
        } else if ((reinterpret_cast<uintptr_t>(J.w + ch.e0) & 15) == 0) {   // 16-B groups
            DFQ_GLOBAL f32x4* w4 = (DFQ_GLOBAL f32x4*)(J.w + ch.e0);
            const int64_t n4 = n >> 2;
            for (int64_t k = threadIdx.x; k < n4; k += blockDim.x) {
                const f32x4 v = w4[k];
                const int64_t i = ch.e0 + 4 * k;
                f32x4 o;
                int rem;
                const float f = fold_factor(J, fold_row(J.row_len, r0, base, inv, i, &rem));
                if (rem + 3 < (int)J.row_len) {   // the 4 elements share a row: one factor
                    o.x = f != 1.0f ? v.x * f : v.x;
                    o.y = f != 1.0f ? v.y * f : v.y;
                    o.z = f != 1.0f ? v.z * f : v.z;
                    o.w = f != 1.0f ? v.w * f : v.w;
                } else {
                    o.x = f != 1.0f ? v.x * f : v.x;
                    o.y = fold_one(J, r0, base, inv, i + 1, v.y);
                    o.z = fold_one(J, r0, base, inv, i + 2, v.z);
                    o.w = fold_one(J, r0, base, inv, i + 3, v.w);
                }
                if (__float_as_uint(o.x) != __float_as_uint(v.x) || __float_as_uint(o.y) != __float_as_uint(v.y) ||
                    __float_as_uint(o.z) != __float_as_uint(v.z) || __float_as_uint(o.w) != __float_as_uint(v.w))
                    w4[k] = o;
                a = fminf(a, fminf(fminf(o.x, o.y), fminf(o.z, o.w)));
                b = fmaxf(b, fmaxf(fmaxf(o.x, o.y), fmaxf(o.z, o.w)));
            }
            done = 4 * n4;
        }
        DFQ_GLOBAL float* wg = (DFQ_GLOBAL float*)J.w;
        for (int64_t k = done + threadIdx.x; k < n; k += blockDim.x) {
            const int64_t i = ch.e0 + k;
            const float v = wg[i];
            const float o = fold_one(J, r0, base, inv, i, v);
            if (__float_as_uint(o) != __float_as_uint(v)) wg[i] = o;
            a = fminf(a, o);
            b = fmaxf(b, o);
        }
        if (J.range_enc) {   // the folded weight's (min, max), dfq_range's encoding
            block_minmax(a, b, smn, smx);
            if (threadIdx.x == 0) {
                atomicMax(&J.range_enc[0], ~enc_ord(a));
                atomicMax(&J.range_enc[1], enc_ord(b));
            }
            __syncthreads();   // smn / smx are rewritten by the next chunk
        }
    }
}

// One block per job: the per-channel update (after every weight has used the old
// BN parameters: a separate launch).
__global__ void bn_fold_channel_batch_kernel(const BnFoldJob* __restrict__ jobs, int32_t njobs) {
    for (int32_t j = blockIdx.x; j < njobs; j += gridDim.x) {
        const BnFoldJob J = jobs[j];
        for (int64_t o = threadIdx.x; o < J.rows; o += blockDim.x) bn_fold_channel(J, o);
    }
}

// ---------------------------------------------------------------------------
// clip_weight: clip_weight.py:29  (layer.weight.data.clamp_(lo, hi))
// ---------------------------------------------------------------------------
// Up to kClampBatch weights per launch, the batch in the kernel arguments
// (blockIdx.y picks the tensor; each is 16-B aligned, float4 body + scalar tail).
constexpr int kClampBatch = 64;
struct ClampBatch {
    float* w[kClampBatch];
    int64_t n[kClampBatch];
};

__global__ void __launch_bounds__(kThreads) clamp_batch_kernel(ClampBatch b, float lo, float hi) {
    float* __restrict__ w = b.w[blockIdx.y];
    const int64_t n = b.n[blockIdx.y];
    const int64_t n4 = n >> 2;
    float4* w4 = reinterpret_cast<float4*>(w);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        float4 v = w4[i];
        v.x = fminf(fmaxf(v.x, lo), hi);
        v.y = fminf(fmaxf(v.y, lo), hi);
        v.z = fminf(fmaxf(v.z, lo), hi);
        v.w = fminf(fmaxf(v.w, lo), hi);
        w4[i] = v;
    }
    for (int64_t i = 4 * n4 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        w[i] = fminf(fmaxf(w[i], lo), hi);
}

// ---------------------------------------------------------------------------
// High-bias absorption: bias_absorption.py:147-197
// ---------------------------------------------------------------------------
__device__ __forceinline__ float absorb_c(float beta, float gamma, float n_sigma) {
    float c = beta - n_sigma * gamma;   // bn_beta - N * bn_gamma
    return (c < 0.0f) ? 0.0f : c;       // clamp_(0), NaN kept
}

// sum_i (sum_k W2[o,i,k]) * c[g*i2 + i] by one wave (every lane ends with it).
__device__ __forceinline__ float absorb_row(const float* w2, const float* bn_w, const float* bn_b, int64_t o,
                                            int64_t i2, int64_t khw2, int64_t o2g, float n_sigma, int lane) {
    const int64_t g = o / o2g;
    const float* row = w2 + o * i2 * khw2;
    float acc = 0.f;
    for (int64_t i = lane; i < i2; i += 64) {
        float ssum = 0.f;
        for (int64_t k = 0; k < khw2; ++k) ssum += row[i * khw2 + k];
        const int64_t ch = g * i2 + i;
        acc += ssum * absorb_c(bn_b[ch], bn_w[ch], n_sigma);
    }
    return wave_sum_f(acc);
}

// b2[o] += absorb_row(o): one wave per output row.
__global__ void absorb_gemv_kernel(const float* __restrict__ w2, float* __restrict__ b2,
                                   const float* __restrict__ bn_w, const float* __restrict__ bn_b,
                                   int64_t o2, int64_t i2, int64_t khw2, int64_t o2g, float n_sigma) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x / 64);
    for (int64_t o = wave; o < o2; o += nwaves) {
        const float acc = absorb_row(w2, bn_w, bn_b, o, i2, khw2, o2g, n_sigma, lane);
        if (lane == 0) b2[o] = b2[o] + acc;
    }
}

__global__ void absorb_channel_kernel(float* __restrict__ b1, float* __restrict__ bn_b, const float* __restrict__ bn_w,
                                      int64_t c1, float n_sigma) {
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < c1; c += (int64_t)gridDim.x * blockDim.x) {
        const float cc = absorb_c(bn_b[c], bn_w[c], n_sigma);
        b1[c] = b1[c] + (-cc);
        bn_b[c] = bn_b[c] + (-cc);
    }
}

// ---- batched absorption (the tables: absorb_tables, dfq_transform_plan.cpp) ----
__global__ void absorb_batch_gemv_kernel(const AbsRel* __restrict__ rels, const AbsRows* __restrict__ tasks,
                                         int64_t ntasks, float* __restrict__ wc, float n_sigma) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x / 64);
    for (int64_t t = wave; t < ntasks; t += nwaves) {
        const AbsRows tk = tasks[t];
        const AbsRel R = rels[tk.r];
        for (int64_t o = tk.o0; o < tk.o1; ++o) {
            const float acc = absorb_row(R.w2, R.bn_w, R.bn_b, o, R.i2, R.khw2, R.o2g, n_sigma, lane);
            if (lane == 0) wc[R.wc + o] = acc;
        }
    }
}

__global__ void absorb_batch_bias_kernel(const AbsRel* __restrict__ rels, const AbsVec* __restrict__ vecs,
                                         const AbsOp* __restrict__ ops, const AbsElems* __restrict__ tasks,
                                         int64_t ntasks, const float* __restrict__ wc, float n_sigma) {
    for (int64_t t = blockIdx.x; t < ntasks; t += gridDim.x) {
        const AbsElems tk = tasks[t];
        const AbsVec V = vecs[tk.v];
        for (int64_t e = tk.e0 + threadIdx.x; e < tk.e1; e += blockDim.x) {
            float b = V.b[e];
            for (int32_t q = 0; q < V.nops; ++q) {
                const AbsOp op = ops[V.op0 + q];
                const AbsRel& R = rels[op.r];
                if (op.kind == 0) {
                    b = b + wc[R.wc + e];
                } else {
                    const float cc = absorb_c(R.bn_b[e], R.bn_w[e], n_sigma);
                    b = b + (-cc);
                    R.bn_b[e] = R.bn_b[e] + (-cc);
                }
            }
            V.b[e] = b;
        }
    }
}

}  // namespace dfq

using namespace dfq;

// ============================================================================
// C ABI
// ============================================================================
extern "C" int dfq_bn_fold(float* w, float* bias, float* bn_w, float* bn_b, float* bn_mean, float* bn_var,
                           float* fake_w, float* fake_b, float eps, int64_t rows, int64_t row_len, void* stream) {
    if (!w || !bias || !bn_w || !bn_b || !bn_mean || !bn_var || rows < 0 || row_len < 0) return DFQ_ERR_INVALID;
    if (rows == 0) return DFQ_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(bn_fold_weight_kernel, dim3(blocks_for(rows * row_len, 4)), dim3(kThreads), 0, s,
                       w, bn_w, bn_var, eps, rows, row_len);
    DFQ_LAUNCH_CHECK();
    hipLaunchKernelGGL(bn_fold_channel_kernel, dim3(blocks_for(rows)), dim3(kThreads), 0, s,
                       bias, bn_w, bn_b, bn_mean, bn_var, fake_w, fake_b, eps, rows);
    DFQ_LAUNCH_CHECK();
    return DFQ_OK;
}

extern "C" int dfq_bn_fold_batch(const dfq_bn_fold_desc* d, int32_t n, void* ws, int64_t ws_bytes, void* stream) {
    if (n < 0 || (n > 0 && !d)) return DFQ_ERR_INVALID;
    if (n == 0) return DFQ_OK;
    std::vector<BnFoldJob> jobs;
    std::vector<BnFoldChunk> chunks;
    const int rc = bn_fold_tables(d, n, jobs, chunks);
    if (rc != DFQ_OK) return rc;
    const BnFoldLayout L = bn_fold_layout(d, n);   // (L.nchunks == chunks.size())
    const int64_t jb = L.o_chunks, need = L.total;
    if (ws && (ws_bytes < need || reinterpret_cast<uintptr_t>(ws) % 256 != 0)) return DFQ_ERR_INVALID;
    hipStream_t s = static_cast<hipStream_t>(stream);
    void* own = nullptr;
    if (!ws) {   // no caller workspace: a private one, freed after a stream sync
        DFQ_HIP_CHECK(hipMalloc(&own, need));
        ws = own;
    }
    char* base = static_cast<char*>(ws);
    BnFoldJob* dj = reinterpret_cast<BnFoldJob*>(base);
    BnFoldChunk* dc = reinterpret_cast<BnFoldChunk*>(base + jb);
    // one staging blob, one copy
    std::vector<char> blob(need, 0);
    std::memcpy(blob.data(), jobs.data(), sizeof(BnFoldJob) * n);
    if (!chunks.empty()) std::memcpy(blob.data() + jb, chunks.data(), sizeof(BnFoldChunk) * chunks.size());
    hipError_t e = own ? hipMemcpyAsync(base, blob.data(), need, hipMemcpyHostToDevice, s)
                       : stage_h2d(base, blob.data(), need, s);
    // zero the range outputs: one memset per run of adjacent 2-word records
    std::vector<uint32_t*> rp;
    for (int32_t j = 0; j < n; ++j)
        if (d[j].range_enc) rp.push_back(d[j].range_enc);
    std::sort(rp.begin(), rp.end());
    for (size_t k = 0; k < rp.size() && e == hipSuccess;) {
        size_t m = k + 1;
        while (m < rp.size() && rp[m] == rp[m - 1] + 2) ++m;
        e = hipMemsetAsync(rp[k], 0, sizeof(uint32_t) * 2 * (m - k), s);
        k = m;
    }
    if (e == hipSuccess && !chunks.empty()) {
        hipLaunchKernelGGL(bn_fold_weight_batch_kernel, dim3((int)std::min<size_t>(chunks.size(), 4096)),
                           dim3(kThreads), 0, s, dj, dc, (int64_t)chunks.size());
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(bn_fold_channel_batch_kernel, dim3(std::min(n, 2048)), dim3(kThreads), 0, s, dj, n);
        e = hipGetLastError();
    }
    // Caller workspace: stream-ordered (pinned staging).  Private tables die with
    // this call: wait for the stream then.
    if (e == hipSuccess && own) e = hipStreamSynchronize(s);
    if (own) (void)hipFree(own);
    if (e != hipSuccess) {
        set_last_hip_error(e);
        return DFQ_ERR_HIP;
    }
    return DFQ_OK;
}

extern "C" int dfq_clamp_batch(float* const* w, const int64_t* n, int32_t count, float lo, float hi, void* stream) {
    if (count < 0 || (count > 0 && (!w || !n))) return DFQ_ERR_INVALID;
    for (int32_t k = 0; k < count; ++k)
        if (!w[k] || n[k] < 0 || reinterpret_cast<uintptr_t>(w[k]) % 16) return DFQ_ERR_INVALID;
    for (int32_t k0 = 0; k0 < count; k0 += kClampBatch) {
        ClampBatch b{};
        int cnt = 0;
        int64_t most = 0;
        for (int32_t k = k0; k < std::min(count, k0 + kClampBatch); ++k) {
            if (n[k] == 0) continue;
            b.w[cnt] = w[k];
            b.n[cnt] = n[k];
            most = std::max(most, n[k]);
            ++cnt;
        }
        if (cnt == 0) continue;
        hipLaunchKernelGGL(clamp_batch_kernel, dim3(blocks_for(most, 16), cnt), dim3(kThreads), 0,
                           static_cast<hipStream_t>(stream), b, lo, hi);
        DFQ_LAUNCH_CHECK();
    }
    return DFQ_OK;
}

// One weight: a batch of one (the same checks in the same order, the same grid).
extern "C" int dfq_clamp(float* w, int64_t n, float lo, float hi, void* stream) {
    return dfq_clamp_batch(&w, &n, 1, lo, hi, stream);
}

extern "C" int dfq_bias_absorb(const float* w2, float* b1, float* b2, float* bn_w, float* bn_b, int64_t c1,
                               int64_t o2, int64_t i2, int64_t khw2, float n_sigma, void* stream) {
    if (!w2 || !b1 || !b2 || !bn_w || !bn_b || c1 <= 0 || o2 <= 0 || i2 <= 0 || khw2 <= 0) return DFQ_ERR_INVALID;
    const int64_t groups = c1 / i2;   // bias_absorption.py:159
    if (groups <= 0 || o2 % groups != 0) return DFQ_ERR_SHAPE;
    const int64_t o2g = o2 / groups;
    // c[start_inner:end_inner] has c1 // groups elements (:44,:66): matmul raises unless that is i2
    if (c1 / groups != i2) return DFQ_ERR_SHAPE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int wave_blocks = (int)std::min<int64_t>(ceil_div(o2, kThreads / 64), 2048);
    hipLaunchKernelGGL(absorb_gemv_kernel, dim3(wave_blocks), dim3(kThreads), 0, s, w2, b2, bn_w, bn_b, o2, i2, khw2,
                       o2g, n_sigma);
    DFQ_LAUNCH_CHECK();
    hipLaunchKernelGGL(absorb_channel_kernel, dim3(blocks_for(c1)), dim3(kThreads), 0, s, b1, bn_b, bn_w, c1, n_sigma);
    DFQ_LAUNCH_CHECK();
    return DFQ_OK;
}

extern "C" int dfq_bias_absorb_batch(const dfq_absorb_desc* d, int32_t n, float n_sigma, void* ws, int64_t ws_bytes,
                                     int32_t* failed, void* stream) {
    if (failed) *failed = -1;
    if (n < 0 || (n > 0 && !d)) return DFQ_ERR_INVALID;
    if (n == 0) return DFQ_OK;
    AbsTables T;
    const int rc = absorb_tables(d, n, T, failed);
    if (rc != DFQ_OK) return rc;
    const AbsLayout L = absorb_layout(T);
    if (!ws || ws_bytes < L.total || reinterpret_cast<uintptr_t>(ws) % 256 != 0) return DFQ_ERR_WORKSPACE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* base = static_cast<char*>(ws);
    std::vector<char> blob(L.host, 0);
    auto put = [&](int64_t off, const auto& v) {
        if (!v.empty()) std::memcpy(blob.data() + off, v.data(), sizeof(v[0]) * v.size());
    };
    put(L.o_rels, T.rels); put(L.o_rows, T.rows); put(L.o_vecs, T.vecs); put(L.o_ops, T.ops); put(L.o_elems, T.elems);
    DFQ_HIP_CHECK(stage_h2d(base, blob.data(), L.host, s));
    const AbsRel* dr = reinterpret_cast<const AbsRel*>(base + L.o_rels);
    float* wc = reinterpret_cast<float*>(base + L.o_wc);
    const int64_t nrow = (int64_t)T.rows.size(), nel = (int64_t)T.elems.size();
    hipLaunchKernelGGL(absorb_batch_gemv_kernel, dim3((int)std::min<int64_t>(ceil_div(nrow, kThreads / 64), 4096)),
                       dim3(kThreads), 0, s, dr, reinterpret_cast<const AbsRows*>(base + L.o_rows), nrow, wc, n_sigma);
    DFQ_LAUNCH_CHECK();
    hipLaunchKernelGGL(absorb_batch_bias_kernel, dim3((int)std::min<int64_t>(nel, 4096)), dim3(kThreads), 0, s, dr,
                       reinterpret_cast<const AbsVec*>(base + L.o_vecs), reinterpret_cast<const AbsOp*>(base + L.o_ops),
                       reinterpret_cast<const AbsElems*>(base + L.o_elems), nel, wc, n_sigma);
    DFQ_LAUNCH_CHECK();
    return DFQ_OK;
}

namespace dfq {
hipError_t preload_transform() {   // see dfq_preload
    hipFuncAttributes a;
    hipError_t e = hipFuncGetAttributes(&a, reinterpret_cast<const void*>(bn_fold_weight_batch_kernel));
    if (e == hipSuccess) e = hipFuncGetAttributes(&a, reinterpret_cast<const void*>(absorb_batch_gemv_kernel));
    return e;
}
}  // namespace dfq
