// Activation ranges and fake quant of the DFQ path (gfx950): the BN-statistics
// range rules of set_quant_minmax, the observers' statistics, whole-tensor and
// chunked ranges, and the given-range fake quant.  HBM/latency-bound elementwise
// passes and (min, max) reductions: no MFMA.  fp32 arithmetic is ordered exactly as
// the reference's torch CPU ops (one rounding per op; -ffp-contract=off, IEEE
// div/sqrt).
#include "dfq_common.h"
#include "dfq_transform_plan.h"   // blocks_for

#include <algorithm>

namespace dfq {

// ---------------------------------------------------------------------------
// Activation ranges from BN statistics: set_quant_minmax,
// utils/layer_transform.py:356-618.  Rectified-Gaussian moments with scipy's
// pdf / ndtr in float64 on the fp32 argument (std_pdf / std_cdf), every fp32 op
// in the reference's expression order (:396-410).
// ---------------------------------------------------------------------------
// kind 0: mean = b, var = w*w; 1: calculate_mean / calculate_var (ReLU);
// 2: calculate_mean_6 / calculate_var_6 (ReLU6).  sqrt_w: w := sqrt(w + eps)
// (torch.sqrt(var + eps)).  accumulate: mean += m, var += v.  mean/var may alias w/b.
__global__ void act_moments_kernel(const float* w_in, const float* b_in, int64_t n, int kind, int sqrt_w, float eps,
                                   int accumulate, float* mean, float* var) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
        const float w = sqrt_w ? sqrtf(w_in[j] + eps) : w_in[j];
        const float b = b_in[j];
        float m, v;
        if (kind == 0) {
            m = b;
            v = w * w;
        } else if (kind == 1) {
            const float x0 = (-b) / w;
            const float P0 = std_pdf(x0), C0 = std_cdf(x0);
            m = w * P0 + b * (1.0f - C0);
            const float B = ((b * b + w * w) + m * m) - (2.0f * m) * b;
            v = ((1.0f - C0) * B + (w * (b - 2.0f * m)) * P0) + (m * m) * C0;
        } else {
            const float x0 = (-b) / w, x6 = (6.0f - b) / w;
            const float P0 = std_pdf(x0), C0 = std_cdf(x0), P6 = std_pdf(x6), C6 = std_cdf(x6);
            m = (w * (P0 - P6) + b * (C6 - C0)) + 6.0f * (1.0f - C6);
            const float B = ((b * b + w * w) + m * m) - (2.0f * m) * b;
            const float d6 = 6.0f - m;
            v = ((((C6 - C0) * B + (w * -6.0f) * P6) + (w * (b - 2.0f * m)) * (P0 - P6)) + (m * m) * C0) +
                (d6 * d6) * (1.0f - C6);
        }
        if (accumulate) {
            m = mean[j] + m;
            v = var[j] + v;
        }
        mean[j] = m;
        var[j] = v;
    }
}

// out = {min(a - N*w), max(a + N*w)} (get_min_value / get_max_value, :391-392);
// w_is_var: w := sqrt(w + eps).  One block of kThreads.
//
// NaN: torch.min / torch.max propagate it (a variance that cancelled below -eps
// makes torch.sqrt(var + eps) NaN, and the reference's range (nan, nan)), where
// fminf / fmaxf drop it.  So a flag per output rides along, as in
// observe_rows_kernel: a NaN among the a - N*w makes the min NaN, one among the
// a + N*w the max.  Without a NaN the outputs keep fminf / fmaxf's bits.
__global__ void __launch_bounds__(kThreads)
act_minmax_kernel(const float* a, const float* w_in, int64_t n, int w_is_var, float eps, float nsig, float* out) {
    __shared__ float smn[kThreads / kWave], smx[kThreads / kWave];
    __shared__ int snan[kThreads / kWave];
    float vmin = INFINITY, vmax = -INFINITY;
    bool nan_lo = false, nan_hi = false;
    for (int64_t j = threadIdx.x; j < n; j += kThreads) {
        const float w = w_is_var ? sqrtf(w_in[j] + eps) : w_in[j];
        const float nw = nsig * w;
        const float lo = a[j] - nw, hi = a[j] + nw;
        vmin = fminf(vmin, lo);
        vmax = fmaxf(vmax, hi);
        nan_lo |= (lo != lo);
        nan_hi |= (hi != hi);
    }
    const int wnan = (__ballot(nan_lo) != 0 ? 1 : 0) | (__ballot(nan_hi) != 0 ? 2 : 0);
    if ((threadIdx.x & (kWave - 1)) == 0) snan[threadIdx.x >> 6] = wnan;   // rides on block_minmax's barrier
    block_minmax(vmin, vmax, smn, smx);
    if (threadIdx.x == 0) {
        int anynan = snan[0];
        for (int q = 1; q < kThreads / kWave; ++q) anynan |= snan[q];
        out[0] = (anynan & 1) ? __uint_as_float(0x7FC00000u) : vmin;
        out[1] = (anynan & 2) ? __uint_as_float(0x7FC00000u) : vmax;
    }
}

// Case (d.) of set_quant_minmax (:470-481): a BN statistic vector pushed through a
// conv (weights summed over KH*KW, ATen order) or linear layer with its bias:
// out[o] = sum_i Wsum[o, i] * x[g*I + i] (+ bias[o]).  One wave per output.
__global__ void act_affine_kernel(const float* x, const float* w, const float* bias, int64_t o, int64_t i2,
                                  int64_t khw, int64_t og, float* out) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x / 64);
    for (int64_t r = wave; r < o; r += nwaves) {
        const int64_t g = r / og;
        float acc = 0.f;
        for (int64_t i = lane; i < i2; i += 64) {
            const float* p = w + (r * i2 + i) * khw;
            const float ws = khw == 1 ? p[0] : aten_inner_sum([&](int64_t k) { return p[k]; }, khw);
            acc += ws * x[g * i2 + i];
        }
        acc = wave_sum_f(acc);
        if (lane == 0) out[r] = bias ? acc + bias[r] : acc;
    }
}

// ---------------------------------------------------------------------------
// Activation fake quant with a given range (QuantMeasure.forward at inference,
// utils/quantize.py:112-126 -> quantize(input, b, float(min), float(max))):
// elementwise, async, no workspace.  The range may live in device memory (the
// observer's running_min / running_max), read as the exact doubles float()
// would produce, so no host round trip is needed.
// ---------------------------------------------------------------------------
// A NaN element stays NaN (torch's clamp_ propagates it; qdq's fminf / fmaxf
// clamp would map it to qmin).
__device__ __forceinline__ float qdq_nan(float x, const QParams& p, float& q) {
    const float y = qdq(x, p, q);
    return x != x ? x : y;
}

__global__ void __launch_bounds__(kThreads)
fq_given_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t n, int bits, int sym, int flags,
                const float* __restrict__ min_dev, const float* __restrict__ max_dev,
                const uint32_t* __restrict__ range_enc, double gmin, double gmax, int vec4) {
    if (min_dev) gmin = (double)min_dev[0];
    if (max_dev) gmax = (double)max_dev[0];
    if (range_enc) {   // dfq_range's {~enc(min), enc(max)}
        gmin = (double)dec_ord(~range_enc[0]);
        gmax = (double)dec_ord(range_enc[1]);
    }
    const QParams p = make_qparams((float)gmin, (float)gmax, bits, sym != 0, flags | DFQ_GIVEN_RANGE, gmin, gmax);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    float q;
    if (vec4) {
        const int64_t n4 = n >> 2;
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
            const float4 v = reinterpret_cast<const float4*>(x)[i];
            float4 o;
            o.x = qdq_nan(v.x, p, q);
            o.y = qdq_nan(v.y, p, q);
            o.z = qdq_nan(v.z, p, q);
            o.w = qdq_nan(v.w, p, q);
            reinterpret_cast<float4*>(y)[i] = o;
        }
    } else {
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
            y[i] = qdq_nan(x[i], p, q);
    }
}

// ---------------------------------------------------------------------------
// The Quant* layers' weight / bias fake quant in one call (dfq_fake_quant_tensor):
// y = quantize(x, b, float(x.min()), float(x.max())) -- the given-range fake quant
// of fq_given_kernel on the tensor's own range, without the fill and the separate
// range launch of dfq_range.  words[8]: caller scratch, zero once; every call leaves
// it armed again.
// ---------------------------------------------------------------------------
constexpr int64_t kFqSmall = 16384;   // one workgroup does range and fake quant

// One workgroup: the range (fminf / fmaxf, as range_enc_kernel), then the fake quant.
__global__ void __launch_bounds__(kThreads)
fq_tensor_small_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t n, int bits, int sym, int flags) {
    __shared__ float smn[kThreads / kWave], smx[kThreads / kWave];
    float a = INFINITY, b = -INFINITY;
    for (int64_t i = threadIdx.x; i < n; i += kThreads) {
        const float v = x[i];
        a = fminf(a, v);
        b = fmaxf(b, v);
    }
    block_minmax<true>(a, b, smn, smx);   // every thread builds the quantizer
    // the range as dfq_range's encoding would give it back (the same float, read as a double)
    const double gmin = (double)dec_ord(~(~enc_ord(a))), gmax = (double)dec_ord(enc_ord(b));
    const QParams p = make_qparams((float)gmin, (float)gmax, bits, sym != 0, flags | DFQ_GIVEN_RANGE, gmin, gmax);
    float q;
    for (int64_t i = threadIdx.x; i < n; i += kThreads) y[i] = qdq_nan(x[i], p, q);
}

// The grid's share of a whole-tensor (min, max): grid-stride fminf / fmaxf, the
// block's result in thread 0's (a, b).
__device__ __forceinline__ void tensor_range_block(const float* __restrict__ x, int64_t n, float& a, float& b) {
    __shared__ float smn[kThreads / kWave], smx[kThreads / kWave];
    a = INFINITY;
    b = -INFINITY;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float v = x[i];
        a = fminf(a, v);
        b = fmaxf(b, v);
    }
    block_minmax(a, b, smn, smx);
}

// Range launch of large tensors: range_enc_kernel's accumulation into words[0..1];
// each block's atomics return before its arrival on words[2] (returning atomics:
// the wave waits for them), and the last block to arrive takes the range with
// atomic exchanges (re-arming words[0..1]), publishes it in words[4..5] for the
// fake-quant launch and re-arms the counter.
__global__ void __launch_bounds__(kThreads)
fq_tensor_range_kernel(const float* __restrict__ x, int64_t n, uint32_t* __restrict__ words) {
    float a, b;
    tensor_range_block(x, n, a, b);
    if (threadIdx.x == 0) {
        const uint32_t o0 = __hip_atomic_fetch_max(&words[0], ~enc_ord(a), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t o1 = __hip_atomic_fetch_max(&words[1], enc_ord(b), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::"v"(o0), "v"(o1) : "memory");   // both performed before the arrival
        const uint32_t last = gridDim.x - 1;
        if (__hip_atomic_fetch_add(&words[2], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == last) {
            const uint32_t r0 = __hip_atomic_exchange(&words[0], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const uint32_t r1 = __hip_atomic_exchange(&words[1], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            words[4] = r0;
            words[5] = r1;
            __hip_atomic_exchange(&words[2], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// Whole-tensor (min, max) as order-preserving uints: {max ~enc(x), max enc(x)}, so
// one zero memset initialises both words (exact, order-independent).
__global__ void __launch_bounds__(kThreads)
range_enc_kernel(const float* __restrict__ x, int64_t n, uint32_t* __restrict__ enc) {
    float a, b;
    tensor_range_block(x, n, a, b);
    if (threadIdx.x == 0) {
        atomicMax(&enc[0], ~enc_ord(a));
        atomicMax(&enc[1], enc_ord(b));
    }
}

// ---------------------------------------------------------------------------
// quantize()'s data range with num_chunks (utils/quantize.py:26-37):
// y = x.view(rows, -1); min = y.min(-1)[0].mean(-1), max likewise (fp32).
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads)
chunk_row_range_kernel(const float* __restrict__ x, int64_t rows, int64_t row_len, float* __restrict__ mins,
                       float* __restrict__ maxs) {
    __shared__ float smn[kThreads / kWave], smx[kThreads / kWave];
    for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
        const float* row = x + r * row_len;
        float a = INFINITY, b = -INFINITY;
        for (int64_t i = threadIdx.x; i < row_len; i += kThreads) {
            const float v = row[i];
            a = fminf(a, v);
            b = fmaxf(b, v);
        }
        block_minmax(a, b, smn, smx);
        if (threadIdx.x == 0) {
            mins[r] = a;
            maxs[r] = b;
        }
        __syncthreads();
    }
}

// One wave: torch.mean over the rows' mins / maxs in ATen's order (sum, then / n).
__global__ void chunk_mean_kernel(const float* __restrict__ mins, const float* __restrict__ maxs, int64_t rows,
                                  float* __restrict__ out2) {
    const int lane = threadIdx.x;
    const float smn = wave_inner_sum([&](int64_t i) { return mins[i]; }, rows, lane);
    const float smx = wave_inner_sum([&](int64_t i) { return maxs[i]; }, rows, lane);
    if (lane == 0) {
        out2[0] = smn / (float)rows;
        out2[1] = smx / (float)rows;
    }
}

// ---------------------------------------------------------------------------
// QuantMeasure.forward's statistics (utils/quantize.py:94-126) in two launches
// instead of ~8 torch ops: the rows' (min, max) of x.view(rows, -1) by a 2-D grid
// (each block a slice of one row, ordered-uint atomics into a per-observer word
// pair), then one wave takes the rows' means in ATen's order and applies the
// observer's updates.  The word pairs are re-armed by that wave (self-cleaning:
// the host arms them once when it allocates them).
// ---------------------------------------------------------------------------
//
// NaN: torch's min / max propagate it, so a slice holding one stores the words of
// -NaN (min) and +NaN (max) -- the largest values of both ordered encodings, so
// the atomics keep them -- and the rows' means, the momentum update and the
// fake-quant range come out NaN as in the reference.
__global__ void __launch_bounds__(kThreads)
observe_rows_kernel(const float* __restrict__ x, int64_t rows, int64_t row_len, int64_t slices,
                    uint32_t* __restrict__ words) {
    __shared__ float smn[kThreads / kWave], smx[kThreads / kWave];
    __shared__ int snan[kThreads / kWave];
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
    const int64_t per = ceil_div(row_len, slices);
    for (int64_t b = blockIdx.x; b < rows * slices; b += gridDim.x) {
        const int64_t r = b / slices, k = b % slices;
        const int64_t e0 = k * per, e1 = min(row_len, e0 + per);
        const float* row = x + r * row_len;
        float a = INFINITY, c = -INFINITY;
        bool nan = false;
        const bool v4 = (row_len % 4 == 0) && (per % 4 == 0) && (reinterpret_cast<uintptr_t>(x) % 16 == 0);
        if (v4) {
            const float4* q = reinterpret_cast<const float4*>(row + e0);
            for (int64_t i = threadIdx.x; i < (e1 - e0) / 4; i += kThreads) {
                const float4 v = q[i];
                a = fminf(a, fminf(fminf(v.x, v.y), fminf(v.z, v.w)));
                c = fmaxf(c, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
                nan |= (v.x != v.x) | (v.y != v.y) | (v.z != v.z) | (v.w != v.w);
            }
        } else {
            for (int64_t i = e0 + threadIdx.x; i < e1; i += kThreads) {
                const float v = row[i];
                a = fminf(a, v);
                c = fmaxf(c, v);
                nan |= (v != v);
            }
        }
        const bool wnan = __ballot(nan) != 0;
        if (lane == 0) snan[w] = wnan ? 1 : 0;   // the NaN word rides on block_minmax's barrier
        block_minmax(a, c, smn, smx);
        if (threadIdx.x == 0) {
            int anynan = snan[0];
            for (int q = 1; q < kThreads / kWave; ++q) anynan |= snan[q];
            if (anynan) {
                a = __uint_as_float(0xFFC00000u);   // -NaN: enc_ord's smallest, so ~enc wins atomicMax
                c = __uint_as_float(0x7FC00000u);   // +NaN: enc_ord's largest
            }
            atomicMax(&words[2 * r], ~enc_ord(a));
            atomicMax(&words[2 * r + 1], enc_ord(c));
        }
        __syncthreads();
    }
}

// One wave.  mn / mx = the means of the rows' mins / maxs (fp32, ATen's sum order,
// as flat.min(-1)[0].mean()).  update_stat: running_max = mx if mx > running_max
// (Python max on tensors), running_min likewise; training: running_* =
// running_* * (1 - m) + (mn|mx) * m, each op rounded to fp32 as the in-place torch
// ops do.  out2 = the range the fake quant uses: (mn, mx) in training, the running
// values otherwise.
__global__ void observe_finish_kernel(uint32_t* __restrict__ words, int64_t rows, float* __restrict__ running_min,
                                      float* __restrict__ running_max, int32_t update_stat, int32_t training,
                                      float one_minus_m, float m, float* __restrict__ out2) {
    const int lane = threadIdx.x;
    const float smn = wave_inner_sum([&](int64_t i) { return dec_ord(~words[2 * i]); }, rows, lane);
    const float smx = wave_inner_sum([&](int64_t i) { return dec_ord(words[2 * i + 1]); }, rows, lane);
    __syncthreads();   // every lane has read the words
    for (int64_t i = lane; i < 2 * rows; i += kWave) words[i] = 0u;   // re-armed for the next call
    if (lane == 0) {
        const float mn = smn / (float)rows, mx = smx / (float)rows;
        float rmn = *running_min, rmx = *running_max;
        if (update_stat) {
            rmx = (mx > rmx) ? mx : rmx;
            rmn = (mn < rmn) ? mn : rmn;
        }
        if (training) {
            const float t0 = rmn * one_minus_m, t1 = mn * m;
            rmn = t0 + t1;
            const float t2 = rmx * one_minus_m, t3 = mx * m;
            rmx = t2 + t3;
        }
        *running_min = rmn;
        *running_max = rmx;
        out2[0] = training ? mn : rmn;
        out2[1] = training ? mx : rmx;
    }
}

// The given-range fake quant of n elements: float4 groups when n and both
// pointers allow.
static void launch_fq_given(const float* x, float* y, int64_t n, int32_t bits, int32_t symmetric, int32_t flags,
                            const float* min_dev, const float* max_dev, const uint32_t* range_enc, double given_min,
                            double given_max, hipStream_t s) {
    const int vec4 = (n % 4 == 0) && (reinterpret_cast<uintptr_t>(x) % 16 == 0) &&
                     (reinterpret_cast<uintptr_t>(y) % 16 == 0);
    const int64_t work = vec4 ? n / 4 : n;
    const int grid = (int)std::min<int64_t>(ceil_div(work, (int64_t)kThreads * 4), 16384);
    hipLaunchKernelGGL(fq_given_kernel, dim3(std::max(grid, 1)), dim3(kThreads), 0, s, x, y, n, bits, symmetric, flags,
                       min_dev, max_dev, range_enc, given_min, given_max, vec4);
}

}  // namespace dfq

using namespace dfq;

// ============================================================================
// C ABI
// ============================================================================
extern "C" int dfq_act_moments(const float* w, const float* b, int64_t n, int32_t kind, int32_t sqrt_w, float eps,
                               int32_t accumulate, float* mean, float* var, void* stream) {
    if (!w || !b || !mean || !var || n < 0 || kind < 0 || kind > 2) return DFQ_ERR_INVALID;
    if (n == 0) return DFQ_OK;
    hipLaunchKernelGGL(act_moments_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), w,
                       b, n, (int)kind, (int)sqrt_w, eps, (int)accumulate, mean, var);
    DFQ_LAUNCH_CHECK();
    return DFQ_OK;
}

extern "C" int dfq_act_minmax(const float* a, const float* w, int64_t n, int32_t w_is_var, float eps, float nsig,
                              float* out2, void* stream) {
    if (!a || !w || !out2 || n <= 0) return DFQ_ERR_INVALID;
    hipLaunchKernelGGL(act_minmax_kernel, dim3(1), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a, w, n,
                       (int)w_is_var, eps, nsig, out2);
    DFQ_LAUNCH_CHECK();
    return DFQ_OK;
}

extern "C" int dfq_act_affine(const float* x, const float* w, const float* bias, int64_t o, int64_t i2, int64_t khw,
                              int64_t groups, float* out, void* stream) {
    if (!x || !w || !out || o <= 0 || i2 <= 0 || khw <= 0 || groups <= 0 || o % groups) return DFQ_ERR_INVALID;
    hipLaunchKernelGGL(act_affine_kernel, dim3((int)std::min<int64_t>(ceil_div(o, (int64_t)4), 2048)), dim3(kThreads),
                       0, static_cast<hipStream_t>(stream), x, w, bias, o, i2, khw, o / groups, out);
    DFQ_LAUNCH_CHECK();
    return DFQ_OK;
}

extern "C" int dfq_chunk_range(const float* x, int64_t rows, int64_t row_len, float* rowbuf, float* out2,
                               void* stream) {
    if (!x || !rowbuf || !out2 || rows < 1) return DFQ_ERR_INVALID;
    if (row_len < 1) return DFQ_ERR_SHAPE;   // torch: min over an empty dim raises
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int grid = (int)std::min<int64_t>(rows, 4096);
    hipLaunchKernelGGL(chunk_row_range_kernel, dim3(grid), dim3(kThreads), 0, s, x, rows, row_len, rowbuf,
                       rowbuf + rows);
    DFQ_LAUNCH_CHECK();
    hipLaunchKernelGGL(chunk_mean_kernel, dim3(1), dim3(kWave), 0, s, rowbuf, rowbuf + rows, rows, out2);
    DFQ_LAUNCH_CHECK();
    return DFQ_OK;
}

extern "C" int dfq_act_observe(const float* x, int64_t rows, int64_t row_len, uint32_t* words, float* running_min,
                               float* running_max, int32_t update_stat, int32_t training, double momentum,
                               float* out2, void* stream) {
    if (!x || !words || !running_min || !running_max || !out2 || rows < 1) return DFQ_ERR_INVALID;
    if (row_len < 1) return DFQ_ERR_SHAPE;   // torch: min over an empty dim raises
    hipStream_t s = static_cast<hipStream_t>(stream);
    // slices of >= 16K elements per block, >= 1024 blocks when the tensor allows
    const int64_t slices = std::max<int64_t>(1, std::min<int64_t>(ceil_div(row_len, (int64_t)16384),
                                                                  ceil_div((int64_t)1024, rows)));
    const int grid = (int)std::min<int64_t>(rows * slices, 8192);
    hipLaunchKernelGGL(observe_rows_kernel, dim3(grid), dim3(kThreads), 0, s, x, rows, row_len, slices, words);
    DFQ_LAUNCH_CHECK();
    hipLaunchKernelGGL(observe_finish_kernel, dim3(1), dim3(kWave), 0, s, words, rows, running_min, running_max,
                       update_stat, training, (float)(1.0 - momentum), (float)momentum, out2);
    DFQ_LAUNCH_CHECK();
    return DFQ_OK;
}

extern "C" int dfq_range(const float* x, int64_t n, uint32_t* range_enc, void* stream) {
    if (n < 1 || !x || !range_enc) return DFQ_ERR_INVALID;
    hipStream_t s = static_cast<hipStream_t>(stream);
    DFQ_HIP_CHECK(hipMemsetAsync(range_enc, 0, 2 * sizeof(uint32_t), s));
    const int grid = (int)std::min<int64_t>(ceil_div(n, (int64_t)kThreads * 8), 2048);
    hipLaunchKernelGGL(range_enc_kernel, dim3(std::max(grid, 1)), dim3(kThreads), 0, s, x, n, range_enc);
    DFQ_LAUNCH_CHECK();
    return DFQ_OK;
}

extern "C" int dfq_fake_quant_tensor(const float* x, float* y, int64_t n, int32_t bits, int32_t symmetric,
                                     int32_t flags, uint32_t* words, void* stream) {
    if (n < 1 || !x || !y || bits < 2 || bits > 16) return DFQ_ERR_INVALID;
    if (flags & ~(DFQ_SCALE_F32)) return DFQ_ERR_INVALID;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n <= kFqSmall) {
        hipLaunchKernelGGL(fq_tensor_small_kernel, dim3(1), dim3(kThreads), 0, s, x, y, n, bits, symmetric, flags);
        DFQ_LAUNCH_CHECK();
        return DFQ_OK;
    }
    if (!words) return DFQ_ERR_INVALID;
    const int grid = (int)std::min<int64_t>(ceil_div(n, (int64_t)kThreads * 8), 2048);
    hipLaunchKernelGGL(fq_tensor_range_kernel, dim3(std::max(grid, 1)), dim3(kThreads), 0, s, x, n, words);
    DFQ_LAUNCH_CHECK();
    launch_fq_given(x, y, n, bits, symmetric, flags, nullptr, nullptr, static_cast<const uint32_t*>(words + 4), 0.0,
                    0.0, s);
    DFQ_LAUNCH_CHECK();
    return DFQ_OK;
}

extern "C" int dfq_fake_quant_given(const float* x, float* y, int64_t n, int32_t bits, int32_t symmetric,
                                    int32_t flags, const float* min_dev, const float* max_dev,
                                    const uint32_t* range_enc, double given_min, double given_max, void* stream) {
    if (n < 0 || (n > 0 && (!x || !y)) || bits < 2 || bits > 16) return DFQ_ERR_INVALID;
    if (flags & ~(DFQ_SCALE_F32)) return DFQ_ERR_INVALID;
    if (n == 0) return DFQ_OK;
    launch_fq_given(x, y, n, bits, symmetric, flags, min_dev, max_dev, range_enc, given_min, given_max,
                    static_cast<hipStream_t>(stream));
    DFQ_LAUNCH_CHECK();
    return DFQ_OK;
}
