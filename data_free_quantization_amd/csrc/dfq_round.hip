// dfq_sum_round_batch: nearest rounding plus the few flips that bound every kernel's
// and every output channel's summed rounding error (include/dfq_hip.h, DESIGN.md
// 3.10).  One workgroup per row of the call's rows (grid-stride beyond the grid),
// the row resident in LDS from its one HBM read to its stores (dfq_round_plan.h):
//   phase 0  the row into LDS with 16-B loads from its first 16-B boundary (4-B
//            loads before it and for the tail) and its (min, max); a TENSOR-mode
//            weight takes the range of sr_range_kernel's launch instead.
//   phase 1  every element in place: t by the IEEE divide, q = rint(t) into Q, the
//            integer perturbation P into S.
//   phase 2  kernel stage: a lane owns whole kernels, sums the taps, flips by a
//            repeated arg-max over them and leaves e' in E.  khw == 1: nothing to do.
//   phase 3  channel stage: the k-th largest of the G keys by a radix select (four
//            8-bit digit passes, LDS integer histograms), keys above it all taken,
//            the keys equal to it in index order by a block-wide prefix count; the
//            owner lane of a taken kernel makes its one flip.
//   phase 4  codes and dst from LDS, coalesced.
// From P on everything is integer and every sum exact, so no order can change a bit.
#include "dfq_common.h"
#include "dfq_round_plan.h"

#include <algorithm>
#include <vector>

namespace dfq {
namespace {

constexpr int kSrWaves = kThreads / kWave;
static_assert(kThreads == 256, "one histogram bin per thread");

// Exact block sum; every thread gets it.  sw: kSrWaves words, free again on return.
__device__ __forceinline__ long long sr_block_sum(long long v, long long* sw) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0) sw[threadIdx.x >> 6] = v;
    block_lds_sync();
    long long r = 0;
#pragma unroll
    for (int w = 0; w < kSrWaves; ++w) r += sw[w];
    block_lds_sync();
    return r;
}

// One flip in the kernel whose taps are s[0, T): down, the unflipped element with the
// largest P > 0; up, the one with the smallest P < 0; equal P: the lower tap.  A
// flipped element's word is beyond +-2^24 (dfq_round_plan.h) and never a candidate.
// Where the kernel has no such element -- only in the channel stage, in a kernel whose
// own flips went the other way and overshot -- the last of those flips is taken back:
// of the elements flipped the other way the one with the largest P (down) / smallest P
// (up), equal P: the lower tap.  The same move of the word does both.  One of the two
// always exists.
__device__ __forceinline__ void sr_flip_one(int32_t* s, int T, bool down) {
    int best = -1;
    int32_t bv = 0;
    for (int k = 0; k < T; ++k) {
        const int32_t v = down ? s[k] : -s[k];
        if (v > bv && v <= kSrHalf) {
            bv = v;
            best = k;
        }
    }
    if (best < 0) {
        bv = kSrStep;
        for (int k = 0; k < T; ++k) {
            const int32_t v = down ? s[k] : -s[k];
            if (v > bv) {
                bv = v;
                best = k;
            }
        }
    }
    if (best >= 0) s[best] += down ? -kSrMark : kSrMark;
}

// The ranges of the TENSOR-mode weights: blockIdx.y = the weight, kSrRangeBlocks
// workgroups stride over it; exact integer maxima of the ordered encoding into the
// weight's two workspace words (uploaded as zeros).
__global__ __launch_bounds__(kThreads) void sr_range_kernel(const SrJob* __restrict__ jobs) {
    __shared__ float smn[kSrWaves], smx[kSrWaves];
    const SrJob J = jobs[blockIdx.y];
    const int64_t n = J.rows * J.row_len;
    if (!J.range || (int64_t)blockIdx.x * kThreads >= n) return;   // the whole workgroup
    const DFQ_GLOBAL float* x = (const DFQ_GLOBAL float*)J.src;
    float a = INFINITY, b = -INFINITY;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
        const float v = x[i];
        a = fminf(a, v);
        b = fmaxf(b, v);
    }
    block_minmax(a, b, smn, smx);
    if (threadIdx.x == 0) {
        atomicMax(&J.range[0], ~enc_ord(a));
        atomicMax(&J.range[1], enc_ord(b));
    }
}

__global__ __launch_bounds__(kThreads) void sr_round_kernel(const SrJob* __restrict__ jobs, int n_jobs,
                                                            int64_t total_rows) {
    extern __shared__ __align__(16) unsigned char sr_lds[];
    __shared__ float smn[kSrWaves], smx[kSrWaves];
    __shared__ long long sw[kSrWaves];
    __shared__ uint32_t hist[256];
    __shared__ uint32_t sel[2];        // a digit pass's result: {digit, keys still to take at or below it}
    __shared__ int wcnt[kSrWaves];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid >> 6;
    for (int64_t r = blockIdx.x; r < total_rows; r += gridDim.x) {
        int lo = 0, hi = n_jobs - 1;   // the weight that holds row r: the last with row0 <= r
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (jobs[mid].row0 <= r) lo = mid; else hi = mid - 1;
        }
        const SrJob J = jobs[lo];
        const int64_t row = r - J.row0;
        const int len = J.row_len, T = J.khw, G = len / T, Tp = sr_pitch(T);
        const SrLds L = sr_lds_layout(len, T);
        int32_t* const S = reinterpret_cast<int32_t*>(sr_lds + L.o_s);
        int32_t* const E = reinterpret_cast<int32_t*>(sr_lds + L.o_e);
        uint8_t* const Q = sr_lds + L.o_q;
        auto at = [&](int i) { return T == 1 ? i : (i / T) * Tp + i % T; };

        // phase 0: the row and its range
        const float* xg = J.src + row * len;
        const DFQ_GLOBAL float* x = (const DFQ_GLOBAL float*)xg;
        float* const X = reinterpret_cast<float*>(S);
        const int to16 = (int)(((16 - (reinterpret_cast<uintptr_t>(xg) & 15)) & 15) >> 2);
        const int head = to16 < len ? to16 : len;
        const int nv = (len - head) >> 2;
        float mn = INFINITY, mx = -INFINITY;
        for (int v = tid; v < nv; v += kThreads) {
            const f32x4 q4 = *(const DFQ_GLOBAL f32x4*)(x + head + 4 * v);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                X[at(head + 4 * v + u)] = q4[u];
                mn = fminf(mn, q4[u]);
                mx = fmaxf(mx, q4[u]);
            }
        }
        for (int i = tid; i < len - 4 * nv; i += kThreads) {   // before the boundary, and the tail
            const int j = i < head ? i : i + 4 * nv;
            const float v = x[j];
            X[at(j)] = v;
            mn = fminf(mn, v);
            mx = fmaxf(mx, v);
        }
        block_minmax<true>(mn, mx, smn, smx);   // (its barrier also hands X over)
        if (J.range) {
            mn = dec_ord(~J.range[0]);
            mx = dec_ord(J.range[1]);
        }
        const QParams p = make_qparams(mn, mx, J.bits, J.sym != 0, 0, 0.0, 0.0);
        if (tid == 0 && (!J.range || row == 0)) {
            const int64_t u = J.range ? 0 : row;
            if (J.scale) J.scale[u] = p.s;
            if (J.zero) J.zero[u] = p.mn;
        }

        // phase 1: every element in place (one thread reads and writes a word)
        for (int i = tid; i < len; i += kThreads) {
            const int a = at(i);
            const float t = qdq_exact_t(X[a], p);
            const float q = rintf(t);
            S[a] = sr_perturb(q, t);
            Q[i] = (uint8_t)(int)q;
        }
        block_lds_sync();

        // phase 2: kernel stage (kernel g on thread g % kThreads, here and in phase 3)
        long long n4 = 0;
        if (T > 1) {
            for (int g = tid; g < G; g += kThreads) {
                int32_t* const s = S + g * Tp;
                int32_t e = 0;   // |e| <= 64 * 2^23
                for (int k = 0; k < T; ++k) e += s[k];
                const int k4 = (int)sr_flip_count(e);
                const bool down = e > 0;
                for (int f = 0; f < k4; ++f) sr_flip_one(s, T, down);
                E[g] = e + (down ? -k4 : k4) * kSrStep;
                n4 += k4;
            }
        }

        // phase 3: channel stage (a thread sums the e' it wrote itself)
        long long part = 0;
        for (int g = tid; g < G; g += kThreads) part += E[g];
        const long long Esum = sr_block_sum(part, sw);
        n4 = sr_block_sum(n4, sw);
        const int k5 = (int)sr_flip_count(Esum);   // <= G / 2
        const bool down = Esum > 0;
        if (k5 > 0) {   // the whole workgroup
            // the k5-th largest key, a digit a pass, most significant first
            uint32_t th = 0, remain = (uint32_t)k5;
            for (int pass = 0; pass < 4; ++pass) {
                const int shift = 24 - 8 * pass;
                hist[tid] = 0;
                if (tid == 0) sel[0] = sel[1] = 0;
                block_lds_sync();
                for (int g = tid; g < G; g += kThreads) {
                    const uint32_t key = sr_key(E[g], down);
                    if (pass == 0 || (key >> (shift + 8)) == th) atomicAdd(&hist[(key >> shift) & 255], 1u);
                }
                block_lds_sync();
                if (wv == 0) {   // lane l: digits 255 - 4l .. 252 - 4l, descending; a scan of the lanes' counts
                    uint32_t c[4], s = 0;
#pragma unroll
                    for (int j = 0; j < 4; ++j) s += c[j] = hist[255 - 4 * lane - j];
                    uint32_t inc = s;
#pragma unroll
                    for (int off = 1; off < kWave; off <<= 1) {
                        const uint32_t o = __shfl_up(inc, off, kWave);
                        if (lane >= off) inc += o;
                    }
                    uint32_t above = inc - s;   // keys with a larger digit
                    if (above < remain && remain <= inc) {   // one lane
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            if (above < remain && remain <= above + c[j]) {
                                sel[0] = 255 - 4 * lane - j;
                                sel[1] = remain - above;
                            }
                            above += c[j];
                        }
                    }
                }
                block_lds_sync();
                th = (th << 8) | sel[0];
                remain = sel[1];
                block_lds_sync();   // sel and hist are rewritten by the next pass
            }
            // keys above th are all taken; of those equal to it the first `remain` in index order
            uint32_t eq_before = 0;
            for (int base = 0; base < G; base += kThreads) {
                const int g = base + tid;
                const uint32_t key = g < G ? sr_key(E[g], down) : 0u;
                const bool eq = g < G && key == th;
                const uint64_t b = __builtin_amdgcn_ballot_w64(eq);
                if (lane == 0) wcnt[wv] = __builtin_popcountll(b);
                block_lds_sync();
                uint32_t mine = eq_before + __builtin_popcountll(b & ((1ull << lane) - 1));
                uint32_t all = 0;
#pragma unroll
                for (int w = 0; w < kSrWaves; ++w) {
                    if (w < wv) mine += wcnt[w];
                    all += wcnt[w];
                }
                if (g < G && (key > th || (eq && mine < remain))) sr_flip_one(S + g * Tp, T, down);
                eq_before += all;
                block_lds_sync();   // wcnt is rewritten by the next round
            }
        }
        if (tid == 0 && J.flips) {
            J.flips[2 * row] = (int32_t)n4;
            J.flips[2 * row + 1] = k5;
        }
        block_lds_sync();

        // phase 4: the outputs
        uint8_t* const codes = static_cast<uint8_t*>(J.codes) + (J.codes ? row * len : 0);
        float* const dst = J.dst + (J.dst ? row * len : 0);
        for (int i = tid; i < len; i += kThreads) {
            const int qi = (J.sym ? (int)(int8_t)Q[i] : (int)Q[i]) + sr_code_offset(S[at(i)]);
            if (J.codes) codes[i] = (uint8_t)qi;
            if (J.dst) {
                const float y = (float)qi * p.s;
                dst[i] = y + p.mn;
            }
        }
        block_lds_sync();   // the next row rewrites the LDS
    }
}

}  // namespace
}  // namespace dfq

using namespace dfq;

extern "C" int dfq_sum_round_batch(const dfq_sum_round_desc* d, int32_t n, void* ws, int64_t ws_bytes,
                                   void* stream) {
    if (n < 0 || (n > 0 && !d)) return DFQ_ERR_INVALID;
    if (n == 0) return DFQ_OK;
    SrLayout L;
    const int rc = sum_round_layout(d, n, L);
    if (rc != DFQ_OK) return rc;
    if (!ws || ws_bytes < L.total) return DFQ_ERR_WORKSPACE;
    if (reinterpret_cast<uintptr_t>(ws) % 256 != 0) return DFQ_ERR_INVALID;
    char* base = static_cast<char*>(ws);
    // one staging blob (the jobs, the range words as zeros), one copy
    std::vector<char> blob((size_t)L.total, 0);
    sum_round_jobs(d, n, reinterpret_cast<uint32_t*>(base + L.o_range), reinterpret_cast<SrJob*>(blob.data() + L.o_jobs));
    hipStream_t s = static_cast<hipStream_t>(stream);
    DFQ_HIP_CHECK(stage_h2d(base, blob.data(), blob.size(), s));
    const SrJob* dj = reinterpret_cast<const SrJob*>(base + L.o_jobs);
    if (L.n_tensor > 0) {
        hipLaunchKernelGGL(sr_range_kernel, dim3(kSrRangeBlocks, n), dim3(kThreads), 0, s, dj);
        DFQ_LAUNCH_CHECK();
    }
    DFQ_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(sr_round_kernel),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, L.lds_bytes));
    hipLaunchKernelGGL(sr_round_kernel, dim3(L.grid), dim3(kThreads), (size_t)L.lds_bytes, s, dj, (int)n,
                       L.total_rows);
    DFQ_LAUNCH_CHECK();
    return DFQ_OK;
}
