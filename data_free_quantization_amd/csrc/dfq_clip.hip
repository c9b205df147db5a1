// dfq_clip_search_batch: for every unit (a row, or a whole tensor) the clamp range,
// out of K candidates, that minimizes the unit's own quantization noise
// (include/dfq_hip.h).  One wave per task of the planner's table (dfq_clip_plan.h):
//   clip_eval_kernel    a whole-unit task reads its units from HBM once into the
//                       wave's LDS copy, reduces each unit's range in its lane group,
//                       evaluates the K candidates from the copy (fp64 sum per lane,
//                       fixed butterfly), keeps the running best and stores the
//                       clamped values and the outputs.  A piece task does the same
//                       for one piece of a split unit against the unit's range and
//                       writes its K partial sums.
//   clip_range_kernel   (split units only, before the evaluation) the range by exact
//                       integer atomic maxima of the ordered encoding.
//   clip_finish_kernel  (split units only) one wave per unit, lane k owning candidate
//                       k: the pieces summed in piece order, the argmin, the outputs.
//   clip_clamp_kernel   (split units only) the chosen clamp over the pieces.
// Nothing is handed from workgroup to workgroup inside a launch.  Every candidate is
// the sweep's arithmetic (make_qparams on the clamped data range, the screened
// quantize-dequantize of dfq_common.h): ~K x 30 lane operations per element against
// 8 B of traffic, so the kernel is VALU-bound and the weights are read with plain
// 4-B loads (a wave reads 256 contiguous bytes; any 4-B alignment).
#include "dfq_common.h"
#include "dfq_clip_plan.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace dfq {
namespace {

constexpr int kClipWaves = kThreads / kWave;

__device__ __forceinline__ float clip_alpha(int k, int K, float min_frac) {
    return K > 1 ? (float)(1.0 - (double)k * (1.0 - (double)min_frac) / (double)(K - 1)) : 1.0f;
}

__device__ __forceinline__ float clip_clamp(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }

// Candidate k of a unit with data range (mn, mx): the clamp, and the parameters the
// sweep builds from the clamped unit's data range (the clamp is monotonic).
struct ClipCand {
    float lo, hi;
    QParams p;
    float rs, band;   // screen_rcp(p.s) for the screened quotient
};
__device__ __forceinline__ ClipCand clip_cand(float mn, float mx, int k, const ClipJob& J) {
    ClipCand c;
    const float a = clip_alpha(k, J.K, J.min_frac);
    c.lo = a * mn;
    c.hi = a * mx;
    c.p = make_qparams(clip_clamp(mn, c.lo, c.hi), clip_clamp(mx, c.lo, c.hi), J.bits, J.sym != 0, 0, 0.0, 0.0);
    c.rs = screen_rcp(c.p.s, c.band);
    return c;
}

// noise of candidate c over elements j, j + G, ... of xs[0, len) (this lane's share,
// added in increasing order; four per round share one ballot).  len is wave-uniform;
// a lane of a group without a unit passes active = false and adds nothing (it reads
// its group's part of the copy, whatever that holds, and masks the result).
// e = fl32(y - x) and its square is exact in fp64, so only the sum rounds (a fused
// multiply-add gives the bits of the multiply followed by the add).
__device__ __forceinline__ double clip_noise(const float* xs, int len, int j, int G, bool active, const ClipCand& c) {
    double acc = 0.0;
#pragma unroll 1
    for (int base = 0; base < len; base += 4 * G) {
        float x[4], cl[4], t[4];
        bool v[4], need = false;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = base + j + u * G;
            v[u] = active && i < len;
            x[u] = xs[i < len ? i : len - 1];   // always inside the copy (no branch around the read); masked below
            cl[u] = clip_clamp(x[u], c.lo, c.hi);
            bool nd;
            t[u] = qdq_screen(cl[u], c.p, c.rs, c.band, nd);
            need |= nd;
        }
        if (__builtin_amdgcn_ballot_w64(need)) {   // wave-uniform, rare: the IEEE divide decides
#pragma unroll
            for (int u = 0; u < 4; ++u) t[u] = qdq_exact_t(cl[u], c.p);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            float q;
            const float y = qdq_finish(t[u], c.p, q);
            const float e = v[u] ? y - x[u] : 0.f;   // +0 leaves the sum's bits as they were
            acc = __builtin_fma((double)e, (double)e, acc);
        }
    }
    return acc;
}

// fp64 sum over aligned groups of G lanes, a fixed butterfly: every lane of a group
// ends with the same bits.  All 64 lanes take part.
__device__ __forceinline__ double clip_group_sum(double v, int G) {
    for (int off = G >> 1; off >= 1; off >>= 1) v += __shfl_xor(v, off, kWave);
    return v;
}

// The evaluation launch.  LDS: one copy of kClipPiece floats per wave (64 KB per
// block, two blocks per CU), written and read by its own wave only.
__global__ __launch_bounds__(kThreads, 2) void clip_eval_kernel(const ClipJob* __restrict__ jobs,
                                                                const ClipTask* __restrict__ tasks,
                                                                int64_t n_tasks) {
    __shared__ float copy[kClipWaves][kClipPiece];
    float* const xs = copy[threadIdx.x >> 6];
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t wave = (int64_t)blockIdx.x * kClipWaves + (threadIdx.x >> 6);
    const int64_t n_waves = (int64_t)gridDim.x * kClipWaves;
    for (int64_t ti = wave; ti < n_tasks; ti += n_waves) {
        const ClipTask t = tasks[ti];
        const ClipJob J = jobs[t.job];
        const int K = J.K;
        if (t.nunits == 0) {
            // one piece of a split unit, the whole wave: K partial sums to its slot
            const int64_t np = clip_pieces(J.unit_len);
            const int64_t unit = t.first / np, start = (t.first % np) * kClipPiece;
            const int len = (int)(J.unit_len - start < kClipPiece ? J.unit_len - start : kClipPiece);
            const DFQ_GLOBAL float* x = (const DFQ_GLOBAL float*)J.w + unit * J.unit_len + start;
            for (int i = lane; i < len; i += kWave) xs[i] = x[i];
            wave_lds_sync();
            const ClipUnit* ur = J.urec + unit;
            const float mn = dec_ord(~ur->enc[0]), mx = dec_ord(ur->enc[1]);
            double* slot = J.slots + t.first * K;
            for (int k = 0; k < K; ++k) {
                const ClipCand c = clip_cand(mn, mx, k, J);
                const double s = clip_group_sum(clip_noise(xs, len, lane, kWave, true, c), kWave);
                if (lane == 0) slot[k] = s;
            }
            wave_lds_sync();   // the copy is rewritten by the next task
            continue;
        }
        // whole units: 64 / G at a time, G lanes each; unit q of the round keeps its
        // copy at xs[g * unit_len, (g + 1) * unit_len)
        const int len = (int)J.unit_len;
        const int G = clip_group_lanes(J.unit_len), per = kWave / G;
        const int g = lane / G, j = lane % G;
        float* const xg = xs + g * len;
        for (int base = 0; base < t.nunits; base += per) {
            const int q = base + g;
            const bool active = q < t.nunits;
            const int64_t unit = t.first + q;
            DFQ_GLOBAL float* x = (DFQ_GLOBAL float*)J.w + unit * J.unit_len;
            float mn = __builtin_inff(), mx = -__builtin_inff();
            if (active)
                for (int i = j; i < len; i += G) {
                    const float v = x[i];
                    xg[i] = v;
                    mn = fminf(mn, v);
                    mx = fmaxf(mx, v);
                }
            group_minmax(mn, mx, G);
            if (!active) mn = mx = 0.f;
            wave_lds_sync();
            double best = 0.0, first = 0.0;
            int bestk = 0;
            for (int k = 0; k < K; ++k) {
                const ClipCand c = clip_cand(mn, mx, k, J);
                const double s = clip_group_sum(clip_noise(xg, len, j, G, active, c), G);
                if (k == 0) first = best = s;
                if (s < best) {   // strict: ties keep the smallest k
                    best = s;
                    bestk = k;
                }
            }
            const ClipCand c = clip_cand(mn, mx, bestk, J);
            if (active) {
                if (bestk > 0 && !J.dry)   // candidate 0 clamps to the data range: nothing changes
                    for (int i = j; i < len; i += G) x[i] = clip_clamp(xg[i], c.lo, c.hi);
                if (j == 0) {
                    if (J.choice) J.choice[unit] = bestk;
                    if (J.range) {
                        J.range[2 * unit] = c.lo;
                        J.range[2 * unit + 1] = c.hi;
                    }
                    if (J.noise) {
                        J.noise[2 * unit] = first;
                        J.noise[2 * unit + 1] = best;
                    }
                    if (J.range_enc) {   // TENSOR modes: the tensor as the call leaves it
                        J.range_enc[0] = ~enc_ord(J.dry ? mn : clip_clamp(mn, c.lo, c.hi));
                        J.range_enc[1] = enc_ord(J.dry ? mx : clip_clamp(mx, c.lo, c.hi));
                    }
                }
            }
            wave_lds_sync();   // the copy is rewritten by the next round
        }
    }
}

// Split units: the range of every piece into its unit's record.  enc_ord is
// monotone, so integer maxima of ~enc and enc are the exact min and max whatever
// the order the pieces arrive in.
__global__ __launch_bounds__(kThreads) void clip_range_kernel(const ClipJob* __restrict__ jobs,
                                                              const ClipTask* __restrict__ tasks,
                                                              int64_t n_piece_tasks) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t wave = (int64_t)blockIdx.x * kClipWaves + (threadIdx.x >> 6);
    const int64_t n_waves = (int64_t)gridDim.x * kClipWaves;
    for (int64_t ti = wave; ti < n_piece_tasks; ti += n_waves) {
        const ClipTask t = tasks[ti];
        const ClipJob J = jobs[t.job];
        const int64_t np = clip_pieces(J.unit_len);
        const int64_t unit = t.first / np, start = (t.first % np) * kClipPiece;
        const int len = (int)(J.unit_len - start < kClipPiece ? J.unit_len - start : kClipPiece);
        const DFQ_GLOBAL float* x = (const DFQ_GLOBAL float*)J.w + unit * J.unit_len + start;
        float mn = __builtin_inff(), mx = -__builtin_inff();
        for (int i = lane; i < len; i += kWave) {
            const float v = x[i];
            mn = fminf(mn, v);
            mx = fmaxf(mx, v);
        }
        mn = wave_min(mn);
        mx = wave_max(mx);
        if (lane == 0) {   // len >= 1: both are finite values of the piece
            ClipUnit* ur = J.urec + unit;
            atomicMax(&ur->enc[0], ~enc_ord(mn));
            atomicMax(&ur->enc[1], enc_ord(mx));
        }
    }
}

// Split units: one wave per unit.  Lane k sums candidate k's partial sums in piece
// order; the argmin over the lanes takes the smaller k on equal noise.
__global__ __launch_bounds__(kThreads) void clip_finish_kernel(const ClipJob* __restrict__ jobs,
                                                               const ClipFin* __restrict__ fin, int64_t n_fin) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t wave = (int64_t)blockIdx.x * kClipWaves + (threadIdx.x >> 6);
    const int64_t n_waves = (int64_t)gridDim.x * kClipWaves;
    for (int64_t fi = wave; fi < n_fin; fi += n_waves) {
        const ClipFin f = fin[fi];
        const ClipJob J = jobs[f.job];
        const int K = J.K;
        const int64_t np = clip_pieces(J.unit_len);
        const double* s = J.slots + f.unit * np * K;
        double sum = 0.0;
        if (lane < K)
            for (int64_t p = 0; p < np; ++p) sum += s[p * K + lane];
        const double first = __shfl(sum, 0, kWave);
        double best = sum;
        int bestk = lane < K ? lane : kClipMaxCand;   // lanes without a candidate never win
        for (int off = 32; off >= 1; off >>= 1) {
            const double ob = __shfl_xor(best, off, kWave);
            const int ok = __shfl_xor(bestk, off, kWave);
            const bool mine = bestk < kClipMaxCand, theirs = ok < kClipMaxCand;
            if (theirs && (!mine || ob < best || (ob == best && ok < bestk))) {
                best = ob;
                bestk = ok;
            }
        }
        if (lane == 0) {
            ClipUnit* ur = J.urec + f.unit;
            const float mn = dec_ord(~ur->enc[0]), mx = dec_ord(ur->enc[1]);
            const ClipCand c = clip_cand(mn, mx, bestk, J);
            ur->lo = c.lo;
            ur->hi = c.hi;
            ur->k = bestk;
            if (J.choice) J.choice[f.unit] = bestk;
            if (J.range) {
                J.range[2 * f.unit] = c.lo;
                J.range[2 * f.unit + 1] = c.hi;
            }
            if (J.noise) {
                J.noise[2 * f.unit] = first;
                J.noise[2 * f.unit + 1] = best;
            }
            if (J.range_enc) {
                J.range_enc[0] = ~enc_ord(J.dry ? mn : clip_clamp(mn, c.lo, c.hi));
                J.range_enc[1] = enc_ord(J.dry ? mx : clip_clamp(mx, c.lo, c.hi));
            }
        }
    }
}

// Split units: the chosen clamp, piece by piece (skipped where the choice is
// candidate 0, which changes nothing, and for dry weights).
__global__ __launch_bounds__(kThreads) void clip_clamp_kernel(const ClipJob* __restrict__ jobs,
                                                              const ClipTask* __restrict__ tasks,
                                                              int64_t n_piece_tasks) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t wave = (int64_t)blockIdx.x * kClipWaves + (threadIdx.x >> 6);
    const int64_t n_waves = (int64_t)gridDim.x * kClipWaves;
    for (int64_t ti = wave; ti < n_piece_tasks; ti += n_waves) {
        const ClipTask t = tasks[ti];
        const ClipJob J = jobs[t.job];
        if (J.dry) continue;
        const int64_t np = clip_pieces(J.unit_len);
        const int64_t unit = t.first / np, start = (t.first % np) * kClipPiece;
        const ClipUnit ur = J.urec[unit];
        if (ur.k == 0) continue;
        const int len = (int)(J.unit_len - start < kClipPiece ? J.unit_len - start : kClipPiece);
        DFQ_GLOBAL float* x = (DFQ_GLOBAL float*)J.w + unit * J.unit_len + start;
        for (int i = lane; i < len; i += kWave) x[i] = clip_clamp(x[i], ur.lo, ur.hi);
    }
}

}  // namespace

hipError_t preload_clip() {   // see dfq_preload
    hipFuncAttributes a;
    hipError_t e = hipFuncGetAttributes(&a, reinterpret_cast<const void*>(clip_eval_kernel));
    if (e == hipSuccess) e = hipFuncGetAttributes(&a, reinterpret_cast<const void*>(clip_range_kernel));
    if (e == hipSuccess) e = hipFuncGetAttributes(&a, reinterpret_cast<const void*>(clip_finish_kernel));
    if (e == hipSuccess) e = hipFuncGetAttributes(&a, reinterpret_cast<const void*>(clip_clamp_kernel));
    return e;
}

}  // namespace dfq

using namespace dfq;

extern "C" int dfq_clip_search_batch(const dfq_clip_search_desc* d, int32_t n, void* ws, int64_t ws_bytes,
                                     void* stream) {
    if (n < 0 || (n > 0 && !d)) return DFQ_ERR_INVALID;
    if (n == 0) return DFQ_OK;
    ClipLayout L;
    std::vector<ClipTask> tasks;
    std::vector<ClipFin> fin;
    std::vector<int64_t> urec_base, slot_base;
    const int rc = clip_search_plan(d, n, L, tasks, fin, urec_base, slot_base);
    if (rc != DFQ_OK) return rc;
    if (!ws || ws_bytes < L.total) return DFQ_ERR_WORKSPACE;
    if (reinterpret_cast<uintptr_t>(ws) % 256 != 0) return DFQ_ERR_INVALID;
    char* base = static_cast<char*>(ws);
    ClipUnit* urec = reinterpret_cast<ClipUnit*>(base + L.o_urec);
    double* slots = reinterpret_cast<double*>(base + L.o_slots);
    // one staging blob (jobs, tasks, the finish list), one copy
    std::vector<char> blob((size_t)L.o_urec, 0);
    ClipJob* hj = reinterpret_cast<ClipJob*>(blob.data() + L.o_jobs);
    for (int32_t p = 0; p < n; ++p) {
        const bool tensor = d[p].mode < DFQ_CHANNEL_ASYM;
        hj[p] = ClipJob{d[p].w,
                        d[p].choice,
                        d[p].range,
                        d[p].noise,
                        tensor ? d[p].range_enc : nullptr,
                        urec_base[p] >= 0 ? urec + urec_base[p] : nullptr,
                        slot_base[p] >= 0 ? slots + slot_base[p] : nullptr,
                        clip_units(d[p]),
                        clip_unit_len(d[p]),
                        d[p].bits,
                        (d[p].mode == DFQ_TENSOR_SYM || d[p].mode == DFQ_CHANNEL_SYM) ? 1 : 0,
                        d[p].candidates,
                        (d[p].flags & DFQ_CLIP_SEARCH_DRY) ? 1 : 0,
                        d[p].min_frac,
                        0};
    }
    std::memcpy(blob.data() + L.o_tasks, tasks.data(), sizeof(ClipTask) * tasks.size());
    if (!fin.empty()) std::memcpy(blob.data() + L.o_fin, fin.data(), sizeof(ClipFin) * fin.size());
    hipStream_t s = static_cast<hipStream_t>(stream);
    DFQ_HIP_CHECK(stage_h2d(base, blob.data(), blob.size(), s));
    const ClipJob* dj = reinterpret_cast<const ClipJob*>(base + L.o_jobs);
    const ClipTask* dt = reinterpret_cast<const ClipTask*>(base + L.o_tasks);
    const ClipFin* df = reinterpret_cast<const ClipFin*>(base + L.o_fin);
    auto grid = [](int64_t waves, int64_t cap) { return (int)std::min<int64_t>(ceil_div(waves, (int64_t)kClipWaves), cap); };
    if (L.n_piece_tasks > 0) {
        DFQ_HIP_CHECK(hipMemsetAsync(urec, 0, sizeof(ClipUnit) * (size_t)L.n_split_units, s));
        hipLaunchKernelGGL(clip_range_kernel, dim3(grid(L.n_piece_tasks, 1 << 16)), dim3(kThreads), 0, s, dj, dt,
                           L.n_piece_tasks);
        DFQ_LAUNCH_CHECK();
    }
    // one wave per task up to 2^18 tasks: blocks dispatched as others retire balance the uneven tasks
    hipLaunchKernelGGL(clip_eval_kernel, dim3(grid(L.n_tasks, 1 << 16)), dim3(kThreads), 0, s, dj, dt, L.n_tasks);
    DFQ_LAUNCH_CHECK();
    if (L.n_piece_tasks > 0) {
        hipLaunchKernelGGL(clip_finish_kernel, dim3(grid(L.n_split_units, 2048)), dim3(kThreads), 0, s, dj, df,
                           L.n_split_units);
        DFQ_LAUNCH_CHECK();
        if (L.n_clamp_piece_tasks > 0) {
            hipLaunchKernelGGL(clip_clamp_kernel, dim3(grid(L.n_piece_tasks, 1 << 16)), dim3(kThreads), 0, s, dj, dt,
                               L.n_piece_tasks);
            DFQ_LAUNCH_CHECK();
        }
    }
    return DFQ_OK;
}
