// dfq_pair_stats_batch: per-channel signal, noise, worst error and range of many
// (reference, compared) tensor pairs (include/dfq_hip.h).  Two plain launches:
//   1. pair_stats_kernel: a grid-stride loop over the planner's task table
//      (dfq_stats_plan.h), one wave per task.  A whole-row task writes its rows'
//      records; a piece task writes one partial slot.
//   2. pair_finish_kernel: one wave per pair sums each split row's pieces in piece
//      order, then the pair's totals over its rows.
// Nothing is handed from workgroup to workgroup inside a launch.  The kernel reads
// 8 B per element and does four fp64 operations on them: HBM-bound.
#include "dfq_common.h"
#include "dfq_stats_plan.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace dfq {
namespace {

constexpr int kPairDepth = 4;   // 16-B loads of each array in flight per lane

struct PairAcc {
    double sig = 0.0, noi = 0.0;
    float me = 0.f, ma = 0.f;
};

// e = fl32(y - x); the two squares are exact in fp64, so only the sums round -- and
// a fused multiply-add gives the bits of the multiply followed by the add
__device__ __forceinline__ void pair_add(PairAcc& a, float x, float y) {
    const float e = y - x;
    a.sig = __builtin_fma((double)x, (double)x, a.sig);
    a.noi = __builtin_fma((double)e, (double)e, a.noi);
    a.me = fmaxf(a.me, fabsf(e));
    a.ma = fmaxf(a.ma, fabsf(x));
}
__device__ __forceinline__ void pair_add4(PairAcc& a, const f32x4 x, const f32x4 y) {
    pair_add(a, x.x, y.x);
    pair_add(a, x.y, y.y);
    pair_add(a, x.z, y.z);
    pair_add(a, x.w, y.w);
}

// Elements [0, len) of one row or piece by the G lanes of a group (this lane: j).
// vec: x and y share their misalignment modulo 16 -- scalars up to the first 16-B
// boundary, 16-B loads, a scalar tail; otherwise 4-B loads throughout.  Nothing
// outside [0, len) is touched.
__device__ __forceinline__ void pair_segment(PairAcc& a, const DFQ_GLOBAL float* x, const DFQ_GLOBAL float* y,
                                             int64_t len, int j, int G, bool vec) {
    if (!vec) {
#pragma unroll 1
        for (int64_t i = j; i < len; i += G) pair_add(a, x[i], y[i]);
        return;
    }
    int64_t head = (int64_t)(((16u - (uint32_t)(reinterpret_cast<uintptr_t>(x) & 15u)) & 15u) >> 2);
    if (head > len) head = len;
    const int64_t nv = (len - head) >> 2;
    const int64_t tail0 = head + 4 * nv;
#pragma unroll 1
    for (int64_t i = j; i < head; i += G) pair_add(a, x[i], y[i]);
    const DFQ_GLOBAL f32x4* xv = reinterpret_cast<const DFQ_GLOBAL f32x4*>(x + head);
    const DFQ_GLOBAL f32x4* yv = reinterpret_cast<const DFQ_GLOBAL f32x4*>(y + head);
    // kPairDepth 16-B loads per array in flight per lane; a lane's vectors are added in
    // increasing order.  Past the end a zero vector stands in: x = y = 0 adds +0 to the
    // sums and changes no maximum, so the padding leaves every bit as it was.
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int64_t k = j; k < nv; k += (int64_t)kPairDepth * G) {
        f32x4 xs[kPairDepth], ys[kPairDepth];
#pragma unroll
        for (int i = 0; i < kPairDepth; ++i) {
            const int64_t q = k + (int64_t)i * G;
            xs[i] = q < nv ? xv[q] : zero;
            ys[i] = q < nv ? yv[q] : zero;
        }
#pragma unroll
        for (int i = 0; i < kPairDepth; ++i) pair_add4(a, xs[i], ys[i]);
    }
#pragma unroll 1
    for (int64_t i = tail0 + j; i < len; i += G) pair_add(a, x[i], y[i]);
}

// Over aligned groups of G lanes (a power of two, wave-uniform), a fixed butterfly:
// every lane ends with its group's result.  All 64 lanes take part.
__device__ __forceinline__ void pair_group_reduce(PairAcc& a, int G) {
    for (int off = G >> 1; off >= 1; off >>= 1) {
        a.sig += __shfl_xor(a.sig, off, kWave);
        a.noi += __shfl_xor(a.noi, off, kWave);
        a.me = fmaxf(a.me, __shfl_xor(a.me, off, kWave));
        a.ma = fmaxf(a.ma, __shfl_xor(a.ma, off, kWave));
    }
}

__device__ __forceinline__ void pair_store(double* rec, const PairAcc& a) {
    rec[0] = a.sig;
    rec[1] = a.noi;
    rec[2] = (double)a.me;
    rec[3] = (double)a.ma;
}

// 4 waves per SIMD: the four-deep loads need 124 VGPRs (at 5 or 6 waves they spill)
__global__ __launch_bounds__(kThreads, 4) void pair_stats_kernel(const PairJob* __restrict__ jobs,
                                                                 const PairTask* __restrict__ tasks,
                                                                 int64_t n_tasks) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t wave = (int64_t)blockIdx.x * (kThreads / kWave) + (threadIdx.x >> 6);
    const int64_t n_waves = (int64_t)gridDim.x * (kThreads / kWave);
    for (int64_t ti = wave; ti < n_tasks; ti += n_waves) {
        const PairTask t = tasks[ti];
        const PairJob J = jobs[t.pair];
        const DFQ_GLOBAL float* x = (const DFQ_GLOBAL float*)J.x;
        const DFQ_GLOBAL float* y = (const DFQ_GLOBAL float*)J.y;
        const bool vec = ((reinterpret_cast<uintptr_t>(J.x) ^ reinterpret_cast<uintptr_t>(J.y)) & 15u) == 0;
        // Segments of the task: its rows, 64 / G at a time with G lanes each, or its one
        // piece with the whole wave.  Segment q writes record `first + q` of rows_buf / slots.
        const bool piece = t.nrows == 0;
        const int nseg = piece ? 1 : t.nrows;
        const int G = piece ? kWave : pair_group_lanes(J.row_len), per = kWave / G;
        const int g = lane / G, j = lane % G;
        const int64_t np = pair_pieces(J.row_len);
        double* out = piece ? J.slots : J.rows_buf;
        for (int base = 0; base < nseg; base += per) {
            const int q = base + g;
            PairAcc a;
            if (q < nseg) {
                int64_t off = (t.first + q) * J.row_len, len = J.row_len;
                if (piece) {
                    const int64_t start = (t.first % np) * kPairPiece;
                    off = (t.first / np) * J.row_len + start;
                    len = J.row_len - start < kPairPiece ? J.row_len - start : kPairPiece;
                }
                pair_segment(a, x + off, y + off, len, j, G, vec);
            }
            pair_group_reduce(a, G);
            if (q < nseg && j == 0) pair_store(out + (t.first + q) * kPairSlotDoubles, a);
        }
    }
}

// One wave per pair.  Lane l takes rows l, l + 64, ... in increasing order: a split
// row's record is its pieces summed in piece order (written to rows_buf); the
// pair's totals are each lane's rows summed in that order, then the 64 lane sums
// in the fixed butterfly.
__global__ __launch_bounds__(kThreads) void pair_finish_kernel(const PairJob* __restrict__ jobs, int64_t n) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t wave = (int64_t)blockIdx.x * (kThreads / kWave) + (threadIdx.x >> 6);
    const int64_t n_waves = (int64_t)gridDim.x * (kThreads / kWave);
    for (int64_t p = wave; p < n; p += n_waves) {
        const PairJob J = jobs[p];
        if (!J.slots && !J.total_out) continue;
        const int64_t np = pair_pieces(J.row_len);
        PairAcc tot;
        for (int64_t r = lane; r < J.rows; r += kWave) {
            double* rec = J.rows_buf + r * kPairSlotDoubles;
            double sig, noi, me, ma;
            if (J.slots) {
                const double* s = J.slots + r * np * kPairSlotDoubles;
                sig = noi = me = ma = 0.0;
                for (int64_t k = 0; k < np; ++k, s += kPairSlotDoubles) {
                    sig += s[0];
                    noi += s[1];
                    me = fmax(me, s[2]);
                    ma = fmax(ma, s[3]);
                }
                rec[0] = sig;
                rec[1] = noi;
                rec[2] = me;
                rec[3] = ma;
            } else {
                sig = rec[0];
                noi = rec[1];
                me = rec[2];
                ma = rec[3];
            }
            tot.sig += sig;
            tot.noi += noi;
            tot.me = fmaxf(tot.me, (float)me);   // fp32 values widened: the narrowing is exact
            tot.ma = fmaxf(tot.ma, (float)ma);
        }
        if (!J.total_out) continue;
        pair_group_reduce(tot, kWave);
        if (lane == 0) pair_store(J.total_out, tot);
    }
}

}  // namespace

hipError_t preload_stats() {   // see dfq_preload
    hipFuncAttributes a;
    hipError_t e = hipFuncGetAttributes(&a, reinterpret_cast<const void*>(pair_stats_kernel));
    if (e == hipSuccess) e = hipFuncGetAttributes(&a, reinterpret_cast<const void*>(pair_finish_kernel));
    return e;
}

}  // namespace dfq

using namespace dfq;

extern "C" int dfq_pair_stats_batch(const dfq_pair_desc* d, int32_t n, void* ws, int64_t ws_bytes, void* stream) {
    if (n < 0 || (n > 0 && !d)) return DFQ_ERR_INVALID;
    if (n == 0) return DFQ_OK;
    PairLayout L;
    std::vector<PairTask> tasks;
    std::vector<int64_t> slot_base, row_base;
    const int rc = pair_stats_plan(d, n, L, tasks, slot_base, row_base);
    if (rc != DFQ_OK) return rc;
    if (!ws || ws_bytes < L.total) return DFQ_ERR_WORKSPACE;
    if (reinterpret_cast<uintptr_t>(ws) % 256 != 0) return DFQ_ERR_INVALID;
    char* base = static_cast<char*>(ws);
    double* slots = reinterpret_cast<double*>(base + L.o_slots);
    double* buf_rows = reinterpret_cast<double*>(base + L.o_rows);
    // one staging blob (jobs, then tasks), one copy
    std::vector<char> blob((size_t)L.o_slots, 0);
    PairJob* hj = reinterpret_cast<PairJob*>(blob.data() + L.o_jobs);
    for (int32_t p = 0; p < n; ++p)
        hj[p] = PairJob{d[p].x,
                        d[p].y,
                        d[p].rows_out ? d[p].rows_out : buf_rows + row_base[p] * kPairSlotDoubles,
                        d[p].total_out,
                        slot_base[p] >= 0 ? slots + slot_base[p] * kPairSlotDoubles : nullptr,
                        d[p].rows,
                        d[p].row_len};
    std::memcpy(blob.data() + L.o_tasks, tasks.data(), sizeof(PairTask) * tasks.size());
    hipStream_t s = static_cast<hipStream_t>(stream);
    DFQ_HIP_CHECK(stage_h2d(base, blob.data(), blob.size(), s));
    const PairJob* dj = reinterpret_cast<const PairJob*>(base + L.o_jobs);
    const PairTask* dt = reinterpret_cast<const PairTask*>(base + L.o_tasks);
    constexpr int kWavesPerBlock = kThreads / kWave;
    // one wave per task up to 2^18 tasks: at 4 waves per SIMD a 2048-block grid is not
    // resident at once, and blocks dispatched as others retire balance the uneven tasks
    const int grid1 = (int)std::min<int64_t>(ceil_div(L.n_tasks, (int64_t)kWavesPerBlock), 1 << 16);
    hipLaunchKernelGGL(pair_stats_kernel, dim3(grid1), dim3(kThreads), 0, s, dj, dt, L.n_tasks);
    DFQ_LAUNCH_CHECK();
    const int grid2 = (int)std::min<int64_t>(ceil_div((int64_t)n, (int64_t)kWavesPerBlock), 2048);
    hipLaunchKernelGGL(pair_finish_kernel, dim3(grid2), dim3(kThreads), 0, s, dj, (int64_t)n);
    DFQ_LAUNCH_CHECK();
    return DFQ_OK;
}
