// dfq_mx_quantize_batch: OCP Microscaling (MX) block-scaled quantization of every
// tensor of a list in one launch and one HBM pass (include/dfq_hip.h).  One wave per
// task of the planner's table (dfq_mx_plan.h).
//
// A task's padded elements (its rows, each padded to whole 32-element MX blocks) are
// numbered v = 0, 1, ...; one wave round takes 256 of them, four consecutive ones per
// lane, so eight neighbouring lanes hold one MX block: the block's amax is a maximum
// over those eight lanes (DPP, on the magnitudes' bit patterns: integer compares,
// no NaN rule, no canonicalisation), each lane converts its four elements and stores
// 16 B of dst, 2 B of packed FP4, 3 B of packed FP6 or 4 B of FP8, and the block's
// first lane its scale byte -- all of them consecutive across the wave.  Codes and
// scales are addressed by v alone ([rows, nb, 16 | 24 | 32] and [rows, nb] are the
// padded numbering), so the padding of a partial block is written as +0 codes by the
// lanes that hold it.  (FP6: a lane's four codes are 24 bits; on the 16-B path a quad
// of lanes regroups its 12 bytes into three dword stores, mx_task.)
// Rows that do not start 16-B aligned take the same walk with 4-B accesses.
// The conversion is plain integer / fp32 arithmetic (mx_encode): exact power-of-two
// scalings, one round-to-nearest-even (v_rndne_f32) and a saturating integer min.
// (gfx950's v_cvt_scalef32_pk_fp8_f32 gives the E4M3 NaN code 0x7F where the contract
// saturates to 448, and a build on the scaled converts was no faster: DESIGN.md 3.7.)
// Error sums: khw == 1 stores fl32(y - x) as it goes; khw > 1 keeps the task's
// errors in the wave's LDS copy and one lane adds each khw group in ATen's order
// (aten_inner_sum, the sweep's helper).  No atomic, nothing handed between waves.
// dfq_mx_quantize_search_batch is the same walk with one more step after the amax: each lane
// encodes its four elements under the floor rule's exponent X0 and under X0 + 1, the block's
// eight lanes add the two candidates' squared errors (mx_noise8: fp32, one instruction
// sequence for both, the amax's three DPP exchanges) and all take X0 + 1 iff its sum is
// strictly smaller.  Equal candidates tie and keep X0; nothing else changes.
#include "dfq_common.h"
#include "dfq_mx_encode.h"
#include "dfq_mx_plan.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace dfq {
namespace {

constexpr int kMxWaves = kThreads / kWave;
constexpr int kMxBatch = 4;   // rounds whose loads are issued together (dst may alias src: the
                              // compiler cannot move a round's loads above the previous round's stores)

// max over aligned groups of 8 lanes (quad swaps, then the half-row mirror)
__device__ __forceinline__ uint32_t max8(uint32_t m) {
    int x = (int)m;   // magnitudes: bit 31 clear, the integer order is the float order
    x = max(x, __builtin_amdgcn_update_dpp(x, x, 0xB1, 0xF, 0xF, false));
    x = max(x, __builtin_amdgcn_update_dpp(x, x, 0x4E, 0xF, 0xF, false));
    x = max(x, __builtin_amdgcn_update_dpp(x, x, 0x141, 0xF, 0xF, false));
    return (uint32_t)x;
}

// A block's noise under one exponent, the same bits in its eight lanes: the lane's four
// fl32(y - x) * s (s = 2^-X0: exact, and a 2^-100 block's squares stay normal), squared and added
// in element order, then added across the lanes by max8's three exchanges.  fp32 add is
// commutative, so both partners of an exchange hold the same sum.  Explicitly rounded
// operations: two candidates that are equal element for element give equal sums.
__device__ __forceinline__ float mx_noise8(const float (&y)[4], const float (&x)[4], float s) {
    float n = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float t = __fmul_rn(__fsub_rn(y[j], x[j]), s);
        n = j == 0 ? __fmul_rn(t, t) : __fadd_rn(n, __fmul_rn(t, t));
    }
    n = __fadd_rn(n, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(n), 0xB1, 0xF, 0xF, false)));
    n = __fadd_rn(n, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(n), 0x4E, 0xF, 0xF, false)));
    n = __fadd_rn(n, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(n), 0x141, 0xF, 0xF, false)));
    return n;
}

// the value of the lane's right-hand neighbour in its quad (lane 3: of lane 0)
__device__ __forceinline__ uint32_t quad_next(uint32_t w) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)w, (int)w, 0x39, 0xF, 0xF, false);
}

// The wave's task.  vtotal padded elements; padded element v lies in row
// t.row + v / lp at column t.col + v % lp (lp: the padded length of a row, or of the piece).
template <int FMT, bool VEC, bool SEARCH = false>
__device__ __forceinline__ void mx_task(const MxJob& J, const MxTask& t, float* edata, int lane) {
    const int64_t row_len = J.row_len;
    const int64_t lpr = J.nb * kMxBlock;   // padded row
    int lp, nrows;
    if (t.nrows > 0) {
        lp = (int)lpr;
        nrows = t.nrows;
    } else {
        const int64_t len = row_len - t.col < J.piece ? row_len - t.col : J.piece;
        lp = (int)(ceil_div(len, kMxBlock) * kMxBlock);
        nrows = 1;
    }
    const int vtotal = nrows * lp;
    const uint32_t magic = 0xFFFFFFFFu / (uint32_t)lp + 1u;   // v / lp == umulhi(v, magic) for v * lp < 2^32
    const int64_t vbase = t.row * lpr + t.col;                 // the task's first padded element of the tensor
    const int64_t ebase = t.row * row_len + t.col;             // its first element
    const int rl = (int)(row_len < (int64_t)1 << 30 ? row_len : (int64_t)1 << 30);   // nrows > 1: row_len <= lp
    const int left0 = (int)(row_len - t.col < (int64_t)1 << 30 ? row_len - t.col : (int64_t)1 << 30);
    // the task's own bases (wave-uniform): a lane adds 32-bit offsets below the task's size
    const DFQ_GLOBAL float* src = (const DFQ_GLOBAL float*)J.src + ebase;
    DFQ_GLOBAL float* dst = (DFQ_GLOBAL float*)J.dst + ebase;
    DFQ_GLOBAL float* esum = (DFQ_GLOBAL float*)J.esum + ebase;   // khw == 1 (the LDS sums index from J.esum)
    DFQ_GLOBAL uint8_t* codes = (DFQ_GLOBAL uint8_t*)J.codes +
                                (FMT == DFQ_MX_FP4_E2M1 ? vbase >> 1 : kMxFp6<FMT> ? (vbase >> 2) * 3 : vbase);   // vbase % 32 == 0
    DFQ_GLOBAL uint8_t* scales = (DFQ_GLOBAL uint8_t*)J.scales + (vbase >> 5);
    const bool want_d = J.dst != nullptr, want_c = J.codes != nullptr, want_s = J.scales != nullptr;
    const bool want_e = J.esum != nullptr, lds_e = J.lds_esum != 0;

    for (int v0 = 0; v0 < vtotal; v0 += 256 * kMxBatch) {
        float x[kMxBatch][4];
        int off[kMxBatch];       // element offset from the task's first element of the lane's first element
        int nval[kMxBatch];      // its elements inside the row (0..4); VEC: 0 or 4
#pragma unroll
        for (int b = 0; b < kMxBatch; ++b) {
            const int v = v0 + b * 256 + 4 * lane;
            const int r = nrows > 1 ? (int)__umulhi((uint32_t)v, magic) : 0;
            const int c = v - r * lp;   // column inside the task's row part
            const int left = left0 - c;
            nval[b] = v < vtotal ? (left >= 4 ? 4 : (left > 0 ? left : 0)) : 0;
            off[b] = r * rl + c;
            x[b][0] = x[b][1] = x[b][2] = x[b][3] = 0.f;   // padding behaves as +0
            if (VEC) {
                if (nval[b]) {
                    const f32x4 q = *(const DFQ_GLOBAL f32x4*)(src + off[b]);
                    x[b][0] = q.x; x[b][1] = q.y; x[b][2] = q.z; x[b][3] = q.w;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < nval[b]) x[b][j] = src[off[b] + j];
            }
        }
#pragma unroll
        for (int b = 0; b < kMxBatch; ++b) {
            const int v = v0 + b * 256 + 4 * lane;
            if (v0 + b * 256 >= vtotal) break;   // wave-uniform
            uint32_t m = __float_as_uint(x[b][0]) & 0x7fffffffu;
#pragma unroll
            for (int j = 1; j < 4; ++j) m = max(m, __float_as_uint(x[b][j]) & 0x7fffffffu);
            m = max8(m);   // every lane takes part
            int X = mx_exponent<FMT>(m);
            const float inv = pow2f(-X), up = pow2f(X);
            float y[4];
            uint32_t c[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) c[j] = mx_encode<FMT>(x[b][j], inv, up, y[j]);
            if (SEARCH) {
                // the block under X + 1 as well, and the two noises N_d = sum ((y_d - x) * 2^-X)^2 (X: the
                // floor rule's), each by mx_noise8; X + 1 <= 127 - emax + 1 < 127.  An all-zero block
                // (X = -127) is termwise equal under -126 and keeps X.
                const float inv1 = pow2f(-(X + 1)), up1 = pow2f(X + 1);
                float y1[4];
                uint32_t c1[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) c1[j] = mx_encode<FMT>(x[b][j], inv1, up1, y1[j]);
                const float n0 = mx_noise8(y, x[b], inv), n1 = mx_noise8(y1, x[b], inv);   // every lane takes part
                if (n1 < n0) {   // the same two sums in the block's eight lanes: one choice
                    X += 1;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        y[j] = y1[j];
                        c[j] = c1[j];
                    }
                }
            }
            // FP6: a lane's codes are the 24 bits w, a quad's 16 elements three dwords
            //   d0 = w0 | w1 << 24,  d1 = w1 >> 8 | w2 << 16,  d2 = w2 >> 16 | w3 << 8
            // lanes 0..2 of the quad build one each from their own w and their neighbour's (every
            // lane takes part; vtotal % 32 == 0, so a quad lies inside the task or outside it)
            uint32_t w6 = 0, d6 = 0;
            if (kMxFp6<FMT>) {
                w6 = c[0] | (c[1] << 6) | (c[2] << 12) | (c[3] << 18);
                if (VEC) {
                    const int sh = 8 * (lane & 3);
                    d6 = (w6 >> sh) | (quad_next(w6) << (24 - sh));   // lane 3: not stored
                }
            }
            if (v >= vtotal) continue;
            // v numbers the task's padded elements: it addresses the codes and scales
            if (want_c) {
                if (FMT == DFQ_MX_FP4_E2M1) {
                    const uint32_t lo = c[0] | (c[1] << 4), hi = c[2] | (c[3] << 4);
                    if (VEC) {
                        *(DFQ_GLOBAL uint16_t*)(codes + (v >> 1)) = (uint16_t)(lo | (hi << 8));
                    } else {
                        codes[v >> 1] = (uint8_t)lo;
                        codes[(v >> 1) + 1] = (uint8_t)hi;
                    }
                } else if (kMxFp6<FMT>) {
                    if (VEC) {   // 48 consecutive dwords per wave round
                        if ((lane & 3) != 3) *(DFQ_GLOBAL uint32_t*)(codes + (v >> 4) * 12 + 4 * (lane & 3)) = d6;
                    } else {
                        DFQ_GLOBAL uint8_t* p = codes + (v >> 2) * 3;
                        p[0] = (uint8_t)w6;
                        p[1] = (uint8_t)(w6 >> 8);
                        p[2] = (uint8_t)(w6 >> 16);
                    }
                } else {
                    if (VEC) {
                        *(DFQ_GLOBAL uint32_t*)(codes + v) = c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24);
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j) codes[v + j] = (uint8_t)c[j];
                    }
                }
            }
            if (want_s && (lane & 7) == 0) scales[v >> 5] = (uint8_t)(X + 127);
            if (!nval[b]) continue;
            const int eg = off[b];
            float e[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) e[j] = y[j] - x[b][j];
            if (VEC) {
                if (want_d) {
                    f32x4 q;
                    q.x = y[0]; q.y = y[1]; q.z = y[2]; q.w = y[3];
                    *(DFQ_GLOBAL f32x4*)(dst + eg) = q;
                }
                if (want_e && !lds_e) {
                    f32x4 q;
                    q.x = e[0]; q.y = e[1]; q.z = e[2]; q.w = e[3];
                    *(DFQ_GLOBAL f32x4*)(esum + eg) = q;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (j >= nval[b]) break;
                    if (want_d) dst[eg + j] = y[j];
                    if (want_e && !lds_e) esum[eg + j] = e[j];
                }
            }
            if (lds_e) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < nval[b]) edata[off[b] + j] = e[j];
            }
        }
    }
    if (lds_e) {
        // E[p] = sum_k e[p * khw + k] in torch.sum(e.view(O, I, khw), -1)'s order: the task holds
        // whole khw groups (rows, or pieces that are multiples of khw)
        wave_lds_sync();
        const int khw = J.khw;
        const int n = t.nrows > 0 ? (int)(nrows * row_len) : (int)(row_len - t.col < J.piece ? row_len - t.col : J.piece);
        const int np = n / khw;
        DFQ_GLOBAL float* out = (DFQ_GLOBAL float*)J.esum + ebase / khw;
        if (khw == 9) {
            for (int pi = lane; pi < np; pi += kWave) {
                const float* e = edata + pi * 9;
                out[pi] = aten_inner_sum([&](int64_t k) { return e[k]; }, (int64_t)9);
            }
        } else {
            for (int pi = lane; pi < np; pi += kWave) {
                const float* e = edata + pi * khw;
                out[pi] = aten_inner_sum([&](int64_t k) { return e[k]; }, (int64_t)khw);
            }
        }
        wave_lds_sync();   // the copy is rewritten by the wave's next task
    }
}

// LDS (dynamic): DFQ_MX_ESUM_TASK_ELEMS floats per wave when some tensor's error sums
// need them, none otherwise; written and read by its own wave only.
// One kernel walks the tasks of two formats, F0 and F1, with or without the scale search
// (dfq_mx_quantize_search_batch): four mx_task variants each.  There are four instantiations
// and not one kernel because all eight floor-rule variants in one kernel take 167 VGPRs and
// spill SGPRs; apart they take 133 (FP4 / FP8) and 149 (FP6), searched 142 and 160, no
// scratch.  The host hands each instantiation its own tasks (mx_quantize_run).  The
// template compiles to the same instructions as four bodies written out.
template <int F0, int F1, bool SEARCH>
__global__ __launch_bounds__(kThreads) void mx_quantize_kernel_t(const MxJob* __restrict__ jobs,
                                                                 const MxTask* __restrict__ tasks, int64_t n_tasks) {
    extern __shared__ __attribute__((aligned(16))) float mx_lds[];
    float* const edata = mx_lds + (threadIdx.x >> 6) * DFQ_MX_ESUM_TASK_ELEMS;
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t wave = (int64_t)blockIdx.x * kMxWaves + (threadIdx.x >> 6);
    const int64_t n_waves = (int64_t)gridDim.x * kMxWaves;
    for (int64_t ti = wave; ti < n_tasks; ti += n_waves) {
        const MxTask t = tasks[ti];
        const MxJob J = jobs[t.job];
        if (J.format == F0) {
            if (J.vec) mx_task<F0, true, SEARCH>(J, t, edata, lane);
            else mx_task<F0, false, SEARCH>(J, t, edata, lane);
        } else {
            if (J.vec) mx_task<F1, true, SEARCH>(J, t, edata, lane);
            else mx_task<F1, false, SEARCH>(J, t, edata, lane);
        }
    }
}
constexpr auto mx_quantize_kernel = mx_quantize_kernel_t<DFQ_MX_FP4_E2M1, DFQ_MX_FP8_E4M3, false>;
constexpr auto mx6_quantize_kernel = mx_quantize_kernel_t<DFQ_MX_FP6_E2M3, DFQ_MX_FP6_E3M2, false>;
constexpr auto mx_search_quantize_kernel = mx_quantize_kernel_t<DFQ_MX_FP4_E2M1, DFQ_MX_FP8_E4M3, true>;
constexpr auto mx6_search_quantize_kernel = mx_quantize_kernel_t<DFQ_MX_FP6_E2M3, DFQ_MX_FP6_E3M2, true>;

}  // namespace

hipError_t preload_mx() {   // see dfq_preload
    hipFuncAttributes a;
    for (const void* k : {reinterpret_cast<const void*>(mx_quantize_kernel), reinterpret_cast<const void*>(mx6_quantize_kernel),
                          reinterpret_cast<const void*>(mx_search_quantize_kernel),
                          reinterpret_cast<const void*>(mx6_search_quantize_kernel)}) {
        const hipError_t e = hipFuncGetAttributes(&a, k);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace dfq

using namespace dfq;

namespace {

// both entry points: `search` picks the kernels, nothing else differs
int mx_quantize_run(const dfq_mx_desc* d, int32_t n, void* ws, int64_t ws_bytes, void* stream, bool search) {
    if (n < 0 || (n > 0 && !d)) return DFQ_ERR_INVALID;
    if (n == 0) return DFQ_OK;
    MxLayout L;
    std::vector<MxTask> tasks;
    const int rc = mx_plan(d, n, L, tasks);
    if (rc != DFQ_OK) return rc;
    if (!ws || ws_bytes < L.total) return DFQ_ERR_WORKSPACE;
    if (reinterpret_cast<uintptr_t>(ws) % 256 != 0) return DFQ_ERR_INVALID;
    char* base = static_cast<char*>(ws);
    std::vector<char> blob((size_t)L.total, 0);   // one staging blob (jobs, tasks), one copy
    MxJob* hj = reinterpret_cast<MxJob*>(blob.data() + L.o_jobs);
    const auto fp6 = [&](int32_t p) { return d[p].format == DFQ_MX_FP6_E2M3 || d[p].format == DFQ_MX_FP6_E3M2; };
    bool lds_of[2] = {false, false};   // [the FP4 / FP8 tasks, the FP6 tasks]: some error sums go through LDS
    int32_t n_fp6 = 0;
    for (int32_t p = 0; p < n; ++p) {
        lds_of[fp6(p)] |= mx_lds_esum(d[p]);
        n_fp6 += fp6(p);
        hj[p] = MxJob{d[p].src, d[p].dst, d[p].codes, d[p].scales, d[p].esum, d[p].row_len, mx_blocks(d[p].row_len),
                      mx_split(d[p]) ? mx_piece_len(d[p]) : 0, d[p].khw, d[p].format, mx_vec(d[p]) ? 1 : 0,
                      mx_lds_esum(d[p]) ? 1 : 0};
    }
    // one launch per kernel that has tasks.  A list of one kind (the usual call) keeps its table
    // as planned; a mixed one keeps the list order inside each kind, the FP6 tasks behind the others
    int64_t n_first = n_fp6 == 0 ? L.n_tasks : 0;
    if (n_fp6 != 0 && n_fp6 != n)
        n_first = std::stable_partition(tasks.begin(), tasks.end(), [&](const MxTask& t) { return !fp6(t.job); }) -
                  tasks.begin();
    std::memcpy(blob.data() + L.o_tasks, tasks.data(), sizeof(MxTask) * tasks.size());
    hipStream_t s = static_cast<hipStream_t>(stream);
    DFQ_HIP_CHECK(stage_h2d(base, blob.data(), blob.size(), s));
    const MxJob* dj = reinterpret_cast<const MxJob*>(base + L.o_jobs);
    const MxTask* dt = reinterpret_cast<const MxTask*>(base + L.o_tasks);
    for (int k = 0; k < 2; ++k) {
        const int64_t first = k == 0 ? 0 : n_first, count = k == 0 ? n_first : L.n_tasks - n_first;
        if (count == 0) continue;
        // one wave per task up to 2^18 tasks: blocks dispatched as others retire balance the uneven tasks
        const int grid = (int)std::min<int64_t>(ceil_div(count, (int64_t)kMxWaves), 1 << 16);
        const size_t lds = lds_of[k] ? sizeof(float) * kMxWaves * DFQ_MX_ESUM_TASK_ELEMS : 0;
        const auto kernel = search ? (k == 0 ? mx_search_quantize_kernel : mx6_search_quantize_kernel)
                                   : (k == 0 ? mx_quantize_kernel : mx6_quantize_kernel);
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(kThreads), lds, s, dj, dt + first, count);
        DFQ_LAUNCH_CHECK();
    }
    return DFQ_OK;
}

}  // namespace

extern "C" int dfq_mx_quantize_batch(const dfq_mx_desc* d, int32_t n, void* ws, int64_t ws_bytes, void* stream) {
    return mx_quantize_run(d, n, ws, ws_bytes, stream, false);
}

extern "C" int dfq_mx_quantize_search_batch(const dfq_mx_desc* d, int32_t n, void* ws, int64_t ws_bytes, void* stream) {
    return mx_quantize_run(d, n, ws, ws_bytes, stream, true);
}
