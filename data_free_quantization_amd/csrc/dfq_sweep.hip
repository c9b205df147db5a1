// Grouped quantize-dequantize sweep over many fp32 weight tensors (gfx950).
//
// Replaces, for every target layer at once:
//   * quantize()/UniformQuantize.forward          utils/quantize.py:16-89
//   * quantize_targ_layer's per-layer loop         utils/layer_transform.py:288-305
//   * clip_weight's clamp                          clip_weight.py:29
//   * the bias-correction error reduction          bias_correction.py:128-131,231
//
// Work decomposition: every tensor is cut on the host into WAVE TASKS of at most
// kChunk (2048) contiguous fp32 elements.  A task is either
//   - "whole rows": up to kMaxRows complete rows; the wave reduces each row's
//     min/max itself (CHANNEL modes, row_len <= kChunk), or
//   - a "block-row piece": rows longer than kChunk (up to 4 pieces, e.g. the
//     4608-element rows of ResNet-50's 512x512x3x3 convs) and small per-tensor
//     ranges are split over the 4 waves of ONE workgroup: the 4 pieces sit at
//     list positions 4k..4k+3, so the 4 waves of a block meet them in the same
//     grid-stride iteration, combine their partial (min, max) through LDS with
//     one s_barrier, and each quantizes its own piece -- a single HBM pass, or
//   - a "piece": its (min, max) come from a workspace slot filled by the
//     reduce launch (large TENSOR-mode ranges; rows longer than 4 pieces).
// One wave owns one task at a time (no workgroup barriers): it streams the chunk
// HBM -> VGPRs with 16-B loads, stages it in a wave-private LDS region for the
// per-row reductions and the KHW error sums, and writes dq (16 B/lane), codes
// (4 B/lane) and E.  Waves walk the task table grid-stride (persistent grid).
#include "dfq_common.h"
#include "dfq_sweep_plan.h"   // Variant, DevTensor, DevTask, the planner (host-only C++)
#ifdef DFQ_DIAGNOSTICS
#include "dfq_diag.h"
#endif

#include <algorithm>
#include <cstring>
#include <cstdlib>
#include <new>
#include <type_traits>
#include <utility>
#include <vector>

namespace dfq {

constexpr int kBlockThreads = kWave * kWavesPerBlock;

__device__ __forceinline__ int64_t task_elem_start(const DevTask& k, const DevTensor& T) { return k.src - T.src; }

// Per-wave LDS image: [NB buffers of CHUNK floats][MAXROWS scales][MAXROWS mins]
// [MAXROWS reciprocal scales],
// carved out of ONE __shared__ array (a second __shared__ object next to an
// LDS-DMA target can make hipcc drain vmcnt before every ds_read).
template <int CHUNK, int MAXROWS, int NB>
struct LdsLayout {
    static constexpr int kPerWave = NB * CHUNK + 3 * MAXROWS;
    static constexpr int kTotal = kWavesPerBlock * kPerWave;
};

__device__ __forceinline__ bool is_sym(int mode) { return mode == DFQ_TENSOR_SYM || mode == DFQ_CHANNEL_SYM; }

typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) void gbl_void_t;

// HBM -> LDS without a VGPR landing (global_load_lds_dwordx4 / _dword): lane l's
// bytes land at lds_base + l*size, so one wave-instruction fills a contiguous
// 1 KiB (16 B/lane) or 256 B (4 B/lane) block of the task's LDS image.
template <bool NT = false>
__device__ __forceinline__ void glds16(const float* g, float* lds_base) {
    __builtin_amdgcn_global_load_lds((gbl_void_t*)g, (lds_void_t*)lds_base, 16, 0, NT ? 2 : 0);
}
template <bool NT = false>
__device__ __forceinline__ void glds4(const float* g, float* lds_base) {
    __builtin_amdgcn_global_load_lds((gbl_void_t*)g, (lds_void_t*)lds_base, 4, 0, NT ? 2 : 0);
}
// The same DMA issued through inline asm, which the compiler's wait-count pass does
// not see as a pending LDS write: with the builtin, every LDS read after a
// partial vmcnt wait got its own vmcnt(0) (the compiler cannot tell which DMA a
// read depends on), which undoes the two-batch overlap (compute_task_split).
// Every LDS read of a task's chunk is then ordered by the explicit waits alone.
template <bool NT = false>
__device__ __forceinline__ void glds16_asm(const float* g, float* lds_base) {
    const uint32_t m0 = (uint32_t)(uintptr_t)(lds_void_t*)lds_base;
    if constexpr (NT) asm volatile("global_load_lds_dwordx4 %0, off nt" ::"v"(g), "{m0}"(m0) : "memory");
    else asm volatile("global_load_lds_dwordx4 %0, off" ::"v"(g), "{m0}"(m0) : "memory");
}
template <bool NT = false>
__device__ __forceinline__ void glds4_asm(const float* g, float* lds_base) {
    const uint32_t m0 = (uint32_t)(uintptr_t)(lds_void_t*)lds_base;
    if constexpr (NT) asm volatile("global_load_lds_dword %0, off nt" ::"v"(g), "{m0}"(m0) : "memory");
    else asm volatile("global_load_lds_dword %0, off" ::"v"(g), "{m0}"(m0) : "memory");
}
// Output stores; NT: non-temporal (streamed out, never re-read by this launch).
// Stores through address_space(1) pointers: the descriptor fields are generic
// pointers, and a flat_store also counts on lgkmcnt, so every LDS wait would
// drain the wave's outstanding stores.  global_store_* does not.
template <bool NT, typename V>
__device__ __forceinline__ void st(V* p, const V& v) {
    if constexpr (sizeof(V) == 16) {
        const f32x4 w = {v.x, v.y, v.z, v.w};
        DFQ_GLOBAL f32x4* g = (DFQ_GLOBAL f32x4*)p;
        if constexpr (NT) __builtin_nontemporal_store(w, g);
        else *g = w;
    } else {
        DFQ_GLOBAL V* g = (DFQ_GLOBAL V*)p;
        if constexpr (NT) __builtin_nontemporal_store(v, g);
        else *g = v;
    }
}
__device__ __forceinline__ void store_code(void* codes, int cb, int64_t idx, float q) {
    if (cb == 1) {
        st<false>(static_cast<int8_t*>(codes) + idx, (int8_t)(int)q);  // same bits as uint8 for 0..255
    } else {
        st<false>(static_cast<int16_t*>(codes) + idx, (int16_t)(int)q);
    }
}
__device__ __forceinline__ float ld(const float* p) { return *(const DFQ_GLOBAL float*)p; }
__device__ __forceinline__ float4 ld(const float4* p) {
    const f32x4 v = *(const DFQ_GLOBAL f32x4*)p;
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void vm_wait_all() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// ---------------------------------------------------------------------------
// Reduce launch: per-slot (min,max) of pieces via ordered-uint atomics.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlockThreads)
sweep_reduce_kernel(const DevTensor* __restrict__ tensors, const DevTask* __restrict__ tasks,
                    int64_t ntasks, uint32_t* __restrict__ slot_min, uint32_t* __restrict__ slot_max) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t wave0 = (int64_t)blockIdx.x * kWavesPerBlock + wave_uniform(threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock;
    for (int64_t t = wave0; t < ntasks; t += nwaves) {
        const DevTask task = tasks[t];
        const float* src = task.src;
        float vmin = INFINITY, vmax = -INFINITY;
        if (task.flags & 2) {
            const int nj = task.n >> 2;
#pragma unroll 8
            for (int j = lane; j < nj; j += kWave) {
                const float4 v = ld(reinterpret_cast<const float4*>(src) + j);
                vmin = fminf(vmin, fminf(fminf(v.x, v.y), fminf(v.z, v.w)));
                vmax = fmaxf(vmax, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
            }
        } else {
#pragma unroll 8
            for (int e = lane; e < task.n; e += kWave) {
                const float x = ld(src + e);
                vmin = fminf(vmin, x);
                vmax = fmaxf(vmax, x);
            }
        }
        vmin = wave_min(vmin);
        vmax = wave_max(vmax);
        if (lane == 0) {
            atomicMin(&slot_min[task.slot], enc_ord(vmin));
            atomicMax(&slot_max[task.slot], enc_ord(vmax));
        }
    }
}

// ---------------------------------------------------------------------------
// Main launch: one wave task.
// ---------------------------------------------------------------------------
// Issue the task's HBM -> LDS DMA (all loads in flight; no wait).
template <bool NT = false, bool ASM = false>
__device__ __forceinline__ void issue_task_load(const DevTask& task, float* data, int lane) {
    const float* src = task.src;
    const int n = task.n;
    if (task.flags & 2) {
        const int nj = n >> 2;
        for (int m = 0; m * kWave < nj; ++m) {
            const int j = lane + m * kWave;
            if (j < nj) {
                if constexpr (ASM) glds16_asm<NT>(src + 4 * j, data + 4 * kWave * m);
                else glds16<NT>(src + 4 * j, data + 4 * kWave * m);
            }
        }
    } else {
        for (int m = 0; m * kWave < n; ++m) {
            const int e = lane + m * kWave;
            if (e < n) {
                if constexpr (ASM) glds4_asm<NT>(src + e, data + kWave * m);
                else glds4<NT>(src + e, data + kWave * m);
            }
        }
    }
}


// The VEC quantize loop with the task's output set fixed at compile time (clip,
// code format, error-sum form): straight-line per-float4 bodies without the
// generic loop's per-iteration flag branches.  Bit-identical with the generic loop
// (same IEEE operation sequence per element); what differs is how each step is
// issued on a wave64 SIMD, where every VALU op costs 4 cycles and this loop is the
// single-model sweep's VALU budget:
//  * fp32 pairs as packed ops (v_pk_add_f32 / v_pk_mul_f32: two lanes' worth per op);
//  * the element -> row map as one v_mul_hi_u32 by ceil(2^32 / row_len) (exact for
//    e < 2^16, row_len < 2^13), the row's 1/s read from LDS next to s and mn (no
//    per-float4 v_rcp);
//  * rint(t) as (t + 1.5*2^23) - 1.5*2^23 (t is clamped to [qmin, qmax], |t| < 2^22:
//    round-to-nearest-even at the integer ulp, the same value as rintf); the sum's
//    low mantissa bits are q's two's complement, so the codes are byte / half
//    selects (v_perm_b32) of it;
//  * the reciprocal screen as |t - rint(t)| >= 0.5 - qabs 2^-20 (qabs = the larger of
//    |qmin|, |qmax| >= |t|): a superset of the elements within |t| 2^-20 of a
//    rounding boundary, which are the only ones whose reciprocal quotient can round
//    differently from the IEEE divide; those take the divide.  band: the task's
//    screen_band -- +inf where a row's 1 / s is not a normal float, and then thr is
//    -inf and every element takes the divide.
//  * clamps as v_med3 (no operand canonicalisation: fminf / fmaxf on values the
//    compiler cannot prove canonical cost a v_max x, x each).
// CB: 0 no codes, 1 int8 / uint8, 2 int16, 3 packed int4.  EM: 0 no error sums,
// 1 E stored (KH*KW = 1), 2 eps back to LDS (KH*KW > 1).
typedef float f32x2 __attribute__((ext_vector_type(2)));
template <bool CLIP, int CB, int EM, bool NT>
__device__ __forceinline__ void quant_vec4(const DevTensor& T, int n, int64_t base, float* data, const float* ls,
                                           const float* lmn, const float* lrs, const QParams& pc, bool whole,
                                           int eoff, int lane, float qmin, float qmax, bool sym, float band) {
    constexpr float kMagic = 12582912.0f;   // 1.5 * 2^23
    const int nj = n >> 2;
    float* dq = T.dst + base;
    const float clo = T.clip_lo, chi = T.clip_hi;
    // whole-row tasks: the element's row; pieces: their one parameter set, in slot 0
    const uint32_t magic = whole ? T.len_magic : 0u;
    const float thr = 0.5f - fmaxf(-qmin, qmax) * band;   // band = +inf (screen_band): every element takes the divide
    const f32x2 mg = {kMagic, kMagic};
    struct Q4 {   // one float4's state between the screen and the stores
        float4 x;
        float s, mn;
        float t[4];
        f32x2 ta, tb, qa, qb, da, db;
    };
    auto prep = [&](int j, uint32_t e, Q4& q) {
        q.x = reinterpret_cast<const float4*>(data)[j];
        const uint32_t r = __umulhi(e, magic);   // one row per float4 (4 | len, 4 | goff)
        q.s = ls[r];
        q.mn = lmn[r];
        const float rs = lrs[r];
        const f32x2 nm = {-q.mn, -q.mn};   // x + (-mn) (symmetric: x + -0.0, which is x)
        const f32x2 rs2 = {rs, rs};
        const f32x2 a = (f32x2{q.x.x, q.x.y} + nm) * rs2, b = (f32x2{q.x.z, q.x.w} + nm) * rs2;
        q.t[0] = __builtin_amdgcn_fmed3f(a.x, qmin, qmax);
        q.t[1] = __builtin_amdgcn_fmed3f(a.y, qmin, qmax);
        q.t[2] = __builtin_amdgcn_fmed3f(b.x, qmin, qmax);
        q.t[3] = __builtin_amdgcn_fmed3f(b.y, qmin, qmax);
        q.ta = f32x2{q.t[0], q.t[1]} + mg;
        q.tb = f32x2{q.t[2], q.t[3]} + mg;
        q.qa = q.ta - mg;
        q.qb = q.tb - mg;
        // opaque to the optimiser: merged with the rare path's values as they are,
        // not recomputed from t after the branch
        asm("" : "+v"(q.ta), "+v"(q.tb), "+v"(q.qa), "+v"(q.qb));
        q.da = f32x2{q.t[0], q.t[1]} - q.qa;
        q.db = f32x2{q.t[2], q.t[3]} - q.qb;
    };
    auto dmax = [&](const Q4& q) { return fmaxf(fmaxf(fabsf(q.da.x), fabsf(q.da.y)), fmaxf(fabsf(q.db.x), fabsf(q.db.y))); };
    auto fix = [&](Q4& q) {   // the IEEE divide for the screened elements
        const float negmn = -q.mn;
        if (fabsf(q.da.x) >= thr) q.t[0] = __builtin_amdgcn_fmed3f((q.x.x + negmn) / q.s, qmin, qmax);
        if (fabsf(q.da.y) >= thr) q.t[1] = __builtin_amdgcn_fmed3f((q.x.y + negmn) / q.s, qmin, qmax);
        if (fabsf(q.db.x) >= thr) q.t[2] = __builtin_amdgcn_fmed3f((q.x.z + negmn) / q.s, qmin, qmax);
        if (fabsf(q.db.y) >= thr) q.t[3] = __builtin_amdgcn_fmed3f((q.x.w + negmn) / q.s, qmin, qmax);
        q.ta = f32x2{q.t[0], q.t[1]} + mg;
        q.tb = f32x2{q.t[2], q.t[3]} + mg;
        q.qa = q.ta - mg;
        q.qb = q.tb - mg;
    };
    auto out = [&](int j, const Q4& q) {
        const f32x2 s2 = {q.s, q.s}, mn2 = {q.mn, q.mn};
        const f32x2 ya = q.qa * s2 + mn2, yb = q.qb * s2 + mn2;   // q * s, then + mn: two roundings (no contraction)
        float y[4] = {ya.x, ya.y, yb.x, yb.y};
        if constexpr (CLIP) {
#pragma unroll
            for (int k = 0; k < 4; ++k) y[k] = __builtin_amdgcn_fmed3f(y[k], clo, chi);
        }
        st<NT>(reinterpret_cast<float4*>(dq) + j, make_float4(y[0], y[1], y[2], y[3]));
        const uint32_t u0 = __float_as_uint(q.ta.x), u1 = __float_as_uint(q.ta.y);
        const uint32_t u2 = __float_as_uint(q.tb.x), u3 = __float_as_uint(q.tb.y);
        if constexpr (CB == 1) {   // bytes 0 of u0..u3
            const uint32_t c = __builtin_amdgcn_perm(u1, u0, 0x0c0c0400u) | __builtin_amdgcn_perm(u3, u2, 0x04000c0cu);
            st<NT>(reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(T.codes) + base) + j, c);
        } else if constexpr (CB == 3) {   // DFQ_PACK_INT4: 4 codes -> 2 bytes (base % 4 == 0)
            const uint32_t c = (u0 & 0xFu) | ((u1 & 0xFu) << 4) | ((u2 & 0xFu) << 8) | ((u3 & 0xFu) << 12);
            st<NT>(reinterpret_cast<uint16_t*>(static_cast<uint8_t*>(T.codes) + base / 2) + j, (uint16_t)c);
        } else if constexpr (CB == 2) {   // halves 0 of u0..u3
            const uint64_t c = (uint64_t)__builtin_amdgcn_perm(u1, u0, 0x05040100u) |
                               ((uint64_t)__builtin_amdgcn_perm(u3, u2, 0x05040100u) << 32);
            st<NT>(reinterpret_cast<uint64_t*>(static_cast<uint16_t*>(T.codes) + base) + j, c);
        }
        if constexpr (EM != 0) {
            const f32x2 ea = f32x2{y[0], y[1]} - f32x2{q.x.x, q.x.y}, eb = f32x2{y[2], y[3]} - f32x2{q.x.z, q.x.w};
            const float4 ev = make_float4(ea.x, ea.y, eb.x, eb.y);
            if constexpr (EM == 1) st<NT>(reinterpret_cast<float4*>(T.esum + base) + j, ev);
            else reinterpret_cast<float4*>(data)[j] = ev;
        }
    };
    // two independent float4s per lane and step (one dependent chain per float4 is
    // too little work between LDS round trips at 2-3 waves per SIMD); the second
    // one past the task's end recomputes the first and stores nothing
    uint32_t e = (uint32_t)(4 * lane + eoff);
    for (int j = lane; j < nj; j += 2 * kWave, e += 8 * kWave) {
        const int j1 = j + kWave;
        const bool has1 = j1 < nj;
        Q4 qa, qb;
        prep(j, e, qa);
        prep(has1 ? j1 : j, has1 ? e + 4 * kWave : e, qb);
        if (__builtin_amdgcn_ballot_w64(fmaxf(dmax(qa), dmax(qb)) >= thr)) {   // wave-uniform, rare
            fix(qa);
            fix(qb);
        }
        out(j, qa);
        if (has1) out(j1, qb);
    }
}

template <bool CLIP, int CB, bool NT>
__device__ __forceinline__ void quant_vec4_e(int em, const DevTensor& T, int n, int64_t base, float* data,
                                             const float* ls, const float* lmn, const float* lrs, const QParams& pc,
                                             bool whole, int eoff, int lane, float qmin, float qmax, bool sym, float band) {
    if (em == 0) quant_vec4<CLIP, CB, 0, NT>(T, n, base, data, ls, lmn, lrs, pc, whole, eoff, lane, qmin, qmax, sym, band);
    else if (em == 1) quant_vec4<CLIP, CB, 1, NT>(T, n, base, data, ls, lmn, lrs, pc, whole, eoff, lane, qmin, qmax, sym, band);
    else quant_vec4<CLIP, CB, 2, NT>(T, n, base, data, ls, lmn, lrs, pc, whole, eoff, lane, qmin, qmax, sym, band);
}

template <bool CLIP, bool NT>
__device__ __forceinline__ void quant_vec4_c(int cb, int em, const DevTensor& T, int n, int64_t base, float* data,
                                             const float* ls, const float* lmn, const float* lrs, const QParams& pc,
                                             bool whole, int eoff, int lane, float qmin, float qmax, bool sym, float band) {
    switch (cb) {
        case 0: quant_vec4_e<CLIP, 0, NT>(em, T, n, base, data, ls, lmn, lrs, pc, whole, eoff, lane, qmin, qmax, sym, band); break;
        case 1: quant_vec4_e<CLIP, 1, NT>(em, T, n, base, data, ls, lmn, lrs, pc, whole, eoff, lane, qmin, qmax, sym, band); break;
        case 2: quant_vec4_e<CLIP, 2, NT>(em, T, n, base, data, ls, lmn, lrs, pc, whole, eoff, lane, qmin, qmax, sym, band); break;
        default: quant_vec4_e<CLIP, 3, NT>(em, T, n, base, data, ls, lmn, lrs, pc, whole, eoff, lane, qmin, qmax, sym, band);
    }
}

// Step 4, the KH*KW error sums of a task whose eps are in ``data``: E[p] = sum_k
// eps[p*khw + k] in ATen's order (torch.sum(eps.view(O, I, -1), -1)).  ESPEC: the
// kernel sizes that get a compile-time length, so the ATen cascade unrolls into
// straight adds -- 2: 3x3 / 7x7 / 5x5 / 2x2, 1: 3x3, 0: none.
template <int ESPEC>
__device__ __forceinline__ void khw_error_sums(const DevTensor& T, const float* data, int n, int64_t base, int lane) {
    const int khw = T.khw;
    const int np = n / khw;
    const int64_t pbase = base / khw;
    auto esums = [&](auto kconst) {
        constexpr int K = decltype(kconst)::value;
        for (int pi = lane; pi < np; pi += kWave) {
            const float* e = data + pi * K;
            st<false>(T.esum + pbase + pi, aten_inner_sum([&](int64_t k) { return e[k]; }, (int64_t)K));
        }
    };
    auto generic = [&]() {
        for (int pi = lane; pi < np; pi += kWave) {
            const float* e = data + pi * khw;
            st<false>(T.esum + pbase + pi, aten_inner_sum([&](int64_t k) { return e[k]; }, khw));
        }
    };
    if constexpr (ESPEC == 2) {
        switch (khw) {
            case 9: esums(std::integral_constant<int, 9>{}); break;     // 3x3
            case 49: esums(std::integral_constant<int, 49>{}); break;   // 7x7
            case 25: esums(std::integral_constant<int, 25>{}); break;   // 5x5
            case 4: esums(std::integral_constant<int, 4>{}); break;     // 2x2
            default: generic();
        }
    } else if constexpr (ESPEC == 1) {
        if (khw == 9) esums(std::integral_constant<int, 9>{});
        else generic();
    } else {
        generic();
    }
}

// Steps 2-4 on a chunk that has landed in ``data``.
// ESPEC: khw_error_sums' compile-time lengths.
// goff >= 0: a row-group piece whose per-row parameters are already in ls / lmn
// (local row 0 = the row holding the piece's first element, goff = that element's
// offset inside it).
// SCREEN: the screened reciprocal quantize (qdq_screen, the IEEE divide only near a
// rounding boundary); false: the IEEE divide for every element (round-2 arithmetic,
// diagnostics variant 14).  Bit-identical results.
template <int MAXROWS, bool VEC, bool NT = false, int ESPEC = 2, bool SCREEN = true, bool FAST = true>
__device__ __forceinline__ void compute_task(const DevTensor& T, const DevTask& task, float* data, float* ls,
                                             float* lmn, const uint32_t* __restrict__ slot_min,
                                             const uint32_t* __restrict__ slot_max, int lane, float bmn = 0.f,
                                             float bmx = 0.f, int goff = -1, uint64_t* tlm = nullptr,
                                             uint32_t abl = 0, float gband = 0x1p-20f) {
    const int n = task.n;
    const bool sym = is_sym(T.mode);
    const int len = (int)T.row_len;

    // 2. per-row parameters (whole-row tasks) or the slot's parameters (pieces)
    QParams pc{};
    const bool group = goff >= 0;
    const bool whole = task.nrows > 0 || group;
    const int eoff = group ? goff : 0;
    float band = gband;   // the task's screen_band (wave-uniform)
    if (group) {
        // parameters set by the caller, gband with them
    } else if (whole) {
        // G lanes per row (G * next_pow2(nrows) = 64): every row of the task is
        // reduced at once; shuffles stay inside a G-lane group and every group
        // leader builds its row's parameters concurrently.
        const int nrows = task.nrows;
        int p2 = 1;
        while (p2 < nrows && p2 < kWave) p2 <<= 1;
        const int G = kWave / p2;
        const int sub = lane / G, sl = lane % G;
        bool wide = false;   // some row's band is not 2^-20
        for (int r0 = 0; r0 < nrows; r0 += p2) {
            const int r = r0 + sub;
            float vmin = INFINITY, vmax = -INFINITY;
            if (abl & 1) {   // diagnostics ablation: no row reduce
                vmin = -1.f;
                vmax = 1.f;
            } else if (r < nrows) {
                const float* row = data + r * len;
                if (VEC) {
                    // 4 LDS loads in flight per lane, then their min / max (a lane walks
                    // up to 16 float4s of its row; one round trip per 4 instead of per 1)
                    const int q4 = len >> 2;
                    const float4* row4 = reinterpret_cast<const float4*>(row);
                    for (int i = sl; i < q4; i += 4 * G) {
                        // past the row's end a lane re-reads the row's last float4 (min / max
                        // are idempotent): no per-load exec masks
                        float4 v[4];
#pragma unroll
                        for (int u = 0; u < 4; ++u) v[u] = row4[min(i + u * G, q4 - 1)];
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            vmin = min3_nc(min3_nc(vmin, v[u].x, v[u].y), v[u].z, v[u].w);
                            vmax = max3_nc(max3_nc(vmax, v[u].x, v[u].y), v[u].z, v[u].w);
                        }
                    }
                } else {
                    for (int i = sl; i < len; i += G) {
                        const float v = row[i];
                        vmin = fminf(vmin, v);
                        vmax = fmaxf(vmax, v);
                    }
                }
            }
            group_minmax(vmin, vmax, G);   // DPP inside 16-lane rows (no LDS round trips)
            if (tlm && r0 == 0) tlm[2] = wall_clock64();   // diagnostics: the first rows' ranges reduced
            if (sl == 0 && r < nrows) {
                const QParams p = make_qparams(vmin, vmax, T.bits, sym, T.flags, T.given_min, T.given_max);
                ls[r] = p.s;
                lmn[r] = p.mn;
                float b;
                lmn[MAXROWS + r] = screen_rcp(p.s, b);   // the quantize loop's 1/s
                wide |= b > 1.f;
                const int64_t row_g = task.row0 + r;
                if (T.scale) st<false>(T.scale + row_g, p.s);
                if (T.zero) st<false>(T.zero + row_g, p.mn);
            }
            if (tlm && r0 == 0) tlm[3] = wall_clock64();   // diagnostics: their parameters built
        }
        band = screen_band(wide);
        wave_lds_sync();
    } else {
        float mn = bmn, mx = bmx;   // block-row piece: the workgroup's combined range
        if (task.slot >= 0) {
            mn = dec_ord(slot_min[task.slot]);
            mx = dec_ord(slot_max[task.slot]);
        } else if (T.flags & DFQ_DEVICE_RANGE) {
            mn = dec_ord(~T.range_enc[0]);
            mx = dec_ord(T.range_enc[1]);
        }
        pc = make_qparams(mn, mx, T.bits, sym, T.flags, T.given_min, T.given_max);
        if ((task.flags & 1) && lane == 0) {
            const int64_t row_g = (T.mode == DFQ_CHANNEL_ASYM || T.mode == DFQ_CHANNEL_SYM) ? task.row0 : 0;
            if (T.scale) st<false>(T.scale + row_g, pc.s);
            if (T.zero) st<false>(T.zero + row_g, pc.mn);
        }
        const float prs = screen_rcp(pc.s, band);   // wave-uniform
        if (VEC && lane == 0) {   // the fixed-form quantize loop reads parameters from slot 0
            ls[0] = pc.s;
            lmn[0] = pc.mn;
            lmn[MAXROWS] = prs;
        }
        if (VEC) wave_lds_sync();
    }

    if (tlm) tlm[0] = wall_clock64();   // diagnostics timeline (variant 13): parameters done
    // 3. quantize / dequantize / clip from LDS; write dq + codes; eps for bias correction.
    //    eps overwrites the x it came from (same lane, same slot), so no hazard.
    const bool clip = (T.flags & DFQ_CLIP) != 0;
    const bool want_e = T.esum != nullptr;
    const int khw = T.khw;
    const float qmin = sym ? -(float)(1 << (T.bits - 1)) : 0.f;
    const float qmax = sym ? (float)((1 << (T.bits - 1)) - 1) : (float)((1 << T.bits) - 1);
    const int64_t base = task_elem_start(task, T);

    auto params_for = [&](int e) -> QParams {
        if (!whole) return pc;
        // row = floor(e / len): (e + 0.5)/len is >= 0.5/len from an integer and
        // e < 2048, so this fp32 estimate is exact.
        int r = (int)(((float)(e + eoff) + 0.5f) * T.inv_len);
        r = min(r, MAXROWS - 1);
        QParams p;
        p.s = ls[r];
        p.mn = lmn[r];
        p.negmn = -p.mn;
        p.qmin = qmin;
        p.qmax = qmax;
        return p;
    };
    auto one = [&](float xv, const QParams& p, float& qv) -> float {
        if constexpr (!SCREEN) {
            float yv = qdq(xv, p, qv);
            if (clip) yv = fminf(fmaxf(yv, T.clip_lo), T.clip_hi);
            return yv;
        }
        bool need;
        float t = qdq_screen(xv, p, screen_rs(p.s), band, need);
        if (__builtin_amdgcn_ballot_w64(need)) {   // wave-uniform, rare
            if (need) t = qdq_exact_t(xv, p);
        }
        float yv = qdq_finish(t, p, qv);
        if (clip) yv = fminf(fmaxf(yv, T.clip_lo), T.clip_hi);
        return yv;
    };
    // four elements sharing one row's parameters: one reciprocal, one ballot
    auto four = [&](const float4& xv, const QParams& p, float& q0, float& q1, float& q2, float& q3) -> float4 {
        if constexpr (!SCREEN) return make_float4(one(xv.x, p, q0), one(xv.y, p, q1), one(xv.z, p, q2), one(xv.w, p, q3));
        const float rs = screen_rs(p.s);
        bool n0, n1, n2, n3;
        float t0 = qdq_screen(xv.x, p, rs, band, n0), t1 = qdq_screen(xv.y, p, rs, band, n1);
        float t2 = qdq_screen(xv.z, p, rs, band, n2), t3 = qdq_screen(xv.w, p, rs, band, n3);
        if (__builtin_amdgcn_ballot_w64(n0 | n1 | n2 | n3)) {   // wave-uniform, rare
            if (n0) t0 = qdq_exact_t(xv.x, p);
            if (n1) t1 = qdq_exact_t(xv.y, p);
            if (n2) t2 = qdq_exact_t(xv.z, p);
            if (n3) t3 = qdq_exact_t(xv.w, p);
        }
        float4 y = make_float4(qdq_finish(t0, p, q0), qdq_finish(t1, p, q1), qdq_finish(t2, p, q2),
                               qdq_finish(t3, p, q3));
        if (clip) {
            y.x = fminf(fmaxf(y.x, T.clip_lo), T.clip_hi);
            y.y = fminf(fmaxf(y.y, T.clip_lo), T.clip_hi);
            y.z = fminf(fmaxf(y.z, T.clip_lo), T.clip_hi);
            y.w = fminf(fmaxf(y.w, T.clip_lo), T.clip_hi);
        }
        return y;
    };

    // the generic VEC loop: every output flag tested per float4
    auto vec_generic = [&]() {
        const int nj = n >> 2;
#pragma unroll 2
        for (int j = lane; j < nj; j += kWave) {
            const float4 xv = reinterpret_cast<const float4*>(data)[j];
            const QParams p = params_for(4 * j);   // 4 | len, 4 | goff: one row per float4
            float q0, q1, q2, q3;
            const float4 yq = four(xv, p, q0, q1, q2, q3);
            const float y0 = yq.x, y1 = yq.y, y2 = yq.z, y3 = yq.w;
            if (T.dst) st<NT>(reinterpret_cast<float4*>(T.dst + base) + j, make_float4(y0, y1, y2, y3));
            if (T.codes) {
                if (T.code_bytes == 1) {
                    const uint32_t c = ((uint32_t)(uint8_t)(int)q0) | ((uint32_t)(uint8_t)(int)q1 << 8) |
                                       ((uint32_t)(uint8_t)(int)q2 << 16) | ((uint32_t)(uint8_t)(int)q3 << 24);
                    st<NT>(reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(T.codes) + base) + j, c);
                } else if (T.code_bytes == 0) {   // DFQ_PACK_INT4: 4 codes -> 2 bytes (base % 4 == 0)
                    const uint32_t c = ((uint32_t)(int)q0 & 0xFu) | (((uint32_t)(int)q1 & 0xFu) << 4) |
                                       (((uint32_t)(int)q2 & 0xFu) << 8) | (((uint32_t)(int)q3 & 0xFu) << 12);
                    st<NT>(reinterpret_cast<uint16_t*>(static_cast<uint8_t*>(T.codes) + base / 2) + j, (uint16_t)c);
                } else {
                    const uint64_t c = ((uint64_t)(uint16_t)(int)q0) | ((uint64_t)(uint16_t)(int)q1 << 16) |
                                       ((uint64_t)(uint16_t)(int)q2 << 32) | ((uint64_t)(uint16_t)(int)q3 << 48);
                    st<NT>(reinterpret_cast<uint64_t*>(static_cast<uint16_t*>(T.codes) + base) + j, c);
                }
            }
            if (want_e) {
                const float4 ev = make_float4(y0 - xv.x, y1 - xv.y, y2 - xv.z, y3 - xv.w);
                if (khw == 1) st<NT>(reinterpret_cast<float4*>(T.esum + base) + j, ev);
                else reinterpret_cast<float4*>(data)[j] = ev;
            }
        }
    };
    if (abl & 6) {   // diagnostics ablation: 2 = stores without the arithmetic, 4 = no quantize loop
        if ((abl & 64) && VEC) {   // 64 (with 4): the arithmetic without the stores
            const int nj = n >> 2;
            float acc = 0.f;
            for (int j = lane; j < nj; j += kWave) {
                const float4 xv = reinterpret_cast<const float4*>(data)[j];
                float q0, q1, q2, q3;
                const float4 y = four(xv, params_for(4 * j), q0, q1, q2, q3);
                acc += (y.x + y.y) + (y.z + y.w) + (q0 + q1) + (q2 + q3);
            }
            if (acc == 1234.5678f) st<false>(T.dst + base, acc);   // keeps the work
        } else if (!(abl & 4) && VEC) {
            const int nj = n >> 2;
            for (int j = lane; j < nj; j += kWave) {
                const float4 xv = reinterpret_cast<const float4*>(data)[j];
                st<NT>(reinterpret_cast<float4*>(T.dst + base) + j, xv);
                if (T.codes) st<NT>(reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(T.codes) + base) + j, __float_as_uint(xv.x));
            }
        } else if (!(abl & 4)) {
            for (int e = lane; e < n; e += kWave) {
                st<false>(T.dst + base + e, data[e]);
                if (T.codes) st<false>(static_cast<uint8_t*>(T.codes) + base + e, (uint8_t)__float_as_uint(data[e]));
            }
        }
    } else if constexpr (VEC) {
        bool done = false;
        if constexpr (SCREEN && FAST && MAXROWS == 64) {
            const float* lrs = lmn + MAXROWS;
            if (T.dst && (!clip || T.clip_lo <= T.clip_hi)) {   // one compile-time body per (clip, codes, E form)
                const int cb = !T.codes ? 0 : (T.code_bytes == 1 ? 1 : (T.code_bytes == 0 ? 3 : 2));
                const int em = !want_e ? 0 : (khw == 1 ? 1 : 2);
                if (clip) quant_vec4_c<true, NT>(cb, em, T, n, base, data, ls, lmn, lrs, pc, whole, eoff, lane, qmin, qmax, sym, band);
                else quant_vec4_c<false, NT>(cb, em, T, n, base, data, ls, lmn, lrs, pc, whole, eoff, lane, qmin, qmax, sym, band);
                done = true;
            }
        }
        if (!done) vec_generic();
    } else if (T.codes && T.code_bytes == 0) {
        // packed nibbles on the scalar path: the task starts at an even element
        // (build()), so even lanes own a byte and take the odd neighbour's code by
        // a shuffle; every lane runs every step so the shuffle sees defined values
        for (int e0 = 0; e0 < n; e0 += kWave) {
            const int e = e0 + lane;
            const bool ok = e < n;
            uint32_t qi = 0;
            if (ok) {
                const float xv = data[e];
                float qv;
                const float yv = one(xv, params_for(e), qv);
                if (T.dst) st<false>(T.dst + base + e, yv);
                qi = (uint32_t)(int)qv & 0xFu;
                if (want_e) {
                    if (khw == 1) st<false>(T.esum + base + e, yv - xv);
                    else data[e] = yv - xv;
                }
            }
            const uint32_t hi = (uint32_t)__shfl_down((int)qi, 1, kWave);
            if (ok && (e & 1) == 0)
                st<false>(static_cast<uint8_t*>(T.codes) + (base + e) / 2, (uint8_t)(qi | (hi << 4)));
        }
    } else {
#pragma unroll 4
        for (int e = lane; e < n; e += kWave) {
            const float xv = data[e];
            float qv;
            const float yv = one(xv, params_for(e), qv);
            if (T.dst) st<false>(T.dst + base + e, yv);
            if (T.codes) store_code(T.codes, T.code_bytes, base + e, qv);
            if (want_e) {
                if (khw == 1) st<false>(T.esum + base + e, yv - xv);
                else data[e] = yv - xv;
            }
        }
    }

    if (tlm) tlm[1] = wall_clock64();   // quantize loop issued
    // 4. KH*KW error sums
    if (want_e && khw > 1) {
        wave_lds_sync();
        khw_error_sums<ESPEC>(T, data, n, base, lane);
    }
    wave_lds_sync();  // LDS is reused by this wave's next task
}

// s_waitcnt vmcnt(n) for a wave-uniform runtime n (the count is an immediate):
// every value 0..8, larger ones round down to 8 (waiting longer is always safe).
__device__ __forceinline__ void vm_wait_le(int n) {
    switch (n < 0 ? 0 : (n > 8 ? 8 : n)) {
        case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
        case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
        case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
        case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
        case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
        case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
        case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
        case 7: asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); break;
        default: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
    }
}

// A whole-row task in two row batches (the single-model latency lever of DESIGN.md
// 3.1): the wave waits only for the load instructions that cover rows [0, h),
// reduces their ranges, builds their parameters and quantizes and STORES them
// while the loads of rows [h, nrows) are still landing; then it waits for those
// (vmcnt counts loads, LDS-DMA and stores together in issue order,
// MI355X_MICROARCH.md: at most lb younger operations outstanding means every load
// of the task has landed, for any lb <= the stores issued since) and does the
// rest.  The same per-row arithmetic and stores as compute_task's fixed-form loop
// (bit-identical); the KH*KW error sums run over the whole task at the end.
// Returns false (nothing done, loads still in flight) when the task does not split:
// the caller takes the one-wait path.
template <int MAXROWS, bool NT, int ESPEC>
__device__ __forceinline__ bool compute_task_split(const DevTensor& T, const DevTask& task, float* data, float* ls,
                                                   float* lmn, int lane) {
    const int n = task.n, nrows = task.nrows, len = (int)T.row_len;
    const bool clip = (T.flags & DFQ_CLIP) != 0;
    if (MAXROWS != 64 || nrows < 2 || !T.vec4 || !T.dst || (clip && !(T.clip_lo <= T.clip_hi))) return false;
    const int nj = n >> 2;
    const int M = (nj + kWave - 1) / kWave;   // load instructions issued (issue_task_load: 1 KiB each)
    const int h = min(nrows - 1, ((M >> 1) * 4 * kWave) / len);   // rows inside the first half of the loads
    if (M < 2 || h < 1) return false;
    const int m1 = (h * len + 4 * kWave - 1) / (4 * kWave);   // load instructions covering rows [0, h)
    const bool sym = is_sym(T.mode);
    const int khw = T.khw;
    const bool want_e = T.esum != nullptr;
    const float qmin = sym ? -(float)(1 << (T.bits - 1)) : 0.f;
    const float qmax = sym ? (float)((1 << (T.bits - 1)) - 1) : (float)((1 << T.bits) - 1);
    const int64_t base = task_elem_start(task, T);
    const int cb = !T.codes ? 0 : (T.code_bytes == 1 ? 1 : (T.code_bytes == 0 ? 3 : 2));
    const int em = !want_e ? 0 : (khw == 1 ? 1 : 2);
    const float* lrs = lmn + MAXROWS;
    const QParams pc{};
    auto rows = [&](int ra, int rb) {
        // ranges and parameters of rows [ra, rb) (compute_task's whole-row reduce)
        const int nr = rb - ra;
        int p2 = 1;
        while (p2 < nr && p2 < kWave) p2 <<= 1;
        const int G = kWave / p2;
        const int sub = lane / G, sl = lane % G;
        bool wide = false;   // some row's band is not 2^-20
        for (int r0 = ra; r0 < rb; r0 += p2) {
            const int r = r0 + sub;
            float vmin = INFINITY, vmax = -INFINITY;
            if (r < rb) {
                const int q4 = len >> 2;
                const float4* row4 = reinterpret_cast<const float4*>(data + r * len);
                for (int i = sl; i < q4; i += 4 * G) {
                    float4 v[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) v[u] = row4[min(i + u * G, q4 - 1)];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        vmin = min3_nc(min3_nc(vmin, v[u].x, v[u].y), v[u].z, v[u].w);
                        vmax = max3_nc(max3_nc(vmax, v[u].x, v[u].y), v[u].z, v[u].w);
                    }
                }
            }
            group_minmax(vmin, vmax, G);
            if (sl == 0 && r < rb) {
                const QParams p = make_qparams(vmin, vmax, T.bits, sym, T.flags, T.given_min, T.given_max);
                ls[r] = p.s;
                lmn[r] = p.mn;
                float b;
                lmn[MAXROWS + r] = screen_rcp(p.s, b);
                wide |= b > 1.f;
                const int64_t row_g = task.row0 + r;
                if (T.scale) st<false>(T.scale + row_g, p.s);
                if (T.zero) st<false>(T.zero + row_g, p.mn);
            }
        }
        const float band = screen_band(wide);
        wave_lds_sync();
        // quantize rows [ra, rb): the fixed-form loop on that element span
        const int e0 = ra * len, ne = (rb - ra) * len;
        if (clip) quant_vec4_c<true, NT>(cb, em, T, ne, base + e0, data + e0, ls, lmn, lrs, pc, true, e0, lane, qmin,
                                         qmax, sym, band);
        else quant_vec4_c<false, NT>(cb, em, T, ne, base + e0, data + e0, ls, lmn, lrs, pc, true, e0, lane, qmin, qmax,
                                     sym, band);
    };
    vm_wait_le(M - m1);   // rows [0, h) have landed
    wave_lds_sync();
    rows(0, h);
    // the loop above issued >= one store per iteration of ceil(h len / 4 / 128)
    vm_wait_le(((h * len >> 2) + 2 * kWave - 1) / (2 * kWave));   // every load of the task has landed
    wave_lds_sync();
    rows(h, nrows);
    if (want_e && khw > 1) {   // the KH*KW error sums run over the whole task
        wave_lds_sync();
        khw_error_sums<ESPEC>(T, data, n, base, lane);
    }
    wave_lds_sync();   // LDS is reused by this wave's next task
    return true;
}

// Diagnostics timeline (variant 13): per main-list task {start, data landed, done}
// in s_memrealtime ticks (100 MHz) plus the executing wave's hardware ids.
__device__ uint64_t* g_timeline = nullptr;
__device__ int64_t g_timeline_cap = 0;
// Diagnostics ablations (variant 13 only; dfq_debug_ablate): 1 no row reduce, 2 stores
// without the quantize arithmetic, 4 no quantize loop, 8 no input loads, 16 return at
// once (the launch alone), 32 task / tensor records and loads only (no compute),
// 64|4 the quantize arithmetic without its stores.
__device__ uint32_t g_ablate = 0;

template <int CHUNK, int MAXROWS, bool PREFETCH, bool NT = false, int ESPEC = 2, bool TL = false, bool SCREEN = true,
          bool FAST = true, bool SPLIT = false>
__global__ void __launch_bounds__(kBlockThreads)
sweep_main_kernel(const DevTensor* __restrict__ tensors, const DevTask* __restrict__ tasks, int64_t ntasks,
                  const uint32_t* __restrict__ slot_min, const uint32_t* __restrict__ slot_max) {
    constexpr int NB = PREFETCH ? 2 : 1;
    using Lay = LdsLayout<CHUNK, MAXROWS, NB>;
    __shared__ __attribute__((aligned(16))) float lds[Lay::kTotal];
    const int lane = threadIdx.x & (kWave - 1);
    const int w = wave_uniform(threadIdx.x >> 6);
    float* wl = lds + w * Lay::kPerWave;
    float* ls = wl + NB * CHUNK;
    float* lmn = ls + MAXROWS;
    const int64_t wave0 = (int64_t)blockIdx.x * kWavesPerBlock + w;
    const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock;
    if constexpr (TL) {
        if (g_ablate & 16) return;   // diagnostics ablation: the launch alone
    }
    if constexpr (!PREFETCH) {
        DevTask task;
        if (wave0 < ntasks) task = tasks[wave0];
        for (int64_t t = wave0; t < ntasks; t += nwaves) {
            uint64_t tl0 = 0, tl1 = 0;
            uint32_t abl = 0;
            if constexpr (TL) {
                tl0 = wall_clock64();
                abl = g_ablate;
            }
            if (!(abl & 8)) issue_task_load<NT, SPLIT>(task, wl, lane);   // needs only the task record
            const DevTensor T = tensors[task.tensor];
            DevTask next = task;   // next record's scalar load overlaps this task
            if (t + nwaves < ntasks) next = tasks[t + nwaves];
            if constexpr (SPLIT && SCREEN && FAST && !TL) {
                // whole-row tasks in two row batches, the first stored while the
                // second's loads land (compute_task_split)
                if (task.nrows > 0 && compute_task_split<MAXROWS, NT, ESPEC>(T, task, wl, ls, lmn, lane)) {
                    task = next;
                    continue;
                }
            }
            vm_wait_all();
            if constexpr (TL) tl1 = wall_clock64();
            wave_lds_sync();
            if constexpr (TL) {
                if (abl & 32) {   // diagnostics ablation: task and tensor records (and loads) only
                    if (lane == 0 && T.row_len == -7) g_timeline[0] = 0;   // keeps T's load
                    task = next;
                    continue;
                }
            }
            float bmn = 0.f, bmx = 0.f, gband = 0x1p-20f;
            int goff = -1;
            if (task.nrows <= kGroupTag) {
                // row-group piece: the 4 waves of this block hold 4 pieces of R complete
                // rows.  Per-row partial (min, max) of this piece's row segments into
                // this wave's ls (max) / lmn (min) slots, one barrier, each wave combines
                // the rows its piece touches, a second barrier, then its row parameters.
                const int R = kGroupTag - task.nrows + 1;
                const int len = (int)T.row_len;
                const int g0 = (int)(task_elem_start(task, T) - (int64_t)task.row0 * len);   // piece offset in the group
                const int rf = g0 / len;
                const int rl = task.n > 0 ? (g0 + task.n - 1) / len : rf - 1;
                for (int r = 0; r < R; ++r) {
                    float vmin = INFINITY, vmax = -INFINITY;
                    if (r >= rf && r <= rl) {
                        const int a = max(r * len, g0) - g0, b = min((r + 1) * len, g0 + task.n) - g0;
                        if (T.vec4) {
                            for (int j = (a >> 2) + lane; j < (b >> 2); j += kWave) {
                                const float4 v = reinterpret_cast<const float4*>(wl)[j];
                                vmin = fminf(vmin, fminf(fminf(v.x, v.y), fminf(v.z, v.w)));
                                vmax = fmaxf(vmax, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
                            }
                        } else {
                            for (int e = a + lane; e < b; e += kWave) {
                                vmin = fminf(vmin, wl[e]);
                                vmax = fmaxf(vmax, wl[e]);
                            }
                        }
                        vmin = wave_min(vmin);
                        vmax = wave_max(vmax);
                    }
                    if (lane == 0) {
                        lmn[r] = vmin;
                        ls[r] = vmax;
                    }
                }
                block_lds_sync();
                constexpr int P = Lay::kPerWave;
                const int rr = rf + lane;   // one lane per row this piece touches
                float gmn = INFINITY, gmx = -INFINITY;
                if (rr <= rl) {
                    const float* b0 = lds + NB * CHUNK;   // wave 0's ls; lmn = ls + MAXROWS
#pragma unroll
                    for (int q = 0; q < kWavesPerBlock; ++q) {
                        gmx = fmaxf(gmx, b0[q * P + rr]);
                        gmn = fminf(gmn, b0[q * P + MAXROWS + rr]);
                    }
                }
                block_lds_sync();   // every wave has read the partials
                bool wide = false;   // some row's band is not 2^-20
                if (rr <= rl) {
                    const QParams p = make_qparams(gmn, gmx, T.bits, is_sym(T.mode), T.flags, T.given_min,
                                                   T.given_max);
                    ls[lane] = p.s;
                    lmn[lane] = p.mn;
                    float b;
                    lmn[MAXROWS + lane] = screen_rcp(p.s, b);
                    wide = b > 1.f;
                    if (rr * len >= g0) {   // the row starts in this piece: its parameters are stored once
                        const int64_t row_g = task.row0 + rr;
                        if (T.scale) st<false>(T.scale + row_g, p.s);
                        if (T.zero) st<false>(T.zero + row_g, p.mn);
                    }
                }
                gband = screen_band(wide);
                wave_lds_sync();
                goff = g0 - rf * len;
            } else if (task.nrows < 0) {   // block-row piece: all 4 waves of this block are here
                float vmin = INFINITY, vmax = -INFINITY;
                if (T.vec4) {
                    for (int j = lane; j < (task.n >> 2); j += kWave) {
                        const float4 v = reinterpret_cast<const float4*>(wl)[j];
                        vmin = fminf(vmin, fminf(fminf(v.x, v.y), fminf(v.z, v.w)));
                        vmax = fmaxf(vmax, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
                    }
                } else {
                    for (int e = lane; e < task.n; e += kWave) {
                        vmin = fminf(vmin, wl[e]);
                        vmax = fmaxf(vmax, wl[e]);
                    }
                }
                vmin = wave_min(vmin);
                vmax = wave_max(vmax);
                // partial (min, max) in this wave's own row-parameter slots (unused by
                // block-row pieces), read by the block's other waves after the barrier
                if (lane == 0) {
                    ls[0] = vmin;
                    ls[1] = vmax;
                }
                block_lds_sync();
                constexpr int P = Lay::kPerWave;
                if (task.nrows == -kWavesPerBlock) {
                    const float* b0 = lds + NB * CHUNK;
                    bmn = fminf(fminf(b0[0], b0[P]), fminf(b0[2 * P], b0[3 * P]));
                    bmx = fmaxf(fmaxf(b0[1], b0[P + 1]), fmaxf(b0[2 * P + 1], b0[3 * P + 1]));
                } else {   // pairs of waves (0,1), (2,3)
                    const float* b0 = lds + (w & ~1) * P + NB * CHUNK;
                    bmn = fminf(b0[0], b0[P]);
                    bmx = fmaxf(b0[1], b0[P + 1]);
                }
                block_lds_sync();   // the slots are rewritten by the next task
            }
            uint64_t marks[4] = {0, 0, 0, 0};
            uint64_t* tlm = TL ? marks : nullptr;
            if (T.vec4)
                compute_task<MAXROWS, true, NT, ESPEC, SCREEN, FAST>(T, task, wl, ls, lmn, slot_min, slot_max, lane,
                                                                     bmn, bmx, goff, tlm, abl, gband);
            else
                compute_task<MAXROWS, false, NT, ESPEC, SCREEN, FAST>(T, task, wl, ls, lmn, slot_min, slot_max, lane,
                                                                      bmn, bmx, goff, tlm, abl, gband);
            if constexpr (TL) {
                if (lane == 0 && t < g_timeline_cap) {
                    uint32_t hw;
                    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
                    uint32_t xcc;
                    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
                    const uint64_t tl2 = wall_clock64();
                    uint64_t* r = g_timeline + 8 * t;   // {start, landed, params, quantized, done, tensor | xcc | hw ids, ...}
                    r[0] = tl0;
                    r[1] = tl1;
                    r[2] = marks[0];
                    r[3] = marks[1];
                    r[4] = tl2;
                    r[5] = ((uint64_t)task.tensor << 40) | ((uint64_t)(xcc & 0xFF) << 32) | hw;
                    r[6] = marks[2];
                    r[7] = marks[3];
                }
            }
            task = next;
        }
    } else {
        // Double-buffered: the next task's DMA is issued before this task computes.
        int cur = 0;
        int64_t t = wave0;
        if (t < ntasks) {
            const DevTask task = tasks[t];
            issue_task_load<NT>(task, wl, lane);
        }
        for (; t < ntasks; t += nwaves) {
            const DevTask task = tasks[t];
            const DevTensor T = tensors[task.tensor];
            vm_wait_all();          // this task's chunk (and the previous task's stores)
            wave_lds_sync();
            const int64_t tn = t + nwaves;
            if (tn < ntasks) {
                const DevTask nt = tasks[tn];
                issue_task_load<NT>(nt, wl + (cur ^ 1) * CHUNK, lane);
            }
            float* data = wl + cur * CHUNK;
            if (T.vec4) compute_task<MAXROWS, true, NT, ESPEC, SCREEN>(T, task, data, ls, lmn, slot_min, slot_max, lane);
            else compute_task<MAXROWS, false, NT, ESPEC, SCREEN>(T, task, data, ls, lmn, slot_min, slot_max, lane);
            cur ^= 1;
        }
    }
}

// ---------------------------------------------------------------------------
// Host: kernel selection, plans (the planner itself: dfq_sweep_plan.cpp).
// ---------------------------------------------------------------------------
using MainKernel = void (*)(const DevTensor*, const DevTask*, int64_t, const uint32_t*, const uint32_t*);

// Row I of kVariants as a kernel: the row is the whole truth about its variant.
template <int I>
static MainKernel variant_kernel() {
    constexpr Variant V = kVariants[I];
    return sweep_main_kernel<V.chunk, V.max_rows, V.prefetch, V.nt, V.espec, V.timeline, V.screen, V.fast, V.split>;
}
template <int... I>
static MainKernel variant_kernel(int variant, std::integer_sequence<int, I...>) {
    static const MainKernel table[] = {variant_kernel<I>()...};
    return table[variant >= 0 && variant < kNumVariants ? variant : 0];
}

static MainKernel main_kernel(int variant) {
#ifndef DFQ_DIAGNOSTICS
    // the product library carries the default variant and the small-list one
    return variant == kSmallVariant ? variant_kernel<kSmallVariant>() : variant_kernel<kDefaultVariant>();
#else
    return variant_kernel(variant, std::make_integer_sequence<int, kNumVariants>{});
#endif
}

// Grid: up to 64 blocks per CU (16384 blocks), far more than are resident (4-5
// per CU for the sweep kernels).  Each wave's grid-stride list is then only a
// few tasks long and the dispatcher hands CUs new blocks as old ones retire --
// dynamic load balance over tasks of uneven cost.  Measured against resident-
// only grids (profiles/r01/ab_grid.txt): MobileNetV2 +25 %, ResNet-50 / DeepLab
// +4-6 %; 32-128 per CU are within a few %, fully unrolled grids (one block per
// 4 tasks) lose 10 %.  DFQ_SWEEP_BLOCKS_PER_CU overrides (A/B).
constexpr int kBlocksPerCu = 64;
static int blocks_per_cu() {
    static const int v = [] {
        const char* e = ab_env("DFQ_SWEEP_BLOCKS_PER_CU");
        return e && *e ? std::max(1, std::min(1024, atoi(e))) : kBlocksPerCu;
    }();
    return v;
}
static int grid_for(int64_t ntasks) {
    const int64_t want = ceil_div(ntasks, kWavesPerBlock);
    return (int)std::max<int64_t>(1, std::min<int64_t>(want, 256 * (int64_t)blocks_per_cu()));
}

// One run of a table on `s`: the slots armed (mins all ones, maxs zero) and one
// reduce launch over every slot piece, if there are any, then one main launch.
static int launch_sweep(int variant, hipStream_t s, const DevTensor* t, const DevTask* reduce, int64_t n_reduce,
                        const DevTask* main, int64_t n_main, uint32_t* slots, int64_t n_slots) {
    if (n_reduce > 0) {
        DFQ_HIP_CHECK(hipMemsetAsync(slots, 0xFF, sizeof(uint32_t) * n_slots, s));
        DFQ_HIP_CHECK(hipMemsetAsync(slots + n_slots, 0x00, sizeof(uint32_t) * n_slots, s));
        hipLaunchKernelGGL(sweep_reduce_kernel, dim3(grid_for(n_reduce)), dim3(kBlockThreads), 0, s, t, reduce,
                           n_reduce, slots, slots + n_slots);
        DFQ_LAUNCH_CHECK();
    }
    if (n_main > 0) {
        hipLaunchKernelGGL(main_kernel(variant), dim3(grid_for(n_main)), dim3(kBlockThreads), 0, s, t, main, n_main,
                           slots, slots + n_slots);
        DFQ_LAUNCH_CHECK();
    }
    return DFQ_OK;
}

// The host-built tables [tensors .. main tasks] as one blob for a single upload:
// each part at its layout offset less the tensors' (the parts between stay zero).
static std::vector<char> table_blob(const SweepTables& T, size_t o_tensors, size_t o_reduce, size_t o_main,
                                    size_t end) {
    std::vector<char> blob(end - o_tensors, 0);
    auto put = [&](size_t off, const void* p, size_t bytes) {
        if (bytes) std::memcpy(blob.data() + (off - o_tensors), p, bytes);
    };
    put(o_tensors, T.tensors.data(), sizeof(DevTensor) * T.tensors.size());
    put(o_reduce, T.reduce.data(), sizeof(DevTask) * T.reduce.size());
    put(o_main, T.main.data(), sizeof(DevTask) * T.main.size());
    return blob;
}

}  // namespace dfq

using namespace dfq;

struct dfq_sweep_plan {
    int variant = kDefaultVariant;
    DevTensor* d_tensors = nullptr;
    DevTask* d_reduce = nullptr;
    DevTask* d_main = nullptr;
    uint32_t* d_slots = nullptr;   // [slots] mins then [slots] maxs
    void* d_owned = nullptr;       // the tables' allocation when no workspace was given
    int64_t n_reduce = 0, n_main = 0, n_slots = 0, n_tensors = 0, n_elems = 0, algo_bytes = 0;
};

// ws == NULL: the plan owns one hipMalloc'ed table block (blocking copy).  Else the
// tables go to the caller's stream-ordered workspace: one copy on `stream`, then a
// sync of that stream (the host staging dies with the call).
static int sweep_plan_create_impl(const dfq_tensor_desc* descs, int32_t n, void* ws, int64_t ws_bytes,
                                  hipStream_t stream, dfq_sweep_plan** out) {
    if (!out || (n > 0 && !descs) || n < 0) return DFQ_ERR_INVALID;
    *out = nullptr;
    SweepTables B;
    PlanLayout Lo;
    int rc = sweep_plan_tables(descs, n, B, Lo);
    if (rc) return rc;
    if (ws && (ws_bytes < Lo.total || reinterpret_cast<uintptr_t>(ws) % 256 != 0)) return DFQ_ERR_WORKSPACE;
    dfq_sweep_plan* p = new (std::nothrow) dfq_sweep_plan();
    if (!p) return DFQ_ERR_NOMEM;
    p->variant = B.variant;
    p->n_reduce = (int64_t)B.reduce.size();
    p->n_main = (int64_t)B.main.size();
    p->n_slots = B.slots;
    p->n_tensors = n;
    p->n_elems = B.elems;
    p->algo_bytes = B.algo_bytes;
    hipError_t e = hipSuccess;
    char* base = static_cast<char*>(ws);
    if (!base) {
        e = hipMalloc(&p->d_owned, Lo.total);
        base = static_cast<char*>(p->d_owned);
    }
    p->d_tensors = reinterpret_cast<DevTensor*>(base + Lo.o_tensors);
    p->d_reduce = reinterpret_cast<DevTask*>(base + Lo.o_reduce);
    p->d_main = reinterpret_cast<DevTask*>(base + Lo.o_main);
    p->d_slots = reinterpret_cast<uint32_t*>(base + Lo.o_slots);
    if (e == hipSuccess) {
        const std::vector<char> blob = table_blob(B, Lo.o_tensors, Lo.o_reduce, Lo.o_main, Lo.o_slots);
        if (ws) {   // stream-ordered: pinned staging, no host synchronisation
            e = stage_h2d(base, blob.data(), Lo.o_slots, stream);
        } else {
            e = hipMemcpy(base, blob.data(), Lo.o_slots, hipMemcpyHostToDevice);
        }
    }
    if (e != hipSuccess) {
        set_last_hip_error(e);
        (void)hipFree(p->d_owned);
        delete p;
        return DFQ_ERR_HIP;
    }
    *out = p;
    return DFQ_OK;
}

extern "C" int dfq_sweep_plan_create(const dfq_tensor_desc* descs, int32_t n, dfq_sweep_plan** out) {
    return sweep_plan_create_impl(descs, n, nullptr, 0, nullptr, out);
}

extern "C" int dfq_sweep_plan_create_ws(const dfq_tensor_desc* descs, int32_t n, void* ws, int64_t ws_bytes,
                                        void* stream, dfq_sweep_plan** out) {
    if (!ws) return DFQ_ERR_WORKSPACE;
    return sweep_plan_create_impl(descs, n, ws, ws_bytes, static_cast<hipStream_t>(stream), out);
}

extern "C" int dfq_sweep_plan_execute(dfq_sweep_plan* p, void* stream) {
    if (!p) return DFQ_ERR_INVALID;
    return launch_sweep(p->variant, static_cast<hipStream_t>(stream), p->d_tensors, p->d_reduce, p->n_reduce, p->d_main,
                        p->n_main, p->d_slots, p->n_slots);
}

extern "C" int dfq_sweep_plan_stats(const dfq_sweep_plan* p, dfq_sweep_stats* st) {
    if (!p || !st) return DFQ_ERR_INVALID;
    st->n_tensors = p->n_tensors;
    st->n_elems = p->n_elems;
    st->n_tasks_reduce = p->n_reduce;
    st->n_tasks_main = p->n_main;
    st->algo_bytes = p->algo_bytes;
    st->launches = (p->n_reduce > 0 ? 1 : 0) + (p->n_main > 0 ? 1 : 0);
    st->grid_blocks = p->n_main > 0 ? grid_for(p->n_main) : 0;
    st->variant = p->variant;
    return DFQ_OK;
}

extern "C" int dfq_sweep_plan_destroy(dfq_sweep_plan* p) {
    if (!p) return DFQ_OK;
    (void)hipFree(p->d_owned);   // NULL for workspace-backed plans
    delete p;
    return DFQ_OK;
}

// ---------------------------------------------------------------------------
// Single-tensor path: the workspace carries [slots | tensor | tasks]; the host-built
// tables go up through the pinned staging ring (stage_h2d), so a call is
// asynchronous on the caller's stream like every other entry point.
// ---------------------------------------------------------------------------
extern "C" int dfq_quantize_tensor(const dfq_tensor_desc* d, void* ws, size_t ws_bytes, void* stream) {
    if (!d) return DFQ_ERR_INVALID;
    SweepTables B;
    SingleLayout Lo;
    int rc = sweep_single_tables(*d, B, Lo);
    if (rc) return rc;
    if (!ws || ws_bytes < Lo.total) return DFQ_ERR_WORKSPACE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* base = static_cast<char*>(ws);
    DevTensor* dt = reinterpret_cast<DevTensor*>(base + Lo.o_tensor);
    // one table blob [tensor | reduce tasks | main tasks] through the pinned staging
    // ring: stream-ordered, no host synchronisation
    const std::vector<char> blob = table_blob(B, Lo.o_tensor, Lo.o_reduce, Lo.o_main, Lo.total);
    DFQ_HIP_CHECK(stage_h2d(dt, blob.data(), blob.size(), s));
    return launch_sweep(B.variant, s, dt, reinterpret_cast<DevTask*>(base + Lo.o_reduce), (int64_t)B.reduce.size(),
                        reinterpret_cast<DevTask*>(base + Lo.o_main), (int64_t)B.main.size(),
                        reinterpret_cast<uint32_t*>(base), B.slots);
}

#ifdef DFQ_DIAGNOSTICS
// Diagnostics: point variant 13's timeline at `buf` (4 uint64 per main-list task,
// `cap` tasks); NULL/0 disables.  Not part of the reference interface.
extern "C" int dfq_debug_timeline(void* buf, int64_t cap) {
    uint64_t* p = static_cast<uint64_t*>(buf);
    DFQ_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_timeline), &p, sizeof(p)));
    DFQ_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_timeline_cap), &cap, sizeof(cap)));
    return DFQ_OK;
}

// Diagnostics: variant 13's ablation bits (g_ablate); results are wrong while set.
extern "C" int dfq_debug_ablate(uint32_t flags) {
    DFQ_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_ablate), &flags, sizeof(flags)));
    return DFQ_OK;
}
#endif  // DFQ_DIAGNOSTICS

// Code-object loading at library initialisation (dfq_preload): the first launch of
// a kernel otherwise pays for loading its translation unit's code object.
namespace dfq {
hipError_t preload_sweep() {
    hipFuncAttributes a;
    hipError_t e = hipFuncGetAttributes(&a, reinterpret_cast<const void*>(main_kernel(kDefaultVariant)));
    if (e == hipSuccess) e = hipFuncGetAttributes(&a, reinterpret_cast<const void*>(sweep_reduce_kernel));
    return e;
}
}  // namespace dfq
