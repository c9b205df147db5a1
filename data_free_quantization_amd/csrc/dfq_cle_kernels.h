// The device code of the device-resident CLE loop (dfq_cle_plan_*): its kernels and the caller's
// stream gate of a launched run.  Included by dfq_cle.hip only, the one translation unit that launches
// them.  fp32 arithmetic is ordered exactly as the reference's torch CPU ops.
#pragma once
#include "dfq_cle_common.h"
namespace dfq {

struct CleState {
    double diff;         // Cross_layer_equal.py `diff`
    double thr;          // Treshhold
    int32_t iter_count;  // consecutive iterations with |diff - diff_tmp| <= 1e-9
    int32_t iters;       // iterations run
    int32_t done;
    int32_t count;       // Count
    int32_t max_iters;
    int32_t error;       // 2: a tile block saw an unexpected iteration parity (never expected)
};

constexpr int kCleW1RowsPerTask = 4;       // one wave per row
constexpr int kCleW2ChansPerTask = 4;      // one wave per contiguous column

__device__ __forceinline__ float group_min(float v, int g) {
    for (int off = g >> 1; off >= 1; off >>= 1) v = fminf(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ float group_max(float v, int g) {
    for (int off = g >> 1; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}
// f(row, active, sub-lane, G) for rows [a, b) of length len < 64: every lane of
// the block calls f the same number of times (shuffles stay convergent)
template <class F>
__device__ __forceinline__ void for_short_rows(int64_t a, int64_t b, int64_t len, F&& f) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int G = row_group_lanes(len), rpw = 64 / G;
    const int sub = lane / G, sl = lane % G;
    for (int64_t base = a + (int64_t)wv * rpw; base < b; base += (int64_t)(kThreads / 64) * rpw) {
        const int64_t c = base + sub;
        f(c, c < b, sl, G);
    }
}
// min / max of n floats at p, one wave, 4 loads in flight per lane
__device__ __forceinline__ void wave_range(const float* __restrict__ p_, int64_t n, bool vec, int lane, float& vmin,
                                           float& vmax) {
    const DFQ_GLOBAL float* __restrict__ p = (const DFQ_GLOBAL float*)p_;   // global: not flat
    vmin = INFINITY;
    vmax = -INFINITY;
    if (vec) {
        const DFQ_GLOBAL f32x4* p4 = (const DFQ_GLOBAL f32x4*)p;
        const int64_t n4 = n >> 2;
        for (int64_t i = lane; i < n4; i += 4 * 64) {
            f32x4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (i + 64 * u < n4) v[u] = p4[i + 64 * u];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (i + 64 * u < n4) {
                    vmin = fminf(vmin, fminf(fminf(v[u].x, v[u].y), fminf(v[u].z, v[u].w)));
                    vmax = fmaxf(vmax, fmaxf(fmaxf(v[u].x, v[u].y), fmaxf(v[u].z, v[u].w)));
                }
        }
    } else {
        for (int64_t i = lane; i < n; i += 4 * 64) {
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (i + 64 * u < n) v[u] = p[i + 64 * u];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (i + 64 * u < n) {
                    vmin = fminf(vmin, v[u]);
                    vmax = fmaxf(vmax, v[u]);
                }
        }
    }
    cle_wave_minmax(vmin, vmax);
}

// p[0..n) *= f(), one wave; 4 loads in flight per lane before the stores.  The
// factor (range-table reads) is evaluated after the first loads are issued, so
// the data and the range words are one memory round trip, not two.
template <class F>
__device__ __forceinline__ void wave_scale(float* __restrict__ p_, int64_t n, bool vec, int lane, F&& factor) {
    DFQ_GLOBAL float* __restrict__ p = (DFQ_GLOBAL float*)p_;   // global: not flat
    float f = 0.f;
    bool have = false;
    if (vec) {
        DFQ_GLOBAL f32x4* p4 = (DFQ_GLOBAL f32x4*)p;
        const int64_t n4 = n >> 2;
        for (int64_t i = lane; i < n4; i += 4 * 64) {
            f32x4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (i + 64 * u < n4) v[u] = p4[i + 64 * u];
            if (!have) {
                f = factor();
                have = true;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (i + 64 * u < n4) {
                    v[u].x = v[u].x * f;
                    v[u].y = v[u].y * f;
                    v[u].z = v[u].z * f;
                    v[u].w = v[u].w * f;
                    p4[i + 64 * u] = v[u];
                }
        }
    } else {
        for (int64_t i = lane; i < n; i += 4 * 64) {
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (i + 64 * u < n) v[u] = p[i + 64 * u];
            if (!have) {
                f = factor();
                have = true;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (i + 64 * u < n) p[i + 64 * u] = v[u] * f;
        }
    }
}

// wave_scale that also returns the (min, max) of the products (every lane).
template <class F>
__device__ __forceinline__ void wave_scale_mm(float* __restrict__ p_, int64_t n, bool vec, int lane, float& vmin,
                                              float& vmax, F&& factor) {
    DFQ_GLOBAL float* __restrict__ p = (DFQ_GLOBAL float*)p_;   // global: not flat
    vmin = INFINITY;
    vmax = -INFINITY;
    float f = 0.f;
    bool have = false;
    if (vec) {
        DFQ_GLOBAL f32x4* p4 = (DFQ_GLOBAL f32x4*)p;
        const int64_t n4 = n >> 2;
        for (int64_t i = lane; i < n4; i += 4 * 64) {
            f32x4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (i + 64 * u < n4) v[u] = p4[i + 64 * u];
            if (!have) {
                f = factor();
                have = true;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (i + 64 * u < n4) {
                    v[u].x = v[u].x * f;
                    v[u].y = v[u].y * f;
                    v[u].z = v[u].z * f;
                    v[u].w = v[u].w * f;
                    p4[i + 64 * u] = v[u];
                    vmin = fminf(vmin, fminf(fminf(v[u].x, v[u].y), fminf(v[u].z, v[u].w)));
                    vmax = fmaxf(vmax, fmaxf(fmaxf(v[u].x, v[u].y), fmaxf(v[u].z, v[u].w)));
                }
        }
    } else {
        for (int64_t i = lane; i < n; i += 4 * 64) {
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (i + 64 * u < n) v[u] = p[i + 64 * u];
            if (!have) {
                f = factor();
                have = true;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (i + 64 * u < n) {
                    const float y = v[u] * f;
                    p[i + 64 * u] = y;
                    vmin = fminf(vmin, y);
                    vmax = fmaxf(vmax, y);
                }
        }
    }
    cle_wave_minmax(vmin, vmax);
}

// p[0..n) *= f() and the (min, max) of the products, one wave (scalar loads:
// used for short depthwise rows); the factor is read after the first load
template <class F>
__device__ __forceinline__ void wave_scale_range(float* __restrict__ p_, int64_t n, int lane, float& vmin, float& vmax,
                                                 F&& factor) {
    DFQ_GLOBAL float* __restrict__ p = (DFQ_GLOBAL float*)p_;   // global: not flat
    vmin = INFINITY;
    vmax = -INFINITY;
    float f = 0.f;
    bool have = false;
    for (int64_t i = lane; i < n; i += 64) {
        const float x = p[i];
        if (!have) {
            f = factor();
            have = true;
        }
        const float y = x * f;
        p[i] = y;
        vmin = fminf(vmin, y);
        vmax = fmaxf(vmax, y);
    }
    cle_wave_minmax(vmin, vmax);
}

// W2 row tiles with KH*KW = khw in (1, kTileMaxKhw] and one group: thread t owns
// the tile's flattened positions p = t + 256 m (m < khw) -- consecutive threads
// on consecutive floats, khw independent loads per row in flight -- instead of
// one thread per column walking its khw floats serially (kTileMaxKhw and
// kPosTileMaxRows, the rows of such a rescale tile: dfq_cle_plan.h).
__device__ __forceinline__ bool tile_by_position(const CleRel& R, const CleTask& tk) {
    return R.khw2 > 1 && R.khw2 <= kTileMaxKhw && (tk.a / R.o2g) == ((tk.b - 1) / R.o2g);
}

// Column ranges of the tile: per-position (min, max) over its rows, then over each
// column's khw positions through LDS (tl: 2 * kThreads * kTileMaxKhw floats).
__device__ void tile_range_by_position(const CleRel& R, const CleTask& tk, uint32_t* __restrict__ mn,
                                       uint32_t* __restrict__ mx, float* __restrict__ tl) {
    const int t = threadIdx.x;
    const int khw = (int)R.khw2;
    const int64_t rowlen = R.i2 * R.khw2;
    const int ncol = (int)(tk.c1 - tk.c0);
    const int npos = ncol * khw;
    const DFQ_GLOBAL float* base = (const DFQ_GLOBAL float*)(R.w2 + tk.c0 * R.khw2);
    float vmn[kTileMaxKhw], vmx[kTileMaxKhw];
#pragma unroll
    for (int m = 0; m < kTileMaxKhw; ++m) {
        vmn[m] = INFINITY;
        vmx[m] = -INFINITY;
    }
    for (int64_t o = tk.a; o < tk.b; ++o) {
        const DFQ_GLOBAL float* rp = base + o * rowlen;
        float v[kTileMaxKhw];
#pragma unroll
        for (int m = 0; m < kTileMaxKhw; ++m)
            if (m < khw && t + kThreads * m < npos) v[m] = rp[t + kThreads * m];
#pragma unroll
        for (int m = 0; m < kTileMaxKhw; ++m)
            if (m < khw && t + kThreads * m < npos) {
                vmn[m] = fminf(vmn[m], v[m]);
                vmx[m] = fmaxf(vmx[m], v[m]);
            }
    }
#pragma unroll
    for (int m = 0; m < kTileMaxKhw; ++m)
        if (m < khw && t + kThreads * m < npos) {
            tl[t + kThreads * m] = vmn[m];
            tl[kThreads * kTileMaxKhw + t + kThreads * m] = vmx[m];
        }
    __syncthreads();
    if (t < ncol) {
        float a = INFINITY, b = -INFINITY;
        for (int k = 0; k < khw; ++k) {
            a = fminf(a, tl[t * khw + k]);
            b = fmaxf(b, tl[kThreads * kTileMaxKhw + t * khw + k]);
        }
        const int64_t c = R.c1 + (tk.a / R.o2g) * R.i2 + tk.c0 + t;
        atomicMin(&mn[c], enc_ord(a));
        atomicMax(&mx[c], enc_ord(b));
    }
    __syncthreads();   // tl is reused by the next task
}

// Range tasks [t0, t1) for parity `par`, taken by blocks blk, blk + nblk, ...
// (tl: 2 * kThreads * kTileMaxKhw floats of LDS).
__device__ __forceinline__ void cle_range_body(const CleRel* __restrict__ rels, const CleTask* __restrict__ tasks,
                                               int64_t t0, int64_t t1, uint32_t* __restrict__ rng, int64_t M, int par,
                                               int64_t blk, int64_t nblk, float* tl) {
    uint32_t* mins = rng + (int64_t)par * 2 * M;
    uint32_t* maxs = mins + M;
    uint32_t* omins = rng + (int64_t)(par ^ 1) * 2 * M;
    uint32_t* omaxs = omins + M;
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    for (int64_t t = t0 + blk; t < t1; t += nblk) {
        const CleTask tk = tasks[t];
        const CleRel& R = rels[tk.rel];
        uint32_t* mn = mins + R.moff;
        uint32_t* mx = maxs + R.moff;
        if (tk.kind == kRangeW1 && R.len1 < 64) {   // short rows: a lane group per row
            for_short_rows(tk.a, tk.b, R.len1, [&](int64_t c, bool act, int sl, int G) {
                float vmin = INFINITY, vmax = -INFINITY;
                if (act)
                    for (int64_t i = sl; i < R.len1; i += G) {
                        const float x = ((DFQ_GLOBAL float*)R.w1)[c * R.len1 + i];
                        vmin = fminf(vmin, x);
                        vmax = fmaxf(vmax, x);
                    }
                vmin = group_min(vmin, G);
                vmax = group_max(vmax, G);
                if (act && sl == 0) {
                    mn[c] = enc_ord(vmin);
                    mx[c] = enc_ord(vmax);
                }
            });
        } else if (tk.kind == kRangeW2Contig && R.o2g * R.khw2 < 64) {
            const int64_t seg = R.o2g * R.khw2;
            for_short_rows(tk.a, tk.b, seg, [&](int64_t c, bool act, int sl, int G) {
                float vmin = INFINITY, vmax = -INFINITY;
                if (act)
                    for (int64_t i = sl; i < seg; i += G) {
                        const float x = ((DFQ_GLOBAL float*)R.w2)[c * seg + i];
                        vmin = fminf(vmin, x);
                        vmax = fmaxf(vmax, x);
                    }
                vmin = group_min(vmin, G);
                vmax = group_max(vmax, G);
                if (act && sl == 0) {
                    mn[R.c1 + c] = enc_ord(vmin);
                    mx[R.c1 + c] = enc_ord(vmax);
                }
            });
        } else if (tk.kind == kRangeW1) {   // one wave per W1 row
            for (int64_t c = tk.a + wv; c < tk.b; c += kThreads / 64) {
                float vmin, vmax;
                wave_range(R.w1 + c * R.len1, R.len1, R.vec1, lane, vmin, vmax);
                if (lane == 0) {
                    mn[c] = enc_ord(vmin);
                    mx[c] = enc_ord(vmax);
                }
            }
        } else if (tk.kind == kRangeW2Contig) {   // one wave per contiguous W2 channel
            const int64_t seg = R.o2g * R.khw2;
            for (int64_t c = tk.a + wv; c < tk.b; c += kThreads / 64) {
                float vmin, vmax;
                wave_range(R.w2 + c * seg, seg, R.vec2, lane, vmin, vmax);
                if (lane == 0) {
                    mn[R.c1 + c] = enc_ord(vmin);
                    mx[R.c1 + c] = enc_ord(vmax);
                }
            }
        } else if (tk.kind == kRangeW2Tile) {   // rows [a, b) of W2, one thread per column
            if (tile_by_position(R, tk)) {
                tile_range_by_position(R, tk, mn, mx, tl);
                continue;
            }
            const int64_t rowlen = R.i2 * R.khw2;
            const bool one_group = (tk.a / R.o2g) == ((tk.b - 1) / R.o2g);
            for (int64_t i = tk.c0 + threadIdx.x; i < tk.c1; i += kThreads) {
                float vmin = INFINITY, vmax = -INFINITY;
                if (one_group && R.khw2 == 1) {   // 1x1 / Linear: the tile's column, 16 loads in flight
                    float v[kColTileRows];
#pragma unroll
                    for (int j = 0; j < kColTileRows; ++j)
                        if (tk.a + j < tk.b) v[j] = ((DFQ_GLOBAL float*)R.w2)[(tk.a + j) * rowlen + i];
#pragma unroll
                    for (int j = 0; j < kColTileRows; ++j)
                        if (tk.a + j < tk.b) {
                            vmin = fminf(vmin, v[j]);
                            vmax = fmaxf(vmax, v[j]);
                        }
                    const int64_t c = R.c1 + (tk.a / R.o2g) * R.i2 + i;
                    atomicMin(&mn[c], enc_ord(vmin));
                    atomicMax(&mx[c], enc_ord(vmax));
                    continue;
                }
                int64_t g_prev = -1;
                for (int64_t o = tk.a; o < tk.b; ++o) {
                    const int64_t g = o / R.o2g;
                    if (g != g_prev && g_prev >= 0) {   // tile straddles groups: flush
                        atomicMin(&mn[R.c1 + g_prev * R.i2 + i], enc_ord(vmin));
                        atomicMax(&mx[R.c1 + g_prev * R.i2 + i], enc_ord(vmax));
                        vmin = INFINITY;
                        vmax = -INFINITY;
                    }
                    g_prev = g;
                    const DFQ_GLOBAL float* p = (const DFQ_GLOBAL float*)(R.w2 + o * rowlen + i * R.khw2);
                    for (int64_t k = 0; k < R.khw2; ++k) {
                        vmin = fminf(vmin, p[k]);
                        vmax = fmaxf(vmax, p[k]);
                    }
                }
                if (g_prev >= 0) {
                    atomicMin(&mn[R.c1 + g_prev * R.i2 + i], enc_ord(vmin));
                    atomicMax(&mx[R.c1 + g_prev * R.i2 + i], enc_ord(vmax));
                }
            }
        } else {   // kRangeReset(W1): the other parity's W2 (W1) words, for the next iteration's atomics
            const int64_t off = R.moff + (tk.kind == kRangeReset ? R.c1 : 0);
            for (int64_t c = tk.a + threadIdx.x; c < tk.b; c += kThreads) {
                omins[off + c] = 0xFFFFFFFFu;
                omaxs[off + c] = 0u;
            }
        }
    }
}

// `next` = 1: the ranges of the NEXT iteration (launched after this iteration's
// last rescale, fused into the metric-tile launch; see cle_loop_step_kernel)
__global__ void __launch_bounds__(kThreads)
cle_loop_range_kernel(const CleRel* __restrict__ rels, const CleTask* __restrict__ tasks, int64_t t0, int64_t t1,
                      uint32_t* __restrict__ rng, int64_t M, const CleState* __restrict__ st, int next) {
    __shared__ float tl[2 * kThreads * kTileMaxKhw];
    if (st->done) return;
    cle_range_body(rels, tasks, t0, t1, rng, M, (st->iters + next) & 1, blockIdx.x, gridDim.x, tl);
}

// The scale of relation R for channel c (mins / maxs: the parity's range words).
// A relation whose W1 is the depthwise W2 of relation Q (R.dw_prev) has no W1
// range words: its W1 row c is Q's filter c after Q's rescale, fl(x * inv_Q[c]),
// and with inv_Q > 0 that product is monotonic in x, so the row's min / max are
// fl(min_c * inv_Q) / fl(max_c * inv_Q) -- Q's W2 range words (the filter at the
// start of the iteration) scaled.  Every task of R can therefore compute its scale
// in the same launch that rescales Q (kApplyDwBoth writes the filter once).
__device__ __forceinline__ CleScale cle_rel_scale(const CleRel* __restrict__ rels, const CleRel& R,
                                                  const uint32_t* __restrict__ mins, const uint32_t* __restrict__ maxs,
                                                  int64_t c, int is_signed, float eps, double smin, double smax) {
    if (R.dw_prev < 0) return cle_scale(mins + R.moff, maxs + R.moff, R.c1, c, is_signed, eps, smin, smax);
    const CleRel& Q = rels[R.dw_prev];
    const CleScale q = cle_scale(mins + Q.moff, maxs + Q.moff, Q.c1, c, is_signed, eps, smin, smax);
    const float mn1 = dec_ord(mins[Q.moff + Q.c1 + c]) * q.inv;
    const float mx1 = dec_ord(maxs[Q.moff + Q.c1 + c]) * q.inv;
    return cle_scale_from(mn1, mx1, dec_ord(mins[R.moff + R.c1 + c]), dec_ord(maxs[R.moff + R.c1 + c]), is_signed, eps,
                          smin, smax);
}

// LDS of one rescale task (the position-parallel and fused tiles)
struct CleApplyLds {
    float red[2][kThreads / 64][kColTileRows];
    float inv_s[kThreads];
    float inv_pos[kThreads * kTileMaxKhw];
    float rows[kColTileRows * kThreads];   // a 1x1 W2 tile's rescaled values, for its per-row ranges
};

// Rescale tasks [t0, t1) of iteration parity `par`, taken by blocks blk, blk + nblk, ...
#ifdef DFQ_DIAGNOSTICS
// DFQ_CLE_TL (diagnostics): per rescale task of one steady-state iteration,
// {start, end} in s_memrealtime ticks (100 MHz) and the block's XCC / CU ids.
__device__ uint64_t* g_cle_tl = nullptr;
// ... and per block of the iteration's last launch (tiles / ranges / stop rule):
// {start, end, role (1 tile, 2 range), 0}; slot kCleTl2Fin: the stop rule's {start,
// end, chunk sums staged, layer means done}
__device__ uint64_t* g_cle_tl2 = nullptr;
// DFQ_CLE_TL_STEP=k: record the blocks of step k's launches instead (the launch whose
// rescale tasks start at table index g_cle_tl2_a0; -1: every launch, the last wins)
__device__ int64_t g_cle_tl2_a0 = -1;
constexpr int kCleTl2Fin = 8192;
#endif

// POS: the step has position-parallel (KH*KW > 1) W2 tiles; without them the
// body needs far fewer VGPRs (more waves per SIMD for the latency-bound tasks)
template <bool POS = true>
__device__ __forceinline__ void cle_apply_body(const CleRel* __restrict__ rels, const CleTask* __restrict__ tasks,
                                               int64_t t0, int64_t t1, uint32_t* __restrict__ rng, int64_t M,
                                               int par, bool first_iter, int is_signed, float eps, double smin,
                                               double smax, int64_t blk, int64_t nblk, CleApplyLds& A,
                                               float* __restrict__ vsave = nullptr, int32_t* __restrict__ vtag = nullptr,
                                               int32_t iter = 0) {
    auto& red = A.red;
    float* rows = A.rows;
    float* inv_s = A.inv_s;
    float* inv_pos = A.inv_pos;
    uint32_t* mins = rng + (int64_t)par * 2 * M;
    uint32_t* maxs = mins + M;
    uint32_t* nmins = rng + (int64_t)(par ^ 1) * 2 * M;   // the next iteration's words (self ranges)
    uint32_t* nmaxs = nmins + M;
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    for (int64_t t = t0 + blk; t < t1; t += nblk) {
#ifdef DFQ_DIAGNOSTICS
        const bool tl_on = g_cle_tl != nullptr;   // block-uniform
        const uint64_t tl_start = tl_on ? __builtin_amdgcn_s_memrealtime() : 0;
        uint64_t tl_sub = 0;   // position tiles: phase ends (10 ns ticks after start, 16 bits each)
#define DFQ_CLE_TL_MARK(k) \
        if (tl_on) tl_sub |= (1ull << 63) | (((__builtin_amdgcn_s_memrealtime() - tl_start) & 0xffffull) << (16 * (k)));
#else
#define DFQ_CLE_TL_MARK(k)
#endif
        const CleTask tk = tasks[t];
        const CleRel& R = rels[tk.rel];
        const uint32_t* mn = mins + R.moff;
        const uint32_t* mx = maxs + R.moff;
        if (tk.kind == kApplyW1 && R.len1 < 64) {   // short rows: a lane group per row
            for_short_rows(tk.a, tk.b, R.len1, [&](int64_t c, bool act, int sl, int G) {
                float y0 = INFINITY, y1 = -INFINITY;
                if (act && sl < R.len1) {   // G >= len1: one element per lane
                    DFQ_GLOBAL float* p = (DFQ_GLOBAL float*)(R.w1 + c * R.len1 + sl);
                    const float x = *p;   // in flight while the scale's range words load
                    const float y = x * cle_rel_scale(rels, R, mins, maxs, c, is_signed, eps, smin, smax).s;
                    *p = y;
                    y0 = y1 = y;
                }
                if (R.w1_self) {   // the row is final for this iteration: its next range
                    y0 = group_min(y0, G);
                    y1 = group_max(y1, G);
                    if (act && sl == 0) {
                        nmins[R.moff + c] = enc_ord(y0);
                        nmaxs[R.moff + c] = enc_ord(y1);
                    }
                }
            });
        } else if (tk.kind == kApplyDwBoth && R.o2g * R.khw2 < 64) {
            const CleRel& N = rels[tk.c0];
            const int64_t seg = R.o2g * R.khw2;
            for_short_rows(tk.a, tk.b, seg, [&](int64_t c, bool act, int sl, int G) {
                float z0 = INFINITY, z1 = -INFINITY;
                if (act && sl < seg) {   // G >= seg: one element per lane
                    DFQ_GLOBAL float* p = (DFQ_GLOBAL float*)(R.w2 + c * seg + sl);
                    const float x = *p;
                    const float inv = cle_rel_scale(rels, R, mins, maxs, c, is_signed, eps, smin, smax).inv;
                    const float sn = cle_rel_scale(rels, N, mins, maxs, c, is_signed, eps, smin, smax).s;
                    const float y = x * inv;
                    const float z = y * sn;
                    *p = z;
                    z0 = z1 = z;
                }
                if (R.w2_self) {   // the filter is final for this iteration: its next range
                    z0 = group_min(z0, G);
                    z1 = group_max(z1, G);
                    if (act && sl == 0) {
                        nmins[R.moff + R.c1 + c] = enc_ord(z0);
                        nmaxs[R.moff + R.c1 + c] = enc_ord(z1);
                    }
                }
            });
        } else if (tk.kind == kApplyW2Contig && R.o2g * R.khw2 < 64) {
            const int64_t seg = R.o2g * R.khw2;
            const bool fuse = R.fuse_next >= 0;
            for_short_rows(tk.a, tk.b, seg, [&](int64_t c, bool act, int sl, int G) {
                float vmin = INFINITY, vmax = -INFINITY;
                if (act && sl < seg) {   // G >= seg: one element per lane
                    DFQ_GLOBAL float* p = (DFQ_GLOBAL float*)(R.w2 + c * seg + sl);
                    const float x = *p;
                    const float y = x * cle_rel_scale(rels, R, mins, maxs, c, is_signed, eps, smin, smax).inv;
                    *p = y;
                    vmin = vmax = y;
                }
                if (fuse) {   // o2g == 1: the segment is row c of the next relation's W1
                    vmin = group_min(vmin, G);
                    vmax = group_max(vmax, G);
                    if (act && sl == 0) {
                        const int64_t off = rels[R.fuse_next].moff;
                        mins[off + c] = enc_ord(vmin);
                        maxs[off + c] = enc_ord(vmax);
                    }
                }
            });
        } else if (tk.kind == kApplyW1) {   // W1[c, :] *= s[c], one wave per row
            for (int64_t c = tk.a + wv; c < tk.b; c += kThreads / 64) {
                auto sc = [&] { return cle_rel_scale(rels, R, mins, maxs, c, is_signed, eps, smin, smax).s; };
                if (R.w1_self) {   // the row is final for this iteration: its next range
                    float y0, y1;
                    wave_scale_mm(R.w1 + c * R.len1, R.len1, R.vec1, lane, y0, y1, sc);
                    if (lane == 0) {
                        nmins[R.moff + c] = enc_ord(y0);
                        nmaxs[R.moff + c] = enc_ord(y1);
                    }
                } else {
                    wave_scale(R.w1 + c * R.len1, R.len1, R.vec1, lane, sc);
                }
            }
        } else if (tk.kind == kApplyDwBoth) {
            // relation R's depthwise W2 filter c, which is relation tk.c0's W1 row c:
            // *= 1/s_R[c], then *= s_next[c] (two roundings, as the reference's two
            // in-place multiplies), written once
            const CleRel& N = rels[tk.c0];
            const int64_t seg = R.o2g * R.khw2;
            for (int64_t c = tk.a + wv; c < tk.b; c += kThreads / 64) {
                const float inv = cle_rel_scale(rels, R, mins, maxs, c, is_signed, eps, smin, smax).inv;
                const float sn = cle_rel_scale(rels, N, mins, maxs, c, is_signed, eps, smin, smax).s;
                DFQ_GLOBAL float* p = (DFQ_GLOBAL float*)(R.w2 + c * seg);
                float z0 = INFINITY, z1 = -INFINITY;
                for (int64_t i = lane; i < seg; i += 64) {
                    const float y = p[i] * inv;
                    const float z = y * sn;
                    p[i] = z;
                    z0 = fminf(z0, z);
                    z1 = fmaxf(z1, z);
                }
                if (R.w2_self) {
                    cle_wave_minmax(z0, z1);
                    if (lane == 0) {
                        nmins[R.moff + R.c1 + c] = enc_ord(z0);
                        nmaxs[R.moff + R.c1 + c] = enc_ord(z1);
                    }
                }
            }
        } else if (tk.kind == kApplyW2Contig) {   // W2 channel segment *= 1/s[c]
            const int64_t seg = R.o2g * R.khw2;
            for (int64_t c = tk.a + wv; c < tk.b; c += kThreads / 64) {
                auto inv = [&] { return cle_rel_scale(rels, R, mins, maxs, c, is_signed, eps, smin, smax).inv; };
                if (R.fuse_next >= 0) {   // o2g == 1: the segment is row c of W2 = row c of the next W1
                    float vmin, vmax;
                    wave_scale_range(R.w2 + c * seg, seg, lane, vmin, vmax, inv);
                    if (lane == 0) {
                        const int64_t off = rels[R.fuse_next].moff;
                        mins[off + c] = enc_ord(vmin);
                        maxs[off + c] = enc_ord(vmax);
                    }
                } else {
                    wave_scale(R.w2 + c * seg, seg, R.vec2, lane, inv);
                }
            }
        } else if (POS && tk.kind == kApplyW2Tile && tile_by_position(R, tk) && tk.b - tk.a <= kPosTileMaxRows) {
            // position-parallel tile (KH*KW > 1): the columns' 1/s into LDS, then each
            // row's positions scaled; fused: the rows' (min, max) for the next W1
            const int t = threadIdx.x;
            const int khw = (int)R.khw2;
            const int64_t rowlen = R.i2 * R.khw2;
            const int ncol = (int)(tk.c1 - tk.c0);
            const int npos = ncol * khw;
            DFQ_GLOBAL float* base = (DFQ_GLOBAL float*)(R.w2 + tk.c0 * R.khw2);
            const bool fuse = R.fuse_next >= 0;
            if (t < ncol)
                inv_s[t] = cle_rel_scale(rels, R, mins, maxs, (tk.a / R.o2g) * R.i2 + tk.c0 + t, is_signed, eps, smin, smax).inv;
            __syncthreads();
            DFQ_CLE_TL_MARK(0)
            for (int q = t; q < npos; q += kThreads) inv_pos[q] = inv_s[q / khw];   // 1/s per position
            __syncthreads();
            DFQ_CLE_TL_MARK(1)
            // Every row's loads in flight together, then the rows' scaled stores:
            // one memory round trip per tile instead of one per row (~5 us a row
            // under the step's load, ResNet-50's 3x3 tiles; DFQ_CLE_TL)
            // (row bases uniform, the lane's offset a 32-bit index: SGPR-base loads
            // sharing one VGPR offset, not 36 64-bit VGPR addresses)
            float v[kPosTileMaxRows][kTileMaxKhw];
#pragma unroll
            for (int r = 0; r < kPosTileMaxRows; ++r) {
                const DFQ_GLOBAL float* rb = base + (tk.a + r) * rowlen;
#pragma unroll
                for (int m = 0; m < kTileMaxKhw; ++m)
                    if (tk.a + r < tk.b && m < khw && t + kThreads * m < npos) v[r][m] = rb[t + kThreads * m];
            }
#pragma unroll
            for (int r = 0; r < kPosTileMaxRows; ++r) {
                if (tk.a + r >= tk.b) break;   // uniform
                DFQ_GLOBAL float* rp = base + (tk.a + r) * rowlen;
                float lo = INFINITY, hi = -INFINITY;
#pragma unroll
                for (int m = 0; m < kTileMaxKhw; ++m)
                    if (m < khw && t + kThreads * m < npos) {
                        const float y = v[r][m] * inv_pos[t + kThreads * m];
                        rp[t + kThreads * m] = y;
                        lo = fminf(lo, y);
                        hi = fmaxf(hi, y);
                    }
                if (fuse) {
                    cle_wave_minmax(lo, hi);
                    if (lane == 0) {
                        red[0][wv][r] = lo;
                        red[1][wv][r] = hi;
                    }
                }
            }
            __syncthreads();
            DFQ_CLE_TL_MARK(2)
            if (fuse && t < tk.b - tk.a) {
                float a = red[0][0][t], b = red[1][0][t];
                for (int w = 1; w < kThreads / 64; ++w) {
                    a = fminf(a, red[0][w][t]);
                    b = fmaxf(b, red[1][w][t]);
                }
                const int64_t off = rels[R.fuse_next].moff + tk.a + t;
                atomicMin(&mins[off], enc_ord(a));
                atomicMax(&maxs[off], enc_ord(b));
            }
            __syncthreads();   // inv_s / red are reused by the next task
        } else if (tk.kind == kApplyW2Tile && R.fuse_next >= 0) {
            // rows [a, b) x columns [c0, c0 + 256) of W2, one thread per column, and the
            // tile's per-row (min, max) of the results -> the next relation's W1 rows
            // (each row's wave reduction in uniform control flow: no per-row arrays)
            const int64_t rowlen = R.i2 * R.khw2;
            const int64_t i = tk.c0 + threadIdx.x;
            const bool act = i < tk.c1;
            const bool one_group = (tk.a / R.o2g) == ((tk.b - 1) / R.o2g);
            const int nr = (int)(tk.b - tk.a);
            if (one_group && R.khw2 == 1) {   // 1x1 / Linear: the column's loads first
                // The tile's values go to LDS as rows[j][column]; after one barrier,
                // lane t reduces 16 columns of row t / 16 and the 16 lanes of a DPP
                // row combine them (4 steps): per task 16 short reductions on 256
                // lanes instead of 16 dependent 64-lane wave reductions (3.3 of
                // these tasks' 7.4 us, DFQ_CLE_TL).  fminf / fmaxf skip the NaN that
                // marks a column past the tile.
                float v[kColTileRows];
#pragma unroll
                for (int j = 0; j < kColTileRows; ++j)
                    if (act && j < nr) v[j] = ((DFQ_GLOBAL float*)R.w2)[(tk.a + j) * rowlen + i];
                const float inv =
                    act ? cle_rel_scale(rels, R, mins, maxs, (tk.a / R.o2g) * R.i2 + i, is_signed, eps, smin, smax).inv : 0.f;
#pragma unroll
                for (int j = 0; j < kColTileRows; ++j) {
                    if (j < nr) {   // uniform
                        float y = __builtin_nanf("");
                        if (act) {
                            y = v[j] * inv;
                            ((DFQ_GLOBAL float*)R.w2)[(tk.a + j) * rowlen + i] = y;
                        }
                        rows[j * kThreads + threadIdx.x] = y;
                    }
                    if (j == 0) {   // the column's loads and its scale have landed
                        DFQ_CLE_TL_MARK(0)
                    }
                }
                DFQ_CLE_TL_MARK(1)   // every row stored
                block_lds_sync();
                const int r = threadIdx.x >> 4, sg = threadIdx.x & 15;
                float lo = INFINITY, hi = -INFINITY;
                if (r < nr) {
                    const float4* q = reinterpret_cast<const float4*>(rows + r * kThreads + sg * 16);
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const float4 x = q[u];
                        lo = fminf(lo, fminf(fminf(x.x, x.y), fminf(x.z, x.w)));
                        hi = fmaxf(hi, fmaxf(fmaxf(x.x, x.y), fmaxf(x.z, x.w)));
                    }
                }
                lo = fminf(lo, dpp_f(lo, 0xB1));
                hi = fmaxf(hi, dpp_f(hi, 0xB1));
                lo = fminf(lo, dpp_f(lo, 0x4E));
                hi = fmaxf(hi, dpp_f(hi, 0x4E));
                lo = fminf(lo, dpp_f(lo, 0x141));
                hi = fmaxf(hi, dpp_f(hi, 0x141));
                lo = fminf(lo, dpp_f(lo, 0x140));
                hi = fmaxf(hi, dpp_f(hi, 0x140));
                DFQ_CLE_TL_MARK(2)
                if (sg == 0 && r < nr) {
                    const int64_t off = rels[R.fuse_next].moff + tk.a + r;
                    atomicMin(&mins[off], enc_ord(lo));
                    atomicMax(&maxs[off], enc_ord(hi));
                }
            } else {
                int64_t g_prev = -1;
                float inv = 0.f;
                for (int j = 0; j < nr; ++j) {
                    const int64_t o = tk.a + j;
                    float lo = INFINITY, hi = -INFINITY;
                    if (act) {
                        const int64_t g = o / R.o2g;
                        if (g != g_prev) {
                            inv = cle_rel_scale(rels, R, mins, maxs, g * R.i2 + i, is_signed, eps, smin, smax).inv;
                            g_prev = g;
                        }
                        DFQ_GLOBAL float* p = (DFQ_GLOBAL float*)(R.w2 + o * rowlen + i * R.khw2);
                        for (int64_t k = 0; k < R.khw2; ++k) {
                            const float y = p[k] * inv;
                            p[k] = y;
                            lo = fminf(lo, y);
                            hi = fmaxf(hi, y);
                        }
                    }
                    float a = lo, b = hi;
                    cle_wave_minmax(a, b);
                    if (lane == 0) {
                        red[0][wv][j] = a;
                        red[1][wv][j] = b;
                    }
                }
                __syncthreads();
                if (threadIdx.x < tk.b - tk.a) {
                    const int j = threadIdx.x;
                    float a = red[0][0][j], b = red[1][0][j];
                    for (int w = 1; w < kThreads / 64; ++w) {
                        a = fminf(a, red[0][w][j]);
                        b = fmaxf(b, red[1][w][j]);
                    }
                    const int64_t off = rels[R.fuse_next].moff + tk.a + j;
                    atomicMin(&mins[off], enc_ord(a));
                    atomicMax(&maxs[off], enc_ord(b));
                }
            }
            __syncthreads();   // red / rows are reused by the next task
        } else if (tk.kind == kApplyW2Tile) {   // rows [a, b) of W2, one thread per column
            const int64_t rowlen = R.i2 * R.khw2;
            const bool one_group = (tk.a / R.o2g) == ((tk.b - 1) / R.o2g);
            for (int64_t i = tk.c0 + threadIdx.x; i < tk.c1; i += kThreads) {
                if (one_group && R.khw2 == 1) {   // 1x1 / Linear: the tile's column, loads first
                    float v[kColTileRows];
#pragma unroll
                    for (int j = 0; j < kColTileRows; ++j)
                        if (tk.a + j < tk.b) v[j] = ((DFQ_GLOBAL float*)R.w2)[(tk.a + j) * rowlen + i];
                    const float inv = cle_rel_scale(rels, R, mins, maxs, (tk.a / R.o2g) * R.i2 + i, is_signed, eps, smin,
                                                smax).inv;
                    ((DFQ_GLOBAL float*)R.w2)[tk.a * rowlen + i] = v[0] * inv;
                    DFQ_CLE_TL_MARK(0)   // the column's loads and its scale have landed
#pragma unroll
                    for (int j = 1; j < kColTileRows; ++j)
                        if (tk.a + j < tk.b) ((DFQ_GLOBAL float*)R.w2)[(tk.a + j) * rowlen + i] = v[j] * inv;
                    DFQ_CLE_TL_MARK(1)
                    continue;
                }
                int64_t g_prev = -1;
                float inv = 0.f;
                for (int64_t o = tk.a; o < tk.b; ++o) {
                    const int64_t g = o / R.o2g;
                    if (g != g_prev) {
                        inv = cle_rel_scale(rels, R, mins, maxs, g * R.i2 + i, is_signed, eps, smin, smax).inv;
                        g_prev = g;
                    }
                    DFQ_GLOBAL float* p = (DFQ_GLOBAL float*)(R.w2 + o * rowlen + i * R.khw2);
                    for (int64_t k = 0; k < R.khw2; ++k) p[k] = p[k] * inv;
                }
            }
        } else {
            // lagged schedule: the per-channel vectors before this iteration's
            // multiply, and the iteration that saved them (per task), for the
            // rollback of a speculative iteration (cle_loop_rollback_kernel)
            if (vtag && threadIdx.x == 0) vtag[t] = iter;
            for (int64_t c = tk.a + threadIdx.x; c < tk.b; c += kThreads) {
                const CleScale cs = cle_rel_scale(rels, R, mins, maxs, c, is_signed, eps, smin, smax);
                if (vsave) {
                    float* v = vsave + 2 * R.moff;   // [b1 | bnw | bnb | sacc] x c1
                    if (R.b1) v[c] = R.b1[c];
                    if (R.bnw) v[R.c1 + c] = R.bnw[c];
                    if (R.bnb) v[2 * R.c1 + c] = R.bnb[c];
                    if (R.sacc) v[3 * R.c1 + c] = R.sacc[c];
                }
                if (R.b1) R.b1[c] = R.b1[c] * cs.s;
                if (R.bnw) R.bnw[c] = R.bnw[c] * cs.s;
                if (R.bnb) R.bnb[c] = R.bnb[c] * cs.s;
                if (R.sacc) R.sacc[c] = (R.sacc_init && first_iter) ? cs.s : R.sacc[c] * cs.s;
            }
        }
#ifdef DFQ_DIAGNOSTICS
        if (tl_on) {   // the last executed iteration's times remain
            __syncthreads();   // the block's task is done (timing only)
            if (threadIdx.x == 0) {
                uint32_t hw, xcc;
                asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
                asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
                uint64_t* r = g_cle_tl + 4 * t;
                r[0] = tl_start;
                r[1] = __builtin_amdgcn_s_memrealtime();
                r[2] = tl_sub ? tl_sub : (((uint64_t)xcc << 32) | hw);
                r[3] = (uint64_t)tk.kind | ((uint64_t)tk.rel << 8) | ((uint64_t)(tk.b - tk.a) << 24);
            }
        }
#endif
    }
}

// The metric's fp32 sums (torch.mean's vectorized_inner_sum over one chunk) as a
// fixed tree.  A chunk of len elements is 32 streams (s = 8k + l: 8 vector lanes x
// ILP 4; stream element i is chunk element 32i + s) of sz = len/32 elements, each
// a 4-level cascade with 16-element level-0 blocks (step 2^4 for every chunk below
// 16M elements).  One level-1 group of all 32 streams is 8192 CONTIGUOUS elements:
//   * cle_tiles_body: one workgroup per 8192-element tile: |W - snap| (snap := W
//     on the way), 512 threads-worth of level-0 block sums, then 32 level-1 sums
//     -> b1buf; the chunk's remainder (partial group, level-0 tail, row_sum tail
//     vectors, scalar tail) is one more "tail tile";
//   * cle_chunk_sum_with: one wave per chunk finishes the cascade in ATen's order
//     (level 2/3, a0 += a1 += a2 += a3, ILP, lanes, scalar tail).
// (kCleTile, kCleTailWords and the tile's record CleUnit: dfq_cle_plan.h)

// Before the first iteration, ONE launch instead of six fills, a state upload and
// the snapshot kernel: both parities' range words armed (mins = 0xFF.., maxs = 0;
// layout [parity][mins M | maxs M]), the chunk sums and arrival counters zeroed,
// the rollback tags set to -1, the loop state from the launch argument, and
// snap := W (one workgroup per metric tile; the chunks of < 8 elements by block 0).
__global__ void __launch_bounds__(kThreads)
cle_loop_init_kernel(const CleLayer* __restrict__ layers, const CleChunk* __restrict__ chunks, int64_t nchunks,
                     const CleUnit* __restrict__ units, int64_t nunits, uint32_t* __restrict__ rng, int64_t M,
                     float* __restrict__ part, int64_t npart, uint32_t* __restrict__ cnt, int64_t ncnt,
                     int32_t* __restrict__ vtag, int64_t nvtag, CleState* __restrict__ st, CleState init) {
    const int64_t gt = (int64_t)blockIdx.x * kThreads + threadIdx.x, gs = (int64_t)gridDim.x * kThreads;
    for (int64_t i = gt; i < 4 * M; i += gs) rng[i] = ((i / M) & 1) ? 0u : 0xFFFFFFFFu;
    for (int64_t i = gt; i < npart; i += gs) part[i] = 0.f;
    for (int64_t i = gt; i < ncnt; i += gs) cnt[i] = 0u;
    for (int64_t i = gt; i < nvtag; i += gs) vtag[i] = -1;
    if (gt == 0) *st = init;
    for (int64_t u = blockIdx.x; u < nunits; u += gridDim.x) {
        const CleUnit un = units[u];
        const CleChunk ch = chunks[un.chunk];
        const CleLayer Ly = layers[ch.layer];
        const int64_t nb1 = (ch.len / 32) / 256;
        const int64_t e0 = (int64_t)un.tile * 8192;
        const int64_t e1 = un.tile < nb1 ? e0 + 8192 : ch.len;
        for (int64_t i = e0 + threadIdx.x; i < e1; i += kThreads) Ly.snap[ch.c0 + i] = Ly.w[ch.c0 + i];
    }
    if (blockIdx.x == 0)
        for (int64_t k = 0; k < nchunks; ++k) {
            const CleChunk ch = chunks[k];
            if (ch.len >= 8) continue;
            const CleLayer Ly = layers[ch.layer];
            for (int64_t i = threadIdx.x; i < ch.len; i += kThreads) Ly.snap[ch.c0 + i] = Ly.w[ch.c0 + i];
        }
}


// Metric tiles taken by blocks blk, blk + nblk, ... (d: kCleTile + kCleTailWords
// floats of LDS, b0: 512).
struct CleNoUnitHook {
    __device__ void operator()(const CleUnit&, const CleChunk&, int64_t) const {}
};

// hook(unit, chunk, nb1) runs after each unit (LDS free again).  (Tried on the
// snapshot stores: issued after the unit's arrival -- out of the arrival's
// vmcnt(0) drain -- no faster, tiles slower, 84 B of spills (cle_ab_r04p);
// non-temporal, the same (cle_ab_r04z).)
template <class Hook = CleNoUnitHook>
__device__ __forceinline__ void cle_tiles_body(const CleLayer* __restrict__ layers, const CleChunk* __restrict__ chunks,
                                               const int64_t* __restrict__ b1off, const CleUnit* __restrict__ units,
                                               int64_t nunits, float* __restrict__ b1buf, float* __restrict__ tailbuf,
                                               int64_t blk, int64_t nblk, float* d, float* b0, Hook hook = Hook()) {
    const int tid = threadIdx.x;
    for (int64_t u = blk; u < nunits; u += nblk) {
        const CleUnit un = units[u];
        const CleChunk ch = chunks[un.chunk];
        const CleLayer Ly = layers[ch.layer];
        const DFQ_GLOBAL float* __restrict__ w = (const DFQ_GLOBAL float*)(Ly.w + ch.c0);
        DFQ_GLOBAL float* __restrict__ sn = (DFQ_GLOBAL float*)(Ly.snap + ch.c0);
        const int64_t len = ch.len, sz = len / 32, vs = len / 8;
        const int64_t nb1 = sz / 256;
        const bool full = un.tile < nb1;
        const int64_t e0 = (int64_t)un.tile * kCleTile;
        const int64_t cnt = full ? kCleTile : len - e0;
        if (full) {
            // level 0 straight from the loads: thread t owns (block m, stream s) for
            // q = t and t + 256; its 16 elements 32 (16 m + j) + s sit at stride 32,
            // so each load instruction covers whole 128-B lines across the lanes,
            // and the 16-term sum runs in ATen's order in registers (32 loads in
            // flight per thread, no LDS staging of |W - W_prev|)
            float xs[2][16], ys[2][16];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int q = tid + h * kThreads;
                const int64_t base = e0 + 32 * (16 * (q >> 5)) + (q & 31);
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    xs[h][j] = w[base + 32 * j];
                    ys[h][j] = sn[base + 32 * j];
                }
            }
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int q = tid + h * kThreads;
                const int64_t base = e0 + 32 * (16 * (q >> 5)) + (q & 31);
                float a = 0.f;
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    a += fabsf(xs[h][j] - ys[h][j]);
                    sn[base + 32 * j] = xs[h][j];
                }
                b0[q] = a;   // b0[m * 32 + s]
            }
            __syncthreads();
            if (tid < 32) {   // level 1
                float a = 0.f;
#pragma unroll
                for (int m = 0; m < 16; ++m) a += b0[m * 32 + tid];
                st_coh(b1buf + b1off[un.chunk] + (int64_t)un.tile * 32 + tid, a);
            }
        } else {
            for (int64_t e = tid; e < cnt; e += 8 * kThreads) {   // |W - W_prev|, snap := W; 8 loads in flight
                float x[8], y[8];
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (e + u * kThreads < cnt) {
                        x[u] = w[e0 + e + u * kThreads];
                        y[u] = sn[e0 + e + u * kThreads];
                    }
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (e + u * kThreads < cnt) {
                        d[e + u * kThreads] = fabsf(x[u] - y[u]);
                        sn[e0 + e + u * kThreads] = x[u];
                    }
            }
            __syncthreads();
            const int64_t ni = sz - nb1 * 256;   // stream elements left: rem_b0 blocks + tail0
            const int64_t rem_b0 = ni / 16, tail0 = ni % 16;
            float* tb = tailbuf + (int64_t)un.chunk * kCleTailWords;
            if (tid < 32) {
                float a1p = 0.f;
                for (int64_t m = 0; m < rem_b0; ++m) {
                    float a = 0.f;
                    for (int j = 0; j < 16; ++j) a += d[32 * (16 * m + j) + tid];
                    a1p += a;
                }
                float a0t = 0.f;
                for (int64_t j = 0; j < tail0; ++j) a0t += d[32 * (16 * rem_b0 + j) + tid];
                float p = a0t;   // a0 += a1 (a2 and a3 follow in the combine)
                p += a1p;
                st_coh(tb + tid, p);
            } else if (tid < 64) {   // raw row_sum-tail vectors (v in [4sz, vs)) and scalar tail
                const int t = tid - 32;
                const int64_t nv = vs - 4 * sz;
                if (t < 24 && t < nv * 8) st_coh(tb + 32 + t, d[8 * (4 * sz) + t - e0]);
                if (t < 8 && t < len - 8 * vs) st_coh(tb + 56 + t, d[8 * vs + t - e0]);
            }
        }
        __syncthreads();   // LDS reused by the next unit
        hook(un, ch, nb1);
    }
}

constexpr int kCleTilesLds = kCleTile + kCleTailWords + 512;
constexpr int kCleRangeLds = 2 * kThreads * kTileMaxKhw;

// One chunk's sum from its tiles' level-1 sums and tail words (one wave; the
// result on every lane): the rest of the cascade, the ILP and lane combines and
// the scalar tail, in ATen's order.  Coherent loads: other blocks wrote b1 / tb.
template <class LdB1, class LdTb>
__device__ __forceinline__ float cle_chunk_sum_with(const CleChunk& ch, LdB1&& b1, LdTb&& tb, int lane) {
    const int64_t len = ch.len;
    const int64_t sz = len / 32, vs = len / 8;
    const int64_t nb1 = sz / 256, nb2 = nb1 / 16, rem_b1 = nb1 % 16;
    float fa = 0.f;
    float p = 0.f;
    if (lane < 32) {
        float a3 = 0.f;
        for (int64_t r = 0; r < nb2; ++r) {
            float b2 = 0.f;
            for (int q = 0; q < 16; ++q) b2 += b1((r * 16 + q) * 32 + lane);
            a3 += b2;
        }
        float a2p = 0.f;
        for (int64_t q = 0; q < rem_b1; ++q) a2p += b1((nb2 * 16 + q) * 32 + lane);
        p = tb(lane);   // a0 + a1
        p += a2p;
        p += a3;
    }
    // the combine on every lane, the 32 stream partials read by readlane (uniform
    // values: no 32-register array, no LDS permute per partial)
    auto ps = [&](int s) { return rl_f(p, s); };
    for (int64_t e = 0; e < len - 8 * vs; ++e) fa += tb(56 + e);   // scalar tail first
    const int64_t nv = vs - 4 * sz;
    for (int l = 0; l < 8; ++l) {
        float p0 = ps(l);
        for (int64_t v = 0; v < nv; ++v) p0 += tb(32 + v * 8 + l);   // row_sum tail into p0
        p0 += ps(l + 8);
        p0 += ps(l + 16);
        p0 += ps(l + 24);
        fa += p0;
    }
    return fa;
}

__device__ __forceinline__ float cle_chunk_sum(const CleChunk& ch, const float* b1, const float* tb, int lane) {
    const DFQ_GLOBAL float* g1 = (const DFQ_GLOBAL float*)b1;
    const DFQ_GLOBAL float* gt = (const DFQ_GLOBAL float*)tb;
    return cle_chunk_sum_with(ch, [g1](int64_t i) { return ld_coh(g1 + i); }, [gt](int64_t i) { return ld_coh(gt + i); },
                              lane);
}

// Tiny chunk (< 8 elements, no tiles): scalar row_sum of |W - snap| on lane 0, snap := W.
__device__ __forceinline__ float cle_tiny_chunk_sum(const CleLayer* __restrict__ layers, const CleChunk& ch) {
    const CleLayer Ly = layers[ch.layer];
    float* w = Ly.w + ch.c0;
    float* sn = Ly.snap + ch.c0;
    return aten_inner_sum([&](int64_t e) {
        const float x = w[e];
        const float dd = fabsf(x - sn[e]);
        sn[e] = x;
        return dd;
    }, ch.len);
}

// numpy pairwise float64 sum (identity 0 + pairwise_sum), as np.sum(diff_list).
// numpy's pairwise leaf: n <= 128 values, 8 accumulators.
template <class P>   // P: a typed (LDS / global) pointer to the values
__device__ __forceinline__ double np_pairwise_leaf(P x, int64_t n) {
    if (n < 8) {
        double res = 0.;
        for (int64_t i = 0; i < n; ++i) res += x[i];
        return res;
    }
    double r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = x[j];
    int64_t i;
    for (i = 8; i < n - (n % 8); i += 8)
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] += x[i + j];
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += x[i];
    return res;
}

// numpy's recursion (blocks of <= 128 with 8 accumulators; split at n/2 rounded
// down to a multiple of 8) as an explicit post-order walk on one thread; a single
// leaf (every model here: <= 128 target layers) skips the frame stack.  The
// stack (kNpFrames frames) lives in the caller's LDS (`stack`: >= kNpStackFloats
// floats, 8-B aligned), so the kernel needs no scratch memory.
struct NpFrame {
    int64_t o, n;
    int64_t state;
};
constexpr int kNpFrames = 48;
constexpr int kNpStackFloats = kNpFrames * (int)(sizeof(NpFrame) + sizeof(double)) / 4;
template <class P>
__device__ double np_pairwise(P a, int64_t n, float* stack) {
    if (n <= 128) return 0. + np_pairwise_leaf(a, n);
    NpFrame* fr = reinterpret_cast<NpFrame*>(stack);
    double* acc = reinterpret_cast<double*>(fr + kNpFrames);
    int fp = 0, ap = 0;
    fr[fp++] = {0, n, 0};
    while (fp > 0) {
        NpFrame& f = fr[fp - 1];
        if (f.n <= 128) {
            acc[ap++] = np_pairwise_leaf(a + f.o, f.n);
            --fp;
        } else if (f.state == 0) {
            int64_t n2 = f.n / 2;
            n2 -= n2 % 8;
            f.state = 1;
            const NpFrame left{f.o, n2, 0}, right{f.o + n2, f.n - n2, 0};
            fr[fp++] = right;   // evaluated second
            fr[fp++] = left;    // evaluated first
        } else {
            const double right = acc[--ap];
            const double left = acc[--ap];
            acc[ap++] = left + right;
            --fp;
        }
    }
    return 0. + acc[0];   // add.reduce starts from the identity
}

// Per-layer fp32 mean from the chunk sums (final_reduce over the 8-slot buffer,
// then / n), np.sum over layers, history and the stop rule.  One block.
// kLeafOnly: nl <= 128 (numpy's pairwise sum is one leaf) -- no frame stack, so
// no scratch in the persistent kernel
// kCoherent: the chunk sums come from other blocks of the same launch (agent-
// coherent loads); else from an earlier launch (plain loads).
template <bool kLeafOnly = false, bool kCoherent = false>
__device__ __forceinline__ void cle_final_body(const CleLayer* __restrict__ layers, int32_t nl,
                                               const float* __restrict__ part, int32_t S, double* __restrict__ means,
                                               double* __restrict__ hist, CleState* __restrict__ st, double* sm,
                                               float* part_lds = nullptr, float* np_stack = nullptr,
                                               uint32_t* hflag = nullptr) {
    // The stop rule's inputs in one parallel pass of loads into LDS (part_lds): the
    // chunk sums, the layers' {(float)n, serial} and the state's 10 words.  Read
    // where they are used instead, they were dependent round trips of a serial
    // stop rule (7.6 us, DFQ_CLE_TL, the last launch's block timeline); loaded
    // into registers up front, they pushed the kernel past its 128 VGPRs.
    // Nothing else writes the state during this launch.
#ifdef DFQ_DIAGNOSTICS
    uint64_t* tlm = (kCoherent && threadIdx.x == 0 && g_cle_tl2) ? g_cle_tl2 + 4 * kCleTl2Fin : nullptr;
#endif
    constexpr int kStateWords = (int)(sizeof(CleState) / 4);
    static_assert(sizeof(CleState) % 4 == 0, "CleState: whole 4-B words");
    const int64_t nps = (int64_t)nl * (S + 2);
    DFQ_LDS float* pls = (DFQ_LDS float*)part_lds;   // typed: LDS / global accesses, not flat
    if (part_lds) {
        for (int64_t i = threadIdx.x; i < nps + kStateWords; i += blockDim.x) {
            const DFQ_GLOBAL float* src = (const DFQ_GLOBAL float*)(i < nps ? part + i
                                                                           : reinterpret_cast<const float*>(st) + (i - nps));
            pls[i] = kCoherent ? ld_coh(src) : *src;
        }
        __syncthreads();
    }
#ifdef DFQ_DIAGNOSTICS
    if (tlm) tlm[2] = __builtin_amdgcn_s_memrealtime();
#endif
    DFQ_LDS double* ms = (DFQ_LDS double*)sm;
    DFQ_GLOBAL double* mg = (DFQ_GLOBAL double*)means;
    const bool m_lds = nl <= 1024;
    double* m = m_lds ? sm : means;
    // (generic pointers here: the typed two-path form spilled 48-60 B in the loop
    // kernel; wave 0 has no stores outstanding at this point, so the flat loads
    // cost no extra wait)
    for (int l = threadIdx.x; l < nl; l += blockDim.x) {
        // serial: sum = 0 + (0 + slot); two_pass_reduction: its S-slot buffer
        // (at::get_num_threads()) summed as a contiguous reduction
        const float* pl = (part_lds ? part_lds : part) + (int64_t)l * S;
        auto ld = [&](int64_t e) { return (part_lds || !kCoherent) ? pl[e] : ld_coh(pl + e); };
        const float* lm = part_lds ? part_lds + (int64_t)nl * S + 2 * l : nullptr;
        const bool serial = lm ? lm[1] != 0.f : layers[l].nt == 1;
        const float sum = serial ? 0.f + (0.f + ld(0)) : 0.f + aten_inner_sum([&](int64_t e) { return ld(e); }, S);
        m[l] = (double)(sum / (lm ? lm[0] : (float)layers[l].n));
    }
    __syncthreads();
#ifdef DFQ_DIAGNOSTICS
    if (tlm) tlm[3] = __builtin_amdgcn_s_memrealtime();
#endif
    if (threadIdx.x == 0) {
        CleState s0;
        if (part_lds) {
            __builtin_memcpy(&s0, part_lds + nps, sizeof(CleState));
        } else {
            s0 = *st;
        }
        double dt = 0.0;
        if constexpr (kLeafOnly) {
            dt = nl > 0 ? 0. + (m_lds ? np_pairwise_leaf(ms, nl) : np_pairwise_leaf(mg, nl)) : 0.0;
        } else {
            dt = nl > 0 ? (m_lds ? np_pairwise(ms, nl, np_stack) : np_pairwise(mg, nl, np_stack)) : 0.0;
        }
        const int it = s0.iters;
        hist[it] = dt;
        int ic = s0.iter_count;
        double diff = s0.diff;
        if (fabs(diff - dt) > 1e-9) {
            ic = 0;
            diff = dt;
        } else {
            ic += 1;
        }
        const bool cont = (diff > s0.thr) && (ic < s0.count);
        const int done = (!cont || it + 1 >= s0.max_iters) ? 1 : 0;
        st->iters = it + 1;
        st->iter_count = ic;
        st->diff = diff;
        st->done = done;
        // the host's copy of the stop rule (pinned host memory; a system-scope
        // vector store), written every iteration: the loop's host side polls it for
        // the stop and paces its enqueue by it (cle_run_locked)
        if (hflag)
            __hip_atomic_store(hflag, ((uint32_t)(it + 1) << 1) | (uint32_t)done, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_SYSTEM);
        // (A launched run's caller gate opens behind the rollback launch that follows
        // the loop -- cle_run_locked -- not here: the lagged schedule's next
        // iteration may be running speculatively beside this stop rule.)
    }
}

// The metric tiles (+ the next iteration's ranges) with the chunk combine and the
// stop rule folded in: the block that finishes a chunk's last tile sums that
// chunk, and the block that finishes the last chunk runs the stop rule -- two
// launches fewer per iteration.  Hand-offs between blocks go through
// agent-coherent stores / loads and monotone arrival counters (cnt: one per
// chunk, then one for the launch; zeroed by plan_run, iteration i's target is
// (i + 1) x members); the ordering of the hand-offs: handoff_arrive.
// Arrival on a block-to-block hand-off counter (chunk tiles -> chunk sum -> stop
// rule).  The words handed over (level-1 sums, chunk tails, chunk sums) are
// written with agent-coherent stores (st_coh) and read with agent-coherent loads
// (ld_coh), and the caller has drained its stores (s_waitcnt vmcnt(0)) first.
// The sc1 hand-off form MI355X_MICROARCH.md lists as valid (section "visibility",
// Valid forms, table row 1; cdna_hip_programming.md Guideline 16): every
// handed-off word stored sc1 and drained by every storing wave before ONE lane's
// agent-scope counter add (behind the workgroup barrier), the workgroup whose add
// came last told by the returned value, and every load of the words an sc1 load to
// registers issued after that add returned (the other waves after a workgroup
// barrier).  No L2 write-back.  (The memory model's release / acquire form gave the
// same results 50 % slower: each release writes the arriving block's XCD L2 back,
// profiles/r03/cle_ab_d.jsonl.)
__device__ __forceinline__ bool handoff_arrive(uint32_t* c, uint32_t target) {
    return __hip_atomic_fetch_add(c, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == target;
}

// Blocks of the lagged schedule's stop rule: one wave per chunk sum (host and kernel).
__host__ __device__ inline int64_t cle_stop_blocks(int64_t nchunks) {
    return nchunks > 0 ? (nchunks + kThreads / 64 - 1) / (kThreads / 64) : 1;
}

struct CleFin {
    uint32_t* cnt;
    float* part;
    double* means;
    double* hist;
    int64_t nchunks, nbig;   // all chunks / chunks with tiles (len >= 8)
    int32_t S, nl;
    int32_t last;            // the round-4 schedule's tiles-only launch (the stop rule's block without tiles)
    uint32_t* hflag;         // pinned host word: (iterations << 1) | done, or null
    int32_t stop_arrival;    // 1: the stop rule runs at the iteration's last tile arrival (round-4 schedule);
                             // 0: as a block of its own (lagged schedule, stop_it)
};

// One launch of iteration group g.  The group's launches k < steps run the
// rescale tasks of chain step k of iteration g (blocks [0, nab)); beside them run
// metric tiles and next-iteration range tasks placed in this launch by the
// planner (dfq_cle_plan_create): "own" ones of iteration g and "prev" ones of
// iteration g - 1 (the lagged schedule: a tensor's tiles and ranges go anywhere
// after its last rescale of iteration g-1 and before its first rescale of
// iteration g).  Blocks: [0, nab) rescale, then nto own tiles, ntp prev tiles,
// nro own ranges, nrp prev ranges.
//
// Lagged schedule: iteration g's first steps run before iteration g-1's stop
// rule (the last tile arrival) has decided -- speculatively.  When that stop rule
// says done, iteration g is discarded: its rescale blocks skip from then on
// (st->done) and cle_loop_rollback_kernel restores the weights from the snapshots
// (= iteration g-1's weights: every tile of g-1 ran before any rescale of g
// touched its tensor) and the per-channel vectors from the saves of iteration g.
// Tiles of iteration i are placed after every tile of i-1 (the planner's band),
// so they start only after stop(i-1): a tile never runs for a discarded
// iteration, and its snapshot writes and arrivals are always real.  Every block
// takes its iteration, parity and arrival round from the launch argument g,
// never from st (the stop rule advances st mid-launch).
static_assert(kCleTilesLds - kCleTile >= kNpStackFloats, "np_pairwise's frame stack after the tile area");
union CleStepLds {
    CleApplyLds apply;
    float tiles[kCleTilesLds > kCleRangeLds ? kCleTilesLds : kCleRangeLds];
};

// Block order of a step launch: metric tiles (the launch's longest blocks: 8,192
// elements, 12 B each), rescale tasks, the stop rule, range tasks.  MobileNetV2's
// first launch holds 1,994 blocks, about two rounds of resident ones; with the tiles
// last they started in the second round and set the launch's tail.  CLE 2.27-2.29
// against 2.39-2.40 ms, ResNet-50 (tiles in a launch of their own) unchanged
// (profiles/r06/cle_ab_tiles_first_r06t/u.jsonl; tiles then ranges first: 2.36).
// DFQ_CLE_TILES_FIRST=0 (diagnostics): the round-6 order, tiles after the stop rule.
constexpr bool kCleTilesFirst = true;
#ifdef DFQ_DIAGNOSTICS
__device__ int g_cle_tiles_first = kCleTilesFirst ? 1 : 0;
#endif

// POS = false (no position-parallel 3x3 rescale tiles): capped at 128 VGPRs,
// 4 waves per SIMD like the rescale body alone
// (POS capped at 3 waves per SIMD -- 168 VGPRs, 124 B of spills -- measured slower:
// profiles/r04/cle_ab_r04t.jsonl)
template <bool POS>
#ifndef DFQ_CLE_POS_WAVES   // waves per SIMD asked of the POS kernel (1: no cap); A/B as above
#define DFQ_CLE_POS_WAVES 1
#endif
__global__ void __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(POS ? DFQ_CLE_POS_WAVES : 4)))
cle_loop_step_kernel(const CleRel* __restrict__ rels, const CleTask* __restrict__ atasks, int64_t a0, int64_t a1,
                     int64_t nab, uint32_t* __restrict__ rng, int64_t M, int is_signed, float eps, double smin,
                     double smax, const CleLayer* __restrict__ layers, const CleChunk* __restrict__ chunks,
                     const int64_t* __restrict__ b1off, const CleUnit* __restrict__ units, int64_t uo, int64_t nuo,
                     int64_t nto, int64_t up, int64_t nup, int64_t ntp, float* __restrict__ b1buf,
                     float* __restrict__ tailbuf, const CleTask* __restrict__ rtasks, int64_t ro, int64_t nro_t,
                     int64_t nro, int64_t rp, int64_t nrp_t, int64_t nrp, CleFin F, CleState* __restrict__ st,
                     int32_t g, float* __restrict__ vsave, int32_t* __restrict__ vtag, int32_t stop_it) {
    __shared__ CleStepLds L;
    __shared__ int flag;
    if (st->done) return;
    int64_t blk = blockIdx.x;
#ifdef DFQ_DIAGNOSTICS
    const bool tiles_first = g_cle_tiles_first != 0;   // DFQ_CLE_TILES_FIRST (A/B)
#else
    constexpr bool tiles_first = kCleTilesFirst;
#endif
    // lagged schedule: the stop rule of iteration stop_it takes cle_stop_blocks blocks
    // (its chunk sums, then the stop rule at their last arrival)
    const int64_t nstop = stop_it >= 0 ? cle_stop_blocks(F.nchunks) : 0;
    if (tiles_first) {   // block order: metric tiles, rescale tasks, the stop rule, ranges
        const int64_t ns = nab + nstop, ntl = nto + ntp;
        if (blk < ntl) blk += ns;
        else if (blk < ntl + ns) blk -= ntl;
    }
    if (blk < nab) {   // this step's rescale tasks (iteration g)
        cle_apply_body<POS>(rels, atasks, a0, a1, rng, M, g & 1, g == 0, is_signed, eps, smin, smax, blk, nab, L.apply,
                            vsave, vtag, g);
        return;
    }
    blk -= nab;
#ifdef DFQ_DIAGNOSTICS
    const bool tl2 = g_cle_tl2 != nullptr && blk < kCleTl2Fin && (g_cle_tl2_a0 < 0 || (a0 == g_cle_tl2_a0 && nab > 0));
    const uint64_t tl2_start = tl2 ? __builtin_amdgcn_s_memrealtime() : 0;
    auto tl2_rec = [&](int role) {
        if (tl2 && threadIdx.x == 0) {
            uint64_t* r = g_cle_tl2 + 4 * blk;
            r[0] = tl2_start;
            r[1] = __builtin_amdgcn_s_memrealtime();
            r[2] = (uint64_t)role;
        }
    };
#else
    auto tl2_rec = [](int) {};
#endif
    float* lds = L.tiles;
    // The last arrival of the iteration: tiny chunks' sums, then the per-layer
    // means, the history and the stop rule.
    auto finish = [&]() {
#ifdef DFQ_DIAGNOSTICS
        const uint64_t tf0 = __builtin_amdgcn_s_memrealtime();
#endif
        if (threadIdx.x == 0 && F.nchunks > F.nbig)   // tiny chunks exist (fallback schedule only)
            for (int64_t k = 0; k < F.nchunks; ++k) {
                const CleChunk c2 = chunks[k];
                if (c2.len < 8) st_coh(F.part + (int64_t)c2.layer * F.S + c2.t, 0.f + cle_tiny_chunk_sum(layers, c2));
            }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        // the chunk sums, layer sizes and state words (cle_final_body) after the means
        const bool stage_part = (int64_t)F.nl * (F.S + 2) + (int64_t)(sizeof(CleState) / 4) + 2048 <= kCleTile;
        if (F.nl <= 128)   // numpy's pairwise sum over the layer means is one leaf
            cle_final_body<true, true>(layers, F.nl, F.part, F.S, F.means, F.hist, st, reinterpret_cast<double*>(lds),
                                       stage_part ? lds + 2048 : nullptr, nullptr, F.hflag);
        else   // the frame stack after the metric tile area (free: this block's units are done)
            cle_final_body<false, true>(layers, F.nl, F.part, F.S, F.means, F.hist, st,
                                        reinterpret_cast<double*>(lds), stage_part ? lds + 2048 : nullptr,
                                        lds + kCleTile, F.hflag);
#ifdef DFQ_DIAGNOSTICS
        if (tl2 && threadIdx.x == 0) {
            uint64_t* r = g_cle_tl2 + 4 * kCleTl2Fin;
            r[0] = tf0;
            r[1] = __builtin_amdgcn_s_memrealtime();
        }
#endif
    };
    if (stop_it >= 0) {   // lagged schedule: the stop rule of iteration stop_it
        if (blk < nstop) {
            // The iteration's chunk sums, one wave per chunk, from the level-1 sums and
            // tail words its tiles wrote in earlier launches (no tile of any iteration
            // runs in this launch: the stop rule's offset follows its iteration's
            // band and precedes the next iteration's; host structure checker); the
            // last block to arrive runs the stop rule.  The tiles themselves no longer
            // arrive anywhere (their chunk's last arrival summed the chunk: a store
            // drain, an arrival and a staged sum on the launch's longest blocks).
            // (Staging each wave's level-1 sums through LDS first measured the same:
            // profiles/r06/cle_lib_ab_stop_chunk_sums_staged_r06z.jsonl.)
            const int64_t c = blk * (kThreads / 64) + (threadIdx.x >> 6);
            if (c < F.nchunks) {
                const CleChunk ch = chunks[c];
                if (ch.len >= 8) {   // (tiny chunks: finish, thread 0)
                    const float fa = cle_chunk_sum(ch, b1buf + b1off[c], tailbuf + c * kCleTailWords, threadIdx.x & 63);
                    if ((threadIdx.x & 63) == 0) st_coh(F.part + (int64_t)ch.layer * F.S + ch.t, 0.f + fa);
                }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (threadIdx.x == 0)
                flag = handoff_arrive(F.cnt + F.nchunks, ((uint32_t)stop_it + 1u) * (uint32_t)nstop - 1u);
            __syncthreads();
            if (flag) finish();
            return;
        }
        blk -= nstop;
    }
    const int64_t ntiles = nto + ntp;
    if (blk >= ntiles) {   // next-iteration ranges of tensors final by now
        blk -= ntiles;
        const bool own = blk < nro;
        const int64_t b = own ? blk : blk - nro;
        // own: iteration g's tasks (ranges of g + 1); prev: iteration g - 1's (ranges of g)
        cle_range_body(rels, rtasks, own ? ro : rp, (own ? ro : rp) + (own ? nro_t : nrp_t), rng, M,
                       own ? (g + 1) & 1 : g & 1, b, own ? nro : nrp, L.tiles);
        tl2_rec(2);
        return;
    }
    const bool own = blk < nto;
    const int32_t it = own ? g : g - 1;                    // the tiles' iteration
    const int64_t tb = own ? blk : blk - nto;
    const int64_t tnb = own ? nto : ntp;
    const uint32_t round = (uint32_t)it + 1u;
    // Arrival on counter c (handoff_arrive); returns whether this block arrived last.
    auto arrive = [&](uint32_t* c, uint32_t members) -> bool {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (threadIdx.x == 0) flag = handoff_arrive(c, round * members - 1u);
        __syncthreads();
        return flag != 0;
    };
    if (F.nbig == 0) {   // no chunk has tiles (tiny or no target layers): the fallback launch's one block finishes
        if (own && tb == 0 && F.last) finish();
        return;
    }
    const uint32_t fin_members = (uint32_t)F.nbig;
    auto hook = [&](const CleUnit& un, const CleChunk& ch, int64_t nb1) {
        if (!arrive(F.cnt + un.chunk, (uint32_t)(nb1 + 1))) return;   // not the chunk's last tile
        {
            // the chunk's level-1 sums and tail words in one parallel pass of coherent
            // loads into LDS (free again: the unit is done), then one wave sums them
            const float* gb1 = b1buf + b1off[un.chunk];
            const float* gtb = tailbuf + (int64_t)un.chunk * kCleTailWords;
            const int64_t nw = 32 * nb1;
            const bool staged = nw + kCleTailWords <= kCleTile;
            if (staged) {
                DFQ_LDS float* ll = (DFQ_LDS float*)lds;
                const DFQ_GLOBAL float* g1 = (const DFQ_GLOBAL float*)gb1;
                for (int64_t i = threadIdx.x; i < nw; i += kThreads) ll[i] = ld_coh(g1 + i);
                if (threadIdx.x < kCleTailWords) ll[nw + threadIdx.x] = ld_coh((const DFQ_GLOBAL float*)gtb + threadIdx.x);
            }
            __syncthreads();
            if (threadIdx.x < 64) {
                const float fa = staged ? cle_chunk_sum_with(ch, [&](int64_t i) { return lds[i]; },
                                                             [&](int64_t i) { return lds[nw + i]; }, threadIdx.x)
                                        : cle_chunk_sum(ch, gb1, gtb, threadIdx.x);
                if (threadIdx.x == 0) st_coh(F.part + (int64_t)ch.layer * F.S + ch.t, 0.f + fa);
            }
        }
        if (F.stop_arrival && arrive(F.cnt + F.nchunks, fin_members)) finish();   // the iteration's last arrival
    };
    if (F.stop_arrival)   // round-4 schedule: chunk sums and the stop rule at the tiles' arrivals
        cle_tiles_body<decltype(hook)>(layers, chunks, b1off, units + (own ? uo : up), own ? nuo : nup, b1buf, tailbuf,
                                       tb, tnb, lds, lds + kCleTile + kCleTailWords, hook);
    else   // lagged schedule: the stop rule's launch sums the chunks (above)
        cle_tiles_body(layers, chunks, b1off, units + (own ? uo : up), own ? nuo : nup, b1buf, tailbuf, tb, tnb, lds,
                       lds + kCleTile + kCleTailWords);
#ifdef DFQ_DIAGNOSTICS
    if (tl2) {   // role 3: the block's unit was a chunk's tail tile
        const CleUnit un0 = units[(own ? uo : up) + tb];
        tl2_rec(un0.tile >= (chunks[un0.chunk].len / 32) / 256 ? 3 : 1);
    }
#else
    tl2_rec(1);
#endif
}

// After the loop: undo a speculative iteration (the lagged schedule's iteration
// A = st->iters, started before stop(A - 1) said done).  Weights: every target
// layer := its snapshot (iteration A - 1's weights; the tiles of A - 1 wrote it
// before any rescale of A touched the tensor).  Vectors (B1, BN fake weight / bias,
// S): restored from the saves of every per-channel task that ran in iteration A.
// Correct whether or not iteration A started: without it the weights equal their
// snapshots already and no save carries A.
__global__ void __launch_bounds__(kThreads)
cle_loop_rollback_kernel(const CleLayer* __restrict__ layers, int32_t nl, const CleRel* __restrict__ rels,
                         const CleTask* __restrict__ atasks, int64_t n_at, const float* __restrict__ vsave,
                         const int32_t* __restrict__ vtag, const CleState* __restrict__ st) {
    const int32_t A = st->iters;
    const int64_t gt = (int64_t)blockIdx.x * kThreads + threadIdx.x, gs = (int64_t)gridDim.x * kThreads;
    for (int32_t l = 0; l < nl; ++l) {
        const CleLayer Ly = layers[l];
        for (int64_t i = gt; i < Ly.n; i += gs) Ly.w[i] = Ly.snap[i];
    }
    for (int64_t t = blockIdx.x; t < n_at; t += gridDim.x) {
        const CleTask tk = atasks[t];
        if (tk.kind != kApplyChannels || vtag[t] != A) continue;
        const CleRel& R = rels[tk.rel];
        const float* v = vsave + 2 * R.moff;
        for (int64_t c = tk.a + threadIdx.x; c < tk.b; c += kThreads) {
            if (R.b1) R.b1[c] = v[c];
            if (R.bnw) R.bnw[c] = v[R.c1 + c];
            if (R.bnb) R.bnb[c] = v[2 * R.c1 + c];
            if (R.sacc) R.sacc[c] = v[3 * R.c1 + c];
        }
    }
}


// The caller's stream gate of a launched loop: one lane polls the signal word
// until the worker has written this run's generation behind the loop's last
// launch, sleeping between polls.  A CP wait packet (hipStreamWaitValue64) in
// the caller's queue measured 1.8x slower loops (MobileNetV2 CLE 2.73 -> 4.97 ms:
// the polling packet holds up the dispatch of the loop's queue), a running
// one-wave kernel costs nothing.  Bounded: past `limit` ticks of the 100 MHz
// clock (kCleGateSeconds: never reached by a loop that is running -- a
// MobileNetV2 loop takes milliseconds) it traps instead of returning, so a lost
// release cannot hang the queue and nothing queued behind the gate runs on weights
// a still-running loop is rescaling.  A loop that FAILS (a HIP error, the launch
// deadline) is not held back this way: the worker releases the gate behind
// whatever the loop enqueued, the caller's queued stages (absorption, the second
// fold, quantize, bias correction) run on the failed loop's weights, and the
// failure is raised at the join (Cross_layer_equal.wait(), which run_dfq,
// main_dfq and every read of the loop's results call), so those results are
// never returned as a success.
__global__ void __launch_bounds__(64) cle_caller_gate_kernel(const uint64_t* sig, uint64_t gen, uint64_t limit) {
    if (threadIdx.x != 0) return;
    const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
    while (__hip_atomic_load(sig, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) < gen) {
        if (__builtin_amdgcn_s_memrealtime() - t0 > limit) __builtin_trap();
        __builtin_amdgcn_s_sleep(32);
    }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
}
}  // namespace dfq
