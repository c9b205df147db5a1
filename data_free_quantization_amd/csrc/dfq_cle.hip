// Cross-layer equalization on the GPU (gfx950): the whole cross_layer_equalization
// loop of Cross_layer_equal.py:63-116 device-resident (dfq_cle_plan_*).
// Relations are grouped into independent chains (connected components of the
// tensors they touch) and the k-th relation of every chain runs in one launch;
// the per-iteration metric sum_l mean|W_l - W_l_prev| (fp32 torch.mean in ATen's
// reduction order, then numpy's pairwise float64 sum) and the stop rule are
// evaluated on the device.  The host enqueues iterations and polls the stop
// rule's word in pinned memory.  One relation at a time: dfq_cle_relation.hip.
// This file: the host runtime -- the plan's device tables, the per-device context and
// its pools, the iteration enqueue, run / launch / join -- and every launch of the
// loop's kernels (dfq_cle_kernels.h; the diagnostics task timeline: dfq_cle_timeline.h).
// The planner -- chains, tasks, metric chunks, placement, the structure cache and its
// checker -- is host-only code in dfq_cle_plan.cpp; dfq_cle_plan.h holds the records and
// constants both share, and the structure (CleStructure) a plan keeps and reads.
#include "dfq_cle_kernels.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <type_traits>
#include <new>
#include <vector>

using namespace dfq;

constexpr int32_t kCleHistCap = 1025;   // per-iteration diffs kept in the plan's tables

// The plan's device tables: ONE allocation, the host-built ones in front so that one
// host->device copy of [0, host_bytes) uploads them.  bind() is the single description:
// it names every table once, in layout order, with its element type (the member's), its
// count and whether the host builds it, and yields both the byte layout (host_bytes,
// total) and, for a base address (null: the layout only), the pointers.
struct CleTables {
    CleRel* rels = nullptr;
    CleTask *rtasks = nullptr, *atasks = nullptr;   // range / rescale tasks
    CleLayer* layers = nullptr;
    CleChunk* chunks = nullptr;
    CleUnit* units = nullptr;
    int64_t* b1off = nullptr;
    float* part = nullptr;        // [layers][slots], then per layer {(float)n, nt == 1}
    float* b1 = nullptr;           // level-1 sums, [chunk][nb1][32]
    float* tail = nullptr;         // [chunk][kCleTailWords]
    uint32_t* rng = nullptr;       // [2 parities][mins M | maxs M]
    double* means = nullptr;
    CleState* state = nullptr;
    double* hist = nullptr;        // kCleHistCap slots (longer histories: the device context's buffer)
    uint32_t* cnt = nullptr;       // tiles_fin arrival counters [nchunks + 1]
    float* vsave = nullptr;        // lagged: per-channel vectors before the iteration's multiply [2 M]
    int32_t* vtag = nullptr;       // ... and the iteration that saved them, per rescale task
    int64_t host_bytes = 0, total = 0;
    void bind(char* base, const CleStructure& S, int32_t slots) {
        constexpr bool kHost = true, kDevice = false;
        int64_t off = 0;
        auto table = [&](auto*& ptr, int64_t count, bool host_built) {
            using T = std::remove_reference_t<decltype(*ptr)>;
            ptr = base ? reinterpret_cast<T*>(base + off) : nullptr;
            off += round256((int64_t)sizeof(T) * std::max<int64_t>(count, 1));
            if (host_built) host_bytes = off;   // (every host-built table comes before the first device-only one)
        };
        const int64_t nl = (int64_t)S.layers.size(), nch = (int64_t)S.chunks.size();
        table(rels, (int64_t)S.R.size(), kHost);
        table(rtasks, (int64_t)S.rt.size(), kHost);
        table(atasks, (int64_t)S.at.size(), kHost);
        table(layers, nl, kHost);
        table(chunks, nch, kHost);
        table(units, (int64_t)S.units.size(), kHost);
        table(b1off, (int64_t)S.b1off.size(), kHost);
        // chunk sums (zeroed per run), then the layers' sizes: the stop rule stages both in one pass of loads
        table(part, (int64_t)(slots + 2) * nl, kHost);
        table(b1, 32 * S.nb1_total, kDevice);
        table(tail, kCleTailWords * nch, kDevice);
        table(rng, 4 * S.M, kDevice);
        table(means, nl, kDevice);
        table(state, 1, kDevice);
        table(hist, kCleHistCap, kDevice);
        table(cnt, nch + 1, kDevice);
        table(vsave, S.lagged ? 2 * S.M : 0, kDevice);
        table(vtag, S.lagged ? (int64_t)S.at.size() : 0, kDevice);
        if (!S.lagged) vsave = nullptr, vtag = nullptr;   // the kernels test the pointers
        total = off;
    }
};

struct dfq_cle_plan {
    // chains, steps, tasks, chunks, units and the placement: shared, read-only, by
    // every plan of the same shapes and tensor-sharing pattern (cle_structure_cached)
    std::shared_ptr<const CleStructure> S;
    CleTables t;                    // where this plan's copy of them, and its scratch, live on the device
    int32_t slots = 8;              // torch.mean's thread buffer (the reference run's thread count)
    double* d_hist = nullptr;       // this run's history (the tables' kCleHistCap slots, or the context's)
    uint32_t* d_flag = nullptr;     // the stop rule's host word (the device context's, set by run)
    uint64_t* d_sig = nullptr;      // a launched run: the caller's gate word and its generation
    uint64_t gen = 0;
    double smin = 1e-8, smax = 1e8;
    int32_t is_signed = 0;
    float eps = 0.f;
    void* d_tables = nullptr;       // every device table: ONE allocation (unless pooled)
    bool pooled = false;            // the tables live in the device context's pool
    void* d_snap_owned = nullptr;   // snapshots when the caller passed no workspace
    int dev = 0;
    struct CleAsync* async = nullptr;   // dfq_cle_plan_launch's worker and result
    bool abandoned = false;             // join gave up waiting for the launched loop
    bool timed = false;                 // dfq_cle_plan_set_timing: HIP events around the loop
    float loop_ms = -1.f;               // the last run's device time, first launch to last (timed runs)
    int32_t launched = 0;               // iteration groups the last run enqueued
    int32_t nl() const { return (int32_t)S->layers.size(); }
    int64_t nchunks() const { return (int64_t)S->chunks.size(); }
    int64_t nunits() const { return (int64_t)S->units.size(); }
};

// DFQ_CLE_TIMING: host-side phase times of create / run / destroy on stderr.
static bool cle_timing() {
    static const bool on = ab_env("DFQ_CLE_TIMING") != nullptr;
    return on;
}

// Per-device loop stream and pinned state word, shared by every plan of the
// process (creating and destroying them per call cost ~0.6 ms); plan_run holds
// the device's lock while it uses them.
struct CleDeviceCtx {
    std::mutex mu;
    hipStream_t st = nullptr;
    CleState* h_state = nullptr;   // pinned: the run's state
    uint32_t* h_flag = nullptr;    // pinned, written by the stop rule: (iterations << 1) | done
    uint32_t* d_flag = nullptr;    // its device address
    // Table pool: one plan at a time keeps its tables here (device + pinned upload
    // mirror), so a plan costs no hipMalloc / hipFree (hipFree waits for the whole
    // device) and its upload is an async DMA on the loop stream.
    char* d_pool = nullptr;
    size_t pool_cap = 0;
    char* h_pool = nullptr;
    size_t hpool_cap = 0;
    bool pool_busy = false;
    uint64_t pool_struct = 0;                      // CleStructure::id whose address-free tables the pool holds
    hipEvent_t pool_ev = nullptr;                  // behind the last upload from h_pool
    double* d_hist = nullptr;                      // histories longer than the tables' kCleHistCap
    int64_t hist_cap = 0;
    double* h_hist = nullptr;                      // pinned: the run's history comes back here
    int64_t h_hist_cap = 0;
    // asynchronous runs (dfq_cle_plan_launch): the signal word callers' streams
    // wait on and its last generation
    void* sig = nullptr;
    int sig_state = 0;                             // -1: the device cannot wait on a value
    uint64_t gen = 0;
    // The launched plan not yet joined (one per device at a time).  The rule:
    //  * read and written only with `mu` held, and only by callers' threads: launch sets it
    //    (in the lock scope that enqueues the gate); join, destroy and cle_ctx_acquire clear it;
    //  * nobody waits for a launched run while holding `mu` (its worker holds it all run long);
    //  * run and launch, which put a loop on `st` and may resize the history buffers,
    //    join it BEFORE taking `mu` (cle_ctx_acquire): its caller's stream is held
    //    behind the gate, hipFree / hipHostFree may wait for the whole device, and
    //    only the worker -- which needs `mu` -- opens that gate.
    // (A plan handle is one caller thread's at a time, as every handle of the C ABI:
    // the plan read here stays alive while it is waited for.)
    struct dfq_cle_plan* pending = nullptr;
    hipEvent_t in_ev = nullptr;                    // the caller's producers, for the loop stream
    struct CleWorker* worker = nullptr;            // drives launched runs
};
static CleDeviceCtx& cle_device_ctx(int dev) {
    static CleDeviceCtx ctx[64];
    return ctx[dev & 63];
}
static std::unique_lock<std::mutex> cle_ctx_acquire(CleDeviceCtx& ctx, bool join_pending);
// The loop stream and the pinned state word (caller holds ctx.mu).  Creating a
// stream can take milliseconds the first time, so dfq_preload does it up front.
static hipError_t cle_ctx_ready(CleDeviceCtx& ctx) {
    hipError_t e = hipSuccess;
    if (!ctx.st) {   // high priority: a hardware queue of its own (see dfq_cle_plan_launch)
        int least = 0, greatest = 0;
        e = hipDeviceGetStreamPriorityRange(&least, &greatest);
        if (e == hipSuccess) e = hipStreamCreateWithPriority(&ctx.st, hipStreamNonBlocking, greatest);
    }
    if (e == hipSuccess && !ctx.h_state) e = hipHostMalloc(&ctx.h_state, sizeof(CleState));
    if (e == hipSuccess && !ctx.h_flag) {
        e = hipHostMalloc(&ctx.h_flag, 64, hipHostMallocMapped | hipHostMallocCoherent);
        if (e == hipSuccess) e = hipHostGetDevicePointer(reinterpret_cast<void**>(&ctx.d_flag), ctx.h_flag, 0);
    }
    if (e == hipSuccess && !ctx.pool_ev) e = hipEventCreateWithFlags(&ctx.pool_ev, hipEventDisableTiming);
    if (e == hipSuccess && !ctx.in_ev) e = hipEventCreateWithFlags(&ctx.in_ev, hipEventDisableTiming);
    return e;
}

// Grows one of the context's buffers (pinned: host memory) to `cap` elements when it holds fewer
// than `need`: free (which may wait for the whole device), clear the capacity, allocate.
template <class T, class N>
static hipError_t cle_grow(T*& buf, N& have, N need, N cap, bool pinned) {
    if (have >= need) return hipSuccess;
    (void)(pinned ? hipHostFree(buf) : hipFree(buf));
    buf = nullptr;
    have = 0;
    const hipError_t e = pinned ? hipHostMalloc(&buf, sizeof(T) * cap, hipHostMallocDefault) : hipMalloc(&buf, sizeof(T) * cap);
    if (e == hipSuccess) have = cap;
    return e;
}
// The context's table pool for dev_bytes of tables and host_bytes of upload mirror
// (headroom: half again as much, so a slightly larger plan does not grow it
// again).  No plan holds the pool.
static hipError_t cle_pool_reserve(CleDeviceCtx& ctx, size_t dev_bytes, size_t host_bytes, bool headroom) {
    const auto cap = [&](size_t n) { return headroom ? n + n / 2 : n; };
    if (ctx.pool_cap < dev_bytes) ctx.pool_struct = 0;   // the tables it held go with it
    hipError_t e = cle_grow(ctx.d_pool, ctx.pool_cap, dev_bytes, cap(dev_bytes), false);
    if (e == hipSuccess) e = cle_grow(ctx.h_pool, ctx.hpool_cap, host_bytes, cap(host_bytes), true);
    return e;
}

static void cle_plan_free(dfq_cle_plan* p) {
    const double t0 = now_us();
    if (p->pooled) {   // hand the pool back (a run has synchronised its stream; an unrun
                       // plan's upload is waited for by the next user of the pool)
        CleDeviceCtx& ctx = cle_device_ctx(p->dev);
        const std::unique_lock<std::mutex> lock = cle_ctx_acquire(ctx, false);
        ctx.pool_busy = false;
    } else {
        (void)hipFree(p->d_tables);
    }
    (void)hipFree(p->d_snap_owned);
    if (cle_timing()) fprintf(stderr, "DFQ_CLE_TIMING free: %.1f us\n", now_us() - t0);
    delete p;
}

static int64_t snap_bytes(int64_t n) { return round256(n * (int64_t)sizeof(float)); }

extern "C" int64_t dfq_cle_plan_ws_bytes(const int64_t* target_n, int32_t n_targets) {
    if (n_targets < 0 || (n_targets > 0 && !target_n)) return -1;
    int64_t b = 0;
    for (int32_t l = 0; l < n_targets; ++l) {
        if (target_n[l] < 0) return -1;
        b += snap_bytes(target_n[l]);
    }
    return b;
}

extern "C" int dfq_cle_plan_create(const dfq_cle_rel* rels, int32_t n_rel, float* const* targets,
                                   const int64_t* target_n, int32_t n_targets, double s_min, double s_max,
                                   int32_t is_signed, float eps, int32_t ref_threads, void* ws, int64_t ws_bytes,
                                   dfq_cle_plan** out) {
    if (!out || n_rel < 0 || n_targets < 0 || (n_rel > 0 && !rels) || (n_targets > 0 && (!targets || !target_n)))
        return DFQ_ERR_INVALID;
    const double tc0 = now_us();
    const int64_t need_ws = dfq_cle_plan_ws_bytes(target_n, n_targets);
    if (need_ws < 0) return DFQ_ERR_INVALID;
    if (ws && (ws_bytes < need_ws || reinterpret_cast<uintptr_t>(ws) % 256 != 0)) return DFQ_ERR_INVALID;
    *out = nullptr;
    std::vector<CleRel> R;
    int64_t M = 0;
    if (const int rc = cle_rels_from_desc(rels, n_rel, R, M); rc != DFQ_OK) return rc;
    const double tp1 = now_us();
    // the structure (chains, tasks, chunks, placement) from the cache when a plan of
    // the same shapes and tensor-sharing pattern was built before
    bool cached = false;
    int rc = DFQ_OK;
    const std::shared_ptr<const CleStructure> S =
        cle_structure_cached(R, M, targets, target_n, n_targets, ref_threads, rc, cached);
    if (!S) return rc;
    const double tp5 = now_us();
    // this plan's addresses into its copy of the relations and layers
    std::vector<CleRel> Rb = S->R;
    for (int32_t r = 0; r < n_rel; ++r) {
        Rb[r].w1 = R[r].w1; Rb[r].w2 = R[r].w2; Rb[r].b1 = R[r].b1;
        Rb[r].bnw = R[r].bnw; Rb[r].bnb = R[r].bnb; Rb[r].sacc = R[r].sacc;
    }
    dfq_cle_plan* p = new (std::nothrow) dfq_cle_plan();
    if (!p) return DFQ_ERR_NOMEM;
    p->S = S;
    std::vector<CleLayer> layers = S->layers;
    {
        char* snap_base = static_cast<char*>(ws);
        if (!snap_base && need_ws > 0) {   // no caller workspace: the plan owns its snapshots
            hipError_t e = hipMalloc(&p->d_snap_owned, need_ws);
            if (e != hipSuccess) { set_last_hip_error(e); cle_plan_free(p); return DFQ_ERR_HIP; }
            snap_base = static_cast<char*>(p->d_snap_owned);
        }
        int64_t snap_off = 0;
        for (int32_t l = 0; l < n_targets; ++l) {
            layers[l].w = targets[l];
            layers[l].snap = reinterpret_cast<float*>(snap_base + snap_off);
            snap_off += snap_bytes(target_n[l]);
        }
    }
    if (cle_timing() && !cached) {   // the schedule: per offset, tile units and range tasks
        fprintf(stderr, "DFQ_CLE_TIMING plan: steps %d nlaunch %d lagged %d stop %d; offsets (units/ranges):", S->steps,
                S->nlaunch, (int)S->lagged, S->stop_off);
        for (int32_t k = 0; k < 2 * S->nlaunch; ++k)
            fprintf(stderr, " %d:%lld/%lld", k, (long long)(S->uoffs[k + 1] - S->uoffs[k]),
                    (long long)(S->roffs[k + 1] - S->roffs[k]));
        fprintf(stderr, "; rescale tasks per step:");
        for (int32_t k = 0; k < S->steps; ++k) fprintf(stderr, " %lld", (long long)(S->astep[k + 1] - S->astep[k]));
        fprintf(stderr, "\n");
    }
    (void)hipGetDevice(&p->dev);
    p->smin = s_min; p->smax = s_max; p->is_signed = is_signed; p->eps = eps;
    p->slots = std::max<int32_t>(ref_threads, 1);
    hipError_t e;
    auto fail = [&](hipError_t err) { set_last_hip_error(err); cle_plan_free(p); return DFQ_ERR_HIP; };
    // every table in one allocation; the host-built ones in one copy
    CleTables& T = p->t;
    T.bind(nullptr, *S, p->slots);   // the layout: the addresses follow once the allocation is known
    const double tm0 = now_us();
    char* base = nullptr;
    char* hblob = nullptr;
    CleDeviceCtx& ctx = cle_device_ctx(p->dev);
    e = hipSuccess;   // a busy pool leaves it untouched: the private path follows
    {   // the pool
        const std::unique_lock<std::mutex> lock = cle_ctx_acquire(ctx, false);
        if (!ctx.pool_busy && (e = cle_ctx_ready(ctx)) == hipSuccess &&
            (e = hipEventSynchronize(ctx.pool_ev)) == hipSuccess &&
            (e = cle_pool_reserve(ctx, (size_t)T.total, (size_t)T.host_bytes, true)) == hipSuccess) {
            ctx.pool_busy = true;
            p->pooled = true;
            base = ctx.d_pool;
            hblob = ctx.h_pool;
        }
        if (e != hipSuccess) return fail(e);
    }
    std::vector<char> blob;
    // The pool already holding this structure's address-free tables (tasks,
    // chunks, units, level-1 offsets, layer sizes: a plan of the same structure
    // came before, and the tables are read-only on the device): only the records
    // that carry addresses -- relations and layers -- are written and uploaded.
    const bool resident = p->pooled && ctx.pool_struct == S->id;
    if (!p->pooled) {
        if ((e = hipMalloc(&p->d_tables, T.total)) != hipSuccess) return fail(e);
        base = static_cast<char*>(p->d_tables);
        blob.assign(T.host_bytes, 0);
        hblob = blob.data();
    } else if (!resident) {
        std::memset(hblob, 0, T.host_bytes);
    }
    T.bind(base, *S, p->slots);
    const double tm1 = now_us();
    // a host-built table's place in the upload mirror
    auto mirror = [&](const auto* d) { return hblob + (reinterpret_cast<const char*>(d) - base); };
    auto put = [&](const auto* d, const auto& v) {
        if (!v.empty()) std::memcpy(mirror(d), v.data(), sizeof(v[0]) * v.size());
    };
    put(T.rels, Rb);
    put(T.layers, layers);
    if (!resident) {
        put(T.rtasks, S->rt); put(T.atasks, S->at); put(T.chunks, S->chunks); put(T.units, S->units); put(T.b1off, S->b1off);
        float* lm = reinterpret_cast<float*>(mirror(T.part)) + (int64_t)p->slots * n_targets;
        for (int64_t l = 0; l < n_targets; ++l) {
            lm[2 * l] = (float)layers[l].n;
            lm[2 * l + 1] = layers[l].nt == 1 ? 1.f : 0.f;
        }
    }
    if (p->pooled) {   // async on the loop stream, which every launch of the plan uses
        if (resident) {
            const size_t nr = sizeof(CleRel) * Rb.size(), nly = sizeof(CleLayer) * layers.size();
            if (nr && (e = hipMemcpyAsync(T.rels, mirror(T.rels), nr, hipMemcpyHostToDevice, ctx.st)) != hipSuccess)
                return fail(e);
            if (nly && (e = hipMemcpyAsync(T.layers, mirror(T.layers), nly, hipMemcpyHostToDevice, ctx.st)) != hipSuccess)
                return fail(e);
        } else if ((e = hipMemcpyAsync(base, hblob, T.host_bytes, hipMemcpyHostToDevice, ctx.st)) != hipSuccess) {
            return fail(e);
        }
        if ((e = hipEventRecord(ctx.pool_ev, ctx.st)) != hipSuccess) return fail(e);
        ctx.pool_struct = S->id;
    } else if ((e = hipMemcpy(base, hblob, T.host_bytes, hipMemcpyHostToDevice)) != hipSuccess) {
        return fail(e);
    }
    if (cle_timing())
        fprintf(stderr, "DFQ_CLE_TIMING create: plan %.1f us (relations %.1f, structure %s %.1f: chains %.1f, tasks %.1f, "
                "chunks %.1f, placement %.1f), tables %lld B %.1f us, copy %lld B %.1f us\n", tm0 - tc0, tp1 - tc0,
                cached ? "cached" : "built", tp5 - tp1, S->t_chains, S->t_tasks, S->t_chunks, S->t_place,
                (long long)T.total, tm1 - tm0, (long long)T.host_bytes, now_us() - tm1);
    *out = p;
    return DFQ_OK;
}

// Iteration group g's launches on stream s: the rescale steps of iteration g
// (g < max_iters), the tiles and ranges of iteration g placed in this group and
// those of iteration g - 1 placed in the next group (cle_loop_step_kernel).
// Groups 0 .. max_iters are enqueued (the last only finishes iteration
// max_iters - 1).  Kernel launches only (cle_run_drive's rule).
static int cle_enqueue_iteration(dfq_cle_plan* p, hipStream_t s, int32_t g, int32_t max_iters) {
    // grid caps: 2,048 / 4,096 blocks (caps of 128-1,024 measured 4-150 % slower on MobileNetV2)
    // step / tile grid caps (A/B: DFQ_CLE_STEP_GRID / DFQ_CLE_TILE_GRID, diagnostics library;
    // read per call, not cached: cle_ab.py switches them between runs of one process)
    const int64_t kStepGrid = [] {
        const char* e = ab_env("DFQ_CLE_STEP_GRID");
        return e && *e ? std::max<int64_t>(1, atoll(e)) : int64_t(2048);
    }();
    const int64_t kTileGrid = [] {
        const char* e = ab_env("DFQ_CLE_TILE_GRID");
        return e && *e ? std::max<int64_t>(1, atoll(e)) : int64_t(4096);
    }();
    const CleStructure& S = *p->S;
    const CleTables& T = p->t;
    CleFin F{T.cnt, T.part, T.means, p->d_hist, p->nchunks(), S.nbig, p->slots, p->nl(), 0, p->d_flag,
             S.stop_off < 0 ? 1 : 0};
    const int32_t NL = S.nlaunch;
    const bool run_g = g < max_iters, prev = g >= 1;
    for (int32_t k = 0; k < NL; ++k) {
        const bool step = k < S.steps;
        const int64_t a0 = step ? S.astep[k] : 0, a1 = step ? S.astep[k + 1] : 0;
        if (step && run_g && !S.fused && S.rstep[k + 1] > S.rstep[k]) {   // unfused: this step's ranges first
            hipLaunchKernelGGL(cle_loop_range_kernel, dim3((int)std::min<int64_t>(S.rstep[k + 1] - S.rstep[k], kStepGrid)),
                               dim3(kThreads), 0, s, T.rels, T.rtasks, S.rstep[k], S.rstep[k + 1], T.rng, S.M, T.state, 0);
            DFQ_LAUNCH_CHECK();
        }
        const int64_t nab = run_g ? std::min<int64_t>(a1 - a0, kStepGrid) : 0;
        const int64_t uo = S.uoffs[k], nuo = run_g ? S.uoffs[k + 1] - uo : 0;
        const int64_t up = S.uoffs[NL + k], nup = prev ? S.uoffs[NL + k + 1] - up : 0;
        const int64_t ro = S.roffs[k], nro_t = (g + 1 < max_iters) ? S.roffs[k + 1] - ro : 0;
        const int64_t rp = S.roffs[NL + k], nrp_t = (prev && run_g) ? S.roffs[NL + k + 1] - rp : 0;
        int64_t nto = std::min<int64_t>(nuo, kTileGrid);
        const int64_t ntp = std::min<int64_t>(nup, kTileGrid);
        F.last = (k == S.steps) ? 1 : 0;
        if (F.last && run_g && S.nbig == 0) nto = std::max<int64_t>(nto, 1);   // the stop rule's block without tiles
        const int64_t nro = std::min<int64_t>(nro_t, kStepGrid), nrp = std::min<int64_t>(nrp_t, kStepGrid);
        // lagged schedule: the stop rule's block (iteration g's, or g - 1's placed in this group)
        int32_t stop_it = -1;
        if (S.stop_off == k && run_g) stop_it = g;
        else if (S.stop_off == NL + k && prev) stop_it = g - 1;
        const int64_t nblk = nab + (stop_it >= 0 ? cle_stop_blocks(p->nchunks()) : 0) + nto + ntp + nro + nrp;
        if (nblk == 0) continue;
        auto kern = (step && S.step_pos[k]) ? cle_loop_step_kernel<true> : cle_loop_step_kernel<false>;
        hipLaunchKernelGGL(kern, dim3((int)nblk), dim3(kThreads), 0, s, T.rels, T.atasks, a0, a1, nab, T.rng,
                           S.M, p->is_signed, p->eps, p->smin, p->smax, T.layers, T.chunks, T.b1off,
                           T.units, uo, nuo, nto, up, nup, ntp, T.b1, T.tail, T.rtasks, ro, nro_t, nro, rp,
                           nrp_t, nrp, F, T.state, g, T.vsave, T.vtag, stop_it);
        DFQ_LAUNCH_CHECK();
    }
    return DFQ_OK;
}

// Iterations the host keeps enqueued behind the running one.  Whatever is queued
// when the loop converges runs as no-op launches (every block returns at
// st->done), and a no-op launch of a full-size grid still costs ~9 us
// (profiles/r04/cle_trace_*): round 3's batches of 4 iterations, one batch
// ahead, wasted 16-28 of them per run.
constexpr int32_t kCleAhead = 1;
// How long the loop's host word may stay unchanged before the host asks the
// stream whether it has drained (hipStreamQuery: a marker packet in the queue).
constexpr double kClePollQuietUs = 1000.0;
// How long the caller's stream gate waits for a launched loop at most (it traps
// after that), and how long join waits on the host (then it reports the loop
// lost).  A launched run stops enqueueing iterations at half the gate's limit and
// fails cleanly (cle_run_drive's deadline), so a slowly converging loop on a busy
// GPU ends with an error at join, not with the gate's trap; blocking runs
// (dfq_cle_plan_run) have no deadline and stop at max_iters
// (Cross_layer_equal.DFQ_CLE_MAX_ITERS) with its warning.
static constexpr int kCleGateSeconds = 120;
static constexpr int kCleJoinSeconds = kCleGateSeconds + 30;
static constexpr double kCleLaunchDeadlineUs = 0.5e6 * kCleGateSeconds;
// The context's history buffer for caps above the tables' kCleHistCap slots,
// grown once (a launched run grows it before its caller's stream waits: hipFree
// synchronises the whole device).
static hipError_t cle_hist_ready(CleDeviceCtx& ctx, int32_t max_iters) {
    const int64_t n = (int64_t)max_iters + 1;
    hipError_t e = cle_grow(ctx.h_hist, ctx.h_hist_cap, n, n, true);   // the pinned copy-back buffer
    if (e == hipSuccess && n > kCleHistCap) e = cle_grow(ctx.d_hist, ctx.hist_cap, n, n, false);
    return e;
}

// Device -> host copy ordered on the loop stream.  Never a blocking hipMemcpy
// here: that runs on the null stream, which the caller of a launched run may be
// holding behind its wait for this very loop (dfq_cle_plan_launch).
static hipError_t cle_copy_back(void* dst, const void* src, size_t bytes, hipStream_t s) {
    hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s);
    return e == hipSuccess ? hipStreamSynchronize(s) : e;
}

#ifdef DFQ_DIAGNOSTICS
#include "dfq_cle_timeline.h"   // DFQ_CLE_TL: CleTimeline
#else
struct CleTimeline {   // the product library records no timeline
    int begin(const dfq_cle_plan*, hipStream_t) { return DFQ_OK; }
    int report(const dfq_cle_plan*, hipStream_t) { return DFQ_OK; }
};
#endif

// One run's host state, handed from stage to stage of cle_run_locked.
struct CleRun {
    double threshold;
    int32_t count, max_iters;
    double deadline_us;           // > 0 (launched runs): no iteration is enqueued past it
    bool idle = false;            // the stop rule holds before the first iteration: nothing to drive
    double t_drive = 0;           // when the drive loop began
    int32_t launched = 0;         // iteration groups enqueued
    bool deadline_hit = false;
    hipEvent_t tev[2] = {nullptr, nullptr};   // timed runs: around the loop's launches
};

// Stage 1, set-up: the run's state and history buffer, the init launch and, fused
// schedule, the first iteration's ranges.  Rule: *ctx.h_flag is reset with no kernel
// of this context's stream running (the caller holds ctx.mu), and cle_hist_ready,
// the only place a run may free memory, comes before anything of the run is on the
// stream (a launched run grew the buffers before its gate was enqueued: this call
// then frees nothing).
static int cle_run_setup(dfq_cle_plan* p, CleDeviceCtx& ctx, CleRun& run) {
    DFQ_HIP_CHECK(cle_ctx_ready(ctx));
    *ctx.h_flag = 0;
    p->d_flag = ctx.d_flag;
    hipStream_t s = ctx.st;
    const CleStructure& S = *p->S;
    const CleTables& T = p->t;
    // the history: the tables' slots, or the context's buffer (grown once) for longer caps
    p->d_hist = T.hist;
    DFQ_HIP_CHECK(cle_hist_ready(ctx, run.max_iters));
    if (run.max_iters + 1 > kCleHistCap) p->d_hist = ctx.d_hist;
    CleState init{};
    init.diff = 1e8;
    init.thr = run.threshold;   // (iter_count, iters, error: 0)
    init.count = run.count;
    init.max_iters = run.max_iters;
    init.done = !((init.diff > run.threshold) && (0 < run.count)) || run.max_iters == 0;
    run.idle = init.done != 0;
    // the range words, chunk sums, counters, rollback tags, the state and the
    // snapshots in one launch (cle_loop_init_kernel; round 5: six fills, a state
    // upload and the snapshot kernel)
    {
        const int64_t npart = (int64_t)p->slots * std::max(p->nl(), 1), ncnt = p->nchunks() + 1;
        const int64_t nvtag = T.vtag ? (int64_t)S.at.size() : 0;
        const int64_t words = std::max({4 * S.M, npart, ncnt, nvtag});
        const int64_t grid = std::min<int64_t>(std::max<int64_t>({p->nunits(), ceil_div(words, (int64_t)kThreads), 1}), 4096);
        hipLaunchKernelGGL(cle_loop_init_kernel, dim3((int)grid), dim3(kThreads), 0, s, T.layers, T.chunks,
                           p->nchunks(), T.units, p->nunits(), T.rng, S.M, T.part, npart, T.cnt, ncnt,
                           T.vtag, nvtag, T.state, init);
        DFQ_LAUNCH_CHECK();
    }
    // fused schedule: the first iteration's ranges (later ones ride with the tiles)
    if (S.fused && S.rstep[1] > S.rstep[0]) {
        hipLaunchKernelGGL(cle_loop_range_kernel, dim3((int)std::min<int64_t>(S.rstep[1] - S.rstep[0], 2048)),
                           dim3(kThreads), 0, s, T.rels, T.rtasks, S.rstep[0], S.rstep[1], T.rng, S.M, T.state, 0);
        DFQ_LAUNCH_CHECK();
    }
    return DFQ_OK;
}

// Stage 2, the drive loop: enqueue and poll.  Rule: between two iterations the
// loop stream receives kernel launches only.  Iteration by iteration, kCleAhead of them queued behind the running one; the
// stop rule writes (iterations << 1) | done into pinned host memory every
// iteration (ctx.h_flag, a system-scope store), and this thread polls that word
// both for the stop and for its pacing -- no copy, event or host round trip
// sits between two iterations on the loop stream, and at convergence at most
// kCleAhead iterations are left to run as no-ops.  (Pacing by an event behind
// each iteration: its marker packet added ~3.7 us before every iteration's
// first launch, profiles/r04/cle_trace_r04v_*.  Round 3 enqueued batches of 4
// iterations a batch ahead and read the state back per batch.)
// hipStreamQuery is NOT polled per iteration: the runtime answers it with a
// marker packet in the loop's queue, which then sits between two iterations'
// launches.  It is asked only when the word has not moved for kClePollQuietUs
// (a kernel error, or everything launched has run).  A drained stream ends the
// polling only when the word, re-read after the drain, says done, or every
// allowed iteration was launched, or the word lags the launches (a lost
// word): a stale read that held back the next enqueue just goes on enqueueing
// (breaking there ended the loop early as DFQ_OK).
// deadline_us > 0 (launched runs): past it no more iterations are enqueued and
// the run fails cleanly, well before the caller's stream gate would trap.
// Timed runs (dfq_cle_plan_set_timing, measurement only): one event pair around
// the loop's launches on its stream (two marker packets per run, none between
// iterations); the first is recorded here, the second by the drain.
static int cle_run_drive(dfq_cle_plan* p, CleDeviceCtx& ctx, CleRun& run) {
    hipStream_t s = ctx.st;
    const int32_t max_iters = run.max_iters;
    run.t_drive = now_us();
    p->loop_ms = -1.f;
    if (p->timed) {
        DFQ_HIP_CHECK(hipEventCreate(&run.tev[0]));
        DFQ_HIP_CHECK(hipEventCreate(&run.tev[1]));
        DFQ_HIP_CHECK(hipEventRecord(run.tev[0], s));
    }
    if (run.idle) return DFQ_OK;
    // test switch (diagnostics library): the polling thread descheduled between its
    // load of the word and the stream query below (the stale-word race of ADVICE
    // r04), with the query on every poll, as round 4 did
    const char* pd = ab_env("DFQ_CLE_TEST_POLL_DELAY_US");
    const int poll_delay_us = pd ? atoi(pd) : 0;
    const double quiet_us = pd ? 0.0 : kClePollQuietUs;
    uint32_t last_f = ~0u;
    double t_moved = run.t_drive;
    for (;;) {
        const uint32_t f = __atomic_load_n(ctx.h_flag, __ATOMIC_ACQUIRE);
        if (f & 1u) break;
        const int32_t ran = (int32_t)(f >> 1);   // iterations complete
        if (run.launched <= max_iters && !run.deadline_hit && run.launched - ran <= kCleAhead) {
            const int rc = cle_enqueue_iteration(p, s, run.launched, max_iters);
            if (rc != DFQ_OK) return rc;
            ++run.launched;
            continue;
        }
        if (poll_delay_us > 0) std::this_thread::sleep_for(std::chrono::microseconds(poll_delay_us));
        const double t = now_us();
        if (f != last_f) {
            last_f = f;
            t_moved = t;
        } else if (t - t_moved >= quiet_us) {
            const hipError_t q = hipStreamQuery(s);
            if (q != hipErrorNotReady) {
                if (q != hipSuccess) break;   // a device error: the drain's synchronize reports it
                const uint32_t f2 = __atomic_load_n(ctx.h_flag, __ATOMIC_ACQUIRE);
                if ((f2 & 1u) || run.launched > max_iters || run.deadline_hit || (int32_t)(f2 >> 1) + 1 < run.launched)
                    break;
            }
            t_moved = t;
        }
        if (run.deadline_us > 0 && t - run.t_drive > run.deadline_us) run.deadline_hit = true;
        __builtin_ia32_pause();
    }
    return DFQ_OK;
}

// Stage 3, the drain.  Rule: this order, and one synchronize (not three) -- the
// rollback of a speculative iteration (lagged schedule), the second timing event, the
// signal write that releases a launched run's caller (behind the rollback: its stages
// must not see a speculative iteration's weights), then the final state and the history
// (at most the groups launched: iterations run <= groups); nothing before the
// synchronize allocates or frees.  Then the timeline's report and the result: a loop
// whose stop rule never said done is an error, never a partial result.
static int cle_run_drain(dfq_cle_plan* p, CleDeviceCtx& ctx, CleRun& run, CleTimeline& timeline, int32_t* iterations,
                         std::vector<double>* hist) {
    hipStream_t s = ctx.st;
    const CleTables& T = p->t;
    if (!run.idle && p->S->lagged) {   // undo a speculative iteration, then release a launched run's caller
        hipLaunchKernelGGL(cle_loop_rollback_kernel, dim3(1024), dim3(kThreads), 0, s, T.layers, p->nl(), T.rels,
                           T.atasks, (int64_t)p->S->at.size(), T.vsave, T.vtag, T.state);
        DFQ_LAUNCH_CHECK();
    }
    if (run.tev[1]) DFQ_HIP_CHECK(hipEventRecord(run.tev[1], s));
    if (p->d_sig) DFQ_HIP_CHECK(hipStreamWriteValue64(s, p->d_sig, p->gen, 0));
    DFQ_HIP_CHECK(hipMemcpyAsync(ctx.h_state, T.state, sizeof(CleState), hipMemcpyDeviceToHost, s));
    const int32_t hn = std::min(run.launched, run.max_iters);
    if (hist && hn > 0) DFQ_HIP_CHECK(hipMemcpyAsync(ctx.h_hist, p->d_hist, sizeof(double) * hn, hipMemcpyDeviceToHost, s));
    DFQ_HIP_CHECK(hipStreamSynchronize(s));
    p->launched = run.launched;
    if (run.tev[0]) {
        float ms = -1.f;
        if (hipEventElapsedTime(&ms, run.tev[0], run.tev[1]) == hipSuccess) p->loop_ms = ms;
        (void)hipEventDestroy(run.tev[0]);
        (void)hipEventDestroy(run.tev[1]);
    }
    if (cle_timing())
        fprintf(stderr, "DFQ_CLE_TIMING run: loop %.1f us (%d iterations launched)\n", now_us() - run.t_drive, run.launched);
    if (const int rc = timeline.report(p, s); rc != DFQ_OK) return rc;
    // the final state (a no-op iteration after convergence changed nothing)
    const CleState fin = *ctx.h_state;
    if (fin.error) {   // a range block saw the wrong parity: never expected
        set_last_hip_error(hipErrorLaunchTimeOut);
        return DFQ_ERR_HIP;
    }
    if (!fin.done) {   // the stop rule never said done: never report a partial loop as a result
        set_last_hip_error_text(run.deadline_hit ? "the launched CLE loop reached its time limit before converging"
                                                 : "the CLE loop stopped before its stop rule said done");
        return DFQ_ERR_HIP;
    }
    if (ab_env("DFQ_CLE_DEBUG")) {   // per-layer chunk sums of the last iteration run
        std::vector<float> part((size_t)p->slots * std::max(p->nl(), 1));
        DFQ_HIP_CHECK(cle_copy_back(part.data(), T.part, sizeof(float) * part.size(), s));
        for (int32_t l = 0; l < p->nl(); ++l) {
            fprintf(stderr, "DFQ_CLE_DEBUG layer %d:", l);
            for (int t = 0; t < p->slots; ++t) fprintf(stderr, " %.9g", part[(size_t)p->slots * l + t]);
            fprintf(stderr, "\n");
        }
    }
    if (iterations) *iterations = fin.iters;
    if (hist) {
        hist->assign((size_t)std::max(fin.iters, 0), 0.0);
        if (fin.iters > 0) std::memcpy(hist->data(), ctx.h_hist, sizeof(double) * std::min(fin.iters, hn));
    }
    return DFQ_OK;
}

// The loop on the device context's stream; the caller holds ctx.mu and has
// ordered the plan's producers before that stream.  iterations / hist: the run's
// result (hist resized to the iterations run).
static int cle_run_locked(dfq_cle_plan* p, CleDeviceCtx& ctx, double threshold, int32_t count, int32_t max_iters,
                          int32_t* iterations, std::vector<double>* hist, double deadline_us = -1.0) {
    CleRun run{threshold, count, max_iters, deadline_us};
    CleTimeline timeline;   // DFQ_CLE_TL (diagnostics library; the product's is empty)
    int rc = cle_run_setup(p, ctx, run);
    if (rc == DFQ_OK) rc = timeline.begin(p, ctx.st);
    if (rc == DFQ_OK) rc = cle_run_drive(p, ctx, run);
    if (rc == DFQ_OK) rc = cle_run_drain(p, ctx, run, timeline, iterations, hist);
    return rc;
}

// ---- asynchronous run (dfq_cle_plan_launch / _join) -------------------------
// The loop needs the host between iterations (it polls the stop rule), so a
// worker thread drives it on the context's stream while the caller's thread goes
// on enqueueing the next stages on its own stream.  That stream waits, in the
// device, behind the gate kernel for a per-device signal word the worker writes
// behind the loop's last launch (hipStreamWriteValue64): no host sync between
// the stages, and nothing of the caller's stream runs before the loop is done.
// The loop stream is a high-priority stream: it gets a hardware queue of its own
// (queues are pooled per priority), so the caller's waiting queue can never hold
// the loop's launches back.
// (the gate's limit and the launched run's deadline: kCleGateSeconds, above)

struct CleAsync {
    std::mutex m;
    std::condition_variable cv;
    bool done = false;
    int rc = DFQ_OK;
    int32_t iters = 0;
    std::vector<double> hist;
    char err[128] = {0};
};

// One long-lived worker thread per device context: a thread created per run paid
// the HIP runtime's per-thread setup on every run.  Detached, never destroyed (a
// process ends with it idle: wait() / destroy join every launched run first).
struct CleWorker {
    std::mutex m;
    std::condition_variable cv;
    std::function<void()> job;
    bool has_job = false;
};
static void cle_worker_loop(CleWorker* w) {
    for (;;) {
        std::function<void()> j;
        {
            std::unique_lock<std::mutex> l(w->m);
            w->cv.wait(l, [w] { return w->has_job; });
            j = std::move(w->job);
            w->has_job = false;
        }
        j();
    }
}
// The context's worker, started at the first need (dfq_preload, else the first
// launch; caller holds ctx.mu).  Throws when no thread can be started.
static void cle_worker_ready(CleDeviceCtx& ctx) {
    if (ctx.worker) return;
    CleWorker* w = new CleWorker();
    std::thread(cle_worker_loop, w).detach();
    ctx.worker = w;
}

// The context's signal word (lazily allocated as HIP signal memory: the gate
// kernel polls it, the worker writes it with hipStreamWriteValue64); when it
// cannot be allocated, callers run synchronously.
static hipError_t cle_signal_ready(CleDeviceCtx& ctx) {
    if (ctx.sig) return hipSuccess;
    if (ctx.sig_state < 0) return hipErrorNotSupported;
    hipError_t e = hipSuccess;
    void* sig = nullptr;
    if ((e = hipExtMallocWithFlags(&sig, sizeof(uint64_t), hipMallocSignalMemory)) != hipSuccess) {
        ctx.sig_state = -1;
        return e;
    }
    // generation 0, in stream order on the loop stream
    if ((e = hipStreamWriteValue64(ctx.st, sig, 0, 0)) != hipSuccess || (e = hipStreamSynchronize(ctx.st)) != hipSuccess) {
        (void)hipFree(sig);
        ctx.sig_state = -1;
        return e;
    }
    ctx.sig = sig;
    ctx.gen = 0;
    return hipSuccess;
}

// Waits for a launched run; false when it has not finished within `seconds`
// (< 0: no limit).
static bool cle_async_join(dfq_cle_plan* p, double seconds = -1.0) {
    if (!p || !p->async) return true;
    CleAsync* a = p->async;
    std::unique_lock<std::mutex> l(a->m);
    if (seconds < 0) {
        a->cv.wait(l, [a] { return a->done; });
        return true;
    }
    return a->cv.wait_for(l, std::chrono::duration<double>(seconds), [a] { return a->done; });
}

// The one way a caller's thread takes the context (CleDeviceCtx::pending's rule).
// join_pending (run, launch): the launched run not yet joined finishes first, waited
// for WITHOUT the lock; the signal's generations then complete in launch order.  Else
// (create, preload, free): the pool only, while no plan holds it; never waits for a run.
static std::unique_lock<std::mutex> cle_ctx_acquire(CleDeviceCtx& ctx, bool join_pending) {
    std::unique_lock<std::mutex> lock(ctx.mu);
    while (dfq_cle_plan* q = join_pending ? ctx.pending : nullptr) {
        lock.unlock();
        cle_async_join(q);
        lock.lock();
        if (ctx.pending == q) ctx.pending = nullptr;
    }
    return lock;
}
static void cle_pending_clear(CleDeviceCtx& ctx, dfq_cle_plan* p) {   // join, destroy: no longer the launched run
    const std::unique_lock<std::mutex> lock = cle_ctx_acquire(ctx, false);
    if (ctx.pending == p) ctx.pending = nullptr;
}

extern "C" int dfq_cle_plan_run(dfq_cle_plan* p, double threshold, int32_t count, int32_t max_iters,
                                int32_t* iterations, double* diffs, void* stream) {
    if (!p || max_iters < 0 || p->async) return DFQ_ERR_INVALID;   // a launched plan is joined instead
    // The loop runs on the device context's stream: wait for the caller's
    // producers first; the call is blocking.
    const double ts0 = now_us();
    DFQ_HIP_CHECK(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    const double ts1 = now_us();
    int dev = 0;
    DFQ_HIP_CHECK(hipGetDevice(&dev));
    CleDeviceCtx& ctx = cle_device_ctx(dev);
    const std::unique_lock<std::mutex> lock = cle_ctx_acquire(ctx, true);
    if (cle_timing()) fprintf(stderr, "DFQ_CLE_TIMING run: caller sync %.1f us, context %.1f us\n", ts1 - ts0,
                              now_us() - ts1);
    std::vector<double> h;
    const int rc = cle_run_locked(p, ctx, threshold, count, max_iters, iterations, diffs ? &h : nullptr);
    if (rc == DFQ_OK && diffs && !h.empty()) std::memcpy(diffs, h.data(), sizeof(double) * h.size());
    return rc;
}

extern "C" int dfq_cle_plan_launch(dfq_cle_plan* p, double threshold, int32_t count, int32_t max_iters,
                                   void* stream) {
    if (!p || max_iters < 0 || p->async) return DFQ_ERR_INVALID;
    // The diagnostics task timeline allocates and frees inside the loop, which may
    // synchronise the whole device -- behind a caller's stream that waits for the
    // loop: it takes the blocking run (the product library reads no switches).
    if (ab_env("DFQ_CLE_TL")) return DFQ_ERR_UNSUPPORTED;
    hipStream_t caller = static_cast<hipStream_t>(stream);
    CleDeviceCtx& ctx = cle_device_ctx(p->dev);
    const double tl0 = now_us();
    std::unique_ptr<CleAsync> rec(new (std::nothrow) CleAsync());   // the worker's record
    uint64_t gen = 0;
    {
        const std::unique_lock<std::mutex> lock = cle_ctx_acquire(ctx, true);
        DFQ_HIP_CHECK(hipSetDevice(p->dev));
        DFQ_HIP_CHECK(cle_ctx_ready(ctx));
        const hipError_t es = cle_signal_ready(ctx);
        if (es == hipErrorNotSupported) return DFQ_ERR_UNSUPPORTED;
        DFQ_HIP_CHECK(es);
        DFQ_HIP_CHECK(cle_hist_ready(ctx, max_iters));   // no hipFree in the worker
        // the caller's producers before the loop; the caller's later work after it
        DFQ_HIP_CHECK(hipEventRecord(ctx.in_ev, caller));
        DFQ_HIP_CHECK(hipStreamWaitEvent(ctx.st, ctx.in_ev, 0));
        gen = ctx.gen + 1;
        // the caller's stream waits behind a gate kernel (cle_caller_gate_kernel);
        // a CP wait packet (hipStreamWaitValue64) there measured 1.8x slower loops
        // (profiles/r03/async_ab/)
        hipLaunchKernelGGL(cle_caller_gate_kernel, dim3(1), dim3(64), 0, caller,
                           static_cast<const uint64_t*>(ctx.sig), gen, (uint64_t)kCleGateSeconds * 100000000ull);
        DFQ_LAUNCH_CHECK();
        ctx.gen = gen;
        // pending under the lock the gate was enqueued under: no other thread's run or
        // launch gets between the gate and this run's worker (ctx.pending's rule)
        if (rec) p->async = rec.get(), ctx.pending = p;
    }
    if (cle_timing()) fprintf(stderr, "DFQ_CLE_TIMING launch: gate and order %.1f us\n", now_us() - tl0);
    // from here on the caller's stream is held until the signal reaches gen: every
    // path below writes it
    CleAsync* a = rec.release();
    const double t_launch = now_us();
    auto body = [p, &ctx, threshold, count, max_iters, gen, t_launch](CleAsync* a) {
        std::lock_guard<std::mutex> lock(ctx.mu);
        int rc = DFQ_OK;
        if (hipSetDevice(p->dev) != hipSuccess) {
            rc = DFQ_ERR_HIP;
        } else {
            rc = cle_run_locked(p, ctx, threshold, count, max_iters, &a->iters, &a->hist, kCleLaunchDeadlineUs);
        }
        if (rc == DFQ_ERR_HIP) copy_error_text(a->err, sizeof(a->err), dfq_last_hip_error());
        // test switch (diagnostics library; test_gpu_cle_plan.py's held caller stream): a late release
        if (const char* d = ab_env("DFQ_CLE_TEST_RELEASE_DELAY_MS"))
            std::this_thread::sleep_for(std::chrono::milliseconds(atoi(d)));
        // release the caller's stream behind everything the loop enqueued
        hipError_t e = hipStreamWriteValue64(ctx.st, ctx.sig, gen, 0);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx.st);
        if (e != hipSuccess) {   // never expected; the gate traps at its time limit
            fprintf(stderr, "dfq_cle_plan_launch: releasing the caller's stream failed (%s)\n", hipGetErrorString(e));
            if (rc == DFQ_OK) rc = DFQ_ERR_HIP;
        }
        if (rc == DFQ_OK && now_us() - t_launch > 0.9e6 * kCleGateSeconds) {   // the gate may have opened early
            set_last_hip_error(hipErrorLaunchTimeOut);
            copy_error_text(a->err, sizeof(a->err), "CLE loop outlived the caller's stream gate");
            rc = DFQ_ERR_HIP;
        }
        {
            std::lock_guard<std::mutex> l(a->m);
            a->rc = rc;
            a->done = true;
        }
        a->cv.notify_all();   // a is the joiner's from here on
    };
    if (!a) {   // no memory for the worker's record: run here, then release
        CleAsync tmp;
        body(&tmp);
        return tmp.rc;
    }
    p->d_sig = static_cast<uint64_t*>(ctx.sig);   // released behind the loop's rollback (cle_run_drain)
    if (ab_env("DFQ_CLE_HOST_RELEASE")) p->d_sig = nullptr;   // diagnostics: only the worker's release, after the run
    p->gen = gen;
    bool posted = false;
    try {   // (the worker, once woken, waits for ctx.mu until this block ends)
        const std::unique_lock<std::mutex> lock = cle_ctx_acquire(ctx, false);
        cle_worker_ready(ctx);
        {
            std::lock_guard<std::mutex> l(ctx.worker->m);
            ctx.worker->job = [body, a] { body(a); };
            ctx.worker->has_job = true;
        }
        ctx.worker->cv.notify_one();
        posted = true;
    } catch (...) {}
    if (!posted) body(a);   // no worker: run on this thread (blocking), which also releases
    if (cle_timing()) fprintf(stderr, "DFQ_CLE_TIMING launch: total %.1f us\n", now_us() - tl0);
    return DFQ_OK;
}

extern "C" int dfq_cle_plan_join(dfq_cle_plan* p, int32_t* iterations, double* diffs) {
    if (!p || !p->async) return DFQ_ERR_INVALID;
    if (p->abandoned) return DFQ_ERR_HIP;
    double limit = kCleJoinSeconds;
    if (const char* j = ab_env("DFQ_CLE_TEST_JOIN_LIMIT_MS")) limit = atoi(j) * 1e-3;   // test switch (diagnostics library)
    if (!cle_async_join(p, limit)) {
        // The loop has not finished: the caller's stream stays held behind the gate
        // (which traps at its own limit); the plan stays with the worker, which may
        // still use it (destroy leaves it alone), and stays the context's pending
        // run, so the next run or launch waits for it.
        p->abandoned = true;
        set_last_hip_error_text("the launched CLE loop did not finish in time; the caller's stream stays held");
        return DFQ_ERR_HIP;
    }
    cle_pending_clear(cle_device_ctx(p->dev), p);
    const CleAsync& a = *p->async;
    if (a.rc == DFQ_ERR_HIP && a.err[0]) set_last_hip_error_text(a.err);
    if (a.rc != DFQ_OK) return a.rc;
    if (iterations) *iterations = a.iters;
    if (diffs && !a.hist.empty()) std::memcpy(diffs, a.hist.data(), sizeof(double) * a.hist.size());
    return DFQ_OK;
}

extern "C" int dfq_cle_plan_info(const dfq_cle_plan* p, int32_t* chains, int32_t* steps, int32_t* launches) {
    if (!p) return DFQ_ERR_INVALID;
    if (chains) *chains = p->S->chains;
    if (steps) *steps = p->S->steps;
    // per iteration: the rescale launches (+ per-step range launches when the
    // schedule is not fused), + a tiles-only launch unless the schedule is lagged
    if (launches) *launches = p->S->fused ? p->S->nlaunch : 2 * p->S->steps + 1;
    return DFQ_OK;
}

extern "C" int dfq_cle_plan_set_timing(dfq_cle_plan* p, int32_t on) {
    if (!p || p->async) return DFQ_ERR_INVALID;
    p->timed = on != 0;
    return DFQ_OK;
}

extern "C" int dfq_cle_plan_stats(const dfq_cle_plan* p, int64_t* bytes, double* loop_ms, int32_t* launched) {
    if (!p) return DFQ_ERR_INVALID;
    if (bytes) {
        bytes[0] = p->S->bytes_rescale;
        bytes[1] = p->S->bytes_metric;
        bytes[2] = p->S->bytes_range;
    }
    if (loop_ms) *loop_ms = p->loop_ms;
    if (launched) *launched = p->launched;
    return DFQ_OK;
}

extern "C" int dfq_cle_plan_destroy(dfq_cle_plan* p) {
    if (!p) return DFQ_OK;
    if (p->abandoned) return DFQ_OK;   // its worker may still run it: left to the worker (leaked)
    if (p->async) {   // a launched run finishes first (its worker uses the plan)
        cle_async_join(p);
        cle_pending_clear(cle_device_ctx(p->dev), p);
        delete p->async;
        p->async = nullptr;
    }
    cle_plan_free(p);
    return DFQ_OK;
}

namespace dfq {
// What a first CLE run on a device would otherwise allocate inside the caller's
// timed region (a cold main_dfq run: plan create 314 against 55 us warm, launch 160
// against 20): the table pools at a size that holds the zoo models' tables, the
// iteration history for the default DFQ_CLE_MAX_ITERS, the signal word of launched
// runs and their worker thread.
constexpr size_t kClePreloadPool = size_t(4) << 20, kClePreloadHostPool = size_t(2) << 20;
constexpr int32_t kClePreloadHistIters = 100000;   // Cross_layer_equal.MAX_ITERS' default
hipError_t preload_cle() {   // see dfq_preload
    int dev = 0;
    hipError_t e0 = hipGetDevice(&dev);
    if (e0 != hipSuccess) return e0;
    {
        CleDeviceCtx& ctx = cle_device_ctx(dev);
        const std::unique_lock<std::mutex> lock = cle_ctx_acquire(ctx, false);
        if ((e0 = cle_ctx_ready(ctx)) != hipSuccess) return e0;
        if (!ctx.pool_busy && (e0 = cle_pool_reserve(ctx, kClePreloadPool, kClePreloadHostPool, false)) != hipSuccess)
            return e0;
        if ((e0 = cle_hist_ready(ctx, kClePreloadHistIters)) != hipSuccess) return e0;
        (void)cle_signal_ready(ctx);   // unsupported: launched runs fall back to blocking ones
        try { cle_worker_ready(ctx); } catch (...) {}   // no thread: created at the first launch instead
    }
    hipFuncAttributes a;
    hipError_t e = hipFuncGetAttributes(&a, reinterpret_cast<const void*>(cle_loop_step_kernel<true>));
    if (e == hipSuccess) e = hipFuncGetAttributes(&a, reinterpret_cast<const void*>(cle_loop_step_kernel<false>));
    return e;
}
}  // namespace dfq
