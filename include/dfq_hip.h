/*
 * dfq_hip.h -- C ABI of libdfq_hip.so, the MI355X (gfx950) data-free-quantization
 * weight-transform path.
 *
 * Every entry point is plain C: raw device pointers, integer sizes, an opaque
 * hipStream_t passed as `void*` (NULL = the legacy default stream).  All compute
 * calls are asynchronous on that stream unless the comment says "blocking".
 * Nothing here allocates device memory on the hot path: the one-shot calls take
 * a caller-provided workspace, and the plan objects allocate once at create().
 *
 * Return value: 0 on success, a negative DFQ_ERR_* code otherwise
 * (dfq_error_string() gives the text).  The Python host layer maps
 * DFQ_ERR_SHAPE to ValueError/RuntimeError exactly where the reference raises.
 *
 * Each function cites the reference interface (KadAMRN/Data_Free_Quantization)
 * whose arithmetic it replaces.  The binding a maintainer adds on the reference
 * side (ctypes) is in INTEGRATION.md.
 */
#ifndef DFQ_HIP_H_
#define DFQ_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with hidden visibility: only these entry points are
 * exported (two builds in one process -- the product and the diagnostics
 * library -- then never bind to each other's internals). */
#pragma GCC visibility push(default)

#define DFQ_ABI_VERSION 1

/* Load every kernel's code object on the current device now (otherwise the first
 * launch from each translation unit pays for it, ~ms), and allocate what a first
 * run would allocate inside the caller's timing: the CLE context's stream, table
 * pools (4 MB device, 2 MB pinned), iteration history, signal word and worker
 * thread, and 8 pinned 1 MB staging slots for table uploads.  main_dfq calls it
 * (`_lib.preload()`) before its timer, as process setup.  Idempotent, blocking;
 * 0 or DFQ_ERR_HIP. */
int dfq_preload(void);

/* ---- error codes ------------------------------------------------------- */
#define DFQ_OK              0
#define DFQ_ERR_INVALID    -1   /* bad argument (null pointer, bits out of range, ...) */
#define DFQ_ERR_HIP        -2   /* a HIP runtime call failed */
#define DFQ_ERR_UNSUPPORTED -3  /* valid request this build does not implement */
#define DFQ_ERR_NOMEM      -4   /* device / host allocation failed (plan create only) */
#define DFQ_ERR_SHAPE      -5   /* shape mismatch the reference would raise on */
#define DFQ_ERR_WORKSPACE  -6   /* caller workspace too small */

/* ---- quantizer modes ---------------------------------------------------- */
/* TENSOR_* use one (min, max) for the whole tensor (reference default,
 * utils/quantize.py:62-66 via utils/layer_transform.py:298).  CHANNEL_* use one
 * (min, max) per row = per output channel (extension: the reference quantize()
 * applied to each W[o] slice).  *_SYM is utils/quantize.py:51-60.              */
#define DFQ_TENSOR_ASYM   0
#define DFQ_TENSOR_SYM    1
#define DFQ_CHANNEL_ASYM  2
#define DFQ_CHANNEL_SYM   3

/* ---- descriptor flags --------------------------------------------------- */
#define DFQ_CLIP          0x1  /* clamp the dequantized output to [clip_lo, clip_hi] (clip_weight.py:29) */
#define DFQ_GIVEN_RANGE   0x2  /* use given_min/given_max (Python doubles) instead of the data range */
#define DFQ_SCALE_F32     0x4  /* scale arithmetic in fp32 (quantize() called with min/max=None,
                                  utils/quantize.py:26-37: 0-d fp32 tensors) instead of fp64;
                                  with DFQ_GIVEN_RANGE the given values are fp32 tensor values */
#define DFQ_PACK_INT4     0x8  /* bits <= 4: codes packed two per byte, element 2k in the low nibble and
                                  2k+1 in the high nibble (two's-complement nibbles when symmetric);
                                  codes holds ceil(rows*row_len/2) bytes.  bits > 4: DFQ_ERR_INVALID.
                                  Every task starts at an even element, so per channel an odd row_len
                                  above half a task (1024 elements by default) with rows > 1 is
                                  DFQ_ERR_UNSUPPORTED (two rows' tasks would share a byte) */

#define DFQ_DEVICE_RANGE  0x10 /* TENSOR modes: the range is read on the device, when the sweep runs,
                                  from range_enc = {~enc(min), enc(max)} (dfq_range's encoding, or
                                  the by-product of dfq_bn_fold_batch): one HBM pass, no reduce
                                  launch.  Arithmetic as for the data range (the values are the
                                  tensor's fp32 min and max).  Not with DFQ_GIVEN_RANGE */

/* One fp32 tensor viewed as [rows, row_len], row_len = I*KH*KW (KCRS) or I (Linear).
 * Outputs are written only where the pointer is non-NULL:
 *   dst    fp32 dequantized values (may alias src: in-place, like weight.data.copy_)
 *   codes  integer grid indices: uint8 (asym, bits<=8), int8 (sym, bits<=8),
 *          uint16/int16 for 8<bits<=16, or packed nibbles (DFQ_PACK_INT4)
 *   scale  fp32 step, [rows] in CHANNEL modes, [1] in TENSOR modes
 *   zero   fp32 value added back after scaling (the range min for asym, +0 for sym)
 *   esum   fp32 bias-correction error sums E[o,i] = sum_k (y - x)[o, i*khw + k],
 *          [rows * row_len/khw]  (bias_correction.py:128-131,231 on the fused output y)
 */
typedef struct dfq_tensor_desc {
    const float* src;
    float*       dst;
    void*        codes;
    float*       scale;
    float*       zero;
    float*       esum;
    int64_t      rows;
    int64_t      row_len;
    int32_t      khw;       /* spatial size for esum (1 for Linear / 1x1) */
    int32_t      bits;      /* 2..16 */
    int32_t      mode;      /* DFQ_TENSOR_ASYM ... DFQ_CHANNEL_SYM */
    int32_t      flags;     /* DFQ_CLIP | DFQ_GIVEN_RANGE | DFQ_SCALE_F32 | DFQ_PACK_INT4 | DFQ_DEVICE_RANGE */
    float        clip_lo;
    float        clip_hi;
    double       given_min;
    double       given_max;
    const uint32_t* range_enc; /* DFQ_DEVICE_RANGE: 2 device words, else NULL */
} dfq_tensor_desc;

/* ---- library ------------------------------------------------------------ */
int         dfq_abi_version(void);
const char* dfq_error_string(int code);
/* Last HIP error text seen by the library on this thread ("" if none). */
const char* dfq_last_hip_error(void);

/* ---- single-tensor quantize (replaces quantize()/UniformQuantize.forward,
 *      utils/quantize.py:16-89) ------------------------------------------- */
/* Workspace bytes dfq_quantize_tensor needs for this descriptor (0 is possible). */
int dfq_quantize_ws_bytes(const dfq_tensor_desc* desc, size_t* bytes);
/* Asynchronous on `stream` (the task table goes up through the library's pinned
 * staging ring; no host wait).  ws: device memory of >= dfq_quantize_ws_bytes
 * bytes that stays allocated until the stream reaches the kernel (a
 * stream-ordered allocator does that). */
int dfq_quantize_tensor(const dfq_tensor_desc* desc, void* ws, size_t ws_bytes, void* stream);
/* quantize()'s data range when min/max are None and num_chunks splits the batch
 * (utils/quantize.py:26-37): x viewed as [rows = B // num_chunks, row_len];
 * out2 = {mean_r min(x[r]), mean_r max(x[r])} in fp32, the mean in ATen's sum
 * order.  rowbuf: 2*rows device floats of scratch.  Async on `stream`. */
int dfq_chunk_range(const float* x, int64_t rows, int64_t row_len, float* rowbuf, float* out2, void* stream);
/* QuantMeasure.forward's statistics (utils/quantize.py:94-126), async, two
 * launches: mn / mx = the means over rows of x.view(rows, -1)'s row mins / maxs
 * (fp32, ATen's sum order); update_stat: running_max = mx if mx > running_max
 * (running_min likewise); training: running_* = running_* * (1 - momentum) +
 * (mn|mx) * momentum (fp32 ops, in that order, after the update).  out2 (2 device
 * floats) = the range the fake quant then uses: (mn, mx) in training, the running
 * values otherwise.  words: 2*rows device uint32 of per-observer scratch, zeroed
 * ONCE by the caller; every call leaves them zeroed again.  Replaces the
 * QuantMeasure statistics of the reference (no C counterpart there). */
int dfq_act_observe(const float* x, int64_t rows, int64_t row_len, uint32_t* words, float* running_min,
                    float* running_max, int32_t update_stat, int32_t training, double momentum, float* out2,
                    void* stream);
/* Whole-tensor (min, max) on the device, async: range_enc (2 device uint32) =
 * {~enc(min), enc(max)} in the library's order-preserving encoding (the input of
 * dfq_fake_quant_given); it is zeroed on `stream` first. */
int dfq_range(const float* x, int64_t n, uint32_t* range_enc, void* stream);
/* quantize(x, bits, min, max, symmetric) with a GIVEN range, elementwise and async
 * (QuantMeasure.forward at inference, utils/quantize.py:112-126, and the Quant*
 * layers' weight/bias fake quant, :225-238): the range is, by priority,
 * range_enc (dfq_range's output), min_dev[0] / max_dev[0] (device floats, e.g. the
 * observer's running_min / running_max, read as float() would: exact doubles), or
 * given_min / given_max.  flags: 0 (scale in double: Python-float bounds) or
 * DFQ_SCALE_F32 (0-d tensor bounds).  No workspace, no host synchronisation. */
int dfq_fake_quant_given(const float* x, float* y, int64_t n, int32_t bits, int32_t symmetric, int32_t flags,
                         const float* min_dev, const float* max_dev, const uint32_t* range_enc, double given_min,
                         double given_max, void* stream);

/* quantize(x, bits, float(x.min()), float(x.max()), symmetric) -- the Quant* layers'
 * weight / bias fake quant (utils/quantize.py:225-238) on the tensor's own range --
 * in one async call: dfq_range + dfq_fake_quant_given without the fill.  n <= 16384:
 * one workgroup, one launch (words may be NULL); larger: a range launch whose last
 * block publishes the range and re-arms `words`, then the elementwise launch.
 * words: 8 device uint32 of caller scratch, zero when allocated, left armed by every
 * call (one set per stream: calls on two streams must not share it).  flags: 0 or
 * DFQ_SCALE_F32, as dfq_fake_quant_given. */
int dfq_fake_quant_tensor(const float* x, float* y, int64_t n, int32_t bits, int32_t symmetric, int32_t flags,
                          uint32_t* words, void* stream);

/* ---- grouped sweep over many tensors (replaces quantize_targ_layer,
 *      utils/layer_transform.py:288-305, fused with clip_weight.py:4-33 and the
 *      bias-correction error reduction bias_correction.py:111-144,231) ------- */
typedef struct dfq_sweep_plan dfq_sweep_plan;
typedef struct dfq_sweep_stats {
    int64_t n_tensors;
    int64_t n_elems;          /* sum of rows*row_len */
    int64_t n_tasks_reduce;   /* wave tasks of the range-reduction launch (0 = launch skipped) */
    int64_t n_tasks_main;     /* wave tasks of the quantize launch */
    int64_t algo_bytes;       /* algorithmic HBM bytes of one execute */
    int32_t launches;         /* kernel launches per execute (1, or 2 with a reduce pass) */
    int32_t grid_blocks;      /* blocks of the quantize launch */
    int32_t variant;          /* kernel variant (env DFQ_SWEEP_VARIANT at create) */
    int32_t reserved;
} dfq_sweep_stats;
/* Uploads the descriptor/task tables once into a private allocation (a blocking
 * copy).  descs is copied. */
int dfq_sweep_plan_create(const dfq_tensor_desc* descs, int32_t n, dfq_sweep_plan** plan);
/* The same with the tables in a caller workspace of >= dfq_sweep_plan_ws_bytes
 * bytes (256-B aligned, stream-ordered with `stream`, alive while the plan runs;
 * e.g. the framework's caching allocator): no hipMalloc / hipFree, and destroy
 * needs no device sync.  The upload is stream-ordered on `stream` (pinned
 * staging ring, no host wait). */
int64_t dfq_sweep_plan_ws_bytes(const dfq_tensor_desc* descs, int32_t n);
int dfq_sweep_plan_create_ws(const dfq_tensor_desc* descs, int32_t n, void* ws, int64_t ws_bytes, void* stream,
                             dfq_sweep_plan** plan);
int dfq_sweep_plan_execute(dfq_sweep_plan* plan, void* stream);
int dfq_sweep_plan_stats(const dfq_sweep_plan* plan, dfq_sweep_stats* stats);
int dfq_sweep_plan_destroy(dfq_sweep_plan* plan);

/* ---- BatchNorm folding (merge_batchnorm, utils/layer_transform.py:255-281) ---
 * w[o,:] *= g[o]/sqrt(v[o]+eps);  bias[o] = bias[o]*f[o] + (b[o] - g[o]*m[o]/sqrt(v[o]+eps));
 * fake_w = |g|, fake_b = b (either may be NULL); then the BN becomes identity:
 * g=1, v=1, b=0, m=0 (the caller sets module.eps = 0).  rows = O, row_len = numel/O. */
int dfq_bn_fold(float* w, float* bias, float* bn_w, float* bn_b, float* bn_mean, float* bn_var,
                float* fake_w, float* fake_b, float eps, int64_t rows, int64_t row_len,
                void* stream);

/* All BN folds of a model in two launches: one descriptor per (BN, producer
 * layer) pair, each weight at most once per call; eps per BN.  Stream-ordered
 * with a workspace, blocking without one (see ws below). */
enum { DFQ_BN_FOLD_ZERO_BIAS = 1 };
typedef struct dfq_bn_fold_desc {
    float* w;
    float* bias;
    float* bn_w;
    float* bn_b;
    float* bn_mean;
    float* bn_var;
    float* fake_w;      /* may be NULL */
    float* fake_b;      /* may be NULL */
    float  eps;
    int32_t flags;      /* DFQ_BN_FOLD_ZERO_BIAS: `bias` holds no value yet and is read as 0
                         * (the zeros the reference gives a bias-less layer) */
    int64_t rows;
    int64_t row_len;
    uint32_t* range_enc; /* may be NULL: 2 device words receiving the folded weight's (min, max) in
                          * dfq_range's encoding (zeroed by the call), for a later sweep with
                          * DFQ_DEVICE_RANGE.  Rows whose factor is exactly 1 (merge_batchnorm #2)
                          * are read, not rewritten (w * 1 == w) */
} dfq_bn_fold_desc;
/* Device workspace bytes for dfq_bn_fold_batch's job tables (-1: bad arguments). */
int64_t dfq_bn_fold_ws_bytes(const dfq_bn_fold_desc* descs, int32_t n);
/* ws: >= dfq_bn_fold_ws_bytes bytes, 256-B aligned, stream-ordered with `stream`
 * (e.g. the framework's caching allocator), or NULL: private tables (a
 * hipMalloc / hipFree per call).  With ws the call is stream-ordered (tables go
 * up through the library's pinned staging ring; no host wait); with NULL it
 * synchronizes the stream before freeing its private tables. */
int dfq_bn_fold_batch(const dfq_bn_fold_desc* descs, int32_t n, void* ws, int64_t ws_bytes, void* stream);

/* ---- weight clipping (clip_weight.py:18-29): w = min(max(w, lo), hi), in place */
int dfq_clamp(float* w, int64_t n, float lo, float hi, void* stream);
/* clip_weight over every target layer: `count` weights (16-B aligned, w[k] of
 * n[k] floats), up to 64 per launch. */
int dfq_clamp_batch(float* const* w, const int64_t* n, int32_t count, float lo, float hi, void* stream);

/* ---- cross-layer equalization (Cross_layer_equal.py) -------------------- */
/* Workspace bytes for one relation with c1 = W1.shape[0] channels. */
size_t dfq_cle_ws_bytes(int64_t c1);
/* One relation (_layer_equalization, Cross_layer_equal.py:11-59), in place:
 *   W1 [c1, len1] rows, W2 [o2, i2, khw2], B1/bn_w/bn_b [c1] (each may be NULL),
 *   groups G = (c1 == i2) ? 1 : c1 / i2.
 * S (may be NULL) receives the per-channel scale; S_acc (may be NULL) is
 * multiplied by it (Relation.set_scale_vec, utils/relation.py:26-30; pass
 * s_acc_init=1 on the first call to store instead of multiply). */
int dfq_cle_relation(float* w1, float* w2, float* b1, float* bn_w, float* bn_b,
                     int64_t c1, int64_t len1, int64_t o2, int64_t i2, int64_t khw2,
                     double s_min, double s_max, int32_t is_signed, float eps,
                     float* S, float* S_acc, int32_t s_acc_init,
                     void* ws, size_t ws_bytes, void* stream);
/* Convergence metric of Cross_layer_equal.py:83,107-108 for a set of layers:
 * out_mean[l] = (double)(float)( sum|W_l - snap_l| / n_l ), then snap_l := W_l.
 * Blocking: waits for the stream and copies the n means to host memory. */
typedef struct dfq_diff_plan dfq_diff_plan;
int dfq_diff_plan_create(float* const* w, float* const* snap, const int64_t* n, int32_t count,
                         dfq_diff_plan** plan);
int dfq_diff_plan_snapshot(dfq_diff_plan* plan, void* stream);  /* snap := W, async */
int dfq_diff_plan_execute(dfq_diff_plan* plan, double* out_mean, void* stream);
int dfq_diff_plan_destroy(dfq_diff_plan* plan);

/* Device-resident cross_layer_equalization loop (Cross_layer_equal.py:63-116).
 * One relation of the loop (:86-104); pointers are device memory, in place. */
typedef struct dfq_cle_rel {
    float* w1;          /* graph[layer_first].weight, [c1, len1] */
    float* w2;          /* graph[layer_second].weight, [o2, i2, khw2] */
    float* b1;          /* graph[layer_first].bias [c1] (the caller adds the zero bias of :93-94) */
    float* bn_w;        /* graph[bn_idx].fake_weight [c1] or NULL */
    float* bn_b;        /* graph[bn_idx].fake_bias [c1] or NULL */
    float* s_acc;       /* Relation.S [c1] (set_scale_vec, utils/relation.py:26-30) or NULL */
    int64_t c1, len1, o2, i2, khw2;
    int32_t s_acc_init; /* Relation.S was None: the first iteration stores s */
    int32_t reserved;
} dfq_cle_rel;
typedef struct dfq_cle_plan dfq_cle_plan;
/* Workspace bytes for the plan's weight snapshots (the `W_prev` of :83,107):
 * one fp32 copy of every target, each 256-B aligned; -1 on bad arguments. */
int64_t dfq_cle_plan_ws_bytes(const int64_t* target_n, int32_t n_targets);
/* targets: the weights of every Target_list layer in graph order (the diff list of
 * :107); ref_threads: torch's intra-op thread count whose fp32 mean order the
 * metric reproduces. Relations touching a common tensor keep their order; the
 * others run concurrently (bit-identical: they commute).
 * ws: caller-owned device workspace of >= dfq_cle_plan_ws_bytes bytes, 256-B
 * aligned, alive until destroy (e.g. from the framework's caching allocator), or
 * NULL: the plan allocates it. */
int dfq_cle_plan_create(const dfq_cle_rel* rels, int32_t n_rel, float* const* targets,
                        const int64_t* target_n, int32_t n_targets, double s_min, double s_max,
                        int32_t is_signed, float eps, int32_t ref_threads, void* ws, int64_t ws_bytes,
                        dfq_cle_plan** plan);
/* Runs the loop `while diff > threshold and iter_count < count` (at most
 * max_iters iterations); blocking.  iterations = iterations run; diffs[i] (room for
 * max_iters doubles, may be NULL) = the per-iteration diff (np.sum of the list). */
int dfq_cle_plan_run(dfq_cle_plan* plan, double threshold, int32_t count, int32_t max_iters,
                     int32_t* iterations, double* diffs, void* stream);
/* The same loop, asynchronous (a worker thread reads the stop rule back between
 * batches): `stream`'s earlier work runs before the loop, and everything enqueued
 * on `stream` after this call waits in the device until the loop is done -- the
 * caller's thread goes on enqueueing the next stages meanwhile (the caller's
 * stream waits behind a one-wave gate kernel that polls the library's signal
 * word; it gives up after 120 s, and the join then reports the run failed).
 * A launched run is time-bounded: it stops enqueueing iterations 60 s after the
 * launch, releases the caller's stream and reports the run failed at join (the
 * stages queued behind it then ran on partially equalized weights, so the join's
 * error must not be ignored); a blocking run (dfq_cle_plan_run) has no time
 * bound and stops at max_iters.
 * One launched plan per device at a time (a launch first joins the previous one).
 * DFQ_ERR_UNSUPPORTED: the device cannot make a stream wait on a value (run
 * dfq_cle_plan_run instead). */
int dfq_cle_plan_launch(dfq_cle_plan* plan, double threshold, int32_t count, int32_t max_iters, void* stream);
/* Waits for a launched run; its result as dfq_cle_plan_run's (diffs: room for
 * max_iters doubles, may be NULL).  destroy also waits. */
int dfq_cle_plan_join(dfq_cle_plan* plan, int32_t* iterations, double* diffs);
/* chains = independent relation groups, steps = relations per chain (max),
 * launches = kernel launches per iteration (fused schedule: one range launch for
 * the whole iteration; DFQ_CLE_FUSED=0: one per step) */
int dfq_cle_plan_info(const dfq_cle_plan* plan, int32_t* chains, int32_t* steps, int32_t* launches);
/* Measurement (no reference counterpart): with timing on, the next run records one
 * HIP event pair on the loop's stream around its launches.  stats: bytes[3] = the
 * algorithmic HBM bytes of ONE iteration (rescales incl. the per-channel vectors,
 * metric tiles, weight-reading range tasks), loop_ms = the last timed run's device
 * time from its first launch to its last (-1 if not timed), launched = the
 * iteration groups it enqueued (iterations + the queued no-op ones). */
int dfq_cle_plan_set_timing(dfq_cle_plan* plan, int32_t on);
int dfq_cle_plan_stats(const dfq_cle_plan* plan, int64_t* bytes, double* loop_ms, int32_t* launched);
int dfq_cle_plan_destroy(dfq_cle_plan* plan);

/* ---- pair statistics: per-channel signal, noise, worst error and range -----
 * (no working reference counterpart: the reference's quantize_error.py raises).
 * Many (reference x, compared y) fp32 tensor pairs in one call, each viewed as
 * [rows, row_len] like the sweep.  With e_i = fl32(y_i - x_i) (the fp32 difference
 * of the sweep's esum), row r's record is 4 doubles:
 *   [0] signal  = sum_i (double)x_i * (double)x_i
 *   [1] noise   = sum_i (double)e_i * (double)e_i
 *   [2] max_err = max_i |e_i|   (an fp32 value widened)
 *   [3] max_abs = max_i |x_i|   (an fp32 value widened)
 * and the pair's totals are {sum_r signal, sum_r noise, max_r max_err, max_r max_abs}.
 * Sums are accumulated in fp64 (every term is an exact double).  A pair's result
 * is the same bits from run to run, whatever the grid, the rest of the list or
 * the pair's place in it: the partition depends on the pair's shape only, partial
 * sums are combined in a fixed index order, and no floating-point atomic is used
 * (which elements a lane adds depends on x's address modulo 16).  Non-finite
 * inputs are outside the contract, as for weights. */
enum { DFQ_PAIR_PIECE_ELEMS = 8192 };   /* a row longer than this is cut into pieces of this many elements */
typedef struct dfq_pair_desc {
    const float* x;         /* reference, 4-B aligned */
    const float* y;         /* compared, same shape, 4-B aligned */
    double*      rows_out;  /* [rows][4] or NULL */
    double*      total_out; /* [4] or NULL (not both NULL) */
    int64_t      rows;      /* >= 1 */
    int64_t      row_len;   /* >= 1 */
} dfq_pair_desc;
/* Device workspace bytes for dfq_pair_stats_batch (-1: bad arguments). */
int64_t dfq_pair_stats_ws_bytes(const dfq_pair_desc* descs, int32_t n);
/* Two launches, asynchronous on `stream`, no host wait (the tables go up through
 * the library's pinned staging ring).  ws: >= dfq_pair_stats_ws_bytes bytes,
 * 256-B aligned, stream-ordered with `stream` (e.g. the framework's caching
 * allocator); DFQ_ERR_WORKSPACE if it is NULL or too small, DFQ_ERR_INVALID if it
 * is misaligned.  x and y are only
 * read; where their addresses differ modulo 16 the pair is read with 4-B loads.
 * n == 0: DFQ_OK, nothing launched. */
int dfq_pair_stats_batch(const dfq_pair_desc* descs, int32_t n, void* ws, int64_t ws_bytes, void* stream);

/* ---- clip-range search: the clamp that minimizes a weight's own quantization
 *      noise (no reference counterpart: the reference's clip_weight.py clamps to
 *      a fixed [-15, 15]) -----------------------------------------------------
 * A unit is one row of the [rows, row_len] view in the CHANNEL modes and the whole
 * tensor in the TENSOR modes.  For a unit with fp32 data range (mn, mx), candidate
 * k of K = `candidates` is
 *   a_k  = (float)(1.0 - k * (1.0 - (double)min_frac) / (K - 1))     (a_0 = 1; K = 1: a_0 only)
 *   lo_k = a_k * mn,  hi_k = a_k * mx                                 (fp32 multiplies)
 *   c_i  = min(max(x_i, lo_k), hi_k)
 *   y_i  = the sweep's quantize-dequantize of c_i on c's data range
 *          (min(max(mn, lo_k), hi_k), min(max(mx, lo_k), hi_k)) at `bits` in `mode`
 *   noise_k = sum_i (double)e_i * (double)e_i,  e_i = fl32(y_i - x_i) -- against the UNCLAMPED x_i
 * and the choice is the smallest noise_k, ties to the smallest k (so a constant
 * unit chooses 0, and the chosen noise never exceeds the min-max range's).  Unless
 * DFQ_CLIP_SEARCH_DRY is set, w then holds c of the chosen k, and a sweep of w in
 * the same mode and bits reproduces y bit for bit.  Every term of a sum is an
 * exact double; the sums round.  A unit's results are the same bits from run to
 * run, whatever the rest of the list or the unit's place in it (the partition
 * depends on the shape alone, partials combine in index order, no floating-point
 * atomic).  Non-finite weights are outside the contract. */
enum { DFQ_CLIP_PIECE_ELEMS = 4096 };  /* a unit longer than this is cut into pieces of this many elements */
enum { DFQ_CLIP_MAX_CANDIDATES = 64 };
enum { DFQ_CLIP_SEARCH_DRY = 1 };      /* search and report; leave w untouched */
typedef struct dfq_clip_search_desc {
    float*    w;          /* in place, 4-B aligned */
    int64_t   rows;       /* >= 1 */
    int64_t   row_len;    /* >= 1 */
    int32_t   bits;       /* 2..16 */
    int32_t   mode;       /* DFQ_TENSOR_ASYM ... DFQ_CHANNEL_SYM */
    int32_t   candidates; /* K: 1..DFQ_CLIP_MAX_CANDIDATES */
    int32_t   flags;      /* DFQ_CLIP_SEARCH_DRY or 0 */
    float     min_frac;   /* the narrowest candidate's share of the range, in [0, 1] */
    int32_t   reserved;
    /* outputs, each may be NULL; units = rows (CHANNEL modes) or 1 (TENSOR modes) */
    int32_t*  choice;     /* [units] the chosen k */
    float*    range;      /* [units][2] the chosen (lo_k, hi_k) */
    double*   noise;      /* [units][2] noise_0 and the chosen noise_k */
    uint32_t* range_enc;  /* TENSOR modes: 2 words, {~enc(min), enc(max)} of the tensor as the call leaves
                           * it (clamped, or untouched under DFQ_CLIP_SEARCH_DRY), dfq_range's encoding:
                           * a later sweep with DFQ_DEVICE_RANGE stays one pass.  CHANNEL modes: ignored */
} dfq_clip_search_desc;
/* Device workspace bytes for dfq_clip_search_batch (-1: bad arguments). */
int64_t dfq_clip_search_ws_bytes(const dfq_clip_search_desc* descs, int32_t n);
/* Asynchronous on `stream`, no host wait (the tables go up through the library's
 * pinned staging ring): one launch when no unit is longer than a piece, else a
 * range, a piece, a finish and a clamp launch (launches without work are skipped).
 * ws as for dfq_pair_stats_batch: >= dfq_clip_search_ws_bytes bytes, 256-B aligned,
 * stream-ordered with `stream`; DFQ_ERR_WORKSPACE if it is NULL or too small,
 * DFQ_ERR_INVALID if it is misaligned or a descriptor is bad (bits, candidates,
 * min_frac outside [0, 1] or NaN, mode, unknown flags, sizes, alignment).  Each
 * weight at most once per call.  n == 0: DFQ_OK, nothing launched. */
int dfq_clip_search_batch(const dfq_clip_search_desc* descs, int32_t n, void* ws, int64_t ws_bytes, void* stream);

/* ---- OCP Microscaling (MX) block-scaled weight quantization (no reference
 *      counterpart; the operand format of CDNA4's scaled matrix instructions) ----
 * Every row of the [rows, row_len] view is cut into blocks of DFQ_MX_BLOCK = 32
 * consecutive elements, nb = ceil(row_len / 32) per row (blocks never cross rows; a
 * last partial block behaves as if padded with +0).  Element formats: FP4 E2M1
 * (magnitudes 0 0.5 1 1.5 2 3 4 6, emax 2), FP8 E4M3 "fn" (bias 7, subnormals,
 * maximum 448, no infinities, emax 8), FP6 E2M3 (bias 1, subnormals m/8, normals
 * (8+m) * 2^(e-4), maximum 7.5, emax 2) and FP6 E3M2 (bias 3, subnormals m/16, normals
 * (4+m) * 2^(e-5), maximum 28, emax 4); the FP6 formats have no infinity or NaN code.
 * For one block of fp32 elements x_i:
 *   amax = max |x_i|;  X = amax == 0 ? -127 : clamp(floor(log2 amax) - emax, -127, 127)
 *   scale byte = X + 127 (E8M0; 0xFF is never written)
 *   q_i  = |x_i| * 2^-X rounded to the nearest magnitude of the format, ties to the
 *          even code, saturating at the maximum (6, 448, 7.5 or 28; no E4M3 NaN code)
 *   code = the sign bit of x_i (kept by -0 and by values that round to zero) above
 *          q_i's encoding: a nibble `s e e m`, a byte `s eeee mmm`, or six bits
 *          `s ee mmm` (E2M3) / `s eee mm` (E3M2)
 *   y_i  = +-q_i * 2^X (exact in fp32)
 * Outputs, each optional (not all NULL):
 *   dst    fp32 y, [rows, row_len]; may alias src
 *   codes  uint8 [rows, nb, 16] (FP4: element 2k in the low nibble, 2k+1 in the high
 *          one), [rows, nb, 32] (FP8) or [rows, nb, 24] (FP6: the block's 32 codes packed
 *          densely, little-endian -- element i is bits [6i, 6i+6) of the block's 192-bit
 *          string, byte b its bits [8b, 8b+8); four elements w = c0 | c1<<6 | c2<<12 |
 *          c3<<18 are the bytes w & 0xFF, (w>>8) & 0xFF, w>>16); the padding of a partial
 *          block is +0 codes
 *   scales uint8 [rows, nb]
 *   esum   fp32 [rows * row_len / khw], the sweep's E[p] = sum_{k<khw} fl32(y - x)[p*khw + k]
 *          in ATen's CPU order; row_len % khw != 0 with esum set: DFQ_ERR_SHAPE
 * Contract domain: finite inputs whose non-zero magnitudes are >= 2^-100.  A
 * tensor's result is the same bits from run to run, whatever the rest of the list or
 * its place in it: a block's result depends on its 32 elements alone, every error sum
 * is added by one lane in a fixed order, and no atomic is used. */
enum { DFQ_MX_BLOCK = 32 };
enum { DFQ_MX_FP4_E2M1 = 0, DFQ_MX_FP8_E4M3 = 1 };
enum { DFQ_MX_FP6_E2M3 = 0x23, DFQ_MX_FP6_E3M2 = 0x32 };   /* (exponent bits, mantissa bits); 2 is no format */
/* Elements one wave task holds at most; with esum and khw > 1 (the errors wait in
 * LDS for their sums) DFQ_MX_ESUM_TASK_ELEMS.  A row longer than that is cut into
 * pieces that are multiples of 32 and, with such an esum, of khw: when no such
 * piece fits (lcm(32, khw) > DFQ_MX_ESUM_TASK_ELEMS) the call returns
 * DFQ_ERR_UNSUPPORTED; every khw <= 64 and every row that fits one task are served. */
enum { DFQ_MX_TASK_ELEMS = 4096, DFQ_MX_ESUM_TASK_ELEMS = 2048 };
typedef struct dfq_mx_desc {
    const float* src;      /* 4-B aligned */
    float*       dst;      /* may be NULL, may alias src */
    uint8_t*     codes;    /* may be NULL */
    uint8_t*     scales;   /* may be NULL */
    float*       esum;     /* may be NULL */
    int64_t      rows;     /* >= 1 */
    int64_t      row_len;  /* >= 1 */
    int32_t      khw;      /* >= 1; spatial size for esum (1 for Linear / 1x1) */
    int32_t      format;   /* DFQ_MX_FP4_E2M1 | DFQ_MX_FP8_E4M3 | DFQ_MX_FP6_E2M3 | DFQ_MX_FP6_E3M2 */
    int32_t      flags;    /* 0 */
    int32_t      reserved;
} dfq_mx_desc;
/* Device workspace bytes for dfq_mx_quantize_batch (-1: bad arguments). */
int64_t dfq_mx_quantize_ws_bytes(const dfq_mx_desc* descs, int32_t n);
/* Every tensor of the list in one launch (two for a list that mixes FP6 tensors with
 * FP4 / FP8 ones) and one HBM pass, asynchronous on `stream`,
 * no host wait (the tables go up through the library's pinned staging ring).  ws as
 * for dfq_clip_search_batch: >= dfq_mx_quantize_ws_bytes bytes, 256-B aligned,
 * stream-ordered with `stream`; DFQ_ERR_WORKSPACE if it is NULL or too small,
 * DFQ_ERR_INVALID if it is misaligned or a descriptor is bad (format, non-zero flags,
 * sizes, khw < 1, a NULL or misaligned src, dst or esum not 4-B aligned, every output
 * NULL).  Rows whose start is 16-B aligned (src, dst and esum 16-B aligned, codes
 * 4-B aligned, row_len % 4 == 0) take 16-B loads; the others a 4-B path with the
 * same results.  Each tensor at most once per call.  n == 0: DFQ_OK, nothing launched. */
int dfq_mx_quantize_batch(const dfq_mx_desc* descs, int32_t n, void* ws, int64_t ws_bytes, void* stream);
/* dfq_mx_quantize_batch with a noise-minimizing choice of the block's exponent: the same
 * descriptors (flags stays 0), workspace (dfq_mx_quantize_ws_bytes), error codes, launches and
 * mixed-list rule; every line of the contract above holds except the one for X.
 * For a block with amax != 0 let X0 be the floor rule's exponent above, X1 = X0 + 1
 * (X0 <= 127 - emax, so the scale byte stays below 0xFF), y0 / y1 the block's y under
 * X0 / X1 and
 *   N_d = sum_i (fl32(y_i^d - x_i) * 2^-X0)^2      (the factor is exact in fp32)
 * The block takes X1 iff N_1 < N_0, strictly, else X0; the chosen X defines codes, scales,
 * dst and esum.  A block with amax == 0 keeps X = -127 (scale byte 0, +0 / -0 codes).
 * X1 lifts the clamp of a block whose amax * 2^-X0 lies above the format's maximum at the
 * price of a grid twice as coarse; no other exponent is tried.
 * The sums are formed in fp32: four rounded squares per lane in element order, then three
 * pairwise exchanges across the block's eight lanes -- within 33 * 2^-24 relative of the
 * real sums, so the choice is the real-number one wherever N_0 and N_1 differ by more than
 * 2^-18 of the larger.  Both sums run through one instruction sequence: a block whose y0 and
 * y1 are equal element for element (zeros, a single power-of-two element) ties and keeps
 * X0.  A tensor's result is the same bits from run to run, alone or anywhere in a list,
 * with dst aliasing src or not, and on the 16-B and the 4-B path. */
int dfq_mx_quantize_search_batch(const dfq_mx_desc* descs, int32_t n, void* ws, int64_t ws_bytes, void* stream);

/* ---- MX matrix multiply on the scaled matrix instruction (no reference counterpart) ----
 * out[m][n] = sum_k A[m][k] * B[n][k] (+ bias[n]), A and B given as MX codes and scale
 * bytes in exactly the layouts dfq_mx_quantize_batch writes (both operands K-contiguous,
 * nb = ceil(K / 32) blocks per row, cb = 16 / 24 / 32 code bytes per block, the padding of
 * a partial last block +0 codes), each in any of the four formats.  The product runs on
 * v_mfma_scale_f32_16x16x128_f8f6f4, which reads the stored code bytes and scale bytes
 * as they are: no dequantized operand is ever written to memory.
 * Numerics: with a_mk, b_nk the values the codes stand for (y = +-q * 2^(scale - 127)),
 * every product a*b has at most 8 significant bits and is exact in fp32.  Domain: scale
 * bytes with |X_a + X_b| <= 100 (X = scale - 127) for every pair of blocks that meet, so
 * nothing leaves the normal range; an all-zero block (scale byte 0, +0 codes)
 * contributes 0.  The instruction's summation order and internal width are not
 * specified, so the contract is a bound, |acc - sum a*b| <= c(nb) * sum |a*b|:
 *   c = 32 * nb * 2^-24, which any-order fp32 accumulation of the exact products meets
 *       and the hardware was measured to meet at nb = 13 and 40 (worst 0.17 of it);
 *   c = 6.4e-5 for nb <= 4 (one K step): with an FP8 operand the instruction's own error,
 *       about 2^-13 of the step's largest product whatever K, was measured at up to
 *       3.2e-5 * sum |a*b| (K = 24), above the derived bound; twice that is documented.
 * Where every partial sum in any order is exact in fp32 (integer-like data) the result is
 * exact; products of FP6 / FP4 operands alone were exact in every measurement (DESIGN.md
 * 3.8).  The bias is one fp32 add after the accumulation.  An element's result is the same bits from run to run
 * and does not depend on ldo, on the addresses or on other calls: one lane's accumulator
 * in K order, no atomics, no split of K.
 * Asynchronous on `stream`, no host wait, no workspace.  Checked on the host before any
 * device call: DFQ_ERR_INVALID for a NULL operand, scale or out pointer, an unknown
 * format, M, N or K < 1 (or beyond 2^31 rows / 2^40 columns), non-zero flags or
 * reserved, a code base not 16-B aligned (FP6: 8-B), out or bias not 4-B aligned;
 * DFQ_ERR_SHAPE for ldo < N.  There is no slow path for misaligned bases. */
typedef struct dfq_mx_gemm_desc {
    const void*  a_codes;   /* uint8 [M, nb, cb(a_format)] */
    const void*  a_scales;  /* uint8 [M, nb] */
    const void*  b_codes;   /* uint8 [N, nb, cb(b_format)] */
    const void*  b_scales;  /* uint8 [N, nb] */
    const float* bias;      /* [N] or NULL */
    float*       out;       /* [M, N] fp32, row stride ldo */
    int64_t      ldo;       /* >= N */
    int64_t      M;
    int64_t      N;
    int64_t      K;         /* nb = ceil(K / 32) */
    int32_t      a_format;  /* DFQ_MX_* as in dfq_mx_desc */
    int32_t      b_format;
    int32_t      flags;     /* 0 */
    int32_t      reserved;  /* 0 */
} dfq_mx_gemm_desc;
int dfq_mx_gemm(const dfq_mx_gemm_desc* d, void* stream);

/* ---- MX linear in one launch: dfq_mx_gemm with the activation quantized in the kernel ----
 * out[m][n] = sum_k Q(x)[m][k] * B[n][k] (+ bias[n]).  B is given as dfq_mx_gemm's B (MX
 * codes and scale bytes); x is fp32 and Q is the MX contract above applied to every row of
 * x in x_format: blocks of 32 along K, a partial last block padded with +0, the floor rule
 * X = floor(log2 amax) - emax, round to nearest with ties to the even code, saturation at
 * the format's maximum, scale byte 0 for an all-zero block.  There is no scale search for
 * the activation.  Each lane of the kernel reads the fp32 elements its operand of the matrix
 * instruction stands for, takes the block's amax and encodes straight into the operand
 * registers (an FP8 lane holds halves of two blocks: one amax exchange with the lane 16
 * away and one gather of the scale byte); Q(x)'s codes never reach memory.
 * The result is bit for bit what dfq_mx_quantize_batch (codes and scales of x) followed by
 * dfq_mx_gemm gives, on all 16 (x_format, b_format) pairs: the same operand registers, one
 * accumulator per output element, the K steps in order, no split of K, no atomics, no
 * workspace, the bias one fp32 add at the end.  So dfq_mx_gemm's numerics and
 * reproducibility statements hold here too.  Domain, the union of the two contracts: finite
 * x whose non-zero magnitudes are >= 2^-100, and |X_a + X_b| <= 100 for blocks that meet.
 * Elements of x at k >= K and rows >= M are never read.  Rows of x that start 16-B aligned
 * and hold whole groups of four (x 16-B aligned, ldx % 4 == 0, K % 4 == 0) take 16-B loads;
 * every other case (K = 30, a column slice that starts at element 3 of a wider tensor) 4-B
 * loads with the same results.
 * Asynchronous on `stream`, no host wait.  Checked on the host before any device call:
 * DFQ_ERR_INVALID for a NULL x, b_codes, b_scales or out, an unknown format, M, N or K < 1
 * (or beyond dfq_mx_gemm's limits; M * ldx beyond 2^50), non-zero flags or reserved, x, out or
 * bias not 4-B aligned, b_codes not 16-B (FP6: 8-B) aligned; DFQ_ERR_SHAPE for ldx < K or
 * ldo < N. */
typedef struct dfq_mx_linear_desc {
    const float* x;         /* fp32 [M, K], K-contiguous, row stride ldx elements; 4-B aligned */
    const void*  b_codes;   /* uint8 [N, nb, cb(b_format)], as dfq_mx_gemm's B */
    const void*  b_scales;  /* uint8 [N, nb] */
    const float* bias;      /* [N] or NULL */
    float*       out;       /* [M, N] fp32, row stride ldo */
    int64_t      ldx;       /* >= K */
    int64_t      ldo;       /* >= N */
    int64_t      M;
    int64_t      N;
    int64_t      K;         /* nb = ceil(K / 32) */
    int32_t      x_format;  /* the MX format x is rounded to (DFQ_MX_*) */
    int32_t      b_format;
    int32_t      flags;     /* 0 */
    int32_t      reserved;  /* 0 */
} dfq_mx_linear_desc;
int dfq_mx_linear(const dfq_mx_linear_desc* d, void* stream);

/* ---- MX convolution in one launch: dfq_mx_linear on the im2col rows, gathered in the kernel ----
 * out[b][n][oh][ow] = sum_k Q(A)[m][k] * B[n][k] (+ bias[n]) with
 *   m = (b * OH + oh) * OW + ow,  k = (c * KH + i) * KW + j,  M = B * OH * OW,  K = C * KH * KW,
 *   A[m][k] = x[b][c][oh * stride_h - pad_h + i * dil_h][ow * stride_w - pad_w + j * dil_w],
 *             +0 where that lies outside the image,
 *   OH = (H + 2 pad_h - dil_h (KH - 1) - 1) / stride_h + 1  (OW alike).
 * x is the fp32 NCHW activation, read in place: the im2col matrix A is never written.  B is
 * the convolution's weight [N, C, KH, KW] as dfq_mx_quantize_batch stores it, rows of K
 * elements with blocks of 32 along (c, kh, kw) -- dfq_mx_gemm's B.  Q is dfq_mx_linear's,
 * applied to the rows of A: blocks of 32 along k, a partial last block padded with +0, the
 * floor rule, no scale search; a padding tap is a +0 element of its block like any other, and
 * a block that lies wholly in padding gets scale byte 0.  Each lane gathers the 32 elements
 * of its operand with 4-B loads (the tap of the run's first k decomposed once per K step,
 * then walked kw -> kh -> c with carries), encodes them with dfq_mx_linear's encoder and
 * exchanges, and the result goes straight to NCHW: a lane's four accumulator registers are
 * four consecutive m of one n, one 16-B store where they lie in one image.
 * The result is bit for bit dfq_mx_linear applied to the materialised [M, K] matrix A, on
 * all 16 (x_format, b_format) pairs: one accumulator per output element, the K steps in
 * order, no split of K, no atomics, no workspace, no LDS, the bias one fp32 add.  Domain and
 * reproducibility: dfq_mx_linear's.
 * Asynchronous on `stream`, no host wait.  Checked on the host before any device call:
 * DFQ_ERR_INVALID for a NULL x, b_codes, b_scales or out, an unknown format, non-zero flags
 * or reserved, an extent (B, C, H, W, N, KH, KW), stride or dilation < 1, a padding < 0, any
 * of these above 2^28, C * H * W, N * OH * OW or K at or above 2^31, M above 2^31, N * K
 * above 2^50 (so every offset stays inside int64 and the offsets inside one image inside
 * int32), x, out or bias not 4-B aligned, b_codes not 16-B (FP6: 8-B) aligned;
 * DFQ_ERR_SHAPE when OH or OW comes out < 1; DFQ_ERR_UNSUPPORTED for a grid beyond int32. */
typedef struct dfq_mx_conv2d_desc {
    const float* x;         /* fp32 [B, C, H, W], contiguous; 4-B aligned */
    const void*  b_codes;   /* uint8 [N, nb, cb(b_format)], nb = ceil(K / 32), as dfq_mx_gemm's B */
    const void*  b_scales;  /* uint8 [N, nb] */
    const float* bias;      /* [N] or NULL */
    float*       out;       /* fp32 [B, N, OH, OW], contiguous */
    int64_t      B;
    int64_t      C;
    int64_t      H;
    int64_t      W;
    int64_t      N;
    int64_t      KH;
    int64_t      KW;
    int64_t      stride_h;
    int64_t      stride_w;
    int64_t      pad_h;
    int64_t      pad_w;
    int64_t      dil_h;
    int64_t      dil_w;
    int32_t      x_format;  /* the MX format the im2col rows are rounded to (DFQ_MX_*) */
    int32_t      b_format;
    int32_t      flags;     /* 0 */
    int32_t      reserved;  /* 0 */
} dfq_mx_conv2d_desc;
int dfq_mx_conv2d(const dfq_mx_conv2d_desc* d, void* stream);

/* ---- integer matrix multiply on the i8 matrix instruction (no reference counterpart) ----
 * out[m][n] = sum_k A[m][k] * B[n][k] (+ bias[n]) of the affine values the sweep's integer
 * codes stand for,
 *   A[m][k] = qa[m][k] * sa + za            (per tensor),
 *   B[n][k] = qb[n][k] * sb[n] + zb[n]      (per tensor, or per row with DFQ_INT_B_PER_ROW),
 * with qa, qb the code bytes read as full 8-bit integers (uint8 when *_signed is 0, int8 when
 * 1; so every 2..8-bit grid in a byte container works and there is no bits field), or, for
 * B with DFQ_INT_B_PACK4, the sweep's DFQ_PACK_INT4 nibbles (element 2k in the low nibble,
 * two's-complement nibbles when b_signed).  Both operands are K-contiguous: a_codes [M, K]
 * bytes, b_codes [N, K] bytes or [N, K / 2] packed bytes (K even, so every row starts on a
 * byte).  The products run on v_mfma_i32_16x16x64_i8 (signed x signed: unsigned bytes are
 * moved to the signed domain by xor 0x80 and the offset is folded back in integers), the row
 * sums on the same instruction against an all-ones operand; no dequantized operand exists.
 * Numerics: with the exact integers
 *   P = sum_k qa * qb,   Sa[m] = sum_k qa,   Sb[n] = sum_k qb
 * (each inside int32 because K <= 32768: 255 * 255 * 32768 < 2^31) the result is
 *   acc  = ((double)sa * (double)sb[n]) * (double)P
 *   acc += ((double)sa * (double)zb[n]) * (double)Sa[m]      -- if b_zero
 *   acc += ((double)za * (double)sb[n]) * (double)Sb[n]      -- if a_zero
 *   acc += ((double)za * (double)zb[n]) * (double)K          -- if both
 *   acc += (double)bias[n]                                   -- if bias
 *   out  = (float)acc
 * in fp64, one IEEE operation per step in this order, no contraction (the float x float
 * products are exact in double): the real-number product of the affine values to within
 * fp64 rounding, rounded once to fp32, and bit for bit what numpy float64 gives.  A NULL
 * zero skips its terms.  An element is one accumulator of one lane, the K steps (64
 * elements) in order, no split of K, no atomics, no workspace: the same bits from run to
 * run, whatever ldo, the addresses or the load path (K % 16 == 0 takes 16-B loads, 8-B for
 * packed B; any other K takes byte loads with the same results).
 * Asynchronous on `stream`, no host wait.  Checked on the host before any device call:
 * DFQ_ERR_INVALID for a NULL a_codes, a_scale, b_codes, b_scale or out, M, N or K < 1 (M or
 * N above 2^40), a_signed or b_signed not 0 / 1, unknown flags, non-zero reserved, a code
 * base not 16-B aligned, out, bias, a scale or a zero not 4-B aligned; DFQ_ERR_SHAPE for
 * ldo < N; DFQ_ERR_UNSUPPORTED for K > 32768, packed B with an odd K, a grid beyond int32. */
#define DFQ_INT_B_PACK4    0x1  /* b_codes holds packed nibbles (DFQ_PACK_INT4's layout) */
#define DFQ_INT_B_PER_ROW  0x2  /* b_scale / b_zero hold N values (per output channel), else 1 */
#define DFQ_INT_MAX_K      32768  /* the largest K: 255 * 255 * 32768 < 2^31 */
typedef struct dfq_int_gemm_desc {
    const void*  a_codes;   /* [M, K] bytes */
    const float* a_scale;   /* device, 1 value */
    const float* a_zero;    /* device, 1 value, or NULL (0) */
    const void*  b_codes;   /* [N, K] bytes, or [N, K / 2] with DFQ_INT_B_PACK4 */
    const float* b_scale;   /* device, 1 or N values */
    const float* b_zero;    /* device, 1 or N values, or NULL (0) */
    const float* bias;      /* [N] or NULL */
    float*       out;       /* [M, N] fp32, row stride ldo */
    int64_t      ldo;       /* >= N */
    int64_t      M;
    int64_t      N;
    int64_t      K;         /* <= 32768 */
    int32_t      a_signed;  /* 0: uint8 codes, 1: int8 codes */
    int32_t      b_signed;
    int32_t      flags;     /* DFQ_INT_B_PACK4 | DFQ_INT_B_PER_ROW */
    int32_t      reserved;  /* 0 */
} dfq_int_gemm_desc;
int dfq_int_gemm(const dfq_int_gemm_desc* d, void* stream);

/* ---- integer linear in one launch: dfq_int_gemm with the activation quantized in the kernel ----
 * The same product with A given as fp32 x [M, K] (row stride ldx), quantized to x_bits
 * (2..8) inside the kernel by dfq_fake_quant_given's quantizer: the range is, by priority,
 * min_dev[0] / max_dev[0] (device floats read as exact doubles) or given_min / given_max;
 * flags may hold DFQ_SCALE_F32 (0-d tensor bounds) next to dfq_int_gemm's; the parameters
 * are make_qparams' and the code of an element is the q of
 *   q = rint(clamp((x + negmn) / s, qmin, qmax)),
 * uint8 when x_symmetric is 0 and int8 when 1, with sa = s and za = min (+0 when symmetric,
 * always present).  Each lane quantizes the 16 elements its operand of the instruction
 * stands for; the codes of x never reach memory.  The result is bit for bit what
 * dfq_quantize_tensor (given range; codes, scale and zero of x) followed by dfq_int_gemm
 * gives.  A NaN element of x takes qmin's code -- fminf(fmaxf(NaN, qmin), qmax), this library's
 * rule, not the reference's -- and the range may have any finite scale (above 2^126, where 1 / s
 * is no normal float, every element takes the IEEE divide).  Elements at k >= K and rows >= M are
 * never read.  x 16-B aligned with ldx % 4 == 0
 * and K % 4 == 0 takes 16-B loads, every other case 4-B loads with the same results.
 * Checks as dfq_int_gemm's, and DFQ_ERR_INVALID for a NULL x, x_bits outside 2..8,
 * x_symmetric not 0 / 1, x, min_dev or max_dev not 4-B aligned; DFQ_ERR_SHAPE for ldx < K. */
typedef struct dfq_int_linear_desc {
    const float* x;         /* fp32 [M, K], K-contiguous, row stride ldx elements */
    const float* min_dev;   /* device float or NULL: the range's min (else given_min) */
    const float* max_dev;   /* device float or NULL: the range's max (else given_max) */
    const void*  b_codes;   /* as dfq_int_gemm's */
    const float* b_scale;
    const float* b_zero;
    const float* bias;
    float*       out;
    double       given_min;
    double       given_max;
    int64_t      ldx;       /* >= K */
    int64_t      ldo;       /* >= N */
    int64_t      M;
    int64_t      N;
    int64_t      K;
    int32_t      x_bits;    /* 2..8 */
    int32_t      x_symmetric;
    int32_t      b_signed;
    int32_t      flags;     /* DFQ_INT_B_PACK4 | DFQ_INT_B_PER_ROW | DFQ_SCALE_F32 */
    int32_t      reserved;  /* 0 */
    int32_t      reserved2; /* 0 */
} dfq_int_linear_desc;
int dfq_int_linear(const dfq_int_linear_desc* d, void* stream);

/* ---- integer convolution in one launch: dfq_int_linear on the im2col rows, gathered in the kernel ----
 * The convolution of the affine values that the codes of x and of the weight stand for, with
 * zero padding: a padding tap has the real value 0 -- its term is absent -- and is NOT the code
 * the quantizer gives 0.0, which on an asymmetric range stands for q0 * s + min != 0.  (F.conv2d
 * of the fake-quantized input pads with a real 0; quantizing the materialised F.unfold matrix
 * does not.)  With
 *   m = (b * OH + oh) * OW + ow,  k = (c * KH + i) * KW + j,  M = B * OH * OW,  K = C * KH * KW,
 *   v[m][k] = 1 where x[b][c][oh * stride_h - pad_h + i * dil_h][ow * stride_w - pad_w + j * dil_w]
 *             lies inside the image, else 0,
 *   OH = (H + 2 pad_h - dil_h (KH - 1) - 1) / stride_h + 1  (OW alike),
 * qa[m][k] the code dfq_fake_quant_given's quantizer gives x at that tap (dfq_int_linear's: the
 * range from min_dev / max_dev or given_min / given_max, x_bits 2..8, sa = s, za = min, +0 when
 * symmetric, always present) and qb [N, K] the weight's codes, rows along (c, kh, kw) -- the order
 * [N, C, KH, KW] is stored in -- as dfq_int_gemm's B (bytes, or nibbles with DFQ_INT_B_PACK4), the
 * exact integers
 *   P[m][n]  = sum_k v qa qb     Sa[m] = sum_k v qa
 *   Sb[m][n] = sum_k v qb        T[m]  = sum_k v
 * (each inside int32 because K <= DFQ_INT_MAX_K) give
 *   acc  = ((double)sa * (double)sb[n]) * (double)P[m][n]
 *   acc += ((double)sa * (double)zb[n]) * (double)Sa[m]       -- if b_zero
 *   acc += ((double)za * (double)sb[n]) * (double)Sb[m][n]
 *   acc += ((double)za * (double)zb[n]) * (double)T[m]        -- if b_zero
 *   acc += (double)bias[n]                                    -- if bias
 *   out[b][n][oh][ow] = (float)acc
 * in fp64, one IEEE operation per step in this order, no contraction.  So the result is bit for
 * bit a numpy float64 statement; where no tap of the geometry falls in padding it is bit for
 * bit dfq_int_linear on the materialised F.unfold matrix [M, K]; and a row wholly in padding
 * stores (float)bias[n] (0 without a bias).  x is read in place, NCHW: a lane gathers the 16
 * consecutive k of its operand with 4-B loads (the run's first tap decomposed once per K step,
 * then walked kw -> kh -> c with carries) and quantizes them; padding taps and k >= K enter the
 * instruction as 0 in its signed domain.  With padding, sum_k v qb depends on the row: the
 * kernel multiplies a 0 / 1 mask operand with B's fragments on the same instruction (ten
 * instructions a K step instead of eight), and T is a closed form of the row's position.  One
 * accumulator per output element, the K steps (64 elements) in order, no split of K, no
 * atomics, no workspace, no LDS: the same bits from run to run.  The result goes straight to
 * NCHW, one 16-B store where a lane's four rows lie in one image.
 * Asynchronous on `stream`, no host wait.  Checked on the host before any device call:
 * DFQ_ERR_INVALID for a NULL x, b_codes, b_scale or out, unknown flags, non-zero reserved or
 * reserved2, b_signed or x_symmetric not 0 / 1, x_bits outside 2..8, an extent (B, C, H, W, N,
 * KH, KW), stride or dilation < 1, a padding < 0, any of these above 2^28, C * H * W,
 * N * OH * OW or K at or above 2^31, M above 2^31, N * K above 2^50, x, out, bias, min_dev,
 * max_dev, b_scale or b_zero not 4-B aligned, b_codes not 16-B aligned; DFQ_ERR_SHAPE when OH
 * or OW comes out < 1; DFQ_ERR_UNSUPPORTED for K > DFQ_INT_MAX_K, packed B with an odd K, a
 * grid beyond int32. */
typedef struct dfq_int_conv2d_desc {
    const float* x;         /* fp32 [B, C, H, W], contiguous; 4-B aligned */
    const float* min_dev;   /* device float or NULL: the range's min (else given_min) */
    const float* max_dev;   /* device float or NULL: the range's max (else given_max) */
    const void*  b_codes;   /* [N, K] bytes, or [N, K / 2] with DFQ_INT_B_PACK4; K = C * KH * KW */
    const float* b_scale;   /* device, 1 or N values */
    const float* b_zero;    /* device, 1 or N values, or NULL (0) */
    const float* bias;      /* [N] or NULL */
    float*       out;       /* fp32 [B, N, OH, OW], contiguous */
    double       given_min;
    double       given_max;
    int64_t      B;
    int64_t      C;
    int64_t      H;
    int64_t      W;
    int64_t      N;
    int64_t      KH;
    int64_t      KW;
    int64_t      stride_h;
    int64_t      stride_w;
    int64_t      pad_h;
    int64_t      pad_w;
    int64_t      dil_h;
    int64_t      dil_w;
    int32_t      x_bits;    /* 2..8 */
    int32_t      x_symmetric;
    int32_t      b_signed;
    int32_t      flags;     /* DFQ_INT_B_PACK4 | DFQ_INT_B_PER_ROW | DFQ_SCALE_F32 */
    int32_t      reserved;  /* 0 */
    int32_t      reserved2; /* 0 */
} dfq_int_conv2d_desc;
int dfq_int_conv2d(const dfq_int_conv2d_desc* d, void* stream);

/* ---- integer depthwise convolution in one launch (packed 8-bit dot products) ----
 * dfq_int_conv2d's statement for groups == C: output channel n of N = C * mult reads input
 * channel c = n / mult and nothing else, so K = KH * KW.  With
 *   k = i * KW + j,
 *   v[b,oh,ow][k] = 1 where the tap (oh * stride_h - pad_h + i * dil_h, ow * stride_w - pad_w + j * dil_w)
 *                   lies inside the image, else 0,
 * qa the code dfq_fake_quant_given's quantizer gives x[b][c] at that tap (dfq_int_linear's: the
 * range from min_dev / max_dev or given_min / given_max, x_bits 2..8, x_symmetric, sa = s,
 * za = min, +0 when symmetric, always present) and qb [N, K] the weight's codes -- the order
 * [N, 1, KH, KW] is stored in; bytes, or [N, K / 2] nibbles with DFQ_INT_B_PACK4 (K even: a
 * 3 x 3 kernel is refused when packed) -- the exact integers
 *   P[b,n,oh,ow]  = sum_k v qa qb     Sa[b,c,oh,ow] = sum_k v qa
 *   Sb[n,oh,ow]   = sum_k v qb        T[oh,ow]      = sum_k v
 * give
 *   acc  = ((double)sa * (double)sb[n]) * (double)P
 *   acc += ((double)sa * (double)zb[n]) * (double)Sa       -- if b_zero
 *   acc += ((double)za * (double)sb[n]) * (double)Sb
 *   acc += ((double)za * (double)zb[n]) * (double)T        -- if b_zero
 *   acc += (double)bias[n]                                 -- if bias
 *   out[b][n][oh][ow] = (float)acc
 * in fp64, one IEEE operation per step in this order, no contraction: bit for bit a numpy
 * float64 statement, and bit for bit dfq_int_conv2d on channel c alone with rows c * mult ..
 * (c + 1) * mult - 1 of B.  A padding tap has the real value 0 (absent from every sum, not the
 * code of 0.0); an output wholly in padding stores (float)bias[n] (0 without a bias).
 * A workgroup owns a tile of at most DFQ_INT_DW_TILE_H x DFQ_INT_DW_TILE_W outputs of one
 * (b, c) plane -- or, where a plane fits one tile, several whole planes -- for all mult output
 * channels: it reads the tile's input footprint with its halo once, quantizes every element
 * once and keeps the code bytes (never the fp32 values) in LDS, 0 where the footprint leaves
 * the image.  The products run on the packed 8-bit dot instruction (v_dot4c_i32_i8, signed x
 * signed: unsigned codes enter as q - 128 on the taps inside the image and the offset is folded
 * back in integers with T where dfq_int_gemm has K); sum_k v qa and sum_k v qb come from the same
 * instruction against an all-ones word and a 0 / 1 mask word.  One accumulator per output
 * element, the taps in order, no atomics, no workspace: the same bits from run to run.
 * Asynchronous on `stream`, no host wait.  Checked on the host before any device call:
 * DFQ_ERR_INVALID for a NULL x, b_codes, b_scale or out, unknown flags, non-zero reserved or
 * reserved2, b_signed or x_symmetric not 0 / 1, x_bits outside 2..8, an extent (B, C, H, W,
 * mult, KH, KW), stride or dilation < 1, a padding < 0, any of these or C * mult above 2^28,
 * C * H * W or N * OH * OW at or above 2^31, B * OH * OW above 2^31, x, out, bias, min_dev,
 * max_dev, b_scale or b_zero not 4-B aligned, b_codes not 16-B aligned; DFQ_ERR_SHAPE when OH or
 * OW comes out < 1; DFQ_ERR_UNSUPPORTED for KH * KW > DFQ_INT_DW_MAX_TAPS, packed B with an odd
 * K, a single output's footprint ((KH - 1) dil_h + 1) * ((KW - 1) dil_w + 1) beyond
 * DFQ_INT_DW_LDS_BYTES, a grid beyond int32. */
#define DFQ_INT_DW_MAX_TAPS   64     /* the largest KH * KW (7 x 7 = 49 fits): a tap mask is one 64-bit word */
#define DFQ_INT_DW_TILE_H     32     /* the largest output tile of a workgroup */
#define DFQ_INT_DW_TILE_W     64
#define DFQ_INT_DW_LDS_BYTES  16384  /* the code bytes a workgroup keeps */
typedef struct dfq_int_dwconv2d_desc {
    const float* x;         /* fp32 [B, C, H, W], contiguous; 4-B aligned */
    const float* min_dev;   /* device float or NULL: the range's min (else given_min) */
    const float* max_dev;   /* device float or NULL: the range's max (else given_max) */
    const void*  b_codes;   /* [N, K] bytes, or [N, K / 2] with DFQ_INT_B_PACK4; N = C * mult, K = KH * KW */
    const float* b_scale;   /* device, 1 or N values */
    const float* b_zero;    /* device, 1 or N values, or NULL (0) */
    const float* bias;      /* [N] or NULL */
    float*       out;       /* fp32 [B, N, OH, OW], contiguous */
    double       given_min;
    double       given_max;
    int64_t      B;
    int64_t      C;
    int64_t      H;
    int64_t      W;
    int64_t      mult;      /* output channels per input channel: N = C * mult */
    int64_t      KH;
    int64_t      KW;
    int64_t      stride_h;
    int64_t      stride_w;
    int64_t      pad_h;
    int64_t      pad_w;
    int64_t      dil_h;
    int64_t      dil_w;
    int32_t      x_bits;    /* 2..8 */
    int32_t      x_symmetric;
    int32_t      b_signed;
    int32_t      flags;     /* DFQ_INT_B_PACK4 | DFQ_INT_B_PER_ROW | DFQ_SCALE_F32 */
    int32_t      reserved;  /* 0 */
    int32_t      reserved2; /* 0 */
} dfq_int_dwconv2d_desc;
int dfq_int_dwconv2d(const dfq_int_dwconv2d_desc* d, void* stream);

/* ---- high-bias absorption (bias_absorption.py:147-197) ------------------
 * c = max(bn_b - N*bn_w, 0) (bn_* = the BN's fake_weight / fake_bias);
 * b2[o] += sum_i (sum_k W2[o,i,k]) * c[g*i2 + i];  b1 -= c;  bn_b -= c.
 * W2 is [o2, i2, khw2], c1 = W1.shape[0], groups = c1 / i2.
 * DFQ_ERR_SHAPE (nothing written): groups must divide o2, and c1 / groups must be
 * i2, as the reference's matmul demands (c1 = 10, i2 = 4 is refused; c1 = 9,
 * i2 = 4 runs, its ninth channel in no group). */
int dfq_bias_absorb(const float* w2, float* b1, float* b2, float* bn_w, float* bn_b,
                    int64_t c1, int64_t o2, int64_t i2, int64_t khw2, float n_sigma,
                    void* stream);
/* Every absorption of a model in two launches (bias_absorption.py:9-121, the
 * relations in the reference's order): all c = clamp(beta - N*gamma, 0) and
 * W2-sum GEMVs first (into the workspace), then one pass per bias element that
 * applies that vector's updates in relation order (b -= c as a layer_first,
 * b += W2sum @ c as a layer_second) and beta -= c -- the same fp32 operations in
 * the same per-element order as one dfq_bias_absorb call per relation.
 * `*failed` = the index of a relation whose shapes are invalid (nothing is
 * enqueued then). */
typedef struct dfq_absorb_desc {
    const float* w2;
    float*       b1;
    float*       b2;
    float*       bn_w;    /* fake_weight of the BN between the layers */
    float*       bn_b;    /* fake_bias (updated) */
    int64_t      c1, o2, i2, khw2;
} dfq_absorb_desc;
int64_t dfq_bias_absorb_ws_bytes(const dfq_absorb_desc* descs, int32_t n);
int dfq_bias_absorb_batch(const dfq_absorb_desc* descs, int32_t n, float n_sigma, void* ws, int64_t ws_bytes,
                          int32_t* failed, void* stream);

/* ---- bias correction (bias_correction.py) -------------------------------
 * dfq_bc_expect: out[j] (+)= relu ? max(0, w*phi(-b/w) + b*(1-Phi(-b/w))) : b
 *                (calculate_mean + branch sum, bias_correction.py:33-53,170-172). */
int dfq_bc_expect(const float* fake_w, const float* fake_b, int64_t n, int32_t relu,
                  int32_t accumulate, float* out, void* stream);
/* dfq_bc_apply: bias_vec[o,j] = E[o, i2>1 ? j : 0] + expect[f>1 ? j : 0] over the
 * broadcast shape [o, bcols]; bias[o] += mean_j bias_vec[o,j] (ATen's sum order)
 * (_compute_final_bias_correction + _apply_bias_correction, :61-106).
 * bias_vec (may be NULL) keeps the [o*bcols] vector for dfq_bc_propagate.
 * A row's order does not depend on the reference's thread count, except for a
 * single row (o == 1) of >= 32768 values, which follows the one-thread order.
 * Returns DFQ_ERR_SHAPE where torch would raise (non-broadcastable, or numel == o). */
int dfq_bc_apply(const float* E, int64_t o, int64_t i2, const float* expect, int64_t f,
                 float* bias, float* bias_vec, int64_t* bcols_out, void* stream);
/* dfq_bc_propagate: fake_b[c] += mean_r ( -bias_vec[r*f + c] ), r < numel/f
 * (bias_prev.view(-1, F).mean(0), bias_correction.py:206-213,251).  The fp32 sums
 * follow ATen's CPU reduction order for `ref_threads` intra-op threads (the
 * reference's torch.get_num_threads()).  f == 1 is the contiguous
 * sum (-v).mean() -- serial, or two passes over ref_threads from 32768 elements on;
 * ref_threads above 1024 is DFQ_ERR_UNSUPPORTED there. */
int dfq_bc_propagate(const float* bias_vec, int64_t numel, float* fake_b, int64_t f,
                     int32_t ref_threads, void* stream);

/* dfq_bc_chain: a whole bias_correction walk's device work in one call -- the
 * ops above, recorded by the host walk in graph order and enqueued back to back
 * on `stream` (bias_correction.py:147-258 issues them one Python call each).
 * COPY ops (the walk's before/after bias snapshots, bias_correction.py:196,255)
 * copy n floats; consecutive ones share a launch.
 * Every op is validated before the first launch; a bad op returns its error code
 * and `*failed_op` = its index, with nothing enqueued. */
enum { DFQ_BC_OP_EXPECT = 0, DFQ_BC_OP_APPLY = 1, DFQ_BC_OP_PROPAGATE = 2, DFQ_BC_OP_COPY = 3 };
/* APPLY flag: out2 (bias_vec) is chain scratch -- only this chain's ops read it,
 * and its contents after the call are unspecified, so the one-launch path may
 * leave it unwritten where every reader recomputes it (the Python walk's vectors). */
enum { DFQ_BC_APPLY_VEC_SCRATCH = 1 };
typedef struct dfq_bc_op {
    int32_t      kind;      /* DFQ_BC_OP_* */
    int32_t      flag;      /* EXPECT: relu | (accumulate << 1); APPLY: DFQ_BC_APPLY_VEC_SCRATCH or 0;
                               PROPAGATE: ref_threads */
    const float* a;         /* EXPECT: fake_w  APPLY: E       PROPAGATE: bias_vec  COPY: src */
    const float* b;         /* EXPECT: fake_b  APPLY: expect */
    float*       out;       /* EXPECT: out     APPLY: bias    PROPAGATE: fake_b    COPY: dst */
    float*       out2;      /* APPLY: bias_vec (may be NULL) */
    int64_t      n;         /* EXPECT: n       APPLY: o       PROPAGATE: numel     COPY: floats */
    int64_t      i2;        /* APPLY: i2 */
    int64_t      f;         /* APPLY: expect numel  PROPAGATE: F */
} dfq_bc_op;
int dfq_bc_chain(const dfq_bc_op* ops, int32_t n_ops, int32_t* failed_op, void* stream);

/* ---- activation ranges from BN statistics (set_quant_minmax,
 *      utils/layer_transform.py:356-618) ---------------------------------------
 * Per channel j, with w = sqrt_w ? sqrt(w[j] + eps) : w[j], b = b[j]:
 *   kind 0: m = b, v = w*w;  1: calculate_mean / calculate_var (ReLU, :396-399);
 *   2: calculate_mean_6 / calculate_var_6 (ReLU6, :400-410);
 *   accumulate ? (mean += m, var += v) : (mean = m, var = v).  mean/var may alias w/b. */
int dfq_act_moments(const float* w, const float* b, int64_t n, int32_t kind, int32_t sqrt_w, float eps,
                    int32_t accumulate, float* mean, float* var, void* stream);
/* out2 = {min(a - nsig*w), max(a + nsig*w)} (get_min_value / get_max_value, :391-392),
 * w := sqrt(w + eps) when w_is_var.  out2: 2 device floats.  NaN propagates as in
 * torch.min / torch.max: one among the a - nsig*w makes out2[0] NaN, one among the
 * a + nsig*w out2[1]. */
int dfq_act_minmax(const float* a, const float* w, int64_t n, int32_t w_is_var, float eps, float nsig,
                   float* out2, void* stream);
/* Case (d.) (:470-481): out[o] = sum_i (sum_k W[o,i,k]) * x[g*i2 + i] (+ bias[o]),
 * W = [o, i2, khw] (khw = 1 for Linear), g = o / (o / groups). */
int dfq_act_affine(const float* x, const float* w, const float* bias, int64_t o, int64_t i2, int64_t khw,
                   int64_t groups, float* out, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* DFQ_HIP_H_ */
