// dfq_int_dwconv2d: the depthwise convolution (groups == C, N = C * mult) of the affine values
// that the activation codes and the weight's integer codes stand for, in one launch on the packed
// 8-bit dot instruction v_dot4c_i32_i8 (include/dfq_hip.h).  A depthwise layer has
// K = KH * KW products per output and one output column per channel: it is bound by bandwidth and
// by the quantizer, not by the matrix instruction, so it does not go through dfq_int_gemm.hip's
// tiles.
//
// A workgroup owns a tile of outputs of one (b, c) plane -- several whole planes where a plane is
// one tile -- for all mult output channels (dfq_int_dwconv_plan.h):
//   1. it reads the tile's input footprint with its halo, four consecutive columns a lane
//      (4-B loads, coalesced along W), quantizes every element ONCE (dfq_int_quant.h: the sweep's
//      screened quotient; the ballot sits in a loop whose trip count is the block's, so every lane
//      reaches it and lanes outside the image or the footprint carry a dummy 0 that is masked
//      afterwards) and writes the code bytes, a word a lane, to LDS -- 0 outside the image;
//   2. per round of mc output channels it writes the planes' weight bytes to LDS as operand
//      words (signed domain, four taps a word);
//   3. a lane takes four consecutive outputs of a row at a time: per word of four taps it
//      gathers the four code bytes of each output from LDS, moves them to the signed domain on
//      the taps inside the image (the tap mask: row bits x column bits) and issues three dot
//      instructions an output -- a' . b', a' . ones, mask . b' -- then folds the offsets back in
//      integers (ig_fold_p / ig_fold_s with T) and runs the contract's fp64 steps in its order;
//      the four results go out as one 16-B store (4-B aligned) where all four exist, else one by
//      one.
// One accumulator per output element, the taps in order, no atomics, no workspace.  All addressing,
// every mask bit and the folds are dfq_int_dwconv_plan.h's.
#include "dfq_common.h"

#include "dfq_int_dwconv_plan.h"
#include "dfq_int_quant.h"

namespace dfq {
namespace {

typedef float dw_v4f_a4 __attribute__((ext_vector_type(4), aligned(4)));

struct DwArgs {
    const float* x;
    const uint8_t* b;
    const float* b_scale;
    const float* b_zero;      // may be null
    const float* bias;        // may be null
    float* out;
    const float* min_dev;
    const float* max_dev;
    double gmin, gmax;
    int x_bits, x_symmetric, x_flags;
    int b_signed, per_row, packed;
    DwcGeom g;
};

__global__ __launch_bounds__(kThreads) void int_dwconv_kernel(const DwArgs a) {
    __shared__ uint32_t codes[kDwCodeBytes / 4];
    __shared__ uint32_t wts[kDwWeightWords];
    const DwcGeom& g = a.g;
    const int tid = threadIdx.x;
    const DwcBlock blk = dwc_block(g, blockIdx.x);
    const IgAParams pa = ig_quant_params(a.min_dev, a.max_dev, a.gmin, a.gmax, a.x_bits, a.x_symmetric, a.x_flags);

    // 1. the footprint's codes.  The trip count is the block's: no lane leaves before the ballot.
    const DFQ_GLOBAL float* x = (const DFQ_GLOBAL float*)a.x;
    const int32_t cells = dwc_cells(g);
    for (int32_t base = 0; base < cells; base += kThreads) {
        const int32_t wq = base + tid;
        const bool active = wq < cells;
        const DwcCell c = dwc_cell(g, active ? wq : 0);
        const int64_t p = blk.p0 + c.pl;
        float v[4];
        uint32_t keep = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const bool on = active && dwc_x_reads(g, blk, p, c.r, c.col + t);
            v[t] = on ? x[dwc_x_offset(g, blk, p, c.r, c.col + t)] : 0.f;
            keep |= on ? 0xFFu << (8 * t) : 0u;
        }
        const uint32_t w = ig_codes4(v, pa) & keep;
        if (active) codes[dwc_lds_byte(g, c.pl, c.r, c.col) >> 2] = w;
    }

    const uint8_t* lds_bytes = reinterpret_cast<const uint8_t*>(codes);
    const DFQ_GLOBAL float* bias = (const DFQ_GLOBAL float*)a.bias;
    const DFQ_GLOBAL float* b_scale = (const DFQ_GLOBAL float*)a.b_scale;
    const DFQ_GLOBAL float* b_zero = (const DFQ_GLOBAL float*)a.b_zero;
    DFQ_GLOBAL float* out = (DFQ_GLOBAL float*)a.out;
    const uint32_t xb = ig_xor_mask(a.b_signed != 0);
    const int ob = ig_offset(a.b_signed != 0);
    const bool has_zb = b_zero != nullptr;
    const double sa = (double)pa.s, za = (double)pa.z;
    const uint64_t full = dwc_full_mask(g.K);
    const int32_t quads = dwc_quads(g);

    for (int32_t m0 = 0; m0 < g.mult; m0 += g.mc) {
        const int32_t mcn = g.mult - m0 < g.mc ? g.mult - m0 : g.mc;
        __syncthreads();   // the codes are written (first round); the last round's weights are read
        // 2. the round's weights as operand words
        for (int32_t t = tid; t < g.pp * mcn * g.words; t += kThreads) {
            const int32_t w = t % g.words, pm = t / g.words, m = pm % mcn, pl = pm / mcn;
            const int64_t p = blk.p0 + pl;
            uint32_t raw = 0;
            if (p < g.planes) {
                const int64_t n = (p % g.C) * g.mult + m0 + m;
                for (int e = 0; e < 4; ++e)
                    if (4 * w + e < g.K) raw |= dwc_b_code(a.b, n, 4 * w + e, g.K, a.packed != 0, a.b_signed != 0) << (8 * e);
            }
            wts[dwc_w_index(g, pl, m, w)] = dwc_operand_word(raw, xb, full, w);
        }
        __syncthreads();
        // 3. the outputs
        for (int32_t q = tid; q < quads; q += kThreads) {
            const DwcQuad d = dwc_quad(g, q);
            const int64_t p = blk.p0 + d.pl;
            const int32_t oh = blk.oh0 + d.r;
            if (p >= g.planes || oh >= g.OH || !dwc_out_on(g, blk, d, 0)) continue;   // no barrier below in this round
            const uint64_t row_bits = g.masked ? dwc_axis_bits(oh * g.sh - g.ph, g.H, g.KH, g.dh) : 0;
            bool on[kDwQuad];
            uint64_t vm[kDwQuad];
            int32_t T[kDwQuad], at[kDwQuad];
#pragma unroll
            for (int e = 0; e < kDwQuad; ++e) {
                on[e] = dwc_out_on(g, blk, d, e);
                const int32_t ow = blk.ow0 + d.c0 + e;
                vm[e] = !on[e] ? 0 : !g.masked ? full : dwc_tap_mask(g, row_bits, dwc_axis_bits(ow * g.sw - g.pw, g.W, g.KW, g.dw));
                T[e] = !on[e] ? 0 : g.masked ? dwc_taps(g, oh, ow) : g.K;
                at[e] = dwc_tap_byte(g, d.pl, d.r, on[e] ? d.c0 + e : d.c0, dwc_tap0());   // an absent output reads the quad's first
            }
            for (int32_t m = 0; m < mcn; ++m) {
                int32_t acc[kDwQuad] = {0, 0, 0, 0}, ra[kDwQuad] = {0, 0, 0, 0}, rb[kDwQuad] = {0, 0, 0, 0};
                DwcTap tap = dwc_tap0();
                for (int32_t w = 0; w < g.words; ++w) {
                    uint32_t raw[kDwQuad] = {0, 0, 0, 0};
                    for (int t = 0; t < 4; ++t) {
                        if (4 * w + t < g.K) {
#pragma unroll
                            for (int e = 0; e < kDwQuad; ++e) raw[e] |= (uint32_t)lds_bytes[at[e] + tap.off] << (8 * t);
                        }
                        dwc_tap_next(g, tap);
                    }
                    const uint32_t bw = wts[dwc_w_index(g, d.pl, m, w)];
#pragma unroll
                    for (int e = 0; e < kDwQuad; ++e) {
                        const uint32_t aw = dwc_operand_word(raw[e], pa.xm, vm[e], w), ones = dwc_ones_word(vm[e], w);
                        acc[e] = dwc_dot4(aw, bw, acc[e]);
                        ra[e] = dwc_dot4(aw, 0x01010101u, ra[e]);
                        rb[e] = dwc_dot4(ones, bw, rb[e]);
                    }
                }
                // the contract's integers, then its fp64 steps in its order
                const int64_t n = (p % g.C) * g.mult + m0 + m;
                const int64_t pc = a.per_row ? n : 0;
                const double sb = (double)b_scale[pc], zb = has_zb ? (double)b_zero[pc] : 0.0;
                const double ss = sa * sb, sz = sa * zb, zs = za * sb, zz = za * zb;
                const double bv = bias != nullptr ? (double)bias[n] : 0.0;
                float v[kDwQuad];
#pragma unroll
                for (int e = 0; e < kDwQuad; ++e) {
                    const int64_t P = ig_fold_p(acc[e], ra[e], rb[e], pa.off, ob, T[e]);
                    double t = ss * (double)P;
                    if (has_zb) t += sz * (double)ig_fold_s(ra[e], pa.off, T[e]);
                    t += zs * (double)ig_fold_s(rb[e], ob, T[e]);
                    if (has_zb) t += zz * (double)T[e];
                    if (bias != nullptr) t += bv;
                    v[e] = (float)t;
                }
                const int64_t o = dwc_out_offset(g, p, m0 + m, oh, blk.ow0 + d.c0);
                if (on[0] && on[1] && on[2] && on[3]) {
                    const dw_v4f_a4 quad = {v[0], v[1], v[2], v[3]};
                    *(DFQ_GLOBAL dw_v4f_a4*)(out + o) = quad;
                } else {
#pragma unroll
                    for (int e = 0; e < kDwQuad; ++e)
                        if (on[e]) out[o + e] = v[e];
                }
            }
        }
    }
}

}  // namespace
}  // namespace dfq

using namespace dfq;

extern "C" int dfq_int_dwconv2d(const dfq_int_dwconv2d_desc* d, void* stream) {
    static_assert(kThreads == 256, "dfq_int_dwconv_plan.h sizes a workgroup's quads for 256 lanes");
    DwArgs a{};
    int64_t grid = 0;
    const int rc = dwc_check(d, a.g, grid);
    if (rc != DFQ_OK) return rc;
    a.x = d->x;
    a.b = static_cast<const uint8_t*>(d->b_codes);
    a.b_scale = d->b_scale;
    a.b_zero = d->b_zero;
    a.bias = d->bias;
    a.out = d->out;
    a.min_dev = d->min_dev;
    a.max_dev = d->max_dev;
    a.gmin = d->given_min;
    a.gmax = d->given_max;
    a.x_bits = d->x_bits;
    a.x_symmetric = d->x_symmetric;
    a.x_flags = d->flags & DFQ_SCALE_F32;
    a.b_signed = d->b_signed;
    a.per_row = (d->flags & DFQ_INT_B_PER_ROW) != 0;
    a.packed = (d->flags & DFQ_INT_B_PACK4) != 0;
    hipLaunchKernelGGL(int_dwconv_kernel, dim3((unsigned)grid), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
    DFQ_LAUNCH_CHECK();
    return DFQ_OK;
}
