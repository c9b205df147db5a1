// dfq_int_mbconv_q: the integer inverted-residual block -- expand 1x1 -> depthwise 3x3 -> project
// 1x1 on stored activation codes -- in one launch, the two hidden tensors in LDS as code bytes
// (include/dfq_hip.h).  Bit for bit dfq_int_conv2d_q -> dfq_int_dwconv2d_q ->
// dfq_int_conv2d_q: the same signed-domain operands and folds (ig_fold_p / ig_fold_s), the same
// five fp64 steps per layer (mb_value, one body for the three), the same quantizer (ig_quant_params
// + ig_codes4) between them.
//
// A workgroup of four waves owns one image, one spatial output tile and all Cout channels
// (dfq_int_mbconv_plan.h has the tile, the LDS map and every address):
//   1. stage   the footprint's code bytes, NCHW -> xs [footprint row][k], signed domain; a lane
//              takes four k of one pixel (four loads, each coalesced along W across lanes; one LDS
//              word).  Then the rows' sums (xs x all-ones on the matrix instruction) -> xsum.
//   2. per chunk of 64 hidden channels, in block-uniform control flow (ig_codes4 holds a ballot):
//      a. expand   wave w: columns 16 w .. 16 w + 15 of the chunk.  Its B fragments (global, all K
//                  steps) stay in registers; per row tile the A fragments are 16-B LDS reads; one
//                  accumulator tile is live.  Epilogue -> hidden1's code, 0 outside the image, a
//                  lane's four rows as one word of the channel's LDS plane.
//      b. depthwise  a lane takes one tile pixel and four channels: nine taps per channel from the
//                  planes, three dots per word as int_dwconv_kernel's phase 3 (tap mask, T, ones
//                  and mask words), epilogue -> hidden2's code in the signed domain, one word of
//                  the project's A tile.
//      c. project  wave w: column tiles w, w + 4, ... of Cout x every row tile of the pixels; the
//                  int32 accumulators stay in registers over all chunks, with sum qa' (A x ones)
//                  and sum qb' (ones x B) beside them.
//   3. epilogue   fold with K = Ch, the fp64 steps, fp32 NCHW or out_quant's bytes: a lane's four
//                 rows are four consecutive ow -- one 16-B / 4-B store where all exist (and the
//                 byte address allows), else element by element.
// CT: column tiles of a wave in the project (Cout <= 64 CT).  OC: the output is code bytes.
// RES (dfq_int_mbconv_res_q; stride 1, pad 1, Cin == Cout): between the epilogue's value and its
// store, the value becomes dq_P(its code on proj_quant) + dq_X(x's code at the pixel) -- the
// shortcut's byte is the one step 1 staged in xs (mb_res_fr), which no chunk overwrites.
// Two barriers a chunk: hid and wts are written in (a) and read in (b); pa is written in (b) and
// read in (c); the next chunk's (a) touches neither pa nor xs.  No scratch, no atomics, no workspace.
#include "dfq_int_mm_sources.h"

#include "dfq_int_mbconv_plan.h"

namespace dfq {
namespace {

struct MbLayer {
    const uint8_t* b;
    const float* b_scale;
    const float* b_zero;      // may be null
    const float* bias;        // may be null
    int b_signed, per_row;
};
struct MbArgs {
    const uint8_t* x;
    void* out;
    MbLayer e, d, p;
    IgOutQ qx, q1, q2, qo;    // the grids of x, hidden1, hidden2 and the output
    IgOutQ qp;                // RES: the grid of the project's output, the add's first operand
    MbGeom g;
};

// A layer's fp64 factors for output channel n, and the contract's steps in their order.
struct MbAffine {
    double ss, sz, zs, zz, bv;
    bool has_zb, has_bias;
};
__device__ __forceinline__ MbAffine mb_affine(const MbLayer& l, const IgAParams& pa, int64_t n) {
    const DFQ_GLOBAL float* b_scale = (const DFQ_GLOBAL float*)l.b_scale;
    const DFQ_GLOBAL float* b_zero = (const DFQ_GLOBAL float*)l.b_zero;
    const DFQ_GLOBAL float* bias = (const DFQ_GLOBAL float*)l.bias;
    MbAffine f;
    f.has_zb = b_zero != nullptr;
    f.has_bias = bias != nullptr;
    const int64_t pc = l.per_row ? n : 0;
    const double sa = (double)pa.s, za = (double)pa.z;
    const double sb = (double)b_scale[pc], zb = f.has_zb ? (double)b_zero[pc] : 0.0;
    f.ss = sa * sb; f.sz = sa * zb; f.zs = za * sb; f.zz = za * zb;
    f.bv = f.has_bias ? (double)bias[n] : 0.0;
    return f;
}
__device__ __forceinline__ float mb_value(const MbAffine& f, int32_t acc, int32_t ra, int32_t rb, int oa, int ob, int32_t T) {
    const int64_t P = ig_fold_p(acc, ra, rb, oa, ob, T);
    double t = f.ss * (double)P;
    if (f.has_zb) t += f.sz * (double)ig_fold_s(ra, oa, T);
    t += f.zs * (double)ig_fold_s(rb, ob, T);
    if (f.has_zb) t += f.zz * (double)T;
    if (f.has_bias) t += f.bv;
    return (float)t;
}

// A lane's B fragment of K step `step`: 16 bytes of weight row `row` from global memory, in the
// signed domain, 0 where row >= rows or k >= K.
__device__ __forceinline__ ig_v4i mb_b_frag(const uint8_t* b, int64_t row, int64_t rows, int64_t K, int64_t step, int lane, bool wide, uint32_t xm) {
    const ig_v4i f = wide ? ig_load_bytes<true>(b, row, rows, K, step, lane) : ig_load_bytes<false>(b, row, rows, K, step, lane);
    return IgBytesB<false>::operand(f, xm, ig_lane_valid(row, rows, ig_lane_k0(step, lane), K));
}

template <int CT, bool OC, bool RES>
__global__ __launch_bounds__(kThreads) void int_mbconv_kernel(const MbArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t mb_lds[];
    uint8_t* lds = mb_lds;
    const MbGeom& g = a.g;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    const int lrow = lane & 15;
    const MbBlock blk = mb_block(g, blockIdx.x);
    const IgAParams px = ig_out_params(a.qx), p1 = ig_out_params(a.q1), p2 = ig_out_params(a.q2);
    const ig_v4i zero4 = {0, 0, 0, 0}, ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101};

    // 1. the footprint's codes, signed domain
    const DFQ_GLOBAL uint8_t* x = (const DFQ_GLOBAL uint8_t*)a.x;
    for (int32_t cell = tid; cell < mb_cells(g); cell += kThreads) {
        const int32_t k0 = mb_cell_k(g, cell), fr = mb_cell_fr(g, cell);
        const MbPixel q = mb_pixel(g, blk, fr);
        uint32_t w = 0, keep = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (q.inside && k0 + t < g.Cin) {
                w |= (uint32_t)x[mb_x_offset(g, blk.b, k0 + t, q.ih, q.iw)] << (8 * t);
                keep |= 0xFFu << (8 * t);
            }
        }
        *reinterpret_cast<uint32_t*>(lds + mb_xs_byte(g, fr, k0)) = (w ^ px.xm) & keep;
    }
    __syncthreads();
    // the rows' sums of a'
    for (int32_t i = wave; i < g.frt; i += kMbWaves) {
        ig_v4i ra = zero4;
        for (int32_t s = 0; s < g.ksteps; ++s)
            ra = __builtin_amdgcn_mfma_i32_16x16x64_i8(*reinterpret_cast<const ig_v4i*>(lds + mb_xs_frag(g, i, s, lane)), ones, ra, 0, 0, 0);
        if (lrow == 0) *reinterpret_cast<ig_v4i*>(lds + mb_xsum_byte(g, mb_acc_row(i, lane))) = ra;
    }
    // bit 4 i + r: the lane's accumulator row r of row tile i is a pixel of the image
    uint64_t inside = 0;
    for (int32_t i = 0; i < g.frt; ++i)
        for (int r = 0; r < 4; ++r)
            if (mb_pixel(g, blk, mb_acc_row(i, lane) + r).inside) inside |= uint64_t(1) << (4 * i + r);

    const uint32_t xb_e = ig_xor_mask(a.e.b_signed != 0), xb_d = ig_xor_mask(a.d.b_signed != 0), xb_p = ig_xor_mask(a.p.b_signed != 0);
    const int ob_e = ig_offset(a.e.b_signed != 0), ob_d = ig_offset(a.d.b_signed != 0), ob_p = ig_offset(a.p.b_signed != 0);
    const uint64_t full = dwc_full_mask(9);
    ig_v4i acc[4][CT], pra[4], prb[CT];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        pra[i] = zero4;
#pragma unroll
        for (int j = 0; j < CT; ++j) acc[i][j] = zero4;
    }
#pragma unroll
    for (int j = 0; j < CT; ++j) prb[j] = zero4;

    __syncthreads();   // xsum is written
    for (int32_t c = 0; c < g.chunks; ++c) {
        const int32_t ch0 = c * kMbChunk;
        // the chunk's depthwise weights as operand words
        if (tid < kMbChunk * 3) {
            const int32_t nl = tid / 3, w = tid % 3;
            uint32_t raw = 0;
            if (ch0 + nl < g.Ch) {
                const DFQ_GLOBAL uint8_t* row = (const DFQ_GLOBAL uint8_t*)a.d.b + ig_byte_offset(ch0 + nl, 0, 9);
                for (int e = 0; e < 4; ++e)
                    if (4 * w + e < 9) raw |= (uint32_t)row[4 * w + e] << (8 * e);
            }
            *reinterpret_cast<uint32_t*>(lds + mb_wts_byte(g, nl, w)) = dwc_operand_word(raw, xb_d, full, w);
        }
        // a. expand: this wave's 16 columns of the chunk, every row tile
        {
            const int32_t nl = wave * 16 + lrow;
            const int64_t n = ch0 + nl;
            ig_v4i b[kMbMaxKSteps], rb = zero4;
#pragma unroll
            for (int s = 0; s < kMbMaxKSteps; ++s) {
                if (s < g.ksteps) {
                    b[s] = mb_b_frag(a.e.b, n, g.Ch, g.Cin, s, lane, g.e_wide != 0, xb_e);
                    rb = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, b[s], rb, 0, 0, 0);   // sum_k b' of the lane's column
                } else {
                    b[s] = zero4;
                }
            }
            const MbAffine f = mb_affine(a.e, px, n < g.Ch ? n : ch0);   // a column >= Ch computes column ch0's and is never read
            for (int32_t i = 0; i < g.frt; ++i) {
                ig_v4i t = zero4;
#pragma unroll
                for (int s = 0; s < kMbMaxKSteps; ++s)
                    if (s < g.ksteps)
                        t = __builtin_amdgcn_mfma_i32_16x16x64_i8(*reinterpret_cast<const ig_v4i*>(lds + mb_xs_frag(g, i, s, lane)), b[s], t, 0, 0, 0);
                const int32_t fr0 = mb_acc_row(i, lane);
                const ig_v4i ra = *reinterpret_cast<const ig_v4i*>(lds + mb_xsum_byte(g, fr0));
                float v[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = mb_value(f, t[r], ra[r], rb[r], px.off, ob_e, g.Cin);
                const uint32_t keep = igc_ones_word((uint32_t)(inside >> (4 * i)) & 0xFu, 0) * 0xFFu;
                *reinterpret_cast<uint32_t*>(lds + mb_hid_byte(g, nl, fr0)) = ig_codes4(v, p1) & keep;   // every lane of the block
            }
        }
        __syncthreads();
        // b. depthwise: one pixel, four channels a lane.  The trip count is the block's.
        for (int32_t u = tid; u < mb_units(g); u += kThreads) {
            const MbUnit q = mb_unit(g, blk, u);
            const uint64_t vm = !q.on ? 0 : !g.dw.masked ? full
                : dwc_tap_mask(g.dw, dwc_axis_bits(q.oh * g.s - g.p, g.H, 3, 1), dwc_axis_bits(q.ow * g.s - g.p, g.W, 3, 1));
            const int32_t T = !q.on ? 0 : g.dw.masked ? dwc_taps(g.dw, q.oh, q.ow) : 9;
            float v[4];
            uint32_t keep = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int32_t nl = q.cq * 4 + e;
                const bool real = ch0 + nl < g.Ch;
                const uint8_t* plane = lds + mb_hid_byte(g, nl, q.at);
                uint32_t raw[3] = {0, 0, 0};
#pragma unroll
                for (int k = 0; k < 9; ++k) raw[k >> 2] |= (uint32_t)plane[mb_tap(g, k)] << (8 * (k & 3));
                int32_t s = 0, ra = 0, rb = 0;
#pragma unroll
                for (int w = 0; w < 3; ++w) {
                    const uint32_t bw = *reinterpret_cast<const uint32_t*>(lds + mb_wts_byte(g, nl, w));
                    const uint32_t aw = dwc_operand_word(raw[w], p1.xm, vm, w), on = dwc_ones_word(vm, w);
                    s = dwc_dot4(aw, bw, s);
                    ra = dwc_dot4(aw, 0x01010101u, ra);
                    rb = dwc_dot4(on, bw, rb);
                }
                const MbAffine f = mb_affine(a.d, p1, real ? ch0 + nl : ch0);
                v[e] = mb_value(f, s, ra, rb, p1.off, ob_d, T);
                keep |= real ? 0xFFu << (8 * e) : 0u;
            }
            *reinterpret_cast<uint32_t*>(lds + mb_pa_byte(g, q.tp, q.cq * 4)) = (ig_codes4(v, p2) ^ p2.xm) & keep;   // every lane of the block
        }
        __syncthreads();
        // c. project: this chunk's 64 k into the accumulators
        ig_v4i fa[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            fa[i] = zero4;
            if (i < g.rt) {
                fa[i] = *reinterpret_cast<const ig_v4i*>(lds + mb_pa_frag(g, i, lane));
                pra[i] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[i], ones, pra[i], 0, 0, 0);   // sum_k a' of the pixels
            }
        }
#pragma unroll
        for (int j = 0; j < CT; ++j) {
            const int32_t tile = j * kMbWaves + wave;
            if (tile < g.nt) {   // wave-uniform
                const ig_v4i fb = mb_b_frag(a.p.b, tile * 16 + lrow, g.Cout, g.Ch, c, lane, g.p_wide != 0, xb_p);
                prb[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, fb, prb[j], 0, 0, 0);   // sum_k b' of the columns
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (i < g.rt) acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[i], fb, acc[i][j], 0, 0, 0);
            }
        }
    }

    // 3. the project's epilogue
    IgAParams po, pp;
    if constexpr (OC) po = ig_out_params(a.qo);
    if constexpr (RES) pp = ig_out_params(a.qp);
#pragma unroll
    for (int j = 0; j < CT; ++j) {
        const int32_t tile = j * kMbWaves + wave;
        if (tile >= g.nt) continue;   // wave-uniform
        const int64_t n = tile * 16 + lrow;
        const bool col_on = n < g.Cout;
        const MbAffine f = mb_affine(a.p, p2, col_on ? n : tile * 16);   // a column >= Cout computes the tile's first and stores nothing
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i >= g.rt) continue;   // block-uniform
            const int32_t tp0 = mb_acc_row(i, lane);
            float v[4];
            bool on[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                v[r] = mb_value(f, acc[i][j][r], pra[i][r], prb[j][r], p2.off, ob_p, g.Ch);
                on[r] = col_on && mb_tp_on(g, blk, tp0 + r);
            }
            if constexpr (RES) {   // v := dq_P(the project's code) + dq_X(x's code at the pixel, from xs)
                const uint32_t pc = ig_codes4(v, pp);   // every lane of the wave
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int8_t xc = (int8_t)lds[mb_xs_byte(g, mb_res_fr(g, tp0 + r, on[r]), (int32_t)n)];
                    v[r] = ig_code_value((int8_t)((pc >> (8 * r)) ^ pp.xm), pp) + ig_code_value(xc, px);
                }
            }
            const int64_t o = mb_out_offset(g, blk.b, n, blk.oh0 + (tp0 >> 3), blk.ow0 + (tp0 & 7));
            const bool all_on = on[0] && on[1] && on[2] && on[3];
            if constexpr (OC) {
                DFQ_GLOBAL uint8_t* out = (DFQ_GLOBAL uint8_t*)a.out;
                const uint32_t w = ig_codes4(v, po);   // every lane of the wave
                if (dwio_out_word(all_on, reinterpret_cast<uintptr_t>(a.out), o)) {
                    *(DFQ_GLOBAL uint32_t*)(out + o) = w;
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (on[r]) out[o + r] = (uint8_t)(w >> (8 * r));
                }
            } else {
                DFQ_GLOBAL float* out = (DFQ_GLOBAL float*)a.out;
                if (all_on) {
                    const ig_v4f_a4 quad = {v[0], v[1], v[2], v[3]};
                    *(DFQ_GLOBAL ig_v4f_a4*)(out + o) = quad;
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (on[r]) out[o + r] = v[r];
                }
            }
        }
    }
}

MbLayer mb_layer(const dfq_int_mbconv_layer& l) {
    return MbLayer{static_cast<const uint8_t*>(l.b_codes), l.b_scale, l.b_zero, l.bias, l.b_signed, (l.flags & DFQ_INT_B_PER_ROW) != 0};
}
IgOutQ mb_quant(const dfq_int_mbconv_quant& q) {
    return IgOutQ{q.min_dev, q.max_dev, q.given_min, q.given_max, q.bits, q.symmetric, q.flags};
}

template <int CT, bool RES>
void mb_launch(const MbArgs& a, bool codes, int64_t grid, hipStream_t s) {
    const dim3 blocks((unsigned)grid), threads(kThreads);
    if (codes) hipLaunchKernelGGL((int_mbconv_kernel<CT, true, RES>), blocks, threads, (size_t)a.g.lds_bytes, s, a);
    else hipLaunchKernelGGL((int_mbconv_kernel<CT, false, RES>), blocks, threads, (size_t)a.g.lds_bytes, s, a);
}

// Both entries: r is null for dfq_int_mbconv_q.
int mb_run(const dfq_int_mbconv_desc* d, const dfq_int_mbconv_res* r, bool res, void* stream) {
    MbArgs a{};
    int64_t grid = 0;
    const int rc = res ? mb_res_check(d, r, a.g, grid) : mb_check(d, a.g, grid);
    if (rc != DFQ_OK) return rc;
    a.x = static_cast<const uint8_t*>(d->x);
    a.out = d->out;
    a.e = mb_layer(d->expand);
    a.d = mb_layer(d->depthwise);
    a.p = mb_layer(d->project);
    a.qx = mb_quant(d->x_quant);
    a.q1 = mb_quant(d->hidden1);
    a.q2 = mb_quant(d->hidden2);
    a.qo = mb_quant(d->out_quant);
    if (res) a.qp = mb_quant(r->proj_quant);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool codes = d->out_quant.bits > 0, wide = a.g.nt > 2 * kMbWaves;
    if (res && wide) mb_launch<5, true>(a, codes, grid, s);
    else if (res) mb_launch<2, true>(a, codes, grid, s);
    else if (wide) mb_launch<5, false>(a, codes, grid, s);
    else mb_launch<2, false>(a, codes, grid, s);
    DFQ_LAUNCH_CHECK();
    return DFQ_OK;
}

}  // namespace
}  // namespace dfq

using namespace dfq;

static_assert(DFQ_INT_MB_MAX_COUT <= 5 * kMbWaves * 16, "the widest project fits five column tiles a wave");

extern "C" int dfq_int_mbconv_q(const dfq_int_mbconv_desc* d, void* stream) { return mb_run(d, nullptr, false, stream); }

extern "C" int dfq_int_mbconv_res_q(const dfq_int_mbconv_desc* d, const dfq_int_mbconv_res* r, void* stream) {
    return mb_run(d, r, true, stream);
}
