// Pooling on stored activation codes (include/dfq_hip.h): the two nodes of the
// zoo's classifiers that are not products, each in one launch on the bytes themselves.
//
// dfq_int_mean_q -- the global average pool.  The sum of a row's codes is an integer, so the work
// is split freely and the result is the statement's bits whatever the split:
//   S = sum q;   m = (double(s) * double(S)) / double(P) + double(z);   y = float(m)
//   1. a workgroup zeroes one int32 a row of its span in LDS;
//   2. a lane takes 16-B chunks counted from the span's first 16-B boundary -- one 16-B load, or
//      predicated bytes at the two ends of x -- and sums them with the packed 8-bit dot
//      instruction against a word of ones, in the signed domain, the bytes outside the piece
//      masked out of the word.  SMALL: every piece of the chunk (the bytes of one row) is one LDS
//      integer add into its row.  Large planes: one int32 a lane over the row's chunks, a wave
//      reduction, then one LDS add a wave;
//   3. after the barrier a lane takes four rows: the fp64 epilogue of each, then four floats, or
//      one ig_codes4 word.  ig_codes4 holds a wave ballot: the loop's trip count is the block's
//      and a lane with no row runs the body with its rows absent.
// dfq_int_maxpool2d_q -- the maximum of codes on one grid is the maximum of the bytes:
//   1. the footprint of the tile (dfq_int_dwconv2d's tiles, several planes a workgroup where a
//      plane is one tile) goes to LDS as words, each code in the order domain (pool_order_mask),
//      a word load where the cell's four columns are read and the address allows;
//   2. a lane produces four consecutive ow of one output row from plain bytes: per window row
//      whose bit is set, the maximum along KW under the column bits, then the maximum of those
//      along KH.  A tap outside the image is a clear bit and is not compared; the start value 0 is
//      the order domain's least element and the host's pad <= K / 2 puts a real tap in every
//      window;
//   3. the four codes go out as they are, or (OC) through ig_code_value and ig_codes4 onto
//      out_quant -- one word where the address allows.  OC: the quad loop's trip count is the
//      block's, for the ballot.
// Every address and predicate comes from dfq_int_pool_plan.h.  No scratch, no atomics on global
// memory, no workspace.
#include "dfq_int_mm_sources.h"

#include "dfq_int_pool_plan.h"

namespace dfq {
namespace {

typedef uint32_t pool_v4u __attribute__((ext_vector_type(4)));

struct MeanArgs {
    const uint8_t* x;
    void* out;
    IgOutQ qx, qo;
    MeanGeom g;
};

// The chunk's 16 bytes as four words; a byte that is not read is 0.
__device__ __forceinline__ void mean_load(const uint8_t* x, const MeanGeom& g, const MeanBlock& b, int32_t e0, uint32_t (&w)[4]) {
    const DFQ_GLOBAL uint8_t* p = (const DFQ_GLOBAL uint8_t*)x + b.b0;
    if (mean_chunk_vector(g, b, e0)) {
        const pool_v4u v = *(const DFQ_GLOBAL pool_v4u*)(p + e0);
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] = v[i];
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] = 0;
#pragma unroll
        for (int i = 0; i < kMeanChunk; ++i)
            if (mean_byte_on(b, e0, i)) w[i >> 2] |= (uint32_t)p[e0 + i] << (8 * (i & 3));
    }
}
// The dot products of bytes [lo, hi) of the chunk against ones, in the signed domain.
__device__ __forceinline__ int32_t mean_piece_dots(const uint32_t (&w)[4], uint32_t xm, int32_t lo, int32_t hi) {
    int32_t s = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) s = dwc_dot4(mean_piece_word(w[j], xm, lo, hi, j), 0x01010101u, s);
    return s;
}

template <bool SMALL, bool OC>
__global__ __launch_bounds__(kThreads) void int_mean_kernel(const MeanArgs a) {
    __shared__ int32_t sums[kMeanMaxRows];
    const MeanGeom& g = a.g;
    const int tid = threadIdx.x;
    const MeanBlock b = mean_block(g, blockIdx.x);
    const IgAParams px = ig_out_params(a.qx);
    IgAParams po;
    if constexpr (OC) po = ig_out_params(a.qo);

    for (int32_t r = tid; r < b.nr; r += kThreads) sums[r] = 0;
    __syncthreads();
    if constexpr (SMALL) {
        for (int32_t c = tid; c < b.chunks; c += kThreads) {
            const int32_t e0 = mean_chunk_e0(b, c), hi = mean_chunk_hi(b, e0);
            uint32_t w[4];
            mean_load(a.x, g, b, e0, w);
            for (int32_t lo = mean_chunk_lo(e0); lo < hi;) {
                const MeanPiece pc = mean_piece(g, e0, lo, hi);
                atomicAdd(&sums[pc.row], mean_piece_dots(w, px.xm, lo, pc.hi));
                lo = pc.hi;
            }
        }
    } else {
        int32_t s = 0;
        for (int32_t c = tid; c < b.chunks; c += kThreads) {
            const int32_t e0 = mean_chunk_e0(b, c);
            uint32_t w[4];
            mean_load(a.x, g, b, e0, w);
            s += mean_piece_dots(w, px.xm, mean_chunk_lo(e0), mean_chunk_hi(b, e0));
        }
#pragma unroll
        for (int off = kWave / 2; off >= 1; off >>= 1) s += __shfl_xor(s, off, kWave);
        if ((tid & (kWave - 1)) == 0) atomicAdd(&sums[0], s);
    }
    __syncthreads();

    // the epilogue: the trip count is the block's (OC: every lane reaches the ballot)
    const double sd = (double)px.s, zd = (double)px.z, pd = (double)g.P;
    const int32_t quads = mean_quads(b);
    for (int32_t t0 = 0; t0 < quads; t0 += kThreads) {
        const int32_t t = t0 + tid;
        float y[kMeanQuad];
#pragma unroll
        for (int e = 0; e < kMeanQuad; ++e) {
            const bool on = t < quads && mean_row_on(b, t, e);
            const int32_t S = mean_row_sum(g, on ? sums[t * kMeanQuad + e] : 0, px.off);
            const double m = (sd * (double)S) / pd + zd;
            y[e] = on ? (float)m : 0.f;
        }
        const int64_t r = b.r0 + (int64_t)t * kMeanQuad;
        if constexpr (OC) {
            DFQ_GLOBAL uint8_t* out = (DFQ_GLOBAL uint8_t*)a.out;
            const uint32_t w = ig_codes4(y, po);   // every lane of the block
            if (t < quads && mean_out_word(b, t, reinterpret_cast<uintptr_t>(a.out))) {
                *(DFQ_GLOBAL uint32_t*)(out + r) = w;
            } else if (t < quads) {
#pragma unroll
                for (int e = 0; e < kMeanQuad; ++e)
                    if (mean_row_on(b, t, e)) out[r + e] = (uint8_t)(w >> (8 * e));
            }
        } else {
            DFQ_GLOBAL float* out = (DFQ_GLOBAL float*)a.out;
            if (t < quads && mean_row_on(b, t, kMeanQuad - 1)) {
                const ig_v4f_a4 quad = {y[0], y[1], y[2], y[3]};
                *(DFQ_GLOBAL ig_v4f_a4*)(out + r) = quad;
            } else if (t < quads) {
#pragma unroll
                for (int e = 0; e < kMeanQuad; ++e)
                    if (mean_row_on(b, t, e)) out[r + e] = y[e];
            }
        }
    }
}

struct MaxArgs {
    const uint8_t* x;
    uint8_t* out;
    IgOutQ qx, qo;
    DwcGeom g;
};

template <bool OC>
__global__ __launch_bounds__(kThreads) void int_maxpool_kernel(const MaxArgs a) {
    __shared__ uint32_t codes[kDwCodeBytes / 4];
    const DwcGeom& g = a.g;
    const int tid = threadIdx.x;
    const DwcBlock blk = dwc_block(g, blockIdx.x);
    const uint32_t om = pool_order_mask(a.qx.symmetric != 0);

    // 1. the footprint's codes in the order domain; 0 where nothing is read
    const DFQ_GLOBAL uint8_t* x = (const DFQ_GLOBAL uint8_t*)a.x;
    const int32_t cells = dwc_cells(g);
    for (int32_t wq = tid; wq < cells; wq += kThreads) {
        const DwcCell c = dwc_cell(g, wq);
        const int64_t p = blk.p0 + c.pl;
        uint32_t w = 0;
        if (dwio_x_word(g, blk, p, c.r, c.col, reinterpret_cast<uintptr_t>(a.x))) {
            w = *(const DFQ_GLOBAL uint32_t*)(x + dwc_x_offset(g, blk, p, c.r, c.col)) ^ om;
        } else {
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (dwc_x_reads(g, blk, p, c.r, c.col + t)) w |= ((uint32_t)x[dwc_x_offset(g, blk, p, c.r, c.col + t)] ^ (om & 0xFFu)) << (8 * t);
        }
        codes[dwc_lds_byte(g, c.pl, c.r, c.col) >> 2] = w;
    }
    __syncthreads();

    const uint8_t* lds_bytes = reinterpret_cast<const uint8_t*>(codes);
    IgAParams px, po;
    if constexpr (OC) {
        px = ig_out_params(a.qx);
        po = ig_out_params(a.qo);
    }
    const uint64_t all_rows = dwc_full_mask(g.KH), all_cols = dwc_full_mask(g.KW);
    // 2. the outputs.  The trip count is the block's (OC: every lane reaches the ballot).
    const int32_t quads = dwc_quads(g);
    for (int32_t q0 = 0; q0 < quads; q0 += kThreads) {
        const int32_t q = q0 + tid;
        const DwcQuad d = dwc_quad(g, q < quads ? q : 0);
        const int64_t p = blk.p0 + d.pl;
        const int32_t oh = blk.oh0 + d.r;
        const bool live = q < quads && p < g.planes && oh < g.OH && dwc_out_on(g, blk, d, 0);
        if (!OC && !live) continue;   // no barrier and no ballot below
        const uint64_t row_bits = !live ? 0 : g.masked ? dwc_axis_bits(oh * g.sh - g.ph, g.H, g.KH, 1) : all_rows;
        bool on[kDwQuad];
        uint64_t cb[kDwQuad];
        int32_t at[kDwQuad];
        uint32_t m[kDwQuad];
#pragma unroll
        for (int e = 0; e < kDwQuad; ++e) {
            on[e] = live && dwc_out_on(g, blk, d, e);
            const int32_t ow = blk.ow0 + d.c0 + e;
            cb[e] = !on[e] ? 0 : g.masked ? dwc_axis_bits(ow * g.sw - g.pw, g.W, g.KW, 1) : all_cols;
            at[e] = dwc_lds_byte(g, d.pl, d.r * g.sh, (on[e] ? d.c0 + e : d.c0) * g.sw);   // an absent output reads the quad's first
            m[e] = 0;
        }
        for (int32_t i = 0; i < g.KH; ++i) {
            if (!((row_bits >> i) & 1u)) continue;
            uint32_t h[kDwQuad] = {0, 0, 0, 0};
            for (int32_t j = 0; j < g.KW; ++j) {
#pragma unroll
                for (int e = 0; e < kDwQuad; ++e) {
                    const uint32_t v = lds_bytes[at[e] + i * g.fwp + j];
                    h[e] = ((cb[e] >> j) & 1u) ? (v > h[e] ? v : h[e]) : h[e];
                }
            }
#pragma unroll
            for (int e = 0; e < kDwQuad; ++e) m[e] = h[e] > m[e] ? h[e] : m[e];
        }
        uint32_t w;
        if constexpr (OC) {
            float y[kDwQuad];
#pragma unroll
            for (int e = 0; e < kDwQuad; ++e) y[e] = ig_code_value((int8_t)(m[e] ^ 0x80u), px);   // order domain -> signed domain
            w = ig_codes4(y, po);   // every lane of the block
        } else {
            w = (m[0] | m[1] << 8 | m[2] << 16 | m[3] << 24) ^ om;
        }
        const int64_t o = dwc_out_offset(g, p, 0, oh, blk.ow0 + d.c0);
        DFQ_GLOBAL uint8_t* out = (DFQ_GLOBAL uint8_t*)a.out;
        if (dwio_out_word(on[0] && on[1] && on[2] && on[3], reinterpret_cast<uintptr_t>(a.out), o)) {
            *(DFQ_GLOBAL uint32_t*)(out + o) = w;
        } else {
#pragma unroll
            for (int e = 0; e < kDwQuad; ++e)
                if (on[e]) out[o + e] = (uint8_t)(w >> (8 * e));
        }
    }
}

IgOutQ pool_quant(const dfq_int_mbconv_quant& q) {
    return IgOutQ{q.min_dev, q.max_dev, q.given_min, q.given_max, q.bits, q.symmetric, q.flags};
}

}  // namespace
}  // namespace dfq

using namespace dfq;

extern "C" int dfq_int_mean_q(const dfq_int_mean_desc* d, void* stream) {
    MeanArgs a{};
    int64_t grid = 0;
    const int rc = mean_check(d, a.g, grid);
    if (rc != DFQ_OK) return rc;
    a.x = static_cast<const uint8_t*>(d->x);
    a.out = d->out;
    a.qx = pool_quant(d->x_quant);
    a.qo = pool_quant(d->out_quant);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 blocks((unsigned)grid), threads(kThreads);
    if (a.g.small) {
        if (a.g.out_codes) hipLaunchKernelGGL((int_mean_kernel<true, true>), blocks, threads, 0, s, a);
        else hipLaunchKernelGGL((int_mean_kernel<true, false>), blocks, threads, 0, s, a);
    } else {
        if (a.g.out_codes) hipLaunchKernelGGL((int_mean_kernel<false, true>), blocks, threads, 0, s, a);
        else hipLaunchKernelGGL((int_mean_kernel<false, false>), blocks, threads, 0, s, a);
    }
    DFQ_LAUNCH_CHECK();
    return DFQ_OK;
}

extern "C" int dfq_int_maxpool2d_q(const dfq_int_maxpool2d_desc* d, void* stream) {
    MaxArgs a{};
    int64_t grid = 0;
    const int rc = maxpool_check(d, a.g, grid);
    if (rc != DFQ_OK) return rc;
    a.x = static_cast<const uint8_t*>(d->x);
    a.out = static_cast<uint8_t*>(d->out);
    a.qx = pool_quant(d->x_quant);
    a.qo = pool_quant(d->out_quant);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 blocks((unsigned)grid), threads(kThreads);
    if (d->out_quant.bits > 0) hipLaunchKernelGGL(int_maxpool_kernel<true>, blocks, threads, 0, s, a);
    else hipLaunchKernelGGL(int_maxpool_kernel<false>, blocks, threads, 0, s, a);
    DFQ_LAUNCH_CHECK();
    return DFQ_OK;
}
