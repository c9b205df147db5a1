// dfq_int_add_q: the residual add on stored activation codes -- two tensors of code bytes, each on
// its own grid, summed elementwise and stored as fp32 or as the code bytes of a third grid, in one
// launch (include/dfq_hip.h):
//   y = fl32(dq_A(a[i]) + dq_B(b[i]));  out[i] = y  or  fake_quant_given's code of y on out_quant
// with dq the two rounded fp32 operations of qdq_finish (ig_code_value) and the code the
// quantizer every integer entry shares (ig_quant_params + ig_codes4).
//
// The kernel is bound by memory -- 3 bytes an element with a code output -- so a lane moves 16
// bytes at a time (dfq_int_add_plan.h has the chunks, every address and every predicate):
//   1. the three grids' parameters, once per lane before the loop;
//   2. per chunk of 16 elements: 16 bytes of a and of b into four words each (one 16-B load where
//      the chunk is full and the address allows, else words or predicated bytes), 16 sums in
//      registers, four ig_codes4 words, one 16-B store -- or, fp32, four 16-B stores.
// The loop is grid-stride over the waves' runs of 64 chunks and its trip count is wave-uniform:
// ig_codes4 holds a ballot, so a ragged end is a predicated load and store, never an early exit.
// OC: the output is code bytes.  No LDS, no scratch, no atomics, no workspace.
#include "dfq_int_mm_sources.h"

#include "dfq_int_add_plan.h"

namespace dfq {
namespace {

typedef uint32_t add_v4u __attribute__((ext_vector_type(4)));
typedef uint32_t add_v4u_a4 __attribute__((ext_vector_type(4), aligned(4)));

struct AddArgs {
    const uint8_t* a;
    const uint8_t* b;
    void* out;
    IgOutQ qa, qb, qo;
    AddGeom g;
};

// A chunk's 16 code bytes as four words; an element that does not exist is byte 0.
__device__ __forceinline__ void add_load(const uint8_t* base, const AddGeom& g, int64_t e0, bool full, int32_t access, uint32_t (&w)[4]) {
    const DFQ_GLOBAL uint8_t* p = (const DFQ_GLOBAL uint8_t*)base;
    if (full && access == kAddVector) {
        const add_v4u v = *(const DFQ_GLOBAL add_v4u*)(p + e0);
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] = v[i];
    } else if (full && access == kAddWords) {
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] = *(const DFQ_GLOBAL uint32_t*)(p + e0 + 4 * i);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] = 0;
#pragma unroll
        for (int i = 0; i < kAddChunk; ++i)
            if (add_elem_on(g, e0, i)) w[i >> 2] |= (uint32_t)p[e0 + i] << (8 * (i & 3));
    }
}

template <bool OC>
__global__ __launch_bounds__(kThreads) void int_add_kernel(const AddArgs a) {
    const AddGeom& g = a.g;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const IgAParams pa = ig_out_params(a.qa), pb = ig_out_params(a.qb);
    IgAParams po;
    if constexpr (OC) po = ig_out_params(a.qo);
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    // c0: the wave's first chunk of this trip -- the same in every lane
    for (int64_t c0 = (int64_t)blockIdx.x * kThreads + wave * kWave; c0 < g.chunks; c0 += stride) {
        const int64_t c = c0 + lane, e0 = add_chunk_e0(g, c);
        const bool full = add_chunk_full(g, c);
        uint32_t wa[4], wb[4];
        add_load(a.a, g, e0, full, kAddVector, wa);
        add_load(a.b, g, e0, full, g.b_access, wb);
        float y[kAddChunk];
#pragma unroll
        for (int i = 0; i < kAddChunk; ++i) {
            const int8_t sa = (int8_t)((wa[i >> 2] ^ pa.xm) >> (8 * (i & 3))), sb = (int8_t)((wb[i >> 2] ^ pb.xm) >> (8 * (i & 3)));
            y[i] = ig_code_value(sa, pa) + ig_code_value(sb, pb);
        }
        if constexpr (OC) {
            DFQ_GLOBAL uint8_t* out = (DFQ_GLOBAL uint8_t*)a.out;
            add_v4u w;
#pragma unroll
            for (int i = 0; i < 4; ++i) w[i] = ig_codes4(y + 4 * i, po);   // every lane of the wave
            if (full && g.o_access == kAddVector) {
                *(DFQ_GLOBAL add_v4u*)(out + e0) = w;
            } else if (full && g.o_access == kAddWords) {
#pragma unroll
                for (int i = 0; i < 4; ++i) *(DFQ_GLOBAL uint32_t*)(out + e0 + 4 * i) = w[i];
            } else {
#pragma unroll
                for (int i = 0; i < kAddChunk; ++i)
                    if (add_elem_on(g, e0, i)) out[e0 + i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
            }
        } else {
            DFQ_GLOBAL float* out = (DFQ_GLOBAL float*)a.out;
            if (full) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const ig_v4f_a4 quad = {y[4 * i], y[4 * i + 1], y[4 * i + 2], y[4 * i + 3]};
                    *(DFQ_GLOBAL ig_v4f_a4*)(out + e0 + 4 * i) = quad;
                }
            } else {
#pragma unroll
                for (int i = 0; i < kAddChunk; ++i)
                    if (add_elem_on(g, e0, i)) out[e0 + i] = y[i];
            }
        }
    }
}

IgOutQ add_quant(const dfq_int_mbconv_quant& q) {
    return IgOutQ{q.min_dev, q.max_dev, q.given_min, q.given_max, q.bits, q.symmetric, q.flags};
}

}  // namespace
}  // namespace dfq

using namespace dfq;

extern "C" int dfq_int_add_q(const dfq_int_add_desc* d, void* stream) {
    AddArgs a{};
    int64_t grid = 0;
    const int rc = add_check(d, a.g, grid);
    if (rc != DFQ_OK) return rc;
    a.a = static_cast<const uint8_t*>(d->a);
    a.b = static_cast<const uint8_t*>(d->b);
    a.out = d->out;
    a.qa = add_quant(d->a_quant);
    a.qb = add_quant(d->b_quant);
    a.qo = add_quant(d->out_quant);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 blocks((unsigned)grid), threads(kThreads);
    if (a.g.out_codes) hipLaunchKernelGGL(int_add_kernel<true>, blocks, threads, 0, s, a);
    else hipLaunchKernelGGL(int_add_kernel<false>, blocks, threads, 0, s, a);
    DFQ_LAUNCH_CHECK();
    return DFQ_OK;
}
