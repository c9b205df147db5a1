// Host-only part of dfq_int_add_q: the argument checks, the chunk origin, the access of each
// tensor and the grid (dfq_int_add_plan.h).  Plain C++: no HIP header, no device code.
#include "dfq_int_add_plan.h"

namespace dfq {

int add_check(const dfq_int_add_desc* d, AddGeom& g, int64_t& grid) {
    const auto addr = [](const void* p) { return reinterpret_cast<uintptr_t>(p); };
    g = AddGeom{};
    grid = 0;
    if (!d) return DFQ_ERR_INVALID;
    if (!d->a || !d->b || !d->out) return DFQ_ERR_INVALID;
    if (d->flags != 0 || d->reserved != 0) return DFQ_ERR_INVALID;
    const dfq_int_mbconv_quant* quants[] = {&d->a_quant, &d->b_quant, &d->out_quant};
    for (int i = 0; i < 3; ++i)
        if (int rc = mb_check_quant(*quants[i], i == 2)) return rc;
    if (d->n < 1 || d->n > kAddMaxN) return DFQ_ERR_INVALID;
    if (d->out_quant.bits == 0 && addr(d->out) % 4) return DFQ_ERR_INVALID;
    for (const auto* q : quants)
        if (!mb_quant_aligned(*q)) return DFQ_ERR_INVALID;

    g.n = d->n;
    g.ha = (int32_t)(addr(d->a) & 15u);
    g.chunks = ceil_div(d->n + g.ha, (int64_t)kAddChunk);
    g.out_codes = d->out_quant.bits > 0;
    g.b_access = add_access(addr(d->b), g.ha);
    g.o_access = g.out_codes ? add_access(addr(d->out), g.ha) : kAddVector;
    const int64_t blocks = ceil_div(g.chunks, (int64_t)kThreads);
    grid = blocks < kAddMaxBlocks ? blocks : kAddMaxBlocks;
    return DFQ_OK;
}

}  // namespace dfq
