// Host-only part of dfq_mx_linear: the argument checks and the grid (dfq_mx_linear_plan.h).
// Plain C++: no HIP header, no device code.
#include "dfq_mx_linear_plan.h"

namespace dfq {

static uintptr_t addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }

int mxl_check(const dfq_mx_linear_desc* d, int64_t& grid) {
    grid = 0;
    if (!d) return DFQ_ERR_INVALID;
    if (!d->x || !d->b_codes || !d->b_scales || !d->out) return DFQ_ERR_INVALID;
    if (mxg_hw_format(d->x_format) < 0 || mxg_hw_format(d->b_format) < 0) return DFQ_ERR_INVALID;
    if (d->flags != 0 || d->reserved != 0) return DFQ_ERR_INVALID;
    if (d->M < 1 || d->N < 1 || d->K < 1) return DFQ_ERR_INVALID;
    // dfq_mx_gemm's limits: byte and element offsets stay far inside int64 and the grid inside int32
    if (d->M > (int64_t(1) << 31) || d->N > (int64_t(1) << 31) || d->K > (int64_t(1) << 40) ||
        d->ldo > (int64_t(1) << 40) || d->ldx > (int64_t(1) << 40))
        return DFQ_ERR_INVALID;
    if (d->M > (int64_t(1) << 50) / d->K || d->N > (int64_t(1) << 50) / d->K) return DFQ_ERR_INVALID;
    if (d->ldx < d->K || d->ldo < d->N) return DFQ_ERR_SHAPE;
    if (d->M > (int64_t(1) << 50) / d->ldx) return DFQ_ERR_INVALID;   // row * ldx + k
    if (addr(d->b_codes) % mxg_code_align(d->b_format)) return DFQ_ERR_INVALID;
    if (addr(d->x) % 4 || addr(d->out) % 4 || addr(d->bias) % 4) return DFQ_ERR_INVALID;
    const int64_t g = mxg_grid(d->M, d->N);
    if (g > 0x7fffffff) return DFQ_ERR_UNSUPPORTED;
    grid = g;
    return DFQ_OK;
}

}  // namespace dfq
