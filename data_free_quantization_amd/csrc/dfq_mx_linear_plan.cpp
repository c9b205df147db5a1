// Host-only part of dfq_mx_linear: the argument checks and the grid (dfq_mx_linear_plan.h).
// Plain C++: no HIP header, no device code.
#include "dfq_mx_linear_plan.h"

namespace dfq {

int mxl_check(const dfq_mx_linear_desc* d, int64_t& grid) {
    grid = 0;
    if (!d) return DFQ_ERR_INVALID;
    return mxm_check(*d, d->x != nullptr, mxg_hw_format(d->x_format), reinterpret_cast<uintptr_t>(d->x) % 4 == 0, d->ldx, grid);
}

}  // namespace dfq
