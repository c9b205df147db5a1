// Host-only part of dfq_mx_gemm: the argument checks and the grid (dfq_mx_gemm_plan.h).
// Plain C++: no HIP header, no device code.
#include "dfq_mx_gemm_plan.h"

namespace dfq {

int mxg_check(const dfq_mx_gemm_desc* d, int64_t& grid) {
    grid = 0;
    if (!d) return DFQ_ERR_INVALID;
    return mxm_check(*d, d->a_codes && d->a_scales, mxg_hw_format(d->a_format),
                     reinterpret_cast<uintptr_t>(d->a_codes) % mxg_code_align(d->a_format) == 0, d->K, grid);
}

}  // namespace dfq
