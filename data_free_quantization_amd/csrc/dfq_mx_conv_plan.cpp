// Host-only part of dfq_mx_conv2d: the argument checks, the geometry and the grid
// (dfq_mx_conv_plan.h).  Plain C++: no HIP header, no device code.
#include "dfq_mx_conv_plan.h"

namespace dfq {

int mxc_check(const dfq_mx_conv2d_desc* d, MxcGeom& g, int64_t& M, int64_t& K, int64_t& grid) {
    const auto addr = [](const void* p) { return reinterpret_cast<uintptr_t>(p); };
    g = MxcGeom{};
    M = K = grid = 0;
    if (!d) return DFQ_ERR_INVALID;
    if (!d->x || !d->b_codes || !d->b_scales || !d->out) return DFQ_ERR_INVALID;
    if (mxg_hw_format(d->x_format) < 0 || mxg_hw_format(d->b_format) < 0) return DFQ_ERR_INVALID;
    if (d->flags != 0 || d->reserved != 0) return DFQ_ERR_INVALID;
    const int rc = mxc_check_extents(*d);
    if (rc != DFQ_OK) return rc;
    if (addr(d->x) % 4 || addr(d->out) % 4 || addr(d->bias) % 4) return DFQ_ERR_INVALID;
    if (addr(d->b_codes) % mxg_code_align(d->b_format)) return DFQ_ERR_INVALID;
    return mxc_check_geometry(*d, g, M, K, grid);
}

}  // namespace dfq
