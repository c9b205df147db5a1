// Host-only part of dfq_int_conv2d: the argument checks, the geometry and the grid
// (dfq_int_conv_plan.h).  Plain C++: no HIP header, no device code.
#include "dfq_int_conv_plan.h"

namespace dfq {

int igc_check(const dfq_int_conv2d_desc* d, MxcGeom& g, int64_t& M, int64_t& K, int64_t& grid) {
    const auto addr = [](const void* p) { return reinterpret_cast<uintptr_t>(p); };
    g = MxcGeom{};
    M = K = grid = 0;
    if (!d) return DFQ_ERR_INVALID;
    if (!d->x || !d->b_codes || !d->b_scale || !d->out) return DFQ_ERR_INVALID;
    // dfq_int_linear's checks of the quantizer and of B
    if ((d->flags & ~(DFQ_INT_B_PACK4 | DFQ_INT_B_PER_ROW | DFQ_SCALE_F32)) != 0 || d->reserved != 0 || d->reserved2 != 0)
        return DFQ_ERR_INVALID;
    if (d->b_signed != 0 && d->b_signed != 1) return DFQ_ERR_INVALID;
    if (d->x_symmetric != 0 && d->x_symmetric != 1) return DFQ_ERR_INVALID;
    if (d->x_bits < 2 || d->x_bits > 8) return DFQ_ERR_INVALID;
    int rc = mxc_check_extents(*d);
    if (rc != DFQ_OK) return rc;
    if (addr(d->x) % 4 || addr(d->out) % 4 || addr(d->bias) % 4 || addr(d->min_dev) % 4 || addr(d->max_dev) % 4) return DFQ_ERR_INVALID;
    if (addr(d->b_codes) % 16 || addr(d->b_scale) % 4 || addr(d->b_zero) % 4) return DFQ_ERR_INVALID;
    int64_t n = 0;
    rc = mxc_check_geometry(*d, g, M, K, n);
    if (rc != DFQ_OK) return rc;
    if (K > kIgMaxK) return DFQ_ERR_UNSUPPORTED;
    if ((d->flags & DFQ_INT_B_PACK4) && K % 2) return DFQ_ERR_UNSUPPORTED;
    grid = n;
    return DFQ_OK;
}

}  // namespace dfq
