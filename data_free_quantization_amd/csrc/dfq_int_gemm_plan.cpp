// Host-only part of dfq_int_gemm and dfq_int_linear: the argument checks and the grid
// (dfq_int_gemm_plan.h).  Plain C++: no HIP header, no device code.
#include "dfq_int_gemm_plan.h"

namespace dfq {

namespace {
inline bool aligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }
}  // namespace

int ig_check(const dfq_int_gemm_desc* d, int64_t& grid) {
    grid = 0;
    if (!d) return DFQ_ERR_INVALID;
    const bool a_ok = d->a_codes && d->a_scale && aligned(d->a_codes, 16) && aligned(d->a_scale, 4) && aligned(d->a_zero, 4) &&
                      (d->a_signed == 0 || d->a_signed == 1);
    return ig_check_common(*d, a_ok, d->K, DFQ_INT_B_PACK4 | DFQ_INT_B_PER_ROW, grid);
}

int igl_check(const dfq_int_linear_desc* d, int64_t& grid) {
    grid = 0;
    if (!d) return DFQ_ERR_INVALID;
    const bool a_ok = d->x && aligned(d->x, 4) && aligned(d->min_dev, 4) && aligned(d->max_dev, 4) && d->x_bits >= 2 && d->x_bits <= 8 &&
                      (d->x_symmetric == 0 || d->x_symmetric == 1) && d->reserved2 == 0;
    return ig_check_common(*d, a_ok, d->ldx, DFQ_INT_B_PACK4 | DFQ_INT_B_PER_ROW | DFQ_SCALE_F32, grid);
}

}  // namespace dfq
