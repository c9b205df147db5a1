// The index arithmetic and checks the code-in / code-out entries add (dfq_int_*_q: dfq_int_io.hip,
// dfq_int_dwconv_io.hip): activations as stored bytes.  A code tensor is NCHW like the fp32 one, a
// byte an element, so an element's byte offset is the element offset the old helpers give
// (mxc_x_offset, mxc_out_offset, dwc_x_offset, dwc_out_offset); what is new is alignment -- a
// byte tensor promises none, so every 4-B access is a predicate of the address:
//   - the matrix kernels' NCHW store: a lane's four bytes are rows m .. m + 3 of one column, one
//     4-B store where mxc_out_quad holds and the byte address is 4-aligned, else byte stores;
//   - the depthwise footprint copy: a cell's four columns as one 4-B load where all four are read
//     and the address is 4-aligned, else byte loads;
//   - the depthwise store: a quad's four outputs as one 4-B store where all exist and the address
//     is 4-aligned.
// The kernels and the host check (tests/native/int_io_plan_check.cpp) use these helpers and
// nothing else for such a decision.  No HIP header: builds as plain C++.
#pragma once
#include "dfq_int_dwconv_plan.h"

namespace dfq {

DFQ_HOST_DEVICE inline bool igio_word_at(uintptr_t base, int64_t byte_offset) { return ((base + (uintptr_t)byte_offset) & 3u) == 0; }

// Rows m .. m + 3 of column n of an NCHW code tensor at `out` go out as one word.
DFQ_HOST_DEVICE inline bool igio_out_word(const MxcGeom& g, int64_t m, int64_t M, int64_t n, uintptr_t out) {
    return mxc_out_quad(g, m, M) && igio_word_at(out, mxc_out_offset(g, m, n));
}
// Footprint columns col .. col + 3 of row r of plane p come in as one word: all four are read
// (dwc_x_reads is monotone between the two ends of a row) and the first one's address is aligned.
DFQ_HOST_DEVICE inline bool dwio_x_word(const DwcGeom& g, const DwcBlock& b, int64_t p, int32_t r, int32_t col, uintptr_t x) {
    return dwc_x_reads(g, b, p, r, col) && dwc_x_reads(g, b, p, r, col + 3) && igio_word_at(x, dwc_x_offset(g, b, p, r, col));
}
// The quad's four outputs, the first at byte offset o, go out as one word.
DFQ_HOST_DEVICE inline bool dwio_out_word(bool all_on, uintptr_t out, int64_t o) { return all_on && igio_word_at(out, o); }

// What the old entry's checks are told (kIgBytesX | kIgBytesOut): a tensor of code bytes is excused
// from fp32's 4-B alignment and from nothing else.
inline unsigned igio_bytes(const dfq_int_io* io) {
    return io ? (io->x_codes == 1 ? kIgBytesX : 0u) | (io->out_bits > 0 ? kIgBytesOut : 0u) : 0u;
}

// The io struct's own checks, after the old entry's.  conv: the entry takes x_codes.
inline int igio_check(const dfq_int_io* io, bool conv) {
    const auto addr = [](const void* p) { return reinterpret_cast<uintptr_t>(p); };
    if (!io) return DFQ_ERR_INVALID;
    if (io->x_codes != 0 && !(conv && io->x_codes == 1)) return DFQ_ERR_INVALID;
    if (io->out_bits != 0 && (io->out_bits < 2 || io->out_bits > 8)) return DFQ_ERR_INVALID;
    if (io->out_symmetric != 0 && io->out_symmetric != 1) return DFQ_ERR_INVALID;
    if ((io->out_flags & ~DFQ_SCALE_F32) != 0) return DFQ_ERR_INVALID;
    if (addr(io->out_min_dev) % 4 || addr(io->out_max_dev) % 4) return DFQ_ERR_INVALID;
    if (io->out_bits > 0 && !io->out_min_dev && !io->out_max_dev && !(io->out_given_max > io->out_given_min)) return DFQ_ERR_INVALID;
    return DFQ_OK;
}

}  // namespace dfq
