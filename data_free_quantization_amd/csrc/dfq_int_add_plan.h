// The index arithmetic of dfq_int_add_q (dfq_int_add.hip): the sum of two tensors of n stored
// code bytes, elementwise, on code bytes or fp32.
//
// A lane owns a chunk of 16 consecutive elements.  Chunks are counted from a's first 16-B
// boundary, not from element 0: with ha = a mod 16, chunk c holds the elements
//   e0 = 16 c - ha  ..  e0 + 15,      c < chunks = ceil((n + ha) / 16),
// so a's bytes of every chunk start on a 16-B boundary, the first chunk holds the 16 - ha
// elements before it (none when ha = 0) and the last one the tail.  A chunk is full when all 16
// elements exist; only the first and the last can be ragged.
//   full chunk    a: one 16-B load.  b and a code output: by their own address at the chunk,
//                 (base - ha) mod 16 -- one 16-B access where that is 0 (the bases agree mod 16),
//                 four 4-B words where it is a multiple of 4, else 16 bytes.  An fp32 output: four
//                 16-B stores (4-B aligned, as the block's store).
//   ragged chunk  predicated byte loads and byte (fp32: element) stores; an absent element is
//                 code 0 on the way in and is not stored.
// A wave takes 64 consecutive chunks; a block of kThreads lanes takes 4 waves' worth, grid-stride.
// The loop's trip count is the wave's (the chunk of lane 0 decides), since the output quantizer
// holds a ballot: a lane whose chunk is past the end runs the body with every element absent.
// The kernel uses these helpers and nothing else for an address or a predicate.  No HIP header:
// the checks (dfq_int_add_plan.cpp) build as plain C++.
#pragma once
#include "dfq_int_mbconv_plan.h"

namespace dfq {

constexpr int kAddChunk = 16;                 // elements of a lane's chunk
constexpr int64_t kAddMaxN = int64_t(1) << 40;
constexpr int kAddMaxBlocks = 2048;           // 256 CUs x 8 resident blocks of kThreads lanes

enum AddAccess : int32_t { kAddBytes = 0, kAddWords = 1, kAddVector = 2 };

struct AddGeom {
    int64_t n, chunks;
    int32_t ha;               // a mod 16: the elements of the first chunk that do not exist
    int32_t b_access, o_access;   // AddAccess of b and of a code output in a full chunk
    int32_t out_codes;
};

// How a full chunk's 16 bytes of the tensor at `base` are accessed.
DFQ_HOST_DEVICE inline int32_t add_access(uintptr_t base, int32_t ha) {
    const uintptr_t at = (base - (uintptr_t)ha) & 15u;
    return at == 0 ? kAddVector : (at & 3u) == 0 ? kAddWords : kAddBytes;
}
DFQ_HOST_DEVICE inline int64_t add_chunk_e0(const AddGeom& g, int64_t c) { return c * kAddChunk - g.ha; }
DFQ_HOST_DEVICE inline bool add_chunk_full(const AddGeom& g, int64_t c) {
    const int64_t e0 = add_chunk_e0(g, c);
    return c < g.chunks && e0 >= 0 && e0 + kAddChunk <= g.n;
}
// Element e0 + i of a chunk exists.
DFQ_HOST_DEVICE inline bool add_elem_on(const AddGeom& g, int64_t e0, int i) { return e0 + i >= 0 && e0 + i < g.n; }

// dfq_int_add_q's argument checks (no device call): DFQ_OK with the geometry and the grid, or the
// error.
int add_check(const dfq_int_add_desc* d, AddGeom& g, int64_t& grid);

}  // namespace dfq
