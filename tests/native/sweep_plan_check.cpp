// The sweep planner on its own: dfq_sweep_plan.cpp linked with this main and nothing
// else, so it runs under AddressSanitizer / UBSan on a machine without a GPU
// (tests/test_sweep_plan_host.py builds and runs it).
// Input: a text file of lists -- `n`, then n lines
//   rows row_len khw bits mode flags want_esum src_byte_offset
// Addresses are fixed stand-ins, never dereferenced.  range_enc is non-null exactly
// when DFQ_DEVICE_RANGE is set, unless the checker's own flag bit 0x100 (stripped
// before the planner sees the flags) asks for a NULL one.
// Each list goes through the list planner, then each distinct descriptor of it
// through the single-tensor planner, and every table is checked here against what
// the kernels take on trust (dfq_sweep.hip reads, reduces and stores from a task
// record with no bounds check): coverage, alignment, the whole-row / block-row /
// row-group / slot-piece rules, the records and both layouts.  A failure is a
// message on stderr and exit status 1.
// Output, one line of numbers per plan:
//   list <i> <switch> rc variant main reduce slots blockrow wholerow slotpieces padding
//        o_reduce o_main o_slots total digest
//   single <i>.<t> <switch> ...   (the same with the single-tensor layout: o_tensor for o_slots)
// blockrow counts group entries (block rows and row groups), padding the empty ones
// among them; digest is FNV-1a (64 bit) over the DevTensor and DevTask bytes with the
// stand-in base addresses subtracted.  With -DDFQ_DIAGNOSTICS every case runs again
// under each diagnostics switch of the planner.
#include <algorithm>
#include <cinttypes>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "dfq_sweep_plan.h"

using namespace dfq;

namespace {

constexpr uintptr_t kSrc = 0x100000000000, kDst = 0x200000000000, kCodes = 0x300000000000, kScale = 0x400000000000,
                    kZero = 0x500000000000, kEsum = 0x600000000000, kRange = 0x700000000000;
constexpr int kNullRange = 0x100;   // input flag of this program: DFQ_DEVICE_RANGE with range_enc NULL

struct Switch {
    const char* tag;
    const char* name;    // the environment switch set for this run (null: none)
    const char* value;
};
const Switch kSwitches[] = {
    {"product", nullptr, nullptr},
#ifdef DFQ_DIAGNOSTICS
    {"group_rows", "DFQ_SWEEP_GROUP_ROWS", "1"},
    {"no_blockrow", "DFQ_SWEEP_BLOCKROW", "0"},
    {"span4096", "DFQ_SWEEP_REDUCE_SPAN", "4096"},
    {"shuffle7", "DFQ_SWEEP_SHUFFLE", "7"},
    {"v0", "DFQ_SWEEP_VARIANT", "0"},
    {"v4", "DFQ_SWEEP_VARIANT", "4"},
    {"v8", "DFQ_SWEEP_VARIANT", "8"},
    {"v11", "DFQ_SWEEP_VARIANT", "11"},
#endif
};

const char* g_where = "";
[[noreturn]] void fail(const char* fmt, ...) {
    fprintf(stderr, "%s: ", g_where);
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputc('\n', stderr);
    exit(1);
}
#define REQUIRE(cond, ...) \
    do {                   \
        if (!(cond)) fail(__VA_ARGS__); \
    } while (0)

struct Fnv {
    uint64_t h = 0xcbf29ce484222325ull;
    void add(const void* p, size_t n) {
        const unsigned char* b = static_cast<const unsigned char*>(p);
        for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001b3ull;
    }
};
template <typename P>
P rebase(P p, uintptr_t base) {
    return p ? reinterpret_cast<P>(reinterpret_cast<uintptr_t>(p) - base + 1) : p;
}

struct Counts {
    int64_t blockrow = 0, wholerow = 0, slotpieces = 0, padding = 0;
};

struct Piece {
    int64_t start, n;
    bool first;
};
// pieces in list order: contiguous from `start`, `len` elements in all
bool tiles(const std::vector<Piece>& p, int64_t start, int64_t len) {
    int64_t at = start;
    for (const Piece& x : p) {
        if (x.start != at) return false;
        at += x.n;
    }
    return at == start + len;
}

// Every invariant of one plan's tables.  `span`: the reduce span in force;
// `ordered`: the main list is in the planner's order (no DFQ_SWEEP_SHUFFLE).
Counts check_tables(const std::vector<dfq_tensor_desc>& d, const SweepTables& T, int64_t span, bool ordered) {
    const Variant V = kVariants[T.variant];
    const int64_t nt = (int64_t)d.size();
    REQUIRE((int64_t)T.tensors.size() == nt, "%zu tensor records for %lld tensors", T.tensors.size(), (long long)nt);
    Counts c;
    int64_t elems = 0, algo = 0;
    for (int64_t t = 0; t < nt; ++t) {
        const dfq_tensor_desc& x = d[t];
        const DevTensor& D = T.tensors[t];
        const int64_t total = x.rows * x.row_len;
        REQUIRE(D.src == x.src && D.rows == x.rows && D.row_len == x.row_len && D.khw == x.khw && D.flags == x.flags &&
                    D.mode == x.mode && D.bits == x.bits, "tensor %lld: record differs from its descriptor", (long long)t);
        REQUIRE((D.range_enc != nullptr) == ((x.flags & DFQ_DEVICE_RANGE) != 0), "tensor %lld: range_enc", (long long)t);
        REQUIRE(D.code_bytes == ((x.flags & DFQ_PACK_INT4) ? 0 : (x.bits <= 8 ? 1 : 2)), "tensor %lld: code_bytes", (long long)t);
        if (D.vec4) {
            REQUIRE(total % 4 == 0 && reinterpret_cast<uintptr_t>(x.src) % 16 == 0 &&
                        (x.mode < DFQ_CHANNEL_ASYM || x.row_len % 4 == 0), "tensor %lld: vec4 on unaligned data", (long long)t);
        }
        elems += total;
        const int64_t npar = x.mode >= DFQ_CHANNEL_ASYM ? x.rows : 1;
        algo += 4 * total + (x.dst ? 4 * total : 0) + (x.codes ? (D.code_bytes ? D.code_bytes * total : total / 2) : 0) +
                (x.esum ? 4 * (total / x.khw) : 0) + (x.scale ? 4 * npar : 0) + (x.zero ? 4 * npar : 0);
    }
    REQUIRE(T.elems == elems && T.algo_bytes == algo, "elems %lld / algo_bytes %lld, expected %lld / %lld",
            (long long)T.elems, (long long)T.algo_bytes, (long long)elems, (long long)algo);

    // records, alignment and the per-kind rules of one task; returns its first element
    auto record = [&](const DevTask& k, const char* list, size_t i) -> int64_t {
        REQUIRE(k.tensor >= 0 && k.tensor < nt, "%s task %zu: tensor %d", list, i, k.tensor);
        const dfq_tensor_desc& x = d[k.tensor];
        const DevTensor& D = T.tensors[k.tensor];
        const int64_t total = x.rows * x.row_len;
        const ptrdiff_t bytes = reinterpret_cast<const char*>(k.src) - reinterpret_cast<const char*>(x.src);
        REQUIRE(bytes >= 0 && bytes % 4 == 0, "%s task %zu: src is not an element of its tensor", list, i);
        const int64_t start = bytes / 4;
        REQUIRE(k.n >= 0 && start + k.n <= total, "%s task %zu: [%lld, +%d) of %lld", list, i, (long long)start, k.n,
                (long long)total);
        REQUIRE((k.flags & ~3) == 0 && ((k.flags & 2) != 0) == (D.vec4 != 0), "%s task %zu: flags %d", list, i, k.flags);
        if (D.vec4) REQUIRE(start % 4 == 0 && k.n % 4 == 0, "%s task %zu: vec4 task off a multiple of 4", list, i);
        if (x.esum) REQUIRE(start % x.khw == 0 && k.n % x.khw == 0, "%s task %zu: an error sum straddles it", list, i);
        if (x.flags & DFQ_PACK_INT4) REQUIRE(start % 2 == 0, "%s task %zu: packed task at an odd element", list, i);
        return start;
    };

    // ---- the main list ----
    const size_t nm = T.main.size();
    std::vector<int64_t> start(nm);
    std::vector<std::vector<Piece>> cover((size_t)nt);           // per tensor, non-empty tasks
    std::map<int32_t, std::vector<Piece>> slot_pieces;           // per slot, list order
    std::vector<int32_t> slot_tensor((size_t)T.slots, -1), slot_row((size_t)T.slots, -1);
    std::map<int32_t, std::vector<Piece>> given_pieces;          // per tensor with a given / device range
    size_t last_group = 0, first_slotted = nm;
    bool any_group = false;
    for (size_t i = 0; i < nm; ++i) {
        const DevTask& k = T.main[i];
        start[i] = record(k, "main", i);
        const dfq_tensor_desc& x = d[k.tensor];
        const bool channel = x.mode >= DFQ_CHANNEL_ASYM;
        const bool given = (x.flags & (DFQ_GIVEN_RANGE | DFQ_DEVICE_RANGE)) != 0;
        REQUIRE(k.n <= V.chunk, "main task %zu: %d elements in a %d-element task", i, k.n, V.chunk);
        if (k.n > 0) cover[k.tensor].push_back(Piece{start[i], k.n, (k.flags & 1) != 0});
        if (k.nrows > 0) {   // whole rows
            ++c.wholerow;
            REQUIRE(channel, "main task %zu: whole rows in a tensor mode", i);
            REQUIRE(k.nrows <= V.max_rows && k.row0 >= 0 && (int64_t)k.row0 + k.nrows <= x.rows, "main task %zu: rows", i);
            REQUIRE(start[i] == (int64_t)k.row0 * x.row_len && k.n == k.nrows * x.row_len && k.n > 0,
                    "main task %zu: not rows [%d, +%d)", i, k.row0, k.nrows);
            REQUIRE(k.slot == -1 && !(k.flags & 1), "main task %zu: whole rows with a slot or `first`", i);
        } else if (k.nrows < 0) {   // a group entry: its quad is checked below
            ++c.blockrow;
            c.padding += k.n == 0;
            any_group = true;
            last_group = i;
            REQUIRE(!given && !V.prefetch, "main task %zu: a group where none may be", i);
        } else {   // a piece
            REQUIRE(k.n > 0 && k.row0 >= 0 && (channel ? k.row0 < x.rows : k.row0 == 0), "main task %zu: piece", i);
            if (k.slot < 0) {
                REQUIRE(k.slot == -1 && given, "main task %zu: a piece without a slot or a given range", i);
                given_pieces[k.tensor].push_back(Piece{start[i], k.n, (k.flags & 1) != 0});
            } else {
                ++c.slotpieces;
                first_slotted = std::min(first_slotted, i);
                REQUIRE(k.slot < T.slots && !given, "main task %zu: slot %d of %lld", i, k.slot, (long long)T.slots);
                REQUIRE(slot_tensor[k.slot] < 0 || (slot_tensor[k.slot] == k.tensor && slot_row[k.slot] == k.row0),
                        "main task %zu: slot %d serves two ranges", i, k.slot);
                slot_tensor[k.slot] = k.tensor;
                slot_row[k.slot] = k.row0;
                slot_pieces[k.slot].push_back(Piece{start[i], k.n, (k.flags & 1) != 0});
            }
        }
    }
    REQUIRE(c.blockrow % kWavesPerBlock == 0, "%lld group entries", (long long)c.blockrow);
    if (ordered) {   // groups first (the 4 waves of a block meet a quad together), slot pieces last
        REQUIRE(!any_group || last_group + 1 == (size_t)c.blockrow, "group entries are no prefix of the main list");
        REQUIRE(first_slotted == nm - (size_t)c.slotpieces, "slot pieces are no tail of the main list");
        for (size_t i = first_slotted; i < nm; ++i)
            REQUIRE(T.main[i].nrows == 0 && T.main[i].slot >= 0, "main task %zu: not a slot piece, among them", i);
    }
    // quads: list positions 4q .. 4q+3 hold one group or no group entry at all
    for (size_t q = 0; q < nm; q += kWavesPerBlock) {
        const size_t e = std::min(nm, q + kWavesPerBlock);
        bool group = false;
        for (size_t i = q; i < e; ++i) group = group || T.main[i].nrows < 0;
        if (!group) continue;
        REQUIRE(e - q == kWavesPerBlock, "main task %zu: a group cut short by the list's end", q);
        const DevTask& k0 = T.main[q];
        const dfq_tensor_desc& x = d[k0.tensor];
        const bool channel = x.mode >= DFQ_CHANNEL_ASYM;
        for (size_t i = q; i < e; ++i)
            REQUIRE(T.main[i].tensor == k0.tensor && T.main[i].nrows == k0.nrows && T.main[i].slot == -1,
                    "main task %zu: its quad mixes tensors, tags or slots", i);
        if (k0.nrows <= kGroupTag) {   // R whole rows in 4 pieces
            const int R = kGroupTag - k0.nrows + 1;
            REQUIRE(channel && R >= 1 && R <= kGroupMaxRows && k0.row0 >= 0 && (int64_t)k0.row0 + R <= x.rows,
                    "main task %zu: row group of %d rows from %d", q, R, k0.row0);
            std::vector<Piece> p;
            for (size_t i = q; i < e; ++i) {
                REQUIRE(T.main[i].row0 == k0.row0 && !(T.main[i].flags & 1), "main task %zu: row group entry", i);
                p.push_back(Piece{start[i], T.main[i].n, false});
            }
            REQUIRE(tiles(p, (int64_t)k0.row0 * x.row_len, R * x.row_len), "main task %zu: row group does not tile its rows", q);
            continue;
        }
        const int gs = -k0.nrows;   // pieces per range
        REQUIRE(gs == 2 || gs == kWavesPerBlock, "main task %zu: nrows %d", q, k0.nrows);
        const int64_t blen = channel ? x.row_len : x.rows * x.row_len;
        for (size_t g = q; g < e; g += gs) {
            std::vector<Piece> p;
            int64_t n = 0;
            for (size_t i = g; i < g + gs; ++i) {
                REQUIRE(T.main[i].row0 == T.main[g].row0, "main task %zu: a range's pieces name two rows", i);
                REQUIRE(((T.main[i].flags & 1) != 0) == (i == g && T.main[i].n > 0), "main task %zu: `first`", i);
                p.push_back(Piece{start[i], T.main[i].n, false});
                n += T.main[i].n;
            }
            if (n == 0) {   // a padding half-group: the second range of the last pair quad
                REQUIRE(gs == 2 && g == q + 2, "main task %zu: an empty range", g);
                continue;
            }
            const int32_t r = T.main[g].row0;
            REQUIRE(r >= 0 && (channel ? r < x.rows : r == 0), "main task %zu: row %d", g, r);
            REQUIRE(tiles(p, (int64_t)r * blen, blen), "main task %zu: block-row pieces do not tile their range", g);
        }
    }
    // coverage: every tensor's non-empty main tasks partition [0, rows * row_len)
    for (int64_t t = 0; t < nt; ++t) {
        std::vector<Piece>& p = cover[t];
        std::sort(p.begin(), p.end(), [](const Piece& a, const Piece& b) { return a.start < b.start; });
        REQUIRE(tiles(p, 0, d[t].rows * d[t].row_len), "tensor %lld: its tasks do not partition it", (long long)t);
    }
    // ranges served in pieces: one `first`, at the range's offset 0, pieces tiling the extent
    auto one_first = [&](const std::vector<Piece>& p, int64_t at, const char* what, int64_t id) {
        int firsts = 0;
        for (const Piece& x : p) {
            firsts += x.first;
            REQUIRE(!x.first || x.start == at, "%s %lld: `first` off the range's start", what, (long long)id);
        }
        REQUIRE(firsts == 1, "%s %lld: %d pieces write its parameters", what, (long long)id, firsts);
    };
    for (auto& kv : given_pieces) {
        std::sort(kv.second.begin(), kv.second.end(), [](const Piece& a, const Piece& b) { return a.start < b.start; });
        REQUIRE(tiles(kv.second, 0, d[kv.first].rows * d[kv.first].row_len), "tensor %d: given-range pieces", kv.first);
        one_first(kv.second, 0, "tensor", kv.first);
    }
    auto extent = [&](int32_t s, int64_t& at, int64_t& len) {
        const dfq_tensor_desc& x = d[slot_tensor[s]];
        const bool channel = x.mode >= DFQ_CHANNEL_ASYM;
        len = channel ? x.row_len : x.rows * x.row_len;
        at = channel ? slot_row[s] * len : 0;
    };
    REQUIRE((int64_t)slot_pieces.size() == T.slots, "%zu of %lld slots have pieces", slot_pieces.size(), (long long)T.slots);
    for (auto& kv : slot_pieces) {
        int64_t at, len;
        extent(kv.first, at, len);
        std::sort(kv.second.begin(), kv.second.end(), [](const Piece& a, const Piece& b) { return a.start < b.start; });
        REQUIRE(tiles(kv.second, at, len), "slot %d: its pieces do not tile its range", kv.first);
        one_first(kv.second, at, "slot", kv.first);
    }
    // ---- the reduce list: each slot's extent exactly once, no task across a slot or past the span ----
    std::map<int32_t, std::vector<Piece>> red;
    for (size_t i = 0; i < T.reduce.size(); ++i) {
        const DevTask& k = T.reduce[i];
        const int64_t s0 = record(k, "reduce", i);
        REQUIRE(k.nrows == 0 && k.slot >= 0 && k.slot < T.slots && slot_tensor[k.slot] == k.tensor && k.n > 0,
                "reduce task %zu: slot %d, tensor %d", i, k.slot, k.tensor);
        REQUIRE(k.n <= std::max<int64_t>(span, V.chunk), "reduce task %zu: %d elements past the span", i, k.n);
        red[k.slot].push_back(Piece{s0, k.n, false});
    }
    REQUIRE((int64_t)red.size() == T.slots, "%zu of %lld slots are reduced", red.size(), (long long)T.slots);
    for (auto& kv : red) {
        int64_t at, len;
        extent(kv.first, at, len);
        std::sort(kv.second.begin(), kv.second.end(), [](const Piece& a, const Piece& b) { return a.start < b.start; });
        REQUIRE(tiles(kv.second, at, len), "slot %d: the reduce tasks do not cover its range once", kv.first);
    }
    return c;
}

uint64_t digest(const SweepTables& T) {
    Fnv f;
    for (DevTensor t : T.tensors) {
        t.src = rebase(t.src, kSrc);
        t.dst = rebase(t.dst, kDst);
        t.codes = rebase(t.codes, kCodes);
        t.scale = rebase(t.scale, kScale);
        t.zero = rebase(t.zero, kZero);
        t.esum = rebase(t.esum, kEsum);
        t.range_enc = rebase(t.range_enc, kRange);
        f.add(&t, sizeof(t));
    }
    for (const std::vector<DevTask>* list : {&T.reduce, &T.main})
        for (DevTask k : *list) {
            k.src = rebase(k.src, kSrc);
            f.add(&k, sizeof(k));
        }
    return f.h;
}

void print_plan(const char* kind, const char* id, const char* tag, int rc, const SweepTables& T, const Counts& c,
                int64_t o_reduce, int64_t o_main, int64_t o_third, int64_t total, uint64_t dg) {
    printf("%s %s %s %d %d %zu %zu %lld %lld %lld %lld %lld %lld %lld %lld %lld %016" PRIx64 "\n", kind, id, tag, rc,
           T.variant, T.main.size(), T.reduce.size(), (long long)T.slots, (long long)c.blockrow, (long long)c.wholerow,
           (long long)c.slotpieces, (long long)c.padding, (long long)o_reduce, (long long)o_main, (long long)o_third,
           (long long)total, dg);
}

bool same_desc(const dfq_tensor_desc& a, const dfq_tensor_desc& b) {
    return a.src == b.src && a.esum == b.esum && a.range_enc == b.range_enc && a.rows == b.rows &&
           a.row_len == b.row_len && a.khw == b.khw && a.bits == b.bits && a.mode == b.mode && a.flags == b.flags;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return fprintf(stderr, "usage: %s lists.txt\n", argv[0]), 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return perror(argv[1]), 2;
    long long n;
    for (int li = 0; fscanf(f, "%lld", &n) == 1; ++li) {
        std::vector<dfq_tensor_desc> d((size_t)n);
        for (dfq_tensor_desc& p : d) {
            long long rows, row_len, khw, bits, mode, flags, esum, off;
            if (fscanf(f, "%lld %lld %lld %lld %lld %lld %lld %lld", &rows, &row_len, &khw, &bits, &mode, &flags, &esum,
                       &off) != 8)
                return fprintf(stderr, "list %d: truncated\n", li), 2;
            p = dfq_tensor_desc{};
            p.src = reinterpret_cast<const float*>(kSrc + (uintptr_t)off);
            p.dst = reinterpret_cast<float*>(kDst);
            p.codes = reinterpret_cast<void*>(kCodes);
            p.scale = reinterpret_cast<float*>(kScale);
            p.zero = reinterpret_cast<float*>(kZero);
            p.esum = esum ? reinterpret_cast<float*>(kEsum) : nullptr;
            p.rows = rows;
            p.row_len = row_len;
            p.khw = (int32_t)khw;
            p.bits = (int32_t)bits;
            p.mode = (int32_t)mode;
            p.flags = (int32_t)(flags & ~kNullRange);
            p.given_min = -1.0;
            p.given_max = 1.0;
            if ((flags & DFQ_DEVICE_RANGE) && !(flags & kNullRange)) p.range_enc = reinterpret_cast<const uint32_t*>(kRange);
        }
        for (const Switch& s : kSwitches) {
            for (const Switch& o : kSwitches)
                if (o.name) unsetenv(o.name);
            if (s.name) setenv(s.name, s.value, 1);
            const int64_t span = (s.name && !strcmp(s.name, "DFQ_SWEEP_REDUCE_SPAN")) ? atoll(s.value) : 16384;
            const bool ordered = !(s.name && !strcmp(s.name, "DFQ_SWEEP_SHUFFLE"));
            char id[64], where[160];
            {
                snprintf(id, sizeof(id), "%d", li);
                snprintf(where, sizeof(where), "list %s (%s)", id, s.tag);
                g_where = where;
                SweepTables T;
                PlanLayout L;
                const int rc = sweep_plan_tables(d.data(), (int32_t)n, T, L);
                const int64_t ws = dfq_sweep_plan_ws_bytes(d.data(), (int32_t)n);
                Counts c;
                if (rc == DFQ_OK) {
                    c = check_tables(d, T, span, ordered);
                    REQUIRE(L.o_tensors == 0 && L.o_reduce % 256 == 0 && L.o_main % 256 == 0 && L.o_slots % 256 == 0 &&
                                L.total % 256 == 0, "layout alignment");
                    REQUIRE(L.o_reduce >= (int64_t)(sizeof(DevTensor) * T.tensors.size()) &&
                                L.o_main >= L.o_reduce + (int64_t)(sizeof(DevTask) * T.reduce.size()) &&
                                L.o_slots >= L.o_main + (int64_t)(sizeof(DevTask) * T.main.size()) &&
                                L.total >= L.o_slots + 8 * T.slots && L.total < L.o_slots + 8 * T.slots + 256,
                            "layout order");
                    REQUIRE(ws == L.total, "dfq_sweep_plan_ws_bytes %lld, layout %lld", (long long)ws, (long long)L.total);
                } else {
                    REQUIRE(ws == -1, "dfq_sweep_plan_ws_bytes %lld for rc %d", (long long)ws, rc);
                    T = SweepTables{};
                    L = PlanLayout{};
                }
                print_plan("list", id, s.tag, rc, T, c, L.o_reduce, L.o_main, L.o_slots,
                           rc == DFQ_OK ? L.total : ws,
                           rc == DFQ_OK ? digest(T) : 0);
            }
            for (size_t t = 0; t < d.size(); ++t) {
                bool seen = false;
                for (size_t u = 0; u < t && !seen; ++u) seen = same_desc(d[u], d[t]);
                if (seen) continue;   // the single-tensor plan depends on the descriptor alone
                snprintf(id, sizeof(id), "%d.%zu", li, t);
                snprintf(where, sizeof(where), "single %s (%s)", id, s.tag);
                g_where = where;
                const std::vector<dfq_tensor_desc> one(1, d[t]);
                SweepTables T;
                SingleLayout L;
                const int rc = sweep_single_tables(one[0], T, L);
                size_t ws = 0;
                const int rc_ws = dfq_quantize_ws_bytes(&one[0], &ws);
                REQUIRE(rc_ws == rc, "dfq_quantize_ws_bytes rc %d, planner %d", rc_ws, rc);
                Counts c;
                if (rc == DFQ_OK) {
                    REQUIRE(T.variant == kDefaultVariant, "single-tensor plan at variant %d", T.variant);
                    c = check_tables(one, T, span, ordered);
                    REQUIRE(L.o_tensor % 64 == 0 && L.o_reduce % 64 == 0 && L.o_main % 64 == 0, "layout alignment");
                    REQUIRE(L.o_tensor >= 8 * (size_t)T.slots && L.o_tensor < 8 * (size_t)T.slots + 64 &&
                                L.o_reduce >= L.o_tensor + sizeof(DevTensor) &&
                                L.o_main >= L.o_reduce + sizeof(DevTask) * T.reduce.size() &&
                                L.total == L.o_main + sizeof(DevTask) * T.main.size(), "layout order");
                    REQUIRE(ws == L.total, "dfq_quantize_ws_bytes %zu, layout %zu", ws, L.total);
                } else {
                    T = SweepTables{};
                    L = SingleLayout{};
                }
                print_plan("single", id, s.tag, rc, T, c, (int64_t)L.o_reduce, (int64_t)L.o_main,
                           (int64_t)L.o_tensor, (int64_t)L.total, rc == DFQ_OK ? digest(T) : 0);
            }
        }
    }
    fclose(f);
    return 0;
}
