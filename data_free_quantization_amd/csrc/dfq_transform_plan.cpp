// Host-only planners of the graph transforms (see dfq_transform_plan.h): no HIP call, no device
// pointer dereferenced.
#include "dfq_transform_plan.h"

#include <utility>

namespace dfq {

// ---- BN fold ---------------------------------------------------------------
int64_t bn_fold_span(const dfq_bn_fold_desc* d, int32_t n) {
    int64_t total = 0;
    for (int32_t j = 0; j < n; ++j) total += d[j].rows * d[j].row_len;
    return std::min<int64_t>(std::max<int64_t>(8192, ceil_div(total, (int64_t)16384 * 8192) * 8192), kBnFoldMaxSpan);
}

BnFoldLayout bn_fold_layout(const dfq_bn_fold_desc* d, int32_t n) {
    BnFoldLayout L;
    L.span = bn_fold_span(d, n);
    for (int32_t j = 0; j < n; ++j) L.nchunks += ceil_div(d[j].rows * d[j].row_len, L.span);
    L.o_chunks = round256((int64_t)sizeof(BnFoldJob) * n);
    L.total = L.o_chunks + round256((int64_t)sizeof(BnFoldChunk) * L.nchunks);
    return L;
}

int bn_fold_tables(const dfq_bn_fold_desc* d, int32_t n, std::vector<BnFoldJob>& jobs,
                   std::vector<BnFoldChunk>& chunks) {
    const int64_t span = bn_fold_span(d, n);
    {   // each weight folded once per call (sequential semantics otherwise)
        std::vector<const float*> ws(n);
        for (int32_t j = 0; j < n; ++j) ws[j] = d[j].w;
        std::sort(ws.begin(), ws.end());
        if (std::adjacent_find(ws.begin(), ws.end()) != ws.end()) return DFQ_ERR_INVALID;
    }
    jobs.resize(n);
    for (int32_t j = 0; j < n; ++j) {
        const dfq_bn_fold_desc& x = d[j];
        if (!x.w || !x.bias || !x.bn_w || !x.bn_b || !x.bn_mean || !x.bn_var || x.rows < 0 || x.row_len < 0)
            return DFQ_ERR_INVALID;
        if (x.row_len > kBnFoldMaxRowLen) return DFQ_ERR_UNSUPPORTED;
        jobs[j] = BnFoldJob{x.w, x.bias, x.bn_w, x.bn_b, x.bn_mean, x.bn_var, x.fake_w, x.fake_b, x.eps, x.flags, x.rows,
                            x.row_len, x.range_enc};
        const int64_t ne = x.rows * x.row_len;
        for (int64_t e = 0; e < ne; e += span) chunks.push_back(BnFoldChunk{j, 0, e, std::min<int64_t>(e + span, ne)});
    }
    return DFQ_OK;
}

// ---- absorption ------------------------------------------------------------
int absorb_tables(const dfq_absorb_desc* d, int32_t n, AbsTables& T, int32_t* failed) {
    // per bias vector, its updates in relation order
    std::vector<std::pair<float*, int64_t>> vlist;
    std::vector<std::vector<AbsOp>> vops;
    auto vec_of = [&](float* b, int64_t len) {
        for (size_t k = 0; k < vlist.size(); ++k)
            if (vlist[k].first == b) return (int32_t)k;
        vlist.push_back({b, len});
        vops.emplace_back();
        return (int32_t)vlist.size() - 1;
    };
    for (int32_t r = 0; r < n; ++r) {
        const dfq_absorb_desc& x = d[r];
        if (failed) *failed = r;
        if (!x.w2 || !x.b1 || !x.b2 || !x.bn_w || !x.bn_b || x.c1 <= 0 || x.o2 <= 0 || x.i2 <= 0 || x.khw2 <= 0)
            return DFQ_ERR_INVALID;
        const int64_t groups = x.c1 / x.i2;   // bias_absorption.py:159
        if (groups <= 0 || x.o2 % groups != 0 || x.c1 / groups != x.i2) return DFQ_ERR_SHAPE;   // as dfq_bias_absorb
        if (x.b1 == x.b2) return DFQ_ERR_SHAPE;
        for (int32_t q = 0; q < r; ++q)   // a BN shared by two relations: the per-relation call keeps its order
            if (d[q].bn_b == x.bn_b) return DFQ_ERR_UNSUPPORTED;
        AbsRel R{x.w2, x.bn_w, x.bn_b, x.o2, x.i2, x.khw2, x.o2 / groups, T.wc_floats};
        T.wc_floats += ceil_div(x.o2, (int64_t)64) * 64;
        T.rels.push_back(R);
        for (int64_t o = 0; o < x.o2; o += 4) T.rows.push_back(AbsRows{r, 0, o, std::min<int64_t>(o + 4, x.o2)});
        // reference order inside a relation: b1 -= c (and beta), then b2 += wc
        const int32_t v1 = vec_of(x.b1, x.c1);
        if (vlist[v1].second != x.c1) return DFQ_ERR_SHAPE;
        vops[v1].push_back(AbsOp{1, r});
        const int32_t v2 = vec_of(x.b2, x.o2);
        if (vlist[v2].second != x.o2) return DFQ_ERR_SHAPE;
        vops[v2].push_back(AbsOp{0, r});
    }
    if (failed) *failed = -1;
    for (size_t k = 0; k < vlist.size(); ++k) {
        T.vecs.push_back(AbsVec{vlist[k].first, vlist[k].second, (int32_t)T.ops.size(), (int32_t)vops[k].size()});
        T.ops.insert(T.ops.end(), vops[k].begin(), vops[k].end());
        for (int64_t e = 0; e < vlist[k].second; e += 1024)
            T.elems.push_back(AbsElems{(int32_t)k, 0, e, std::min<int64_t>(e + 1024, vlist[k].second)});
    }
    return DFQ_OK;
}

AbsLayout absorb_layout(const AbsTables& T) {
    AbsLayout L{};
    int64_t o = 0;
    auto add = [&](int64_t bytes) {
        const int64_t at = o;
        o += round256(std::max<int64_t>(bytes, 1));
        return at;
    };
    L.o_rels = add(sizeof(AbsRel) * T.rels.size());
    L.o_rows = add(sizeof(AbsRows) * T.rows.size());
    L.o_vecs = add(sizeof(AbsVec) * T.vecs.size());
    L.o_ops = add(sizeof(AbsOp) * T.ops.size());
    L.o_elems = add(sizeof(AbsElems) * T.elems.size());
    L.host = o;
    L.o_wc = add(sizeof(float) * T.wc_floats);
    L.total = o;
    return L;
}

// ---- bias correction -------------------------------------------------------
int bc_check_op(const dfq_bc_op& op) {
    switch (op.kind) {
        case DFQ_BC_OP_EXPECT:
            return (!op.a || !op.b || !op.out || op.n < 0) ? DFQ_ERR_INVALID : DFQ_OK;
        case DFQ_BC_OP_APPLY: {
            if (!op.a || !op.b || !op.out || op.n <= 0 || op.i2 <= 0 || op.f <= 0) return DFQ_ERR_INVALID;
            const int64_t bcols = bc_bcols(op.i2, op.f);   // torch broadcasting of [o, i2] + [f]
            // _apply_bias_correction: sizes never equal (2-D vs 1-D); numel must exceed o
            return (bcols == 0 || op.n * bcols <= op.n) ? DFQ_ERR_SHAPE : DFQ_OK;
        }
        case DFQ_BC_OP_PROPAGATE:
            if (!op.a || !op.out || op.n <= 0 || op.f <= 0 || op.flag < 1) return DFQ_ERR_INVALID;
            if (op.n % op.f != 0) return DFQ_ERR_SHAPE;   // .view(-1, F) fails
            return (op.f == 1 && op.flag > kBcScratch) ? DFQ_ERR_UNSUPPORTED : DFQ_OK;   // wave_full_sum's slots
        case DFQ_BC_OP_COPY:
            return (!op.a || !op.out || op.n < 0) ? DFQ_ERR_INVALID : DFQ_OK;
        default:
            return DFQ_ERR_INVALID;
    }
}

namespace {
struct Span {
    uintptr_t lo, hi;
};
Span span(const void* p, int64_t floats) {
    const uintptr_t lo = reinterpret_cast<uintptr_t>(p);
    return Span{lo, lo + 4 * (uintptr_t)std::max<int64_t>(floats, 0)};
}
bool overlap(const Span& x, const Span& y) { return x.lo < x.hi && y.lo < y.hi && x.lo < y.hi && y.lo < x.hi; }
}  // namespace

int32_t bc_layer_group(const dfq_bc_op* ops, int32_t n_ops, int32_t k, BcLayerJob& J) {
    const dfq_bc_op& e0 = ops[k];
    if (e0.kind != DFQ_BC_OP_EXPECT || (e0.flag & 2) || e0.n <= 0 || e0.n > kBcMaxExpect) return 0;
    int32_t m = k;
    J.nterms = 0;
    while (m < n_ops && ops[m].kind == DFQ_BC_OP_EXPECT && ops[m].out == e0.out && ops[m].n == e0.n &&
           (m == k || (ops[m].flag & 2))) {
        if (J.nterms == kBcMaxTerms) return 0;
        J.ew[J.nterms] = ops[m].a;
        J.eb[J.nterms] = ops[m].b;
        J.relu[J.nterms] = ops[m].flag & 1;
        ++J.nterms;
        ++m;
    }
    if (m >= n_ops) return 0;
    const dfq_bc_op& ap = ops[m];
    if (ap.kind != DFQ_BC_OP_APPLY || ap.b != e0.out || ap.f != e0.n) return 0;
    J.bcols = bc_bcols(ap.i2, ap.f);
    if (J.bcols == 0) return 0;   // the launches report the shape error
    J.f = e0.n;
    J.expect_out = e0.out;
    J.E = ap.a;
    J.o = ap.n;
    J.i2 = ap.i2;
    // the kernel stages a row / column in LDS and indexes bias_vec in 32 bits;
    // larger ones take the per-op launches
    if (J.bcols > kBcStage || J.o * J.bcols >= (int64_t(1) << 31)) return 0;
    J.bias = ap.out;
    J.vec = ap.out2;
    J.apply_blocks = std::min<int64_t>(ceil_div(J.o, (int64_t)4), 2048);
    int32_t used = m - k + 1;
    const dfq_bc_op* pr = (m + 1 < n_ops) ? &ops[m + 1] : nullptr;
    if (pr && pr->kind == DFQ_BC_OP_PROPAGATE && ap.out2 && pr->a == ap.out2 && pr->n == J.o * J.bcols &&
        pr->f > 0 && pr->n % pr->f == 0 && pr->flag >= 1 && pr->n / pr->f <= kBcStage) {
        J.fake_b = pr->out;
        J.F = pr->f;
        J.nrows = pr->n / pr->f;
        J.threads = pr->flag;
        ++used;
    }
    // hazards: what the group writes (slot, bias, bias_vec, fake_b) against what it
    // only reads (BN stats, E), and the writes among themselves.  bias and fake_b
    // are read too, each by the thread that then writes it: as writes they are
    // compared with every other write, which is all that their reads need.
    // (fixed-size span lists: this runs once per layer on the host, between launches)
    Span rd[2 * kBcMaxTerms + 1], wr[4];
    int nr = 0, nw = 0;
    for (int t = 0; t < J.nterms; ++t) {
        rd[nr++] = span(J.ew[t], J.f);
        rd[nr++] = span(J.eb[t], J.f);
    }
    rd[nr++] = span(J.E, J.o * (J.i2 > 1 ? J.i2 : 1));
    wr[nw++] = span(J.expect_out, J.f);
    wr[nw++] = span(J.bias, J.o);
    if (J.vec) wr[nw++] = span(J.vec, J.o * J.bcols);
    if (J.fake_b) wr[nw++] = span(J.fake_b, J.F);
    for (int a = 0; a < nw; ++a) {
        for (int b = 0; b < nr; ++b)
            if (overlap(wr[a], rd[b])) return 0;
        for (int b = a + 1; b < nw; ++b)
            if (overlap(wr[a], wr[b])) return 0;
    }
    return used;
}

int32_t bc_copy_run(const dfq_bc_op* ops, int32_t n_ops, int32_t k, CopyBatch& b, int& cnt, int64_t& most) {
    cnt = 0;
    most = 0;
    int32_t j = k;
    for (; j < n_ops && ops[j].kind == DFQ_BC_OP_COPY && cnt < kCopyBatch; ++j) {
        if (ops[j].n == 0) continue;
        b.src[cnt] = ops[j].a;
        b.dst[cnt] = ops[j].out;
        b.n[cnt] = ops[j].n;
        most = std::max(most, ops[j].n);
        ++cnt;
    }
    return j - k;
}

}  // namespace dfq

// The workspace sizes need no device: they live with the layouts.
extern "C" int64_t dfq_bn_fold_ws_bytes(const dfq_bn_fold_desc* d, int32_t n) {
    if (n < 0 || (n > 0 && !d)) return -1;
    for (int32_t j = 0; j < n; ++j)
        if (d[j].rows < 0 || d[j].row_len < 0) return -1;
    return dfq::bn_fold_layout(d, n).total;
}

extern "C" int64_t dfq_bias_absorb_ws_bytes(const dfq_absorb_desc* d, int32_t n) {
    if (n < 0 || (n > 0 && !d)) return -1;
    dfq::AbsTables T;
    if (dfq::absorb_tables(d, n, T, nullptr) != DFQ_OK) return -1;
    return dfq::absorb_layout(T).total;
}
