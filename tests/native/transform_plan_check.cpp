// The graph transforms' planners on their own: dfq_transform_plan.cpp linked with
// this main and nothing else, so they run under AddressSanitizer / UBSan on a
// machine without a GPU (tests/test_transform_plan_host.py builds and runs it).
// (Addresses are stand-ins: the planners never dereference them.  0 is NULL.)
// Input: a text file of commands, one answer block each.
//   fold_row <row_len>
//       walks fold_row over every chunk-local index in [0, 2^20 + row_len) of a chunk
//       that starts in row 3 and compares with integer / and %:
//       fold_row <row_len> checked <n> bad <n> minus <n> plus <n> qsum <s> remsum <s>
//       (minus / plus: the indices whose fp32 quotient took the -1 / +1 correction)
//   bn <n>, then n lines `rows row_len w null_member`
//       bn rc <code> span <e> nchunks <n> o_chunks <B> total <B> ws <B> job_bytes <B> chunk_bytes <B>
//       chunk <job> <e0> <e1>                          (rc 0 only, in table order)
//   absorb <n>, then n lines `w2 b1 b2 bn_w bn_b c1 o2 i2 khw2`
//       absorb rc <code> failed <r> ws <B> wc_floats <n> o_rels .. o_rows .. o_vecs .. o_ops .. o_elems ..
//              host .. o_wc .. total .. rel_bytes .. rows_bytes .. vec_bytes .. op_bytes .. elems_bytes ..
//       rel <o2> <i2> <khw2> <o2g> <wc> / rows <r> <o0> <o1> / vec <b> <n> <op0> <nops> /
//       op <kind> <r> / elems <v> <e0> <e1>           (rc 0 only, in table order)
//   bc <n_ops> <k>, then n_ops lines `kind flag a b out out2 n i2 f`
//       the chain's validation (the first op bc_check_op refuses), then -- when every op
//       is valid -- bc_layer_group and bc_copy_run at ops[k]:
//       bc bad <k> rc <code> used <n> nterms .. threads .. expect_out .. f .. E .. o .. i2 .. bcols ..
//          bias .. vec .. fake_b .. F .. nrows .. apply_blocks .. copy_used <n> copy_cnt <n> copy_most <n>
//       term <ew> <eb> <relu>                          (used > 0 only)
//       copy <src> <dst> <n>                           (one per batched copy)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dfq_transform_plan.h"

template <typename T>
static T* ptr(long long a) {
    return reinterpret_cast<T*>((uintptr_t)a);
}
static long long addr(const void* p) { return (long long)reinterpret_cast<uintptr_t>(p); }

static int do_fold_row(FILE* f) {
    long long row_len;
    if (fscanf(f, "%lld", &row_len) != 1) return 2;
    const int64_t r0 = 3, base = r0 * row_len, n = dfq::kBnFoldMaxSpan + row_len;
    const float inv = 1.0f / (float)row_len;
    long long bad = 0, minus = 0, plus = 0, qsum = 0, remsum = 0;
    for (int64_t li = 0; li < n; ++li) {
        int rem;
        const int64_t row = dfq::fold_row(row_len, r0, base, inv, base + li, &rem);
        bad += row != r0 + li / row_len || rem != li % row_len;
        const int q = (int)((float)(int)li * inv);   // the quotient before its correction
        minus += (int64_t)q > li / row_len;
        plus += (int64_t)q < li / row_len;
        qsum += row - r0;
        remsum += rem;
    }
    printf("fold_row %lld checked %lld bad %lld minus %lld plus %lld qsum %lld remsum %lld\n", row_len, (long long)n,
           bad, minus, plus, qsum, remsum);
    return 0;
}

static int do_bn(FILE* f) {
    long long n;
    if (fscanf(f, "%lld", &n) != 1) return 2;
    std::vector<dfq_bn_fold_desc> d((size_t)n);
    for (dfq_bn_fold_desc& x : d) {
        long long rows, row_len, w, null_member;
        if (fscanf(f, "%lld %lld %lld %lld", &rows, &row_len, &w, &null_member) != 4) return 2;
        x = dfq_bn_fold_desc{};
        x.w = ptr<float>(w);
        x.bias = ptr<float>(0x100);
        x.bn_w = ptr<float>(0x200);
        x.bn_b = ptr<float>(0x300);
        x.bn_mean = ptr<float>(0x400);
        x.bn_var = ptr<float>(null_member ? 0 : 0x500);
        x.rows = rows;
        x.row_len = row_len;
    }
    std::vector<dfq::BnFoldJob> jobs;
    std::vector<dfq::BnFoldChunk> chunks;
    const int rc = dfq::bn_fold_tables(d.data(), (int32_t)n, jobs, chunks);
    const dfq::BnFoldLayout L = dfq::bn_fold_layout(d.data(), (int32_t)n);
    printf("bn rc %d span %lld nchunks %lld o_chunks %lld total %lld ws %lld job_bytes %zu chunk_bytes %zu\n", rc,
           (long long)L.span, (long long)L.nchunks, (long long)L.o_chunks, (long long)L.total,
           (long long)dfq_bn_fold_ws_bytes(d.data(), (int32_t)n), sizeof(dfq::BnFoldJob), sizeof(dfq::BnFoldChunk));
    if (rc != DFQ_OK) return 0;
    if ((long long)chunks.size() != L.nchunks || (long long)jobs.size() != n)
        return fprintf(stderr, "bn: table sizes differ from the layout\n"), 1;
    for (const dfq::BnFoldChunk& c : chunks) printf("chunk %d %lld %lld\n", c.job, (long long)c.e0, (long long)c.e1);
    return 0;
}

static int do_absorb(FILE* f) {
    long long n;
    if (fscanf(f, "%lld", &n) != 1) return 2;
    std::vector<dfq_absorb_desc> d((size_t)n);
    for (dfq_absorb_desc& x : d) {
        long long w2, b1, b2, bn_w, bn_b, c1, o2, i2, khw2;
        if (fscanf(f, "%lld %lld %lld %lld %lld %lld %lld %lld %lld", &w2, &b1, &b2, &bn_w, &bn_b, &c1, &o2, &i2,
                   &khw2) != 9)
            return 2;
        x = dfq_absorb_desc{ptr<float>(w2), ptr<float>(b1), ptr<float>(b2), ptr<float>(bn_w), ptr<float>(bn_b),
                            c1, o2, i2, khw2};
    }
    dfq::AbsTables T;
    int32_t failed = -7;
    const int rc = dfq::absorb_tables(d.data(), (int32_t)n, T, &failed);
    const dfq::AbsLayout L = rc == DFQ_OK ? dfq::absorb_layout(T) : dfq::AbsLayout{};
    printf("absorb rc %d failed %d ws %lld wc_floats %lld o_rels %lld o_rows %lld o_vecs %lld o_ops %lld o_elems %lld "
           "host %lld o_wc %lld total %lld rel_bytes %zu rows_bytes %zu vec_bytes %zu op_bytes %zu elems_bytes %zu\n",
           rc, failed, (long long)dfq_bias_absorb_ws_bytes(d.data(), (int32_t)n), (long long)T.wc_floats,
           (long long)L.o_rels, (long long)L.o_rows, (long long)L.o_vecs, (long long)L.o_ops, (long long)L.o_elems,
           (long long)L.host, (long long)L.o_wc, (long long)L.total, sizeof(dfq::AbsRel), sizeof(dfq::AbsRows),
           sizeof(dfq::AbsVec), sizeof(dfq::AbsOp), sizeof(dfq::AbsElems));
    if (rc != DFQ_OK) return 0;
    for (const dfq::AbsRel& r : T.rels)
        printf("rel %lld %lld %lld %lld %lld\n", (long long)r.o2, (long long)r.i2, (long long)r.khw2, (long long)r.o2g,
               (long long)r.wc);
    for (const dfq::AbsRows& r : T.rows) printf("rows %d %lld %lld\n", r.r, (long long)r.o0, (long long)r.o1);
    for (const dfq::AbsVec& v : T.vecs) printf("vec %lld %lld %d %d\n", addr(v.b), (long long)v.n, v.op0, v.nops);
    for (const dfq::AbsOp& o : T.ops) printf("op %d %d\n", o.kind, o.r);
    for (const dfq::AbsElems& e : T.elems) printf("elems %d %lld %lld\n", e.v, (long long)e.e0, (long long)e.e1);
    return 0;
}

static int do_bc(FILE* f) {
    long long n, k;
    if (fscanf(f, "%lld %lld", &n, &k) != 2 || k < 0 || k >= n) return 2;
    std::vector<dfq_bc_op> ops((size_t)n);
    for (dfq_bc_op& op : ops) {
        long long kind, flag, a, b, out, out2, cnt, i2, ff;
        if (fscanf(f, "%lld %lld %lld %lld %lld %lld %lld %lld %lld", &kind, &flag, &a, &b, &out, &out2, &cnt, &i2,
                   &ff) != 9)
            return 2;
        op = dfq_bc_op{(int32_t)kind, (int32_t)flag, ptr<float>(a), ptr<float>(b), ptr<float>(out), ptr<float>(out2),
                       cnt, i2, ff};
    }
    int bad = -1, rc = DFQ_OK;
    for (int32_t j = 0; j < (int32_t)n && rc == DFQ_OK; ++j) {
        rc = dfq::bc_check_op(ops[j]);
        if (rc != DFQ_OK) bad = j;
    }
    dfq::BcLayerJob J{};
    dfq::CopyBatch cb{};
    int32_t used = 0, copy_used = 0;
    int cnt = 0;
    int64_t most = 0;
    if (rc == DFQ_OK) {
        used = dfq::bc_layer_group(ops.data(), (int32_t)n, (int32_t)k, J);
        if (ops[k].kind == DFQ_BC_OP_COPY) copy_used = dfq::bc_copy_run(ops.data(), (int32_t)n, (int32_t)k, cb, cnt, most);
    }
    if (used == 0) J = dfq::BcLayerJob{};   // (a refused group leaves the job half filled)
    printf("bc bad %d rc %d used %d nterms %d threads %d expect_out %lld f %lld E %lld o %lld i2 %lld bcols %lld "
           "bias %lld vec %lld fake_b %lld F %lld nrows %lld apply_blocks %lld copy_used %d copy_cnt %d copy_most %lld\n",
           bad, rc, used, J.nterms, J.threads, addr(J.expect_out), (long long)J.f, addr(J.E), (long long)J.o,
           (long long)J.i2, (long long)J.bcols, addr(J.bias), addr(J.vec), addr(J.fake_b), (long long)J.F,
           (long long)J.nrows, (long long)J.apply_blocks, copy_used, cnt, (long long)most);
    for (int t = 0; t < J.nterms; ++t) printf("term %lld %lld %d\n", addr(J.ew[t]), addr(J.eb[t]), J.relu[t]);
    for (int c = 0; c < cnt; ++c) printf("copy %lld %lld %lld\n", addr(cb.src[c]), addr(cb.dst[c]), (long long)cb.n[c]);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) return fprintf(stderr, "usage: %s commands.txt\n", argv[0]), 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return perror(argv[1]), 2;
    char cmd[32];
    for (int ci = 0; fscanf(f, "%31s", cmd) == 1; ++ci) {
        const int rc = !strcmp(cmd, "fold_row") ? do_fold_row(f)
                       : !strcmp(cmd, "bn")     ? do_bn(f)
                       : !strcmp(cmd, "absorb") ? do_absorb(f)
                       : !strcmp(cmd, "bc")     ? do_bc(f)
                                                : 2;
        if (rc == 2) fprintf(stderr, "command %d (%s): malformed\n", ci, cmd);
        if (rc) return rc;
    }
    fclose(f);
    return 0;
}
