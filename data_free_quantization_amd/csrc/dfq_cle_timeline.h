// DFQ_CLE_TL (diagnostics library only; dfq_cle.hip includes this under
// DFQ_DIAGNOSTICS, the product library compiles an empty stand-in): the task
// timeline of one blocking CLE run.  begin(), before the first iteration, points the
// kernels' recording symbols (g_cle_tl / g_cle_tl2) at fresh buffers and uploads the
// per-run DFQ_CLE_TILES_FIRST switch; report(), after the drain, prints the
// DFQ_CLE_TL lines scripts/cle_trace_summary.py parses.  Both allocate, free and
// synchronise (dfq_cle_plan_launch refuses DFQ_CLE_TL runs); neither puts anything
// between two iterations on the loop stream.
#pragma once
struct CleTimeline {
    uint64_t* d_tl = nullptr;   // per rescale task timestamps (cle_apply_body)
    uint64_t* d_tl2 = nullptr;  // ... and per block of the last launch
    int64_t n_at = 0;
    static constexpr size_t n_tl2 = 4 * (size_t)(kCleTl2Fin + 1);
    int begin(const dfq_cle_plan* p, hipStream_t s) {
        const CleStructure& S = *p->S;
        n_at = S.astep.empty() ? 0 : S.astep.back();
        const char* e = ab_env("DFQ_CLE_TILES_FIRST");
        const int tf = e && *e ? (e[0] == '1' ? 1 : 0) : (kCleTilesFirst ? 1 : 0);
        DFQ_HIP_CHECK(hipMemcpyToSymbolAsync(HIP_SYMBOL(g_cle_tiles_first), &tf, sizeof(tf), 0, hipMemcpyHostToDevice, s));
        if (ab_env("DFQ_CLE_TL") && n_at > 0) {
            DFQ_HIP_CHECK(hipMalloc(&d_tl, sizeof(uint64_t) * 4 * n_at));
            DFQ_HIP_CHECK(hipMemsetAsync(d_tl, 0, sizeof(uint64_t) * 4 * n_at, s));
            DFQ_HIP_CHECK(hipMemcpyToSymbolAsync(HIP_SYMBOL(g_cle_tl), &d_tl, sizeof(d_tl), 0, hipMemcpyHostToDevice, s));
            DFQ_HIP_CHECK(hipMalloc(&d_tl2, sizeof(uint64_t) * n_tl2));
            DFQ_HIP_CHECK(hipMemsetAsync(d_tl2, 0, sizeof(uint64_t) * n_tl2, s));
            DFQ_HIP_CHECK(hipMemcpyToSymbolAsync(HIP_SYMBOL(g_cle_tl2), &d_tl2, sizeof(d_tl2), 0, hipMemcpyHostToDevice, s));
            const char* ek = ab_env("DFQ_CLE_TL_STEP");
            const int kk = ek && *ek ? atoi(ek) : -1;
            const int64_t a0v = (kk >= 0 && kk < S.steps) ? S.astep[kk] : -1;
            DFQ_HIP_CHECK(hipMemcpyToSymbolAsync(HIP_SYMBOL(g_cle_tl2_a0), &a0v, sizeof(a0v), 0, hipMemcpyHostToDevice, s));
            DFQ_HIP_CHECK(hipStreamSynchronize(s));
        }
        return DFQ_OK;
    }
    // per step: span, task durations, the slowest tasks (shapes and tasks: the plan's structure)
    int report(const dfq_cle_plan* p, hipStream_t s) {
        if (!d_tl) return DFQ_OK;
        const CleStructure& S = *p->S;
        std::vector<uint64_t> tl(4 * (size_t)n_at);
        DFQ_HIP_CHECK(cle_copy_back(tl.data(), d_tl, sizeof(uint64_t) * tl.size(), s));
        uint64_t* null_tl = nullptr;
        DFQ_HIP_CHECK(hipMemcpyToSymbolAsync(HIP_SYMBOL(g_cle_tl), &null_tl, sizeof(null_tl), 0, hipMemcpyHostToDevice, s));
        std::vector<uint64_t> tl2(n_tl2);
        DFQ_HIP_CHECK(cle_copy_back(tl2.data(), d_tl2, sizeof(uint64_t) * n_tl2, s));
        DFQ_HIP_CHECK(hipMemcpyToSymbolAsync(HIP_SYMBOL(g_cle_tl2), &null_tl, sizeof(null_tl), 0, hipMemcpyHostToDevice, s));
        DFQ_HIP_CHECK(hipStreamSynchronize(s));
        (void)hipFree(d_tl2);
        {   // the last launch: per role, when blocks started / ended (us after the first start)
            uint64_t t0 = ~0ull;
            for (int b = 0; b < kCleTl2Fin; ++b)
                if (tl2[4 * b]) t0 = std::min(t0, tl2[4 * b]);
            fprintf(stderr, "DFQ_CLE_TL last launch%s:", ab_env("DFQ_CLE_TL_STEP") ? " of DFQ_CLE_TL_STEP" : "");
            for (int role = 1; role <= 3; ++role) {
                std::vector<double> st, en, du;
                for (int b = 0; b < kCleTl2Fin; ++b) {
                    const uint64_t* r = &tl2[4 * b];
                    if (!r[0] || (int)r[2] != role) continue;
                    st.push_back((double)(r[0] - t0) * 0.01);
                    en.push_back((double)(r[1] - t0) * 0.01);
                    du.push_back((double)(r[1] - r[0]) * 0.01);
                }
                if (st.empty()) continue;
                std::sort(st.begin(), st.end());
                std::sort(en.begin(), en.end());
                double m = 0;
                for (double x : du) m += x;
                fprintf(stderr, " [%s: %zu blocks, start p50 %.2f max %.2f, end p50 %.2f max %.2f, dur mean %.2f]",
                        role == 1 ? "tiles" : role == 2 ? "ranges" : "tail tiles", st.size(), st[st.size() / 2], st.back(), en[en.size() / 2],
                        en.back(), m / du.size());
            }
            const uint64_t* f = &tl2[4 * kCleTl2Fin];
            if (f[0] && t0 != ~0ull)
                fprintf(stderr, " [stop rule: %.2f - %.2f, sums staged %.2f, means %.2f]", (double)(f[0] - t0) * 0.01,
                        (double)(f[1] - t0) * 0.01, f[2] ? (double)(f[2] - t0) * 0.01 : -1.0,
                        f[3] ? (double)(f[3] - t0) * 0.01 : -1.0);
            fprintf(stderr, "\n");
        }
        DFQ_HIP_CHECK(hipStreamSynchronize(s));
        (void)hipFree(d_tl);
        for (int32_t k = 0; k < S.steps; ++k) {
            const int64_t a0 = S.astep[k], a1 = S.astep[k + 1];
            uint64_t t_lo = ~0ull, t_hi = 0;
            double sum = 0;
            std::vector<std::pair<double, int64_t>> d;
            for (int64_t t = a0; t < a1; ++t) {
                const uint64_t* r = &tl[4 * t];
                if (!r[0]) continue;
                t_lo = std::min(t_lo, r[0]);
                t_hi = std::max(t_hi, r[1]);
                const double us = (double)(r[1] - r[0]) * 0.01;
                sum += us;
                d.push_back({us, t});
            }
            std::sort(d.rbegin(), d.rend());
            fprintf(stderr, "DFQ_CLE_TL step %d: %lld tasks, span %.2f us, task mean %.2f us, max %.2f us; slowest:",
                    k, (long long)(a1 - a0), t_hi > t_lo ? (double)(t_hi - t_lo) * 0.01 : 0.0,
                    d.empty() ? 0.0 : sum / d.size(), d.empty() ? 0.0 : d[0].first);
            for (size_t i = 0; i < d.size() && i < 6; ++i) {
                const uint64_t m = tl[4 * d[i].second + 3];
                const int rel = (int)((m >> 8) & 0xffff);
                const CleRel& q = S.R[rel];
                const CleTask& tk = S.at[d[i].second];
                fprintf(stderr, " [%.2f us kind %d rel %d n %lld c1 %lld o2 %lld i2 %lld khw2 %lld o2g %lld fuse %d cols %lld",
                        d[i].first, (int)(m & 255), rel, (long long)(m >> 24), (long long)q.c1, (long long)q.o2,
                        (long long)q.i2, (long long)q.khw2, (long long)q.o2g, q.fuse_next, (long long)(tk.c1 - tk.c0));
                const uint64_t sub = tl[4 * d[i].second + 2];
                if (sub >> 63)   // phase marks (us after the task's start)
                    fprintf(stderr, q.khw2 > 1 ? " scales %.2f inv_pos %.2f rows %.2f" : " landed %.2f rows %.2f barrier %.2f",
                            (double)(sub & 0xffff) * 0.01, (double)((sub >> 16) & 0xffff) * 0.01,
                            (double)((sub >> 32) & 0xffff) * 0.01);
                fprintf(stderr, "]");
            }
            // start-time histogram: when the tasks began relative to the first
            fprintf(stderr, "\nDFQ_CLE_TL step %d starts (us after first):", k);
            std::vector<double> st;
            for (int64_t t = a0; t < a1; ++t)
                if (tl[4 * t]) st.push_back((double)(tl[4 * t] - t_lo) * 0.01);
            std::sort(st.begin(), st.end());
            for (double q : {0.1, 0.5, 0.9, 0.99, 1.0})
                if (!st.empty()) fprintf(stderr, " p%.0f %.2f", q * 100, st[std::min(st.size() - 1, (size_t)(q * st.size()))]);
            // per task kind: count, mean / max duration, mean start
            fprintf(stderr, "\nDFQ_CLE_TL step %d kinds:", k);
            for (int kind = 0; kind < 8; ++kind) {
                int64_t cnt = 0;
                double sum = 0, mx = 0, s0 = 0;
                for (int64_t t = a0; t < a1; ++t) {
                    const uint64_t* r = &tl[4 * t];
                    if (!r[0] || (int)(r[3] & 255) != kind) continue;
                    const double us = (double)(r[1] - r[0]) * 0.01;
                    ++cnt;
                    sum += us;
                    mx = std::max(mx, us);
                    s0 += (double)(r[0] - t_lo) * 0.01;
                }
                if (cnt)
                    fprintf(stderr, " [kind %d: %lld tasks, mean %.2f max %.2f us, start mean %.2f]", kind,
                            (long long)cnt, sum / cnt, mx, s0 / cnt);
            }
            fprintf(stderr, "\n");
        }
        return DFQ_OK;
    }
};
