// api_pagerank.cpp — one-GPU PageRank and DegreeCounter (spmv.hip).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include "ctx.hpp"

using namespace tgo;

namespace tgo {

// PageRank diagnostics (engine.hpp PrTuning): TGO_PR_DIAG=lo:hi gathers only sources in
// [lo, hi) — a timing attribution tool, its ranks are wrong (scripts/pr_probe.py).
static PrTuning pr_tuning() {
    PrTuning t;
    if (const char* d = std::getenv("TGO_PR_DIAG")) {
        long lo = 0, hi = 0;
        if (std::sscanf(d, "%ld:%ld", &lo, &hi) == 2) { t.diag_lo = static_cast<int32_t>(lo); t.diag_hi = static_cast<int32_t>(hi); }
    }
    return t;
}

// After a program's updates: did any fixed-point pass see a message outside its exact range?
// Clears the flag.  (A synchronising read, once per program.)
int fx_take_bad(tgo_ctx* ctx, ColdBlocks& cb, bool* bad) {
    *bad = false;
    if (!cb.fx_bad) return TGO_OK;
    unsigned h = 0;
    HIP_TRY(hipMemcpyAsync(&h, cb.fx_bad, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (h) {
        HIP_TRY(hipMemsetAsync(cb.fx_bad, 0, sizeof(unsigned), ctx->stream));
        // a long row's accumulators may hold the discarded run's chunks: back to zero
        if (cb.fx_long_acc)
            HIP_TRY(hipMemsetAsync(cb.fx_long_acc, 0, 2 * std::max<int64_t>(cb.fx_nlong, 1) * sizeof(unsigned long long),
                                   ctx->stream));
        *bad = true;
    }
    return TGO_OK;
}

}  // namespace tgo

extern "C" {

int tgo_pagerank(tgo_ctx* ctx, const tgo_pr_args* a, double* pr_out) {
    if (!ctx) return TGO_E_INVALID;
    ctx->res_kind = -1;
    if (!a) return fail(ctx, TGO_E_INVALID, "null args");
    if (!ctx->loaded) return fail(ctx, TGO_E_STATE, "no graph loaded");
    if (ctx->g.scope == TGO_SCOPE_BOTH_E)
        return fail(ctx, TGO_E_INVALID, "PageRank uses the inE/outE scopes; load the graph with a single-direction scope");
    if (a->max_iterations < 0) return fail(ctx, TGO_E_INVALID, "max_iterations < 0");
    // PageRankVertexProgram has no combiner: two messages of one scope meeting at a vertex cut
    // hit FulgoraUtil's ThrowingCombiner (:80-91) and the job fails.  Iteration 1 receives the
    // inE messages over OUT entries, iterations >= 2 the outE messages over IN entries.
    if ((a->max_iterations >= 1 && ctx->pv_max_out >= 2) || (a->max_iterations >= 2 && ctx->pv_max_in >= 2))
        return fail(ctx, TGO_E_PROGRAM, "The VertexProgram needs to define a message combiner in order to "
                                        "preserve memory and handle partitioned vertices");
    (void)hipSetDevice(ctx->opts.device);
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    const int64_t n = g.n;
    hipStream_t st = ctx->stream;
    HIP_TRY(hipEventRecord(ctx->ev0, st));
    double* edge_count = s.vec[0];
    double* contrib = s.vec[1];
    double* contrib_next = s.vec[2];
    double* pr = reinterpret_cast<double*>(s.dist);    // int64-sized scratch reused for PR
    const double N = static_cast<double>(a->vertex_count);
    ctx->st.exact_reruns = 0;
    const PrTuning tune = pr_tuning();
    bool blocked = g.cold_in_ready && tune.diag_hi <= tune.diag_lo;
    if (a->max_iterations == 0) {
        HIP_TRY(k_fill_f64(pr, NAN, n, st));           // iteration 0 sets no PAGE_RANK property
    } else for (;;) {
        contrib = s.vec[1];
        contrib_next = s.vec[2];
        HIP_TRY(k_pr_init(g.out, edge_count, contrib, pr, 1.0 / N, n, st));
        const double base = (1.0 - a->alpha) / N;
        for (int it = 2; it <= a->max_iterations; ++it) {
            // the PAGE_RANK property is only read after the last superstep: write it there
            double* pr_it = it == a->max_iterations ? pr : nullptr;
            DevSpan span(st, "pagerank.update", {"iteration", it});
            if (blocked) {
                {
                    DevSpan ph(st, "pagerank.window_cold_phase", {"iteration", it});
                    HIP_TRY(k_pr_cold_phase(g.cold_in, contrib, st, it == 2));
                }
                DevSpan ph(st, "pagerank.hot_phase", {"iteration", it});
                HIP_TRY(k_pr_hot_phase(g.cold_in, contrib, edge_count, pr_it, contrib_next, s.partial, a->alpha, base,
                                       st, it == 2));
            } else
                HIP_TRY(k_pr_iter(g.in, g.rb_in, contrib, edge_count, pr_it, contrib_next, s.partial, a->alpha, base,
                                  n, tune, st));
            std::swap(contrib, contrib_next);
        }
        if (blocked && a->max_iterations >= 2 && g.cold_in.n_rows < n)   // entry-less rows: PR = (1-a)/N
            HIP_TRY(k_fill_f64(pr + g.cold_in.n_rows, base, n - g.cold_in.n_rows, st));
        // a message outside the fixed-point passes' exact range (an infinity from edgeCount 0,
        // NaN, or a magnitude the 128-bit form cannot hold): the whole program again on the
        // plain fp64 gather, whose sums are Java double sums
        bool bad = false;
        if (blocked && a->max_iterations >= 2)
            if (int rc = fx_take_bad(ctx, g.cold_in, &bad)) return rc;
        if (!bad) break;
        blocked = false;
        ++ctx->st.exact_reruns;
    }
    int rc = program_end(ctx, a->max_iterations);
    if (!rc && pr_out) rc = rows_out(ctx, pr, pr_out);
    if (rc) return rc;
    // PAGE_RANK / OUTGOING_EDGE_COUNT are set at iteration 1: after 0 iterations the result is empty
    publish_result(ctx, TGO_RESULT_PAGERANK, ResultSource{pr, edge_count}, a->max_iterations == 0);
    return TGO_OK;
}

int tgo_walkcount(tgo_ctx* ctx, int32_t k, int32_t* out) {
    if (!ctx) return TGO_E_INVALID;
    ctx->res_kind = -1;
    if (!ctx->loaded) return fail(ctx, TGO_E_STATE, "no graph loaded");
    if (k <= 0) return fail(ctx, TGO_E_INVALID, "DegreeCounter length must be > 0");   // OLAPTest.java:347
    if (ctx->g.scope != TGO_SCOPE_IN_E)
        return fail(ctx, TGO_E_INVALID, "DegreeCounter uses the inE scope; load the graph with TGO_SCOPE_IN_E");
    (void)hipSetDevice(ctx->opts.device);
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    const int64_t n = g.n;
    hipStream_t st = ctx->stream;
    HIP_TRY(hipEventRecord(ctx->ev0, st));
    int32_t* a = reinterpret_cast<int32_t*>(s.vec[0]);
    int32_t* b = reinterpret_cast<int32_t*>(s.vec[1]);
    HIP_TRY(k_fill_i32(a, 1, n, st));                  // iteration 0: every vertex sends 1
    for (int it = 1; it <= k; ++it) {
        DevSpan span(st, "degree_counter.superstep", {"iteration", it});
        HIP_TRY(k_walk_iter(g.out, g.rb_out, a, b, reinterpret_cast<int32_t*>(s.partial), n, st));
        std::swap(a, b);
    }
    if (int rc = program_end(ctx, k)) return rc;
    if (out) {      // 4-byte counts: their own copy-out, through sc.level
        HIP_TRY(k_unpermute_i32(a, g.perm, s.level, n, st));
        HIP_TRY(hipMemcpyAsync(out, s.level, n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    publish_result(ctx, TGO_RESULT_DEGREE, ResultSource{a, nullptr});
    return TGO_OK;
}

}  // extern "C"
