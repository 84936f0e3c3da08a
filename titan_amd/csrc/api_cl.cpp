// api_cl.cpp — closeness and harmonic centrality of any one-GPU load (cl.hip) out of the multi-source
// sweep (run_ms_sweep, api_msbfs.cpp): tgo_closeness, tgo_copy_closeness.  Device arrays, internal order,
// kept across the batches of one run and published as its result: sc.cl_far / cl_reach (u64), sc.cl_ecc
// (int32), sc.cl_harm, sc.cl_close (fp64; the result source of tgo_result_rows); the sweep's own state is
// sc.ms_*; row-order staging = sc.msg; the two reductions of the finish = Counters::red[0..1] after a turn.
#include <climits>
#include "ctx.hpp"

using namespace tgo;

namespace {

int cl_alloc(tgo_ctx* ctx) {
    Scratch& s = ctx->sc;
    if (s.cl_close) return TGO_OK;
    const int64_t n = ctx->g.n;
    AllocScope all(ctx);            // the five arrays or none
    HIP_TRY(dev_alloc(ctx, s.cl_far, n));
    HIP_TRY(dev_alloc(ctx, s.cl_reach, n));
    HIP_TRY(dev_alloc(ctx, s.cl_ecc, n));
    HIP_TRY(dev_alloc(ctx, s.cl_harm, n));
    double* close = nullptr;
    HIP_TRY(dev_alloc(ctx, close, n));
    all.commit();
    s.cl_close = close;
    return TGO_OK;
}

// The whole run's device time: the sweeps record ctx->ev0 / ev1 for themselves.
struct ClTimer {
    hipEvent_t t0 = nullptr, t1 = nullptr;
    ~ClTimer() {
        if (t0) (void)hipEventDestroy(t0);
        if (t1) (void)hipEventDestroy(t1);
    }
};

}  // namespace

extern "C" {

int tgo_closeness(tgo_ctx* ctx, const tgo_cl_args* a, const int64_t* seeds, int64_t nseeds, double* closeness_out,
                  double* harmonic_out, tgo_cl_info* info) {
    int rc = program_open(ctx, a);
    if (rc) return rc;
    if (a->flags != 0) return fail(ctx, TGO_E_INVALID, "tgo_cl_args.flags must be 0");
    if (a->max_depth < 0) return fail(ctx, TGO_E_INVALID, "max_depth < 0");
    // (ahead of resolve_seeds, which repeats it: a malformed seed list is reported before the load's kind)
    if ((rc = seed_list_check(ctx, seeds, nseeds))) return rc;
    if (ctx->g.partitioned) return fail(ctx, TGO_E_UNSUPPORTED, "closeness centrality runs on a one-GPU load");
    (void)hipSetDevice(ctx->opts.device);
    if ((rc = ms_alloc(ctx))) return rc;
    if ((rc = cl_alloc(ctx))) return rc;
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    const int64_t n = g.n;
    // the seeds that are executed vertices as internal ids, in the order given
    std::vector<int64_t> internal;
    if ((rc = resolve_seeds(ctx, seeds, nseeds, a->seed_is_dense, false, internal))) return rc;
    const int64_t sources = static_cast<int64_t>(internal.size());
    const int64_t batches = (sources + TGO_MAX_SOURCES - 1) / TGO_MAX_SOURCES;
    if (batches > INT32_MAX) return fail(ctx, TGO_E_INVALID, "too many seeds");
    ClTimer tm;
    HIP_TRY(hipEventCreate(&tm.t0));
    HIP_TRY(hipEventCreate(&tm.t1));
    HIP_TRY(hipEventRecord(tm.t0, st));
    if (n > 0) {
        HIP_TRY(hipMemsetAsync(s.cl_far, 0, n * sizeof(unsigned long long), st));
        HIP_TRY(hipMemsetAsync(s.cl_reach, 0, n * sizeof(unsigned long long), st));
        HIP_TRY(hipMemsetAsync(s.cl_ecc, 0, n * sizeof(int32_t), st));
        HIP_TRY(hipMemsetAsync(s.cl_harm, 0, n * sizeof(double), st));      // +0.0
        HIP_TRY(hipMemsetAsync(s.cl_close, 0, n * sizeof(double), st));
    }
    for (int64_t b = 0; b < batches; ++b) {
        const int32_t m = static_cast<int32_t>(std::min<int64_t>(TGO_MAX_SOURCES, sources - b * TGO_MAX_SOURCES));
        DevSpan batch(st, "closeness.batch", {"batch", b}, {"sources", m});
        {
            DevSpan span(st, "closeness.sweep", {"batch", b});
            if ((rc = run_ms_sweep(ctx, internal.data() + b * TGO_MAX_SOURCES, m, a->max_depth, a->scope, 0))) return rc;
        }
        DevSpan span(st, "closeness.fold", {"batch", b}, {"planes", s.ms_nplanes});
        HIP_TRY(k_cl_fold(s.ms_vis, ms_planes(ctx), s.ms_nplanes, n, s.cl_far, s.cl_reach, s.cl_ecc, s.cl_harm, st));
    }
    tgo_cl_info out{sources, 0, static_cast<int32_t>(batches), 0};
    {
        DevSpan span(st, "closeness.finish");
        HIP_TRY(k_level_prep(s.cnt, nullptr, 0, nullptr, st));
        HIP_TRY(k_cl_finish(s.cl_far, s.cl_reach, s.cl_ecc, n, s.cl_close, &s.cnt->red[0], &s.cnt->red[1], st));
        if ((rc = turn(ctx))) return rc;
        out.reached_pairs = static_cast<int64_t>(s.hcnt->red[0]);
        out.max_depth = static_cast<int32_t>(s.hcnt->red[1]);
    }
    HIP_TRY(hipEventRecord(tm.t1, st));
    HIP_TRY(hipEventSynchronize(tm.t1));
    trace_resolve(st);
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, tm.t0, tm.t1));
    ctx->st.last_kernel_ms = ms;
    ctx->st.iterations = out.batches;
    ctx->st.levels = out.max_depth;
    if (info) *info = out;
    if (closeness_out && n > 0 && (rc = rows_out(ctx, s.cl_close, closeness_out))) return rc;
    if (harmonic_out && n > 0 && (rc = rows_out(ctx, s.cl_harm, harmonic_out))) return rc;
    publish_result(ctx, TGO_RESULT_CLOSENESS, ResultSource{s.cl_close, s.cl_harm});
    return TGO_OK;
}

int tgo_copy_closeness(tgo_ctx* ctx, int64_t* far_out, int64_t* reach_out, int64_t* ecc_out, double* closeness_out,
                       double* harmonic_out) {
    if (!ctx) return TGO_E_INVALID;
    int rc = copy_open(ctx, TGO_RESULT_CLOSENESS, "tgo_closeness");
    if (rc) return rc;
    Scratch& s = ctx->sc;
    const int64_t n = ctx->g.n;
    if (n <= 0) return TGO_OK;
    if (far_out && (rc = rows_out(ctx, s.cl_far, far_out))) return rc;
    if (reach_out && (rc = rows_out(ctx, s.cl_reach, reach_out))) return rc;
    if (ecc_out) {
        HIP_TRY(k_cl_ecc_rows(s.cl_ecc, ctx->g.perm, s.msg, n, ctx->stream));
        HIP_TRY(hipMemcpyAsync(ecc_out, s.msg, n * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    if (closeness_out && (rc = rows_out(ctx, s.cl_close, closeness_out))) return rc;
    if (harmonic_out && (rc = rows_out(ctx, s.cl_harm, harmonic_out))) return rc;
    return TGO_OK;
}

}  // extern "C"
