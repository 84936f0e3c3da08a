// program.hpp — the frame every program driver is written in (included by ctx.hpp, after the
// counter helpers): the checks that open a program, the epilogue that times it, the copy-out of a
// result in row order, and how the result is published to tgo_result_rows / tgo_copy_*.
#pragma once

namespace tgo {

// Opens a program that takes an args struct A with a scope: the last result is forgotten, a graph is
// loaded for that scope.  The program's own argument checks follow it.
template <class A>
int program_open(tgo_ctx* ctx, const A* a) {
    if (!ctx) return TGO_E_INVALID;
    ctx->res_kind = -1;
    if (!a) return fail(ctx, TGO_E_INVALID, "null args");
    return check_program(ctx, a->scope);
}

// Opens an analytic of a bothE load (A: its args struct, named `args`): `runs` is the "<what> <verb>" of
// its messages, `noun` what an asymmetric neighbour relation leaves undefined (null: it takes one).
template <class A>
int bothE_program_check(tgo_ctx* ctx, const A* a, const char* args, const std::string& runs, const char* noun) {
    if (int rc = program_open(ctx, a)) return rc;
    if (a->scope != TGO_SCOPE_BOTH_E)
        return fail(ctx, TGO_E_INVALID, runs + " over bothE; load the graph with TGO_SCOPE_BOTH_E");
    if (a->flags != 0) return fail(ctx, TGO_E_INVALID, std::string(args) + ".flags must be 0");
    if (ctx->g.partitioned) return fail(ctx, TGO_E_UNSUPPORTED, runs + " on a one-GPU load");
    if (noun && ctx->g.has_transpose)
        return fail(ctx, TGO_E_UNSUPPORTED,
                    "the loaded OUT and IN lists are not each other's transpose (tgo_load_csr with asymmetric rows): "
                    "the neighbour relation is asymmetric, " + std::string(noun) + " are not defined on it");
    (void)hipSetDevice(ctx->opts.device);
    return TGO_OK;
}

// A seed list (seeds, nseeds): nseeds >= 0 seeds, or -1 for every vertex.
inline int seed_list_check(tgo_ctx* ctx, const int64_t* seeds, int64_t nseeds) {
    if (nseeds < -1) return fail(ctx, TGO_E_INVALID, "nseeds must be >= 0, or -1 for every vertex");
    if (nseeds > 0 && !seeds) return fail(ctx, TGO_E_INVALID, "null seeds");
    return TGO_OK;
}

// ... as internal ids in `out`, in the order given (every vertex: in row order).  A Titan id that no
// executed vertex has is kept as -1 (out[i] is seed i's) or dropped.
inline int resolve_seeds(tgo_ctx* ctx, const int64_t* seeds, int64_t nseeds, int is_dense, bool keep_unknown,
                         std::vector<int64_t>& out) {
    if (int rc = seed_list_check(ctx, seeds, nseeds)) return rc;
    const int64_t count = nseeds < 0 ? ctx->g.n : nseeds;
    out.clear();
    out.reserve(static_cast<size_t>(count));
    for (int64_t i = 0; i < count; ++i) {
        int64_t v = -1;
        if (nseeds < 0) v = ctx->perm[i];
        else if (int rc = resolve_seed(ctx, seeds[i], is_dense, v)) return rc;
        if (v >= 0 || keep_unknown) out.push_back(v);
    }
    return TGO_OK;
}

// ev0 .. ev1 (both recorded, ev1 reached) into tgo_stats.last_kernel_ms.
inline int program_elapsed(tgo_ctx* ctx) {
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    ctx->st.last_kernel_ms = ms;
    return TGO_OK;
}

// The one-GPU epilogue: the program's work is queued; waits for it and fills in the stats.
inline int program_end(tgo_ctx* ctx, int32_t iterations) {
    HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
    HIP_TRY(hipEventSynchronize(ctx->ev1));
    trace_resolve(ctx->stream);
    if (int rc = program_elapsed(ctx)) return rc;
    ctx->st.iterations = iterations;
    return TGO_OK;
}

// An array of n 8-byte values in internal order to the host in row order, through sc.msg: queued
// (rows_out_async) or finished (rows_out; a second copy-out reuses sc.msg only after that).
inline int rows_out_async(tgo_ctx* ctx, const void* internal8, void* host_out) {
    HIP_TRY(k_unpermute_i64(static_cast<const int64_t*>(internal8), ctx->g.perm, ctx->sc.msg, ctx->g.n, ctx->stream));
    HIP_TRY(hipMemcpyAsync(host_out, ctx->sc.msg, ctx->g.n * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    return TGO_OK;
}
inline int rows_out(tgo_ctx* ctx, const void* internal8, void* host_out) {
    if (int rc = rows_out_async(ctx, internal8, host_out)) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return TGO_OK;
}

// {vertices with a distance in sc.dist, entries of their pull lists} (both lists for bothE).
inline int reach_stats(tgo_ctx* ctx, int scope, int64_t out[2]) {
    Scratch& s = ctx->sc;
    HIP_TRY(hipMemsetAsync(s.cnt, 0, sizeof(Counters), ctx->stream));
    HIP_TRY(k_reach_stats(pull_view(ctx->g, scope), s.dist, ctx->g.n, s.cnt->red, ctx->stream));
    if (int rc = read_counters(ctx)) return rc;
    out[0] = static_cast<int64_t>(s.hcnt->red[0]);
    out[1] = static_cast<int64_t>(s.hcnt->red[1]);
    return TGO_OK;
}

// The finished program's result, for tgo_result_rows and its tgo_copy_* (empty: no property set).
inline void publish_result(tgo_ctx* ctx, int kind, const ResultSource& src, bool empty = false) {
    ctx->res_kind = kind;
    ctx->res_empty = empty;
    ctx->res_src = src;
}

// A tgo_copy_* of `program`'s result: a graph is loaded and that program was the last one run.
inline int last_result_check(tgo_ctx* ctx, int kind, const char* program) {
    if (!ctx->loaded) return fail(ctx, TGO_E_STATE, "no graph loaded");
    if (ctx->res_kind != kind) return fail(ctx, TGO_E_STATE, std::string(program) + " is not the last program run on this ctx");
    return TGO_OK;
}

// Opens a tgo_copy_* (after its null-pointer checks): the check above, then the device and the queued work.
inline int copy_open(tgo_ctx* ctx, int kind, const char* program) {
    if (int rc = last_result_check(ctx, kind, program)) return rc;
    (void)hipSetDevice(ctx->opts.device);
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return TGO_OK;
}

// All-or-nothing device allocations: what dev_alloc / upload / adopt added since the scope opened is
// released when it closes without commit() (after a stream wait: queued kernels may still use it);
// commit() keeps it and counts it in tgo_stats.device_bytes.
struct AllocScope {
    tgo_ctx* ctx;
    size_t mark;
    int64_t bytes;
    bool committed = false;
    explicit AllocScope(tgo_ctx* c) : ctx(c), mark(c->allocs.size()), bytes(c->dev_bytes) {}
    void commit() {
        committed = true;
        ctx->st.device_bytes = ctx->dev_bytes;
    }
    ~AllocScope() {
        if (committed) return;
        if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
        for (size_t i = mark; i < ctx->allocs.size(); ++i) (void)hipFree(ctx->allocs[i]);
        ctx->allocs.resize(mark);
        ctx->dev_bytes = bytes;
    }
};

}  // namespace tgo
