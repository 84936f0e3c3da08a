// api_bc.cpp — Brandes' betweenness centrality of a bothE load (bc.hip): tgo_betweenness,
// tgo_copy_betweenness.  The simple adjacency of the undirected reading lives with the graph (dev_alloc:
// released with it).  Per run: the running sum bc in internal order = sc.vec[2] (it is the published
// result: nothing else writes it before the next program); per seed: the BFS levels = sc.level (run_bfs,
// which also uses sc.q[*], sc.qdeg, sc.qpre, the bitmaps and sc.dist while it runs), then the level
// histogram and the scatter's cursors = sc.qdeg, the level offsets = sc.qpre (depth + 2 <= n + 1 words;
// once the host has them, word L of sc.qdeg / sc.qpre counts the long rows that level L of the forward /
// backward sweep queues), the level-ordered list = sc.q[0], the long rows' queue = sc.q[1], sigma =
// sc.vec[0], delta = sc.vec[1]; row-order staging = sc.msg.  The level offsets reach the host through
// read_words; the overflow flag is Counters::err after a turn.
#include <climits>
#include "ctx.hpp"

using namespace tgo;

namespace {

// Default of TGO_TUNE_BC_WAVE_ROW.
constexpr int64_t kBcWaveRow = 64;

}  // namespace

int tgo::bc_simple_adjacency(tgo_ctx* ctx) {
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    const int64_t n = g.n;
    DevSpan span(st, "betweenness.lists", {"entries", g.out.nnz + g.in.nnz});
    AllocScope lists(ctx);          // both arrays or none, as the forward lists
    int64_t* soff = nullptr;
    int32_t* sadj = nullptr;
    HIP_TRY(dev_alloc(ctx, soff, n + 1));
    // count, scan, fill: the rows' lengths in sc.qdeg (n + 2), the longest in Counters::red[0]
    HIP_TRY(k_level_prep(s.cnt, nullptr, 0, nullptr, st));
    HIP_TRY(k_bc_adj_count(g.out, g.in, n, s.qdeg, &s.cnt->red[0], st));
    HIP_TRY(scan_exclusive_i64(s.cub_tmp, s.cub_bytes, s.qdeg, soff, n + 1, st));
    int64_t snnz = -1;
    unsigned long long longest = 0;
    HIP_TRY(hipMemcpyAsync(&snnz, soff + n, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&longest, &s.cnt->red[0], sizeof(longest), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    // (checked before the fill, which writes a row's share of sadj and no more)
    if (snnz < 0 || snnz > g.out.nnz + g.in.nnz) return fail(ctx, TGO_E_HIP, "simple adjacency: inconsistent entry count");
    HIP_TRY(dev_alloc(ctx, sadj, snnz));
    HIP_TRY(k_bc_adj_fill(g.out, g.in, n, soff, sadj, st));
    HIP_TRY(hipStreamSynchronize(st));
    lists.commit();
    g.bc_soff = soff;
    g.bc_sadj = sadj;
    g.bc_snnz = snnz;
    g.bc_smax = static_cast<int64_t>(longest);
    return TGO_OK;
}

namespace {

// The lists one run walks: predecessors for sigma, successors for delta.
struct BcRun {
    const int64_t *poff, *soff;
    const int32_t *padj, *sadj;
    bool dedup;
    int bfs_scope;
    bool long_rows;         // some row may reach wave_row: the sweeps launch the queued rows' kernel
    int64_t wave_row;
    double *sigma, *delta, *bc;
    int32_t rounds = 0;
};

// delta_seed added to r.bc; depth and reached: the deepest level and the vertices reached (seed included).
int bc_one_seed(tgo_ctx* ctx, BcRun& r, int64_t seed, int64_t shown, std::vector<int64_t>& loff, int32_t& depth,
                int64_t& reached) {
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    const int64_t n = g.n;
    int rc = TGO_OK;
    {
        DevSpan span(st, "betweenness.bfs", {"seed", shown});
        if ((rc = run_bfs(ctx, seed, INT_MAX, r.bfs_scope))) return rc;
    }
    depth = ctx->st.levels - 1;
    if (depth < 0 || depth >= n) return fail(ctx, TGO_E_HIP, "betweenness: inconsistent BFS depth");
    // the level-ordered list: histogram, scan, scatter
    const int64_t words = static_cast<int64_t>(depth) + 2;      // offsets 0..depth + 1
    int32_t* const order = s.q[0];
    HIP_TRY(k_level_prep(s.cnt, nullptr, 0, nullptr, st));
    HIP_TRY(hipMemsetAsync(s.qdeg, 0, words * sizeof(int64_t), st));
    HIP_TRY(k_bc_level_count(s.level, n, depth, s.qdeg, s.cnt, st));
    HIP_TRY(scan_exclusive_i64(s.cub_tmp, s.cub_bytes, s.qdeg, s.qpre, words, st));
    HIP_TRY(hipMemcpyAsync(s.qdeg, s.qpre, words * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    HIP_TRY(k_bc_level_scatter(s.level, n, depth, s.qdeg, order, s.cnt, st));
    loff.resize(static_cast<size_t>(words));
    if ((rc = read_words(ctx, s.qpre, words, loff.data()))) return rc;
    // Counters::err as a flag: the scatter's overflow, then sigma's
    if ((rc = turn(ctx))) return rc;
    bool sane = !s.hcnt->err && loff[0] == 0 && loff[1] == 1 && loff[static_cast<size_t>(depth) + 1] <= n;
    for (int64_t L = 0; sane && L <= depth; ++L) sane = loff[L + 1] > loff[L];
    if (!sane) return fail(ctx, TGO_E_HIP, "betweenness: inconsistent level counts");
    reached = loff[static_cast<size_t>(depth) + 1];
    // the host has the offsets: both arrays now count the levels' long rows
    HIP_TRY(hipMemsetAsync(s.qdeg, 0, words * sizeof(int64_t), st));
    HIP_TRY(hipMemsetAsync(s.qpre, 0, words * sizeof(int64_t), st));
    HIP_TRY(k_fill_f64(r.delta, 0.0, n, st));
    HIP_TRY(k_bc_seed(r.sigma, static_cast<int32_t>(seed), st));
    {
        DevSpan span(st, "betweenness.sigma", {"seed", shown}, {"depth", depth});
        for (int32_t L = 1; L <= depth; ++L) {
            HIP_TRY(k_bc_sigma(order + loff[L], loff[L + 1] - loff[L], r.poff, r.padj, r.dedup, s.level, L, r.sigma,
                               r.wave_row, s.q[1], s.qdeg + L, r.long_rows, s.cnt, st));
            r.rounds += r.long_rows ? 2 : 1;
        }
    }
    if ((rc = turn(ctx))) return rc;
    if (s.hcnt->err)
        return fail(ctx, TGO_E_PROGRAM, "betweenness: the number of shortest paths from seed " + std::to_string(shown) +
                                            " leaves the range of a double");
    {
        DevSpan span(st, "betweenness.delta", {"seed", shown}, {"depth", depth});
        for (int32_t L = depth - 1; L >= 1; --L) {
            HIP_TRY(k_bc_delta(order + loff[L], loff[L + 1] - loff[L], r.soff, r.sadj, r.dedup, s.level, L, r.sigma, r.delta,
                               r.bc, r.wave_row, s.q[1], s.qpre + L, r.long_rows, st));
            r.rounds += r.long_rows ? 2 : 1;
        }
    }
    return TGO_OK;
}

}  // namespace

extern "C" {

int tgo_betweenness(tgo_ctx* ctx, const tgo_bc_args* a, const int64_t* seeds, int64_t nseeds, double* bc_out,
                    tgo_bc_info* info) {
    int rc = bothE_program_check(ctx, a, "tgo_bc_args", "betweenness centrality runs", "shortest paths");
    if (rc) return rc;
    if (a->directed != 0 && a->directed != 1) return fail(ctx, TGO_E_INVALID, "tgo_bc_args.directed must be 0 or 1");
    // the seeds as internal ids, in the order given (an unknown Titan id: -1, nothing runs for it)
    std::vector<int64_t> internal;
    if ((rc = resolve_seeds(ctx, seeds, nseeds, a->seed_is_dense, true, internal))) return rc;
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    const int64_t n = g.n;
    const int64_t count = static_cast<int64_t>(internal.size());
    BcRun r{};
    if (a->directed) {
        r = BcRun{g.in.off, g.out.off, g.in.adj, g.out.adj, true, TGO_SCOPE_OUT_E};
    } else {
        if (n > 0 && !g.bc_sadj && (rc = bc_simple_adjacency(ctx))) return rc;
        r = BcRun{g.bc_soff, g.bc_soff, g.bc_sadj, g.bc_sadj, false, TGO_SCOPE_BOTH_E};
    }
    r.wave_row = tuned(ctx->tune.i64(TGO_TUNE_BC_WAVE_ROW), kBcWaveRow);
    r.long_rows = a->directed ? true : g.bc_smax >= r.wave_row;     // (the raw rows' lengths are not kept)
    r.sigma = s.vec[0];
    r.delta = s.vec[1];
    r.bc = s.vec[2];
    HIP_TRY(hipEventRecord(ctx->ev0, st));
    tgo_bc_info out{0, 0, 0, 0};
    if (n > 0) HIP_TRY(k_fill_f64(r.bc, 0.0, n, st));
    std::vector<int64_t> loff;
    for (int64_t i = 0; i < count; ++i) {
        if (internal[i] < 0) continue;
        int32_t depth = 0;
        int64_t reached = 0;
        const int64_t shown = nseeds < 0 ? ctx->titan_id[i] : seeds[i];
        if ((rc = bc_one_seed(ctx, r, internal[i], shown, loff, depth, reached))) return rc;
        ++out.sources;
        out.reached_pairs += reached - 1;
        out.max_depth = std::max(out.max_depth, depth);
    }
    out.rounds = r.rounds;
    if ((rc = program_end(ctx, static_cast<int32_t>(std::min<int64_t>(out.sources, INT32_MAX))))) return rc;
    ctx->st.levels = out.max_depth;
    if (info) *info = out;
    if (bc_out && n > 0 && (rc = rows_out(ctx, r.bc, bc_out))) return rc;
    publish_result(ctx, TGO_RESULT_BETWEENNESS, ResultSource{r.bc, nullptr});
    return TGO_OK;
}

int tgo_copy_betweenness(tgo_ctx* ctx, double* bc_out) {
    if (!ctx || !bc_out) return TGO_E_INVALID;
    if (int rc = copy_open(ctx, TGO_RESULT_BETWEENNESS, "tgo_betweenness")) return rc;
    return rows_out(ctx, ctx->sc.vec[2], bc_out);
}

}  // extern "C"
