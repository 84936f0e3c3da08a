// api_tri.cpp — triangle counts and clustering coefficients of a bothE load (tri.hip): tgo_triangles,
// tgo_copy_triangles.  The forward lists, the degrees and the totals' words live with the graph
// (dev_alloc: released with it); per run: counts in internal order = sc.dist, coefficients = sc.vec[0],
// the block and wave kernels' row queues = sc.level and sc.q[0], row-order staging = sc.msg.
#include "ctx.hpp"

using namespace tgo;

// Defaults of TGO_TUNE_TRI_WAVE_ROW / _BLOCK_ROW (DESIGN.md 4.5 has the sweep).
constexpr int64_t kTriWaveRow = 8, kTriBlockRow = 8;

int tgo::tri_forward_lists(tgo_ctx* ctx) {
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    const int64_t n = g.n;
    if (g.tri_fadj) return TGO_OK;
    DevSpan span(st, "triangles.forward_lists");
    AllocScope lists(ctx);          // the lists reach the graph all built, or a failure releases them all
    unsigned long long* tot = nullptr;
    int64_t *deg = nullptr, *foff = nullptr;
    int32_t* fadj = nullptr;
    HIP_TRY(dev_alloc(ctx, tot, 16));
    HIP_TRY(dev_alloc(ctx, deg, n));
    HIP_TRY(dev_alloc(ctx, foff, n + 1));
    HIP_TRY(hipMemsetAsync(tot, 0, 16 * sizeof(unsigned long long), st));
    // count, scan, fill: |fwd(v)| in sc.qdeg (n + 2)
    HIP_TRY(k_tri_fwd_count(g.out, g.in, n, s.qdeg, deg, &tot[0], st));
    HIP_TRY(scan_exclusive_i64(s.cub_tmp, s.cub_bytes, s.qdeg, foff, n + 1, st));
    int64_t fnnz = 0;
    unsigned long long longest = 0;
    HIP_TRY(hipMemcpyAsync(&fnnz, foff + n, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&longest, tot, sizeof(longest), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (fnnz < 0 || fnnz > g.out.nnz + g.in.nnz) return fail(ctx, TGO_E_HIP, "forward lists: inconsistent entry count");
    HIP_TRY(dev_alloc(ctx, fadj, fnnz));
    HIP_TRY(k_tri_fwd_fill(g.out, g.in, n, foff, fadj, st));
    HIP_TRY(hipStreamSynchronize(st));
    lists.commit();
    g.tri_tot = tot;
    g.tri_deg = deg;
    g.tri_foff = foff;
    g.tri_fadj = fadj;
    g.tri_fnnz = fnnz;
    g.tri_max_fwd = static_cast<int64_t>(longest);
    return TGO_OK;
}

extern "C" {

int tgo_triangles(tgo_ctx* ctx, const tgo_tri_args* a, int64_t* tri_out, tgo_tri_info* info) {
    int rc = bothE_program_check(ctx, a, "tgo_tri_args", "triangles are counted", "triangles");
    if (rc) return rc;
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    const int64_t n = g.n;
    if ((rc = tri_forward_lists(ctx))) return rc;
    int64_t* const tri = s.dist;
    double* const lcc = s.vec[0];
    HIP_TRY(hipEventRecord(ctx->ev0, st));
    HIP_TRY(k_fill_i64(tri, 0, n, st));
    HIP_TRY(hipMemsetAsync(g.tri_tot + 1, 0, 15 * sizeof(unsigned long long), st));
    {
        DevSpan span(st, "triangles.count", {"forward_entries", g.tri_fnnz}, {"max_forward", g.tri_max_fwd});
        HIP_TRY(k_tri_count(g.tri_foff, g.tri_fadj, n, tuned(ctx->tune.i64(TGO_TUNE_TRI_WAVE_ROW), kTriWaveRow),
                            tuned(ctx->tune.i64(TGO_TUNE_TRI_BLOCK_ROW), kTriBlockRow), g.tri_max_fwd, tri, s.level,
                            s.q[0], &g.tri_tot[5], st));
    }
    {
        DevSpan span(st, "triangles.finish");
        HIP_TRY(k_tri_finish(tri, g.tri_deg, n, lcc, g.tri_tot + 1, st));
    }
    unsigned long long tot[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(tot, g.tri_tot + 1, sizeof tot, hipMemcpyDeviceToHost, st));
    if ((rc = program_end(ctx, 1))) return rc;
    ctx->tri_max = static_cast<int64_t>(tot[3]);
    if (info)
        *info = tgo_tri_info{static_cast<int64_t>(tot[0] / 3), static_cast<int64_t>(tot[1]),
                             static_cast<int64_t>(tot[2] / 2), g.tri_max_fwd};
    if (tri_out && (rc = rows_out(ctx, tri, tri_out))) return rc;
    publish_result(ctx, TGO_RESULT_TRIANGLES, ResultSource{tri, lcc});
    return TGO_OK;
}

int tgo_copy_triangles(tgo_ctx* ctx, int64_t* tri_out, int64_t* deg_out, double* lcc_out) {
    if (!ctx) return TGO_E_INVALID;
    int rc = copy_open(ctx, TGO_RESULT_TRIANGLES, "tgo_triangles");
    if (rc) return rc;
    // each copy-out finishes before the next reuses sc.msg
    if (tri_out && (rc = rows_out(ctx, ctx->sc.dist, tri_out))) return rc;
    if (deg_out && (rc = rows_out(ctx, ctx->g.tri_deg, deg_out))) return rc;
    if (lcc_out && (rc = rows_out(ctx, ctx->sc.vec[0], lcc_out))) return rc;
    return TGO_OK;
}

}  // extern "C"
