// api_kcore.cpp — k-core decomposition of a bothE load (core.hip): tgo_kcore, tgo_copy_cores.  The backward
// lists and the totals' words live with the graph (dev_alloc: released with it), beside the forward lists
// and degrees they share with tgo_triangles.  Level control: Counters through turn_checked.
#include <climits>
#include "ctx.hpp"

using namespace tgo;

namespace {

// Defaults of TGO_TUNE_CORE_WAVE_ROW / _TAIL / _LDS_QUEUE: DESIGN.md 4.6 has the sweep they come from.
constexpr int64_t kCoreWaveRow = 64, kCoreTail = 1024, kCoreLdsQueue = 256;

// The Scratch arrays one run uses, under the types it uses them as (row-order staging: sc.msg).
struct CoreArrays {
    int32_t* deg;               // sc.level: n x int32; the working degrees, the core numbers at the end
    int64_t* core;              // sc.dist: n x int64; the cores in internal order, the published result
    int32_t* alive_list[2];     // sc.q[0] / sc.q[1]: n + 1 x int32 each
    int32_t* queue[2];          // sc.vec[0] / sc.vec[1]: n x 8 bytes each, of which n x int32 hold a level queue
};

CoreArrays core_arrays(Scratch& s) {
    return CoreArrays{s.level, s.dist, {s.q[0], s.q[1]},
                      {reinterpret_cast<int32_t*>(s.vec[0]), reinterpret_cast<int32_t*>(s.vec[1])}};
}

int core_backward_lists(tgo_ctx* ctx) {
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    const int64_t n = g.n;
    if (g.core_badj) return TGO_OK;
    DevSpan span(st, "kcore.lists", {"forward_entries", g.tri_fnnz});
    AllocScope lists(ctx);          // all three arrays or none, as the forward lists
    unsigned long long* tot = nullptr;
    int64_t* boff = nullptr;
    int32_t* badj = nullptr;
    HIP_TRY(dev_alloc(ctx, tot, 2));
    HIP_TRY(dev_alloc(ctx, boff, n + 1));
    HIP_TRY(dev_alloc(ctx, badj, g.tri_fnnz));
    // count, scan, fill: |bwd(v)| in sc.qdeg (n + 2), the fill's cursors in sc.qpre (n + 2)
    HIP_TRY(hipMemsetAsync(s.qdeg, 0, (n + 1) * sizeof(int64_t), st));
    HIP_TRY(k_core_bwd_count(g.tri_fadj, g.tri_fnnz, s.qdeg, st));
    HIP_TRY(scan_exclusive_i64(s.cub_tmp, s.cub_bytes, s.qdeg, boff, n + 1, st));
    HIP_TRY(hipMemcpyAsync(s.qpre, boff, (n + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    int64_t bnnz = -1;
    HIP_TRY(hipMemcpyAsync(&bnnz, boff + n, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    // (checked before the fill: its cursors stay inside badj only when the counts add up)
    if (bnnz != g.tri_fnnz) return fail(ctx, TGO_E_HIP, "backward lists: inconsistent entry count");
    HIP_TRY(k_core_bwd_fill(g.tri_foff, g.tri_fadj, n, s.qpre, badj, st));
    HIP_TRY(hipStreamSynchronize(st));
    lists.commit();
    g.core_tot = tot;
    g.core_boff = boff;
    g.core_badj = badj;
    return TGO_OK;
}

constexpr char kPeel[] = "k-core peel";     // turn_checked's name of the level loop

// The peel: A.deg (a copy of d(v)) ends as the core numbers.  Out: levels, peel launches, the largest
// core number and the vertices peeled at it.
int core_peel_levels(tgo_ctx* ctx, const CoreArrays& A, int32_t& levels, int32_t& rounds, int64_t& top,
                     int64_t& innermost) {
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    const int64_t n = g.n;
    const CoreView lists{g.tri_foff, g.tri_fadj, g.core_boff, g.core_badj};
    const int64_t wave_row = tuned(ctx->tune.i64(TGO_TUNE_CORE_WAVE_ROW), kCoreWaveRow);
    const int64_t tail = std::min<int64_t>(tuned(ctx->tune.i64(TGO_TUNE_CORE_TAIL), kCoreTail), kCoreQueue);
    const int64_t lds_cap = tuned(ctx->tune.i64(TGO_TUNE_CORE_LDS_QUEUE), kCoreLdsQueue);
    int32_t* const deg = A.deg;
    int rc = TGO_OK;
    HIP_TRY(k_core_deg_init(g.tri_deg, n, deg, st));
    HIP_TRY(k_level_prep(s.cnt, nullptr, 0, nullptr, st));
    // the smallest degree: a scan that queues nothing
    HIP_TRY(k_core_scan(nullptr, n, deg, -1, nullptr, nullptr, s.cnt, st));
    if ((rc = turn_checked(ctx, kPeel))) return rc;
    int64_t next_k = level_min(s.hcnt->red[0]);
    int64_t alive = n, k = -1;
    AliveList al(n, A.alive_list[0], A.alive_list[1]);
    while (alive > 0) {
        if (next_k == INT64_MAX) return fail(ctx, TGO_E_HIP, "k-core peel: alive vertices without a degree");
        if (tail > 0 && alive <= tail) {
            if (al.len > 2 * alive) {   // the one workgroup scans the list once per level: compact it first
                HIP_TRY(k_core_scan(al.list, al.len, deg, static_cast<int32_t>(k), nullptr, al.keep_buffer(), s.cnt, st));
                if ((rc = turn_checked(ctx, kPeel))) return rc;
                al.adopt(static_cast<int64_t>(s.hcnt->mf));
                if (al.len != alive) return fail(ctx, TGO_E_HIP, "k-core peel: inconsistent alive count");
            }
            HIP_TRY(k_core_tail(al.list, al.len, lists, deg, static_cast<int32_t>(k), wave_row, s.cnt, st));
            if ((rc = turn_checked(ctx, kPeel))) return rc;
            ++rounds;
            levels += static_cast<int32_t>(s.hcnt->qlen);
            innermost = static_cast<int64_t>(s.hcnt->mf);
            top = static_cast<int64_t>(s.hcnt->red[0]);
            return TGO_OK;
        }
        k = next_k;
        const bool rebuild = al.wants_rebuild(alive);
        HIP_TRY(k_core_scan(al.list, al.len, deg, static_cast<int32_t>(k), A.queue[0], rebuild ? al.keep_buffer() : nullptr,
                            s.cnt, st));
        if ((rc = turn_checked(ctx, kPeel))) return rc;
        int64_t qlen = static_cast<int64_t>(s.hcnt->qlen);
        next_k = level_min(s.hcnt->red[0]);
        if (rebuild) al.adopt(static_cast<int64_t>(s.hcnt->mf));
        // the minimum named a vertex that the level before went on to drop and peel: nobody is
        // left at k, and this scan's minimum is exact (nothing has changed since it ran)
        if (qlen == 0) continue;
        if (qlen > alive) return fail(ctx, TGO_E_HIP, "k-core peel: inconsistent level queue");
        ++levels;
        top = k;
        innermost = qlen;
        alive -= qlen;
        for (int cur = 0; qlen > 0 && k > 0; cur ^= 1) {    // (a vertex of level 0 has no neighbour)
            HIP_TRY(k_core_peel(A.queue[cur], qlen, lists, deg, static_cast<int32_t>(k), wave_row, lds_cap,
                                A.queue[cur ^ 1], n, s.cnt, st));
            if ((rc = turn_checked(ctx, kPeel))) return rc;
            ++rounds;
            const int64_t drops = static_cast<int64_t>(s.hcnt->mf);     // queued for the next launch or not
            qlen = static_cast<int64_t>(s.hcnt->qlen);
            if (drops > alive || qlen > drops) return fail(ctx, TGO_E_HIP, "k-core peel: inconsistent drop count");
            innermost += drops;
            alive -= drops;
            next_k = std::min(next_k, level_min(s.hcnt->red[0]));
        }
    }
    return TGO_OK;
}

}  // namespace

extern "C" {

int tgo_kcore(tgo_ctx* ctx, const tgo_core_args* a, int64_t* core_out, tgo_core_info* info) {
    int rc = bothE_program_check(ctx, a, "tgo_core_args", "core numbers are computed", "core numbers");
    if (rc) return rc;
    DevGraph& g = ctx->g;
    hipStream_t st = ctx->stream;
    const int64_t n = g.n;
    if ((rc = tri_forward_lists(ctx))) return rc;
    if ((rc = core_backward_lists(ctx))) return rc;
    const CoreArrays A = core_arrays(ctx->sc);
    HIP_TRY(hipEventRecord(ctx->ev0, st));
    int32_t levels = 0, rounds = 0;
    int64_t top = 0, innermost = 0;
    unsigned long long tot[2] = {0, 0};
    if (g.tri_fnnz == 0) {
        // no simple edge: nothing is peeled, every core number is 0 and the info stays zero
        HIP_TRY(k_fill_i64(A.core, 0, n, st));
    } else {
        {
            DevSpan span(st, "kcore.peel", {"simple_edges", g.tri_fnnz});
            if ((rc = core_peel_levels(ctx, A, levels, rounds, top, innermost))) return rc;
        }
        DevSpan span(st, "kcore.finish");
        HIP_TRY(hipMemsetAsync(g.core_tot, 0, 2 * sizeof(unsigned long long), st));
        HIP_TRY(k_core_finish(A.deg, n, static_cast<int32_t>(top), A.core, g.core_tot, st));
        span.end();
        HIP_TRY(hipMemcpyAsync(tot, g.core_tot, sizeof tot, hipMemcpyDeviceToHost, st));
    }
    if ((rc = program_end(ctx, levels))) return rc;
    // the device's own count of the result against the level loop's bookkeeping
    if (static_cast<int64_t>(tot[1]) != top || static_cast<int64_t>(tot[0]) != innermost)
        return fail(ctx, TGO_E_HIP, "k-core: the core numbers disagree with the peel's level counts");
    if (info) *info = tgo_core_info{top, innermost, g.tri_fnnz, levels, rounds};
    if (core_out && (rc = rows_out(ctx, A.core, core_out))) return rc;
    publish_result(ctx, TGO_RESULT_CORE, ResultSource{A.core, nullptr});
    return TGO_OK;
}

int tgo_copy_cores(tgo_ctx* ctx, int64_t* core_out) {
    if (!ctx || !core_out) return TGO_E_INVALID;
    if (int rc = copy_open(ctx, TGO_RESULT_CORE, "tgo_kcore")) return rc;
    return rows_out(ctx, ctx->sc.dist, core_out);
}

}  // extern "C"
