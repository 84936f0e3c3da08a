// api_truss.cpp — k-truss decomposition of a bothE load (truss.hip): tgo_ktruss, tgo_copy_truss,
// tgo_copy_truss_edges.  The entry-to-edge-id map and the per-edge arrays live with the graph (dev_alloc:
// released with it), beside the forward lists (tgo_triangles) and the simple adjacency (tgo_betweenness)
// they index.  Per run: the support pass's row queues = sc.level and sc.q[0], the per-vertex result in
// internal order = sc.dist, row-order staging = sc.msg.  Level control: Counters through turn_checked.
#include <climits>
#include "ctx.hpp"

using namespace tgo;

namespace {

// Defaults of tgo_truss_args.wave_row / block_row / peel_wave_row.
constexpr int64_t kTrussWaveRow = 8, kTrussBlockRow = 8, kTrussPeelWaveRow = 32;
constexpr int64_t kTrussMaxEdges = (int64_t(1) << 31) - 2;      // edge ids are int32

// The per-edge arrays of one run (m = g.tri_fnnz entries each).
struct TrussArrays {
    int32_t *sup0, *sup, *tr;
    int32_t* queue[2];
    int32_t* alive_list[2];
    int64_t* stage;             // m x int64 over the queues: a column of the edge result after the run
};

TrussArrays truss_arrays(const DevGraph& g) {
    const int64_t m = g.tri_fnnz;
    return TrussArrays{g.truss_sup0, g.truss_sup, g.truss_tr, {g.truss_q, g.truss_q + m},
                       {g.truss_q + 2 * m, g.truss_q + 3 * m}, reinterpret_cast<int64_t*>(g.truss_q)};
}

int truss_lists(tgo_ctx* ctx) {
    DevGraph& g = ctx->g;
    hipStream_t st = ctx->stream;
    const int64_t n = g.n, m = g.tri_fnnz;
    if (g.truss_seid) return TGO_OK;
    int rc = TGO_OK;
    if (!g.bc_sadj && (rc = bc_simple_adjacency(ctx))) return rc;
    if ((rc = titan_ids_by_index(ctx))) return rc;
    if (g.bc_snnz != 2 * m) return fail(ctx, TGO_E_HIP, "k-truss lists: the simple adjacency and the forward lists disagree");
    DevSpan span(st, "ktruss.lists", {"simple_edges", m});
    AllocScope lists(ctx);          // every array or none, as the forward lists
    unsigned long long* tot = nullptr;
    int32_t *seid = nullptr, *erow = nullptr, *sup0 = nullptr, *sup = nullptr, *tr = nullptr, *q = nullptr;
    HIP_TRY(dev_alloc(ctx, tot, 16));
    HIP_TRY(dev_alloc(ctx, seid, 2 * m));
    HIP_TRY(dev_alloc(ctx, erow, m));
    HIP_TRY(dev_alloc(ctx, sup0, m));
    HIP_TRY(dev_alloc(ctx, sup, m));
    HIP_TRY(dev_alloc(ctx, tr, m));
    HIP_TRY(dev_alloc(ctx, q, 4 * m));
    HIP_TRY(hipMemsetAsync(tot, 0, 16 * sizeof(unsigned long long), st));
    HIP_TRY(k_truss_edge_rows(g.tri_foff, n, erow, st));
    HIP_TRY(k_truss_seid(g.bc_soff, g.bc_sadj, n, g.bc_snnz, g.tri_foff, g.tri_fadj, seid, &tot[0], st));
    unsigned long long bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, tot, sizeof bad, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (bad) return fail(ctx, TGO_E_HIP, "k-truss lists: an adjacency entry without a forward entry");
    lists.commit();
    g.truss_tot = tot;
    g.truss_seid = seid;
    g.truss_erow = erow;
    g.truss_sup0 = sup0;
    g.truss_sup = sup;
    g.truss_tr = tr;
    g.truss_q = q;
    return TGO_OK;
}

constexpr char kPeel[] = "k-truss peel";    // turn_checked's name of the level loop

// The peel: A.tr ends as the truss values (clamped at `stop` + 2 when stop >= 0: the levels from `stop` on
// are not walked).  Out: distinct values, peel launches, the largest value and the edges at it.
int truss_peel_levels(tgo_ctx* ctx, const TrussArrays& A, int64_t stop, int64_t peel_wave_row, int32_t& levels,
                      int32_t& rounds, int64_t& top, int64_t& innermost) {
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    const int64_t m = g.tri_fnnz;
    const TrussView lists{g.tri_foff, g.tri_fadj, g.bc_soff, g.bc_sadj, g.truss_seid, g.truss_erow};
    int rc = TGO_OK;
    HIP_TRY(hipMemcpyAsync(A.sup, A.sup0, m * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemsetAsync(A.tr, 0, m * sizeof(int32_t), st));
    HIP_TRY(k_level_prep(s.cnt, nullptr, 0, nullptr, st));
    // the smallest support: a scan that queues nothing
    HIP_TRY(k_truss_scan(nullptr, m, A.sup, A.tr, -1, nullptr, nullptr, s.cnt, st));
    if ((rc = turn_checked(ctx, kPeel))) return rc;
    int64_t next_l = level_min(s.hcnt->red[0]);
    int64_t alive = m;
    AliveList al(m, A.alive_list[0], A.alive_list[1]);
    while (alive > 0) {
        if (next_l == INT64_MAX) return fail(ctx, TGO_E_HIP, "k-truss peel: alive edges without a support");
        if (stop >= 0 && next_l >= stop) break;
        const int64_t l = next_l;
        const bool rebuild = al.wants_rebuild(alive);
        HIP_TRY(k_truss_scan(al.list, al.len, A.sup, A.tr, static_cast<int32_t>(l), A.queue[0],
                             rebuild ? al.keep_buffer() : nullptr, s.cnt, st));
        if ((rc = turn_checked(ctx, kPeel))) return rc;
        int64_t qlen = static_cast<int64_t>(s.hcnt->qlen);
        next_l = level_min(s.hcnt->red[0]);
        if (rebuild) al.adopt(static_cast<int64_t>(s.hcnt->mf));
        // the minimum named an edge that the level before went on to drop and peel: nobody is left
        // at l, and this scan's minimum is exact (nothing has changed since it ran)
        if (qlen == 0) continue;
        if (qlen > alive) return fail(ctx, TGO_E_HIP, "k-truss peel: inconsistent level queue");
        ++levels;
        top = l + 2;
        innermost = qlen;
        alive -= qlen;
        for (int cur = 0; qlen > 0; cur ^= 1) {
            int64_t nlen = 0;
            if (l > 0) {                // (an edge of level 0 is in no triangle: nothing to lower)
                HIP_TRY(k_truss_peel(A.queue[cur], qlen, lists, A.sup, A.tr, static_cast<int32_t>(l), peel_wave_row,
                                     A.queue[cur ^ 1], m, s.cnt, st));
                if ((rc = turn_checked(ctx, kPeel))) return rc;
                ++rounds;
                nlen = static_cast<int64_t>(s.hcnt->qlen);
                if (nlen > alive) return fail(ctx, TGO_E_HIP, "k-truss peel: inconsistent drop count");
                next_l = std::min(next_l, level_min(s.hcnt->red[0]));
            }
            HIP_TRY(k_truss_settle(A.queue[cur], qlen, static_cast<int32_t>(l + 2), A.queue[cur ^ 1], nlen, A.tr, st));
            innermost += nlen;
            alive -= nlen;
            qlen = nlen;
        }
    }
    if (alive > 0) {                    // the levels from `stop` on: one value, stop + 2
        HIP_TRY(k_truss_clamp(A.tr, m, static_cast<int32_t>(stop + 2), st));
        ++levels;
        top = stop + 2;
        innermost = alive;
    }
    return TGO_OK;
}

}  // namespace

extern "C" {

int tgo_ktruss(tgo_ctx* ctx, const tgo_truss_args* a, int64_t* vtruss_out, tgo_truss_info* info) {
    int rc = bothE_program_check(ctx, a, "tgo_truss_args", "truss numbers are computed", "truss numbers");
    if (rc) return rc;
    if (a->k < 0 || a->k == 1) return fail(ctx, TGO_E_INVALID, "tgo_truss_args.k must be 0 (every level) or >= 2");
    if (a->wave_row < 0 || a->block_row < 0 || a->peel_wave_row < 0)
        return fail(ctx, TGO_E_INVALID, "tgo_truss_args.wave_row, block_row and peel_wave_row must be >= 0 (0: the default)");
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    const int64_t n = g.n;
    if ((rc = tri_forward_lists(ctx))) return rc;
    const int64_t m = g.tri_fnnz;
    if (m > kTrussMaxEdges)
        return fail(ctx, TGO_E_UNSUPPORTED, "tgo_ktruss: more than 2^31 - 2 simple edges (edge ids are int32)");
    if (m > 0 && (rc = truss_lists(ctx))) return rc;
    int64_t* const vtruss = s.dist;
    HIP_TRY(hipEventRecord(ctx->ev0, st));
    int32_t levels = 0, rounds = 0;
    int64_t top = 0, innermost = 0;
    unsigned long long tot[3] = {0, 0, 0};
    if (m == 0) {
        // no simple edge: nothing is peeled, every value is 0 and the info stays zero
        HIP_TRY(k_fill_i64(vtruss, 0, n, st));
    } else {
        const TrussArrays A = truss_arrays(g);
        HIP_TRY(hipMemsetAsync(g.truss_tot, 0, 16 * sizeof(unsigned long long), st));
        {
            DevSpan span(st, "ktruss.support", {"forward_entries", m}, {"max_forward", g.tri_max_fwd});
            HIP_TRY(hipMemsetAsync(A.sup0, 0, m * sizeof(int32_t), st));
            HIP_TRY(k_truss_support(g.tri_foff, g.tri_fadj, n, a->wave_row ? a->wave_row : kTrussWaveRow,
                                    a->block_row ? a->block_row : kTrussBlockRow, g.tri_max_fwd, A.sup0, s.level, s.q[0],
                                    &g.truss_tot[0], st));
        }
        {
            DevSpan span(st, "ktruss.peel", {"simple_edges", m});
            if ((rc = truss_peel_levels(ctx, A, a->k ? a->k - 2 : -1, a->peel_wave_row ? a->peel_wave_row : kTrussPeelWaveRow,
                                        levels, rounds, top, innermost)))
                return rc;
        }
        DevSpan span(st, "ktruss.finish");
        HIP_TRY(k_truss_vertex(g.bc_soff, g.truss_seid, A.tr, n, vtruss, st));
        HIP_TRY(k_truss_totals(A.tr, A.sup0, m, static_cast<int32_t>(top), &g.truss_tot[4], st));
        span.end();
        HIP_TRY(hipMemcpyAsync(tot, &g.truss_tot[4], sizeof tot, hipMemcpyDeviceToHost, st));
    }
    if ((rc = program_end(ctx, levels))) return rc;
    // the device's own count of the result against the level loop's bookkeeping
    if (static_cast<int64_t>(tot[1]) != top || static_cast<int64_t>(tot[0]) != innermost || tot[2] % 3 != 0)
        return fail(ctx, TGO_E_HIP, "k-truss: the truss values disagree with the peel's level counts");
    if (info) *info = tgo_truss_info{top, innermost, static_cast<int64_t>(tot[2] / 3), m, levels, rounds};
    if (vtruss_out && (rc = rows_out(ctx, vtruss, vtruss_out))) return rc;
    publish_result(ctx, TGO_RESULT_TRUSS, ResultSource{vtruss, nullptr});
    return TGO_OK;
}

int tgo_copy_truss(tgo_ctx* ctx, int64_t* vtruss_out) {
    if (!ctx || !vtruss_out) return TGO_E_INVALID;
    if (int rc = copy_open(ctx, TGO_RESULT_TRUSS, "tgo_ktruss")) return rc;
    return rows_out(ctx, ctx->sc.dist, vtruss_out);
}

int tgo_copy_truss_edges(tgo_ctx* ctx, int64_t* u_ids, int64_t* v_ids, int64_t* truss, int64_t* support) {
    if (!ctx) return TGO_E_INVALID;
    if (int rc = copy_open(ctx, TGO_RESULT_TRUSS, "tgo_ktruss")) return rc;
    DevGraph& g = ctx->g;
    hipStream_t st = ctx->stream;
    const int64_t m = g.tri_fnnz;
    if (m == 0) return TGO_OK;
    const TrussArrays A = truss_arrays(g);
    int64_t* const out[4] = {u_ids, v_ids, truss, support};
    for (int which = 0; which < 4; ++which) {
        if (!out[which]) continue;
        // each column finishes before the next reuses the staging
        HIP_TRY(k_truss_edge_column(which, g.truss_erow, g.tri_fadj, g.cc_tid, A.tr, A.sup0, m, A.stage, st));
        HIP_TRY(hipMemcpyAsync(out[which], A.stage, m * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return TGO_OK;
}

}  // extern "C"
