// api_pp.cpp — peer-pressure clustering of a bothE load (pp.hip): tgo_peer_pressure, tgo_copy_peer_pressure.
// The ranks of the Titan ids (and their inverse) live with the graph beside cc_tid (dev_alloc: released
// with it).  Round control: Counters through turn, one publish per round.
#include "ctx.hpp"

using namespace tgo;

namespace {

// Defaults of TGO_TUNE_PP_WAVE_ROW / _BLOCK_ROW / _SLOTS.
constexpr int64_t kPpWaveRow = 16, kPpBlockRow = 2048, kPpSlots = 512;

// The Scratch arrays one run uses, under the types it uses them as (row-order staging: sc.msg).
struct PpArrays {
    void* votes[2];     // distribute = 0: sc.level (n x int32) and sc.vec[0] (n x 8 bytes), n x int32 labels each;
                        // distribute = 1: sc.vec[1] and sc.vec[2], n x 8-byte words each
    int32_t *wq, *bq;   // sc.q[0] / sc.q[1]: n + 1 x int32 each; the wave and block queues
    int32_t* hist;      // sc.qdeg: n + 2 x int64, of which n x int32 hold the clusters' populations
    int64_t* label;     // sc.dist: n x int64; the labels in internal order, the published result
};

PpArrays pp_arrays(Scratch& s, bool distribute) {
    PpArrays A{{s.level, s.vec[0]}, s.q[0], s.q[1], reinterpret_cast<int32_t*>(s.qdeg), s.dist};
    if (distribute) { A.votes[0] = s.vec[1]; A.votes[1] = s.vec[2]; }
    return A;
}

// g.pp_rank / g.pp_inv: once per graph.
int pp_ranks(tgo_ctx* ctx) {
    DevGraph& g = ctx->g;
    const int64_t n = g.n;
    if (g.pp_rank || n == 0) return TGO_OK;
    // row order -> rank of the Titan id (an edge load's rows are in id order already)
    std::vector<int32_t> order(static_cast<size_t>(n));
    for (int64_t i = 0; i < n; ++i) order[i] = static_cast<int32_t>(i);
    if (!ctx->id_sorted)
        std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
            return ctx->titan_id[a] != ctx->titan_id[b] ? ctx->titan_id[a] < ctx->titan_id[b] : a < b;
        });
    std::vector<int32_t> rank(static_cast<size_t>(n)), inv(static_cast<size_t>(n));
    for (int64_t r = 0; r < n; ++r) {
        const int32_t v = ctx->perm[order[r]];
        if (v < 0 || v >= n) return fail(ctx, TGO_E_HIP, "peer pressure: inconsistent row permutation");
        rank[v] = static_cast<int32_t>(r);
        inv[r] = v;
    }
    AllocScope both(ctx);           // both arrays or none
    int32_t *d_rank = nullptr, *d_inv = nullptr;
    HIP_TRY(upload(ctx, d_rank, rank));
    HIP_TRY(upload(ctx, d_inv, inv));
    both.commit();
    g.pp_rank = d_rank;
    g.pp_inv = d_inv;
    return TGO_OK;
}

}  // namespace

extern "C" {

int tgo_peer_pressure(tgo_ctx* ctx, const tgo_pp_args* a, int64_t* cluster_out, tgo_pp_info* info) {
    int rc = bothE_program_check(ctx, a, "tgo_pp_args", "peer-pressure clustering runs", "votes along the edges");
    if (rc) return rc;
    if (a->pad != 0) return fail(ctx, TGO_E_INVALID, "tgo_pp_args.pad must be 0");
    if (a->vote_scope != TGO_SCOPE_OUT_E && a->vote_scope != TGO_SCOPE_IN_E && a->vote_scope != TGO_SCOPE_BOTH_E)
        return fail(ctx, TGO_E_INVALID, "tgo_pp_args.vote_scope must be TGO_SCOPE_OUT_E, TGO_SCOPE_IN_E or TGO_SCOPE_BOTH_E");
    if (a->distribute != 0 && a->distribute != 1) return fail(ctx, TGO_E_INVALID, "tgo_pp_args.distribute must be 0 or 1");
    if (a->max_rounds < 0) return fail(ctx, TGO_E_INVALID, "tgo_pp_args.max_rounds must be >= 0");
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    const int64_t n = g.n;
    const PpArrays A = pp_arrays(s, a->distribute != 0);
    if ((rc = titan_ids_by_index(ctx))) return rc;
    if ((rc = pp_ranks(ctx))) return rc;
    HIP_TRY(hipEventRecord(ctx->ev0, st));
    tgo_pp_info out{0, 0, 0, 0, n == 0 ? 1 : 0};
    if (n > 0) {
        PpRun r;
        // votes travel along vote_scope's entries: a vertex tallies the rows that name its senders
        r.recv = pull_view(g, a->vote_scope);
        const View send = a->vote_scope == TGO_SCOPE_OUT_E ? make_view(&g.out, nullptr)
                          : a->vote_scope == TGO_SCOPE_IN_E ? make_view(&g.in, nullptr) : make_view(&g.out, &g.in);
        r.n = n;
        r.wave_row = tuned(ctx->tune.i64(TGO_TUNE_PP_WAVE_ROW), kPpWaveRow);
        r.block_row = tuned(ctx->tune.i64(TGO_TUNE_PP_BLOCK_ROW), kPpBlockRow);
        r.slots = static_cast<int32_t>(tuned(ctx->tune.i64(TGO_TUNE_PP_SLOTS), kPpSlots));
        r.distribute = a->distribute != 0;
        r.wq = A.wq;
        r.bq = A.bq;
        int cur = 0;
        HIP_TRY(k_level_prep(s.cnt, nullptr, 0, nullptr, st));
        HIP_TRY(k_pp_init(r, send, g.pp_rank, A.votes[cur], s.cnt, st));
        if ((rc = turn(ctx))) return rc;
        r.nwave = static_cast<int64_t>(s.hcnt->qlen);
        r.nblock = static_cast<int64_t>(s.hcnt->mf);
        if (r.nwave + r.nblock > n) return fail(ctx, TGO_E_HIP, "peer pressure: inconsistent row queues");
        while (out.rounds < a->max_rounds) {
            const bool first = out.rounds == 0;
            {
                DevSpan span(st, first ? "peer_pressure.first" : "peer_pressure.vote", {"round", out.rounds + 1});
                HIP_TRY(k_pp_round(r, first, 0, A.votes[cur], A.votes[cur ^ 1], s.cnt, st));
            }
            if (r.nwave > 0) {
                DevSpan span(st, "peer_pressure.queue", {"round", out.rounds + 1}, {"wave_rows", r.nwave});
                HIP_TRY(k_pp_round(r, first, 1, A.votes[cur], A.votes[cur ^ 1], s.cnt, st));
            }
            if (r.nblock > 0) {
                DevSpan span(st, "peer_pressure.queue", {"round", out.rounds + 1}, {"block_rows", r.nblock});
                HIP_TRY(k_pp_round(r, first, 2, A.votes[cur], A.votes[cur ^ 1], s.cnt, st));
            }
            if ((rc = turn(ctx))) return rc;
            cur ^= 1;
            ++out.rounds;
            out.changed_last = static_cast<int64_t>(s.hcnt->red[0]);
            if (out.changed_last > n) return fail(ctx, TGO_E_HIP, "peer pressure: inconsistent change count");
            if (out.changed_last == 0) break;
        }
        out.converged = out.rounds > 0 && out.changed_last == 0;
        {
            DevSpan span(st, "peer_pressure.label");
            HIP_TRY(k_fill_i32(A.hist, 0, n, st));
            HIP_TRY(k_pp_finish(r, A.votes[cur], g.pp_inv, g.cc_tid, A.label, A.hist, s.cnt, st));
        }
        if ((rc = turn(ctx))) return rc;
        out.clusters = static_cast<int64_t>(s.hcnt->qlen);
        out.largest = static_cast<int64_t>(s.hcnt->red[0]);
    }
    if ((rc = program_end(ctx, out.rounds))) return rc;
    if (info) *info = out;
    if (cluster_out && n > 0 && (rc = rows_out(ctx, A.label, cluster_out))) return rc;
    publish_result(ctx, TGO_RESULT_PEER_PRESSURE, ResultSource{A.label, nullptr});
    return TGO_OK;
}

int tgo_copy_peer_pressure(tgo_ctx* ctx, int64_t* cluster_out) {
    if (!ctx || !cluster_out) return TGO_E_INVALID;
    if (int rc = copy_open(ctx, TGO_RESULT_PEER_PRESSURE, "tgo_peer_pressure")) return rc;
    return rows_out(ctx, ctx->sc.dist, cluster_out);
}

}  // extern "C"
