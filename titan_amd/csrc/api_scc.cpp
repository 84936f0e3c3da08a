// api_scc.cpp — strongly connected components of a bothE load (scc.hip): tgo_scc, tgo_copy_scc.  Nothing
// is cached with the graph but the Titan ids it shares with tgo_components.  Level control: Counters
// through turn_checked.
#include "ctx.hpp"

using namespace tgo;

namespace {

// Defaults of TGO_TUNE_SCC_WAVE_ROW / _TAIL.
constexpr int64_t kSccWaveRow = 64, kSccTailDefault = kSccTail;
enum : int { kSccTrimWalk = 0, kSccForward = 1, kSccBackward = 2, kSccColourBack = 3 };
constexpr char kScc[] = "strongly connected components";        // turn_checked's name of the program

// The Scratch arrays one run uses, under the types it uses them as (row-order staging: sc.msg).
struct SccArrays {
    SccState S;             // comp (-1 = live, else the representative) = sc.level: n x int32;
                            // din, dout (the live degrees) = the halves of sc.vec[0]: n x 8 bytes = 2n x int32;
                            // colour, mark = the halves of sc.vec[1]: as sc.vec[0]
    int32_t* queue[2];      // sc.q[0] / sc.q[1]: n + 1 x int32 each; the walks' queues
    int32_t* live_list[2];  // sc.qdeg / sc.qpre: n + 2 x int64 each, of which n x int32 hold a live list
    int32_t* pos;           // sc.vec[2]: n x 8 bytes, of which n x int32: a live vertex's place in its list
    int64_t* minid;         // sc.vec[2] again, all of it, once the passes are over: the per-representative minimum
    int32_t* size;          // = S.din once the passes are over: the components' sizes
};                          // (the labels in internal order, the published result: sc.dist as it is)

SccArrays scc_arrays(Scratch& s, int64_t n) {
    int32_t* const half0 = reinterpret_cast<int32_t*>(s.vec[0]);
    int32_t* const half1 = reinterpret_cast<int32_t*>(s.vec[1]);
    return SccArrays{SccState{s.level, half0, half0 + n, half1, half1 + n},
                     {s.q[0], s.q[1]},
                     {reinterpret_cast<int32_t*>(s.qdeg), reinterpret_cast<int32_t*>(s.qpre)},
                     reinterpret_cast<int32_t*>(s.vec[2]),
                     reinterpret_cast<int64_t*>(s.vec[2]),
                     half0};
}

struct SccRun {
    SccGraph G;
    SccArrays A;
    int64_t n, wave_row;
    bool trim;
    int64_t live;           // vertices without a component yet
    int32_t rounds = 0;
};

// Walks queue[0][0, qlen) and whatever the walks discover, launch after launch, until a launch leaves
// nothing queued.  A vertex is discovered at most once per walk: the loop ends within n discoveries.
int scc_walk_all(tgo_ctx* ctx, SccRun& r, int mode, int64_t qlen, int64_t& found) {
    Scratch& s = ctx->sc;
    found = 0;
    for (int cur = 0; qlen > 0; cur ^= 1) {
        HIP_TRY(k_scc_walk(mode, r.A.queue[cur], qlen, r.G, r.A.S, r.wave_row, r.A.queue[cur ^ 1], r.n, s.cnt, ctx->stream));
        if (int rc = turn_checked(ctx, kScc)) return rc;
        ++r.rounds;
        const int64_t got = static_cast<int64_t>(s.hcnt->mf);
        qlen = static_cast<int64_t>(s.hcnt->qlen);
        found += got;
        if (qlen > got || found > r.n)
            return fail(ctx, TGO_E_HIP, "strongly connected components: inconsistent discovery count");
    }
    return TGO_OK;
}

// The trim walk of the qlen retired vertices in queue[0] and of every vertex it retires in turn.
int scc_trim(tgo_ctx* ctx, SccRun& r, int64_t qlen) {
    if (!r.trim || qlen == 0) return TGO_OK;
    DevSpan span(ctx->stream, "scc.trim", {"queued", qlen}, {"live", r.live});
    int64_t found = 0;
    if (int rc = scc_walk_all(ctx, r, kSccTrimWalk, qlen, found)) return rc;
    if (found > r.live) return fail(ctx, TGO_E_HIP, "strongly connected components: inconsistent trim count");
    r.live -= found;
    return TGO_OK;
}

// The vertices of list (null: all) whose mark holds `bits` retire under rep (< 0: their colour), then the trim.
int scc_retire(tgo_ctx* ctx, SccRun& r, const int32_t* list, int64_t len, int32_t bits, int32_t rep) {
    Scratch& s = ctx->sc;
    HIP_TRY(k_scc_retire(list, len, r.A.S, bits, rep, r.trim ? r.A.queue[0] : nullptr, r.n, s.cnt, ctx->stream));
    if (int rc = turn_checked(ctx, kScc)) return rc;
    const int64_t got = static_cast<int64_t>(s.hcnt->mf), qlen = static_cast<int64_t>(s.hcnt->qlen);
    if (got < 1 || got > r.live) return fail(ctx, TGO_E_HIP, "strongly connected components: no progress (a pass retired no vertex)");
    r.live -= got;
    return scc_trim(ctx, r, qlen);
}

// Forward-backward from the live vertex with the largest din * dout (the smallest id among equals).
int scc_pivot(tgo_ctx* ctx, SccRun& r) {
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    HIP_TRY(k_scc_pivot_pick(r.A.S, r.n, 0, 0, s.cnt, st));
    int rc = turn_checked(ctx, kScc);
    if (rc) return rc;
    const unsigned long long product = s.hcnt->red[0];
    if (!product) return fail(ctx, TGO_E_HIP, "strongly connected components: live vertices without a pivot");
    HIP_TRY(k_scc_pivot_pick(r.A.S, r.n, 1, product, s.cnt, st));
    if ((rc = turn_checked(ctx, kScc))) return rc;
    const int64_t pivot = static_cast<int64_t>(0xFFFFFFFFULL - s.hcnt->red[0]);
    if (pivot < 0 || pivot >= r.n) return fail(ctx, TGO_E_HIP, "strongly connected components: inconsistent pivot");
    HIP_TRY(k_fill_i32(r.A.S.mark, 0, r.n, st));
    int64_t found = 0;
    {
        DevSpan span(st, "scc.pivot_forward", {"pivot", pivot}, {"live", r.live});
        HIP_TRY(k_scc_seed(r.A.S, static_cast<int32_t>(pivot), 3, r.A.queue[0], st));
        if ((rc = scc_walk_all(ctx, r, kSccForward, 1, found))) return rc;
    }
    {
        DevSpan span(st, "scc.pivot_backward", {"pivot", pivot}, {"forward", found + 1});
        HIP_TRY(k_scc_seed(r.A.S, static_cast<int32_t>(pivot), 3, r.A.queue[0], st));
        if ((rc = scc_walk_all(ctx, r, kSccBackward, 1, found))) return rc;
    }
    return scc_retire(ctx, r, nullptr, r.n, 3, static_cast<int32_t>(pivot));
}

// Colouring passes (on the grid, or all that remain in one workgroup) until no vertex is live.
int scc_colour_passes(tgo_ctx* ctx, SccRun& r, int64_t tail, int32_t& passes) {
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    const int32_t* list = nullptr;      // the live list in use (null: every vertex)
    int64_t len = r.n;
    int spare = 0, rc = TGO_OK;
    while (r.live > 0) {
        HIP_TRY(k_scc_live_list(list, len, r.A.S, r.A.live_list[spare], r.A.pos, r.n, s.cnt, st));
        if ((rc = turn_checked(ctx, kScc))) return rc;
        list = r.A.live_list[spare];
        spare ^= 1;
        len = static_cast<int64_t>(s.hcnt->qlen);
        if (len != r.live) return fail(ctx, TGO_E_HIP, "strongly connected components: inconsistent live count");
        if (tail > 0 && r.live <= tail) {
            DevSpan span(st, "scc.tail", {"live", r.live});
            HIP_TRY(k_scc_tail(list, len, r.G, r.A.S.comp, r.A.pos, r.trim, r.wave_row, s.cnt, st));
            if ((rc = turn_checked(ctx, kScc))) return rc;
            ++r.rounds;
            passes += static_cast<int32_t>(s.hcnt->qlen);
            if (static_cast<int64_t>(s.hcnt->mf) != r.live)
                return fail(ctx, TGO_E_HIP, "strongly connected components: the tail left vertices without a component");
            r.live = 0;
            return TGO_OK;
        }
        ++passes;
        {
            DevSpan span(st, "scc.colour", {"pass", passes}, {"live", r.live});
            HIP_TRY(k_scc_colour_init(list, len, r.A.S, st));
            // a colour travels at least one arc per launch and no simple path has more than live - 1
            for (int64_t launches = 1;; ++launches) {
                HIP_TRY(k_scc_colour_round(list, len, r.G, r.A.S, r.wave_row, s.cnt, st));
                if ((rc = turn_checked(ctx, kScc))) return rc;
                ++r.rounds;
                if (!s.hcnt->qlen) break;
                if (launches > r.live)
                    return fail(ctx, TGO_E_HIP, "strongly connected components: no progress (the colours do not settle)");
            }
        }
        {
            DevSpan span(st, "scc.colour_backward", {"pass", passes});
            HIP_TRY(k_scc_roots(list, len, r.A.S, r.A.queue[0], r.n, s.cnt, st));
            if ((rc = turn_checked(ctx, kScc))) return rc;
            const int64_t roots = static_cast<int64_t>(s.hcnt->qlen);
            if (roots < 1 || roots > r.live)
                return fail(ctx, TGO_E_HIP, "strongly connected components: no progress (a pass without a root)");
            int64_t found = 0;
            if ((rc = scc_walk_all(ctx, r, kSccColourBack, roots, found))) return rc;
        }
        if ((rc = scc_retire(ctx, r, list, len, 1, -1))) return rc;
    }
    return TGO_OK;
}

}  // namespace

extern "C" {

int tgo_scc(tgo_ctx* ctx, const tgo_scc_args* a, int64_t* label_out, tgo_scc_info* info) {
    int rc = bothE_program_check(ctx, a, "tgo_scc_args", "strongly connected components are computed",
                                 "strongly connected components");
    if (rc) return rc;
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    const int64_t n = g.n;
    int64_t* const label = s.dist;
    if ((rc = titan_ids_by_index(ctx))) return rc;
    HIP_TRY(hipEventRecord(ctx->ev0, st));
    tgo_scc_info out{n, std::min<int64_t>(n, 1), n, 0, 0};
    if (n == 0 || g.out.nnz + g.in.nnz == 0) {
        // no arc: every vertex is its own component and nothing is launched for it
        if (n > 0) HIP_TRY(hipMemcpyAsync(label, g.cc_tid, n * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
        if ((rc = program_end(ctx, 0))) return rc;
    } else {
        SccRun r{};
        r.G = SccGraph{g.out.off, g.out.adj, g.in.off, g.in.adj};
        r.A = scc_arrays(s, n);
        r.n = n;
        r.wave_row = tuned(ctx->tune.i64(TGO_TUNE_SCC_WAVE_ROW), kSccWaveRow);
        r.trim = ctx->tune.i64(TGO_TUNE_SCC_TRIM) != 0;
        r.live = n;
        const int64_t tail = std::min<int64_t>(tuned(ctx->tune.i64(TGO_TUNE_SCC_TAIL), kSccTailDefault), kSccTail);
        HIP_TRY(k_level_prep(s.cnt, nullptr, 0, nullptr, st));
        {
            DevSpan span(st, "scc.trim", {"live", n});
            HIP_TRY(k_scc_init(r.G, n, r.A.S, r.trim, r.wave_row, r.A.queue[0], s.cnt, st));
            if ((rc = turn_checked(ctx, kScc))) return rc;
            ++r.rounds;
        }
        const int64_t first = static_cast<int64_t>(s.hcnt->qlen);
        if (first > n) return fail(ctx, TGO_E_HIP, "strongly connected components: inconsistent trim count");
        r.live -= first;
        if ((rc = scc_trim(ctx, r, first))) return rc;
        if (ctx->tune.i64(TGO_TUNE_SCC_PIVOT) != 0 && r.live > tail && (rc = scc_pivot(ctx, r))) return rc;
        if ((rc = scc_colour_passes(ctx, r, tail, out.passes))) return rc;
        // labels, and the device's own count of the vertices that have a component
        {
            DevSpan span(st, "scc.label");
            HIP_TRY(k_fill_i64(r.A.minid, INT64_MAX, n, st));
            HIP_TRY(k_fill_i32(r.A.size, 0, n, st));
            HIP_TRY(k_scc_fold(r.A.S.comp, g.cc_tid, n, r.A.minid, r.A.size, st));
            HIP_TRY(k_scc_label(r.A.S.comp, r.A.minid, r.A.size, n, label, s.cnt, st));
        }
        if ((rc = turn_checked(ctx, kScc))) return rc;
        out.components = static_cast<int64_t>(s.hcnt->qlen);
        out.singletons = static_cast<int64_t>(s.hcnt->mf);
        out.largest = static_cast<int64_t>(s.hcnt->red[0]);
        out.rounds = r.rounds;
        const int64_t retired = static_cast<int64_t>(s.hcnt->red[1]);
        if ((rc = program_end(ctx, r.rounds))) return rc;
        if (retired != n) return fail(ctx, TGO_E_HIP, "strongly connected components: vertices were left without a component");
    }
    if (info) *info = out;
    if (label_out && (rc = rows_out(ctx, label, label_out))) return rc;
    publish_result(ctx, TGO_RESULT_SCC, ResultSource{label, nullptr});
    return TGO_OK;
}

int tgo_copy_scc(tgo_ctx* ctx, int64_t* label_out) {
    if (!ctx || !label_out) return TGO_E_INVALID;
    if (int rc = copy_open(ctx, TGO_RESULT_SCC, "tgo_scc")) return rc;
    return rows_out(ctx, ctx->sc.dist, label_out);
}

}  // extern "C"
