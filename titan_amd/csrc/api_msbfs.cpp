// api_msbfs.cpp — multi-source BFS of the C-ABI (up to 64 sources a sweep, msbfs.hip): the level
// loop, its scratch and cold layout, and the resolvers of its tuning knobs.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include "ctx.hpp"

using namespace tgo;

namespace tgo {

int ms_alloc(tgo_ctx* ctx) {
    Scratch& s = ctx->sc;
    if (s.ms_vis) return TGO_OK;
    const int64_t n = ctx->g.n;
    HIP_TRY(dev_alloc(ctx, s.ms_vis, n + 1));
    HIP_TRY(dev_alloc(ctx, s.ms_fr, n + 1));
    HIP_TRY(dev_alloc(ctx, s.ms_nx, n + 1));
    HIP_TRY(dev_alloc(ctx, s.ms_lvl, n * kLevelPlanes + 1));
    // the entry-less rows of every plane, once: no level writes them (record_level sees rows with
    // entries only) and the readers (ms_extract, the closeness fold) take them under vis, so the
    // sweeps fill [0, n_active) only
    s.ms_clean = 0;
    if (n > ctx->g.n_active)
        for (int k = 0; k < kLevelPlanes; ++k)
            HIP_TRY(hipMemsetAsync(s.ms_lvl + static_cast<int64_t>(k) * n + ctx->g.n_active, 0,
                                   (n - ctx->g.n_active) * sizeof(uint64_t), ctx->stream));
    HIP_TRY(dev_alloc(ctx, s.ms_fbm, (n + 63) / 64 + 1));
    HIP_TRY(dev_alloc(ctx, s.ms_seeds, TGO_MAX_SOURCES));
    HIP_TRY(dev_alloc(ctx, s.ms_stat, 2 * TGO_MAX_SOURCES));
    HIP_TRY(dev_alloc(ctx, s.ms_srcent, TGO_MAX_SOURCES));
    ctx->st.device_bytes = ctx->dev_bytes;
    return TGO_OK;
}

// The sweep's knobs (env.hpp tuned: the ctx's tgo_set_tuning value, else the variable, else the
// default).  Push budget of the pull levels' sparse sources (the source split), as a fraction of
// the list entries (default 0.5 %)
double ms_split_of(const tgo_ctx* ctx) {
    static const double env = env_double("TGO_MS_SPLIT", 0.005);
    return tuned(ctx->tune.f64(TGO_TUNE_MS_SPLIT), env);
}
// gamma of the stay-in-pull rule, and the sparse push levels' fraction of n_active (tgo_bfs_multi)
double ms_stay_of(const tgo_ctx* ctx) {
    static const double env = env_clamped("TGO_MS_STAY", kMsStayDefault, 0.0, HUGE_VAL);
    return tuned(ctx->tune.f64(TGO_TUNE_MS_STAY), env);
}
double ms_sparse_of(const tgo_ctx* ctx) {
    static const double env = env_clamped("TGO_MS_SPARSE", kMsSparseDefault, 0.0, HUGE_VAL);
    return tuned(ctx->tune.f64(TGO_TUNE_MS_SPARSE), env);
}
// head probe of ms_pull's long lists, in entries (clamped before the cast)
int64_t ms_head_of(const tgo_ctx* ctx) {
    static const int64_t env = static_cast<int64_t>(
        env_clamped("TGO_MS_HEAD", static_cast<double>(kMsHeadDefault), 0.0, static_cast<double>(kMsHeadMax)));
    return tuned(ctx->tune.i64(TGO_TUNE_MS_HEAD), env);
}

}  // namespace tgo

// The cold layout of the scope's pull view for the split first pull level (built once per
// graph and scope, on first use): neighbours >= hot (TGO_MS_COLD_HOT, 384 K = 3 MB of masks,
// the hot head every XCD's L2 keeps) in segments of TGO_MS_COLD_SEG (384 K) neighbours.
static int ms_cold_layout(tgo_ctx* ctx, int32_t scope, const View& pull, int64_t hot_req) {
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    static const int64_t hot_env = static_cast<int64_t>(env_double("TGO_MS_COLD_HOT", 393216.0));
    static const int64_t seg_env = static_cast<int64_t>(env_double("TGO_MS_COLD_SEG", 393216.0));
    const int64_t hot = hot_req > 1 ? hot_req : hot_env, seg = hot_req > 1 ? hot_req : seg_env;
    if (g.msc_scope == scope && g.msc_req == hot) return TGO_OK;
    g.msc_scope = scope;
    g.msc_req = hot;
    g.msc_C = 0;
    if (hot <= 0 || hot >= INT32_MAX || seg <= 0) return TGO_OK;
    Span span("msbfs.cold_layout");
    DevArray<int32_t> cadj, crow;
    int64_t C = 0;
    std::string err;
    if (int rc = build_ms_cold(pull, g.n, static_cast<int32_t>(hot), seg, cadj, crow, C, ctx->stream, err))
        return fail(ctx, rc, err);
    if (C == 0) return TGO_OK;
    adopt(ctx, g.msc_adj, cadj);
    adopt(ctx, g.msc_row, crow);
    if (!s.ms_cacc) {
        HIP_TRY(dev_alloc(ctx, s.ms_cacc, g.n + 1));
        HIP_TRY(dev_alloc(ctx, s.ms_need, g.n + 1));
        HIP_TRY(hipMemsetAsync(s.ms_need, 0, g.n + 1, ctx->stream));
    }
    g.msc_C = C;
    g.msc_hot = static_cast<int32_t>(hot);
    ctx->st.device_bytes = ctx->dev_bytes;
    return TGO_OK;
}

namespace tgo {

// One sweep of up to 64 sources: `in` holds the sources as internal ids (all >= 0; one given twice
// takes two bits).  On return sc.ms_vis holds the reached-by masks, sc.ms_lvl the level planes
// [0, sc.ms_nplanes), sc.ms_nsrc = nseeds; tgo_stats.levels = the levels run.
int run_ms_sweep(tgo_ctx* ctx, const int64_t* in, int32_t nseeds, int32_t max_depth, int32_t scope, int32_t flags) {
    int rc = TGO_OK;
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    const int64_t n = g.n;
    const View pull = pull_view(g, scope), push = push_view(g, scope);
    std::vector<int32_t> uniq;
    for (int r = 0; r < nseeds; ++r)
        if (std::find(uniq.begin(), uniq.end(), static_cast<int32_t>(in[r])) == uniq.end())
            uniq.push_back(static_cast<int32_t>(in[r]));
    s.ms_nsrc = nseeds;
    HIP_TRY(hipEventRecord(ctx->ev0, st));
    HIP_TRY(hipMemcpyAsync(s.ms_seeds, in, nseeds * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(s.q[0], uniq.data(), uniq.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(s.ms_vis, 0, n * 8, st));
    // both mask buffers are still zero when the last sweep ended on an empty sparse level; the
    // flag is down while a sweep runs, so a failed or depth-cut sweep leaves it down
    const bool masks_zero = s.ms_masks_zero;
    s.ms_masks_zero = false;
    if (!masks_zero) HIP_TRY(hipMemsetAsync(s.ms_fr, 0, n * 8, st));
    s.ms_nplanes = 0;
    HIP_TRY(k_ms_seed(s.ms_seeds, nseeds, s.ms_vis, s.ms_fr, INT64_MAX, st));
    HIP_TRY(k_degree_i64(push, s.q[0], static_cast<int64_t>(uniq.size()), s.qdeg, st));
    const uint64_t full = nseeds == 64 ? ~0ULL : ((1ULL << nseeds) - 1ULL);
    const int64_t total = pull.nlists > 1 ? g.out.nnz + g.in.nnz : (scope == TGO_SCOPE_IN_E ? g.out.nnz : g.in.nnz);
    static const double ms_alpha = env_double("TGO_MS_ALPHA", 12.0);
    static const bool trace = trace_on();
    // frontier-bitmap filter of pull levels: measured slower (every pull level: 3.07 -> 3.99 ms,
    // 0.95 -> 1.25, 0.18 -> 0.19; MS-BFS 3146 -> 2471 GTEPS, profiles/r02ad_*): the mask gathers
    // mostly hit L2 / the Infinity Cache already and the probe adds a dependent load.  Opt-in.
    // TGO_MS_FILTER_FROM=H probes the bitmap only for neighbours >= H (the cold ids whose
    // gathers miss L2); TGO_MS_FILTER=1 is H=0, the filter for every neighbour.  Measured on
    // RMAT-24 (profiles/r03h_ms_filter.log): off 5.59 ms/sweep; H = 0 7.05, 128K 6.32, 256K 6.10,
    // 384K 5.93, 1M 5.62 — monotone towards no filter, so the probe's dependent load costs more
    // than the cold gathers it saves.  Off by default.
    static const int32_t filter_from = env_double("TGO_MS_FILTER", 0.0) != 0.0
        ? 0 : static_cast<int32_t>(env_double("TGO_MS_FILTER_FROM", -1.0));
    const bool filter = filter_from >= 0 && filter_from < n;
    // TGO_MS_SPLIT: push budget of the pull levels' sparse sources, as a fraction of the
    // list entries (0 = every source pulled)
    const double split_frac = tgo::ms_split_of(ctx);
    // TGO_TUNE_MS_STAY (gamma): after a pull level the next one pulls too while the list entries
    // of the still-open vertices (mu, what a pull walks at most) are <= gamma x the frontier's
    // entries (mf, what a push ORs atomically) — both directions pay one pass over the masks
    // (the pull itself / ms_queue).  TGO_TUNE_MS_SPARSE: a push level whose frontier is queued
    // and has at most that fraction of n_active entries (level 0 always) runs in the sparse
    // form (k_ms_push_sparse / k_ms_settle_sparse): no pass over every mask.
    const double stay_gamma = tgo::ms_stay_of(ctx), sparse_frac = tgo::ms_sparse_of(ctx);
    // TGO_TUNE_MS_HEAD: the entries of its own lists a lane with a long list probes before the
    // whole wave takes the list (0 = off)
    const int64_t head = tgo::ms_head_of(ctx);
    // TGO_MS_COMPACT (default on, 0 = off): the pull levels that count mu — the level after the
    // frontier's peak and every stay-rule level after it — run ms_pull_compact; TGO_MS_CHUNK: the
    // vertices a wave scans before it walks the open ones (512 / 1024 / 2048).  Not with the
    // diagnostic tallies (TGO_MS_DIAG), which the word form keeps.
    static const bool diag = env_double("TGO_MS_DIAG", 0.0) != 0.0;
    static const bool compact_on = env_i64("TGO_MS_COMPACT", 1) != 0 && !diag;
    static const int32_t compact_chunk = [] {
        const int64_t c = env_i64("TGO_MS_CHUNK", kMsChunkDefault);
        return static_cast<int32_t>(c == 512 || c == 1024 || c == 2048 ? c : kMsChunkDefault);
    }();
    int64_t qlen = static_cast<int64_t>(uniq.size());
    int64_t mf = 0;             // the seeds' entries are not read back: level 0 always pushes (a
                                // direction is policy only; the read cost a stream drain, ~45 us)
    int64_t reached = qlen;     // vertices reached by any source so far
    bool srcent_ready = false;  // ms_srcent holds the current frontier's push entries per source
    static const double push_light = env_double("TGO_MS_PUSH_LIGHT", 1.0 / 16.0);
    static const bool push_probe = env_double("TGO_MS_PUSH_PROBE", 1.0) != 0.0;
    // measured slower at RMAT-24 (second level 446 -> 561 us, profiles/r04t_ms_push_ab.log): off
    static const int push_range_log2 = static_cast<int>(env_double("TGO_MS_PUSH_RANGE", 0.0));
    static const int64_t push_range_min = static_cast<int64_t>(env_double("TGO_MS_PUSH_RANGE_MIN", 1048576.0));
    const int depth = std::min(max_depth, 65534);
    uint64_t* fr = s.ms_fr;
    uint64_t* nx = s.ms_nx;
    int cur = 0, levels = 0;
    bool queued = true;         // q[cur] holds the frontier (pull levels only count it)
    bool pulled = false;        // the previous level pulled
    bool cnt_zero = false;      // the counters are zero (k_publish_turn leaves them so)
    bool nx_clean = masks_zero; // nx is zero over the active rows (no fill before a push)
    int64_t prev_mf = 0;        // the entries of the frontier one level back
    int64_t mu = -1;            // after a pull level: list entries of the still-open vertices (< 0: not counted)
    bool level0_sparse = false, last_sparse = false;
    unsigned long long se_pub[TGO_MAX_SOURCES] = {};   // the per-source entries the last settle published
    const volatile unsigned long long* hw = host_words(ctx);
    for (int L = 0; L < depth && qlen > 0; ++L) {
        const bool stay = pulled && mu >= 0 && stay_gamma > 0.0 &&
                          static_cast<double>(mu) <= stay_gamma * static_cast<double>(mf);
        const bool use_pull = stay || static_cast<double>(mf) * ms_alpha > static_cast<double>(total);
        DevSpan span(st, "msbfs.level", {"level", L}, {"pull", use_pull ? 1 : 0}, {"compact", 0});
        if ((rc = ms_planes_for(ctx, L + 1, true))) return rc;
        // this level writes the planes of L + 1's set bits: not clean while it runs (a failed or
        // depth-cut sweep leaves them so); clean again if it turns out to have found nothing
        const uint32_t was_clean = s.ms_clean & ms_planes_written(L + 1);
        s.ms_clean &= ~was_clean;
        const bool queued_before = queued;
        if (!use_pull && !queued) {     // the frontier's queue, for the push level's scan
            if (!cnt_zero) HIP_TRY(hipMemsetAsync(s.cnt, 0, sizeof(Counters), st));
            HIP_TRY(k_ms_queue(push, g.n_active, fr, s.q[cur], s.qdeg, s.cnt, st));
        }
        queued = !use_pull;
        const bool prev_pull = pulled;
        pulled = use_pull;
        bool sums = false;          // this push level's settle sums the per-source entries
        if (!use_pull && !queued_before) cnt_zero = false;      // ms_queue counted into them
        bool sparse_level = false;  // this push level runs in the sparse form
        bool count_open = false;    // this pull level counts mu
        if (use_pull) {
            if (!cnt_zero) HIP_TRY(hipMemsetAsync(s.cnt, 0, sizeof(Counters), st));
            cnt_zero = true;
            // Split the sources: the pull's walk of a vertex stops once every open source is
            // covered, and one source whose frontier never reaches the vertex (a source far
            // from it, or one whose sweep is over) makes every walk scan its whole list.  The
            // sources with the smallest frontiers (exact push entries per source, within a
            // budget of split_frac of the list entries; every source with an empty frontier)
            // are pushed into candidate masks instead, and the pull covers only the rest.
            // (tried at the first pull level of a run of pull levels, where the frontiers
            // are most unequal; later pull levels found nothing to split on RMAT-24)
            uint64_t sparse = 0;
            if (split_frac > 0.0 && !prev_pull) {
                // every source's exact push entries in one pass, then the smallest within the budget
                // after a push level its settle summed them already (srcent_ready)
                // (published with that level's counts: no copy, no stream synchronisation here)
                static const bool srcent_check = env_double("TGO_MS_SRCENT_CHECK", 0.0) != 0.0;
                if (srcent_ready && srcent_check) {     // dev check: the settle's sums = a pass of their own
                    HIP_TRY(k_ms_source_entries(push, fr, g.n_active, full, s.ms_stat, st));
                    unsigned long long x[TGO_MAX_SOURCES];
                    HIP_TRY(hipMemcpyAsync(x, s.ms_stat, sizeof(x), hipMemcpyDeviceToHost, st));
                    HIP_TRY(hipStreamSynchronize(st));
                    if (std::memcmp(x, se_pub, sizeof(x)) != 0)
                        return fail(ctx, TGO_E_HIP, "multi-source BFS: settle per-source entries differ from ms_source_entries");
                    if (trace) std::fprintf(stderr, "[tgo] ms level %d: settle per-source entries checked\n", L);
                }
                unsigned long long se[TGO_MAX_SOURCES];
                if (srcent_ready) {
                    std::memcpy(se, se_pub, sizeof(se));
                } else {
                    s.ms_srcent_zero = false;
                    HIP_TRY(k_ms_source_entries(push, fr, g.n_active, full, s.ms_srcent, st));
                    HIP_TRY(hipMemcpyAsync(se, s.ms_srcent, sizeof(se), hipMemcpyDeviceToHost, st));
                    HIP_TRY(hipStreamSynchronize(st));
                }
                int order[TGO_MAX_SOURCES];
                for (int r = 0; r < nseeds; ++r) order[r] = r;
                std::sort(order, order + nseeds, [&](int a, int b) { return se[a] < se[b]; });
                const double budget = split_frac * static_cast<double>(total);
                double used = 0.0;
                for (int i = 0; i < nseeds; ++i) {
                    const int r = order[i];
                    if (used + static_cast<double>(se[r]) > budget) break;
                    used += static_cast<double>(se[r]);
                    sparse |= 1ULL << r;
                }
                if (sparse == full) sparse = 0;            // nothing left to pull: plain pull
                if (sparse) {
                    bool any = false;
                    for (int r = 0; r < nseeds; ++r) any |= ((sparse >> r) & 1ULL) && se[r] > 0;
                    if (!nx_clean) HIP_TRY(hipMemsetAsync(nx, 0, g.n_active * 8, st));
                    if (any) {                           // push the sparse sources' frontiers
                        HIP_TRY(k_ms_queue(push, g.n_active, fr, s.q[cur ^ 1], s.qdeg, s.cnt, st, sparse));
                        if ((rc = turn(ctx))) return rc;         // the counters zero again after it
                        const int64_t sq = static_cast<int64_t>(s.hcnt->qlen);
                        if (sq > 0) {
                            if ((rc = scan_frontier(ctx, sq))) return rc;
                            HIP_TRY(k_ms_push(push, s.q[cur ^ 1], s.qpre, sq, fr, s.ms_vis, nx, st, PackTouch{}, sparse));
                        }
                    }
                    if (trace) std::fprintf(stderr, "[tgo] ms level %d split: %d sparse sources, %.0f push entries\n", L,
                                            __builtin_popcountll(sparse), used);
                }
            }
            if (filter) HIP_TRY(k_ms_fbitmap(fr, n, s.ms_fbm, st));
            // The first pull level of a run walks long lists to their end (its frontiers are the
            // most unequal: few walks are covered early).  Opt-in split (TGO_TUNE_MS_COLD /
            // TGO_MS_COLD=1): the walk covers the hot head only, a blocked pass over the cold
            // entries in (segment, row) order ORs the open rows' cold masks from L2, ms_finish
            // settles those rows — same masks, same result.  Measured slower at RMAT-24 (level 2
            // 2.01 -> 2.69 ms, sweep 4.54 -> 5.22 ms, gpurun_out/r04m): of the level's 227 M
            // gathers only 44 M are cold (profiles/r04l_ms_diag.log), and the pass streams every
            // cold entry of every row to reach them.
            MsColdSplit cs;
            static const bool cold_env = env_double("TGO_MS_COLD", 0.0) != 0.0;
            const int64_t cold = ctx->tune.i64(TGO_TUNE_MS_COLD);
            const bool cold_on = tuned_on(cold, cold_env);
            if (cold_on && !prev_pull && !filter) {
                if ((rc = ms_cold_layout(ctx, scope, pull, cold))) return rc;
                if (g.msc_C > 0) {
                    cs.hot_lim = g.msc_hot;
                    cs.acc = s.ms_cacc;
                    cs.need = s.ms_need;
                }
            }
            // mu for the next level's direction.  The rows a cold split leaves to ms_finish are
            // not in it: no stay rule after such a level.  Counted once the frontier shrinks (mf
            // below the level before), since only then can the next level fall under the push
            // threshold: the count is one more atomic per block, 9 - 25 us at RMAT-24's two
            // large levels.
            count_open = stay_gamma > 0.0 && !cs.acc && mf < prev_mf;
            // ... and where it counts mu it runs compact: past the peak few vertices are open (a
            // source-split level stays on the word form, which takes the split's candidates)
            const bool compact = compact_on && count_open && !sparse;
            if (compact) span.set_third(1);
            HIP_TRY(k_ms_pull(pull, push, g.n_active, full, fr, filter ? s.ms_fbm : nullptr, s.ms_vis, nx,
                              ms_planes(ctx), s.cnt, L + 1, st, filter ? filter_from : 0, full & ~sparse,
                              sparse ? nx : nullptr, cs, count_open, cs.acc ? 0 : head,    // hot_lim's cut rule as it was
                              compact ? compact_chunk : 0));
            if (cs.acc) {
                HIP_TRY(k_ms_cold(g.msc_adj, g.msc_row, g.msc_C, fr, s.ms_need, s.ms_cacc, st));
                HIP_TRY(k_ms_finish(push, g.n_active, full, s.ms_vis, nx, sparse ? nx : nullptr, ms_planes(ctx), s.cnt,
                                    L + 1, s.ms_need, s.ms_cacc, st));
            }
        } else {
            // candidates only land on rows with entries (< n_active); the tail is never read
            // one kernel zeroes the counters, the candidate masks and the scan's tail entry
            // (three fills of ~5 us launch each before)
            // (the counters only when a queue build counted into them, the masks only when nx
            // is not known to be zero: after a dense push or a pull)
            HIP_TRY(k_level_prep(cnt_zero ? nullptr : s.cnt, nx, nx_clean ? 0 : g.n_active, s.qdeg + qlen, st));
            cnt_zero = true;
            // A small frontier of long lists pushes target-ranged (k_ms_push_ranged: XCD x on
            // the x-th eighth of the (target range, entry) enumeration, its ranges' masks in
            // its L2); TGO_MS_PUSH_RANGE = log2 of the range (0 = off).
            const int64_t rng = static_cast<int64_t>(1) << std::min(40, std::max(0, push_range_log2));
            const int64_t nr = (g.n_active + rng - 1) / rng;
            const bool ranged = push_range_log2 > 0 && mf >= push_range_min && nr > 1 &&
                                (nr + 1) * qlen <= kMsRangePairs && nr * qlen + 1 <= n + 2;
            // the sparse form: the frontier (queued, as for every push) has little to push (the
            // ranged push is for large frontiers and does not combine with it)
            sparse_level = sparse_frac > 0.0 && !ranged &&
                           (L == 0 || static_cast<double>(mf) <= sparse_frac * static_cast<double>(g.n_active));
            sums = split_frac > 0.0 && (L == 0 || static_cast<double>(mf) * ms_alpha * 64.0 > static_cast<double>(total));
            if (ranged) {
                for (int b = 0; b < 2; ++b)
                    if (!s.ms_rp[b]) HIP_TRY(dev_alloc(ctx, s.ms_rp[b], kMsRangePairs));
                const bool light = static_cast<double>(reached) < push_light * static_cast<double>(n);
                HIP_TRY(k_ms_push_ranged(push, s.q[cur], qlen, g.n_active, rng, s.ms_rp[0], s.ms_rp[1], s.qdeg, s.qpre,
                                         s.cub_tmp, s.cub_bytes, fr, light ? nullptr : s.ms_vis, nx, st));
            } else {
            HIP_TRY(scan_exclusive_i64(s.cub_tmp, s.cub_bytes, s.qdeg, s.qpre, qlen + 1, st));   // tail zeroed above
            if (sparse_level)
                HIP_TRY(k_ms_push_sparse(push, s.q[cur], s.qpre, qlen, fr, s.ms_vis, nx, s.q[cur ^ 1], s.cnt, st));
            else {
            // While few vertices are reached the push skips the reached-mask read of its
            // targets (ms_settle drops the reached bits anyway): one random 8-byte read less
            // per entry at the second level's 12.7 M entries (RMAT-24).  TGO_MS_PUSH_PROBE=0
            // also drops the read of the candidate mask before the atomic there.
            const bool light = static_cast<double>(reached) < push_light * static_cast<double>(n);
            HIP_TRY(k_ms_push(push, s.q[cur], s.qpre, qlen, fr, light ? nullptr : s.ms_vis, nx, st, PackTouch{}, ~0ULL,
                              light ? push_probe : true));
            }
            }
            // the new frontier's push entries per source, for the next level's split — when that
            // level may pull (this frontier's entries within 64x of the pull threshold; a
            // frontier grows at most ~40x a level on RMAT-24), else the split computes them
            // (level 0: the seeds' entries are not known, so always)
            if (sums && !s.ms_srcent_zero) HIP_TRY(hipMemsetAsync(s.ms_srcent, 0, 64 * sizeof(unsigned long long), st));
            if (sums) s.ms_srcent_zero = false;
            // a frontier within 8x of the pull threshold: the next level will likely pull and
            // needs no queue — settle and count only (ms_queue builds it if the level pushes)
            const bool next_pull = static_cast<double>(mf) * ms_alpha * 8.0 > static_cast<double>(total);
            if (sparse_level) {
                HIP_TRY(k_ms_settle_sparse(push, s.q[cur ^ 1], s.qdeg, s.ms_vis, nx, ms_planes(ctx), s.cnt, L + 1, st,
                                           sums ? s.ms_srcent : nullptr, s.q[cur], qlen, fr));
            } else if (next_pull) {
                HIP_TRY(k_ms_settle_count(push, g.n_active, s.ms_vis, nx, ms_planes(ctx), s.cnt, L + 1, st,
                                          sums ? s.ms_srcent : nullptr));
                queued = false;
            } else {
                HIP_TRY(k_ms_settle(push, g.n_active, s.ms_vis, nx, ms_planes(ctx), s.q[cur ^ 1], s.qdeg, s.cnt, L + 1,
                                    st, sums ? s.ms_srcent : nullptr));
            }
        }
        srcent_ready = !use_pull && sums;
        {
            // publish the counts, then queue the next level's direction-independent prefix (its
            // level planes, zeroed counters) before the host waits: the GPU runs it during the
            // host's round trip (≈ 10–25 us a level)
            // (the same launch zeroes the counters, and publishes and zeroes the per-source sums)
            unsigned long long seq = 0;
            if ((rc = turn_begin(ctx, seq, sums ? s.ms_srcent : nullptr))) return rc;
            cnt_zero = true;
            if (sums) s.ms_srcent_zero = true;
            if (L + 1 < depth && (rc = ms_planes_for(ctx, L + 2, true))) return rc;
            if ((rc = wait_publish(ctx, seq))) return rc;
        }
        qlen = static_cast<int64_t>(s.hcnt->qlen);
        if (qlen == 0) s.ms_clean |= was_clean;      // nothing found: nothing recorded
        prev_mf = mf;
        mf = static_cast<int64_t>(s.hcnt->mf);
        mu = count_open ? static_cast<int64_t>(s.hcnt->open) : -1;
        if (sums)
            for (int r = 0; r < TGO_MAX_SOURCES; ++r) se_pub[r] = hw[kPublishExtra + r];
        reached += qlen;
        // the consumed frontier's masks were cleared by the sparse settle: zero when they are nx
        nx_clean = sparse_level;
        last_sparse = sparse_level;
        if (L == 0) level0_sparse = sparse_level;
        if (trace) std::fprintf(stderr, "[tgo] ms level %d %s -> %lld vertices, %lld entries, %llu source-bits%s\n", L,
                                use_pull ? "pull" : "push", (long long)qlen, (long long)mf, s.hcnt->red[0],
                                use_pull ? (stay ? " (stayed in pull)" : "") : (sparse_level ? " (sparse)" : ""));
        if (trace && count_open) std::fprintf(stderr, "[tgo]   %lld list entries of still-open vertices\n", (long long)mu);
        if (trace && diag && use_pull) {
            unsigned long long d[kMsDiagWords] = {};
            HIP_TRY(k_ms_diag_take(d, st));
            std::fprintf(stderr, "[tgo]   pull: %llu entries examined, %llu hot / %llu cold mask gathers, %llu open vertices, "
                         "%llu stopped early; long lists: %llu, %llu entries examined (%llu hot / %llu cold gathers), "
                         "%llu stopped early\n", d[0], d[1], d[2], d[3], d[4], d[6], d[5], d[8], d[9], d[7]);
            std::fprintf(stderr, "[tgo]   long lists covered within 4 / 8 / 16 / 32 / 64 entries: %llu / %llu / %llu / %llu / %llu, "
                         "later %llu, never %llu (head %lld)\n", d[10], d[11], d[12], d[13], d[14], d[15], d[16],
                         static_cast<long long>(head));
        }
        std::swap(fr, nx);
        cur ^= 1;
        ++levels;
    }
    if (qlen > 0 && max_depth > depth)
        return fail(ctx, TGO_E_UNSUPPORTED, "multi-source BFS stores levels as uint16: depth > 65534");
    if (int rc = program_end(ctx, max_depth)) return rc;
    ctx->st.levels = levels;
    // the last level was sparse and found nothing: its frontier's masks are cleared, nothing was
    // written to the other buffer; ms_fr's entry-less tail (seeds only) was cleared at level 0
    s.ms_masks_zero = level0_sparse && last_sparse && qlen == 0;
    if (flags & TGO_FLAG_STATS) {
        HIP_TRY(hipMemsetAsync(s.ms_stat, 0, 2 * TGO_MAX_SOURCES * sizeof(unsigned long long), st));
        HIP_TRY(k_ms_reach(pull, s.ms_vis, n, nseeds, s.ms_stat, s.ms_stat + TGO_MAX_SOURCES, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return TGO_OK;
}

}  // namespace tgo

extern "C" {

int tgo_bfs_multi(tgo_ctx* ctx, const int64_t* seeds, int32_t nseeds, const tgo_bfs_args* a, int64_t* dist_out) {
    if (!ctx) return TGO_E_INVALID;
    ctx->res_kind = -1;
    if (!a || !seeds) return fail(ctx, TGO_E_INVALID, "null args");
    if (nseeds < 1 || nseeds > TGO_MAX_SOURCES) return fail(ctx, TGO_E_INVALID, "nseeds must be in [1, 64]");
    int rc = check_program(ctx, a->scope);
    if (rc) return rc;
    if (a->max_depth < 0) return fail(ctx, TGO_E_INVALID, "max_depth < 0");
    (void)hipSetDevice(ctx->opts.device);
    if ((rc = ms_alloc(ctx))) return rc;
    std::vector<int64_t> in(nseeds);
    for (int r = 0; r < nseeds; ++r) {
        if ((rc = resolve_seed(ctx, seeds[r], a->seed_is_dense, in[r]))) return rc;
        if (in[r] < 0) return fail(ctx, TGO_E_INVALID, "multi-source BFS needs seeds that are executed vertices");
    }
    if ((rc = run_ms_sweep(ctx, in.data(), nseeds, a->max_depth, a->scope, a->flags))) return rc;
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    const int64_t n = ctx->g.n;
    if (dist_out)
        for (int r = 0; r < nseeds; ++r) {
            HIP_TRY(k_ms_extract(ms_planes(ctx), s.ms_nplanes, s.ms_vis, ctx->g.perm, r, s.msg, n, st));
            HIP_TRY(hipMemcpyAsync(dist_out + static_cast<int64_t>(r) * n, s.msg, n * sizeof(int64_t),
                                   hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
    return TGO_OK;
}

int tgo_copy_multi_distances(tgo_ctx* ctx, int32_t source, int64_t* dist_out) {
    if (!ctx || !dist_out) return TGO_E_INVALID;
    Scratch& s = ctx->sc;
    if (!ctx->loaded || !s.ms_vis) return fail(ctx, TGO_E_STATE, "no multi-source BFS has run");
    if (source < 0 || source >= s.ms_nsrc) return fail(ctx, TGO_E_INVALID, "source index out of range");
    (void)hipSetDevice(ctx->opts.device);
    HIP_TRY(k_ms_extract(ms_planes(ctx), s.ms_nplanes, s.ms_vis, ctx->g.perm, source, s.msg, ctx->g.n, ctx->stream));
    HIP_TRY(hipMemcpyAsync(dist_out, s.msg, ctx->g.n * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return TGO_OK;
}

int tgo_multi_stats(tgo_ctx* ctx, int64_t* reached, int64_t* reached_entries) {
    if (!ctx) return TGO_E_INVALID;
    Scratch& s = ctx->sc;
    if (!ctx->loaded || !s.ms_vis) return fail(ctx, TGO_E_STATE, "no multi-source BFS has run");
    (void)hipSetDevice(ctx->opts.device);
    std::vector<unsigned long long> h(2 * TGO_MAX_SOURCES);
    HIP_TRY(hipMemcpy(h.data(), s.ms_stat, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (int r = 0; r < s.ms_nsrc; ++r) {
        if (reached) reached[r] = static_cast<int64_t>(h[r]);
        if (reached_entries) reached_entries[r] = static_cast<int64_t>(h[TGO_MAX_SOURCES + r]);
    }
    return TGO_OK;
}

}  // extern "C"
