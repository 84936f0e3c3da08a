// api_traverse.cpp — the single-source traversals of the C-ABI: direction-optimizing BFS,
// hop-bounded SSSP and delta-stepping (plain, light/heavy, and the device-driven loop).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include "ctx.hpp"

using namespace tgo;

namespace tgo {

// Direction-optimizing level loop for unit weights (Beamer et al., SC'12 heuristics).
int run_bfs(tgo_ctx* ctx, int64_t seed, int max_depth, int scope) {
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    const int64_t n = g.n, words = (n + 63) / 64 + 1;
    const View pull = pull_view(g, scope), push = push_view(g, scope);
    HIP_TRY(k_fill_i32(s.level, -1, n, st));
    HIP_TRY(hipMemsetAsync(s.vb, 0, words * 8, st));
    HIP_TRY(hipMemsetAsync(s.fb, 0, words * 8, st));
    int levels = 0;
    if (seed >= 0) {
        HIP_TRY(k_bfs_seed(push, s.level, s.vb, s.fb, s.q[0], s.qdeg, seed, st));
        HIP_TRY(k_level_prep(s.cnt, s.nb, words, s.qdeg + 1, st));   // level 0: counters, nb, scan tail
        int64_t qlen = 1;
        int cur = 0;
        bool bottom_up = false;
        // Beamer's switch thresholds; TGO_BFS_ALPHA / TGO_BFS_BETA override for tuning.  Round 5:
        // alpha 30 (bottom-up once the frontier's entries pass 1/30 of the unexplored ones) and
        // beta 5000 (top-down again only below n/5000 frontier vertices), against Beamer's 15 / 18:
        // hmean 301-318 -> 327-338 GTEPS over the 64 bench roots (profiles/r05ab_bfs_switch_ab.log).
        // The roots that gain have a level-1 frontier of ~2300 hubs with ~18 M entries, just under
        // mu / 15: top-down spent ~0.68 ms on that level, where the bottom-up finds nearly every
        // vertex's parent among the hubs within a few entries.
        static const double alpha = env_double("TGO_BFS_ALPHA", 30.0);
        static const double beta = env_double("TGO_BFS_BETA", 5000.0);
        static const bool trace = trace_on();
        // m_u: entries of unexplored vertices (push degrees); m_f: of the frontier.
        const int64_t total_push = push.nlists > 1 ? (g.out.nnz + g.in.nnz)
                                                   : (g.has_transpose ? g.push_t.nnz
                                                                      : (scope == TGO_SCOPE_IN_E ? g.in.nnz : g.out.nnz));
        int64_t mf = -1, mu = total_push;
        bool queued = true;         // q[cur] holds the frontier (bottom-up levels only count it)
        for (int L = 0; L < max_depth && qlen > 0; ++L) {
            if (mf < 0) {   // degree of the seed, through the mapped counter page (a copy and a
                            // stream synchronisation cost ~30 us before the first level)
                int64_t d = 0;
                if (int rc = read_words(ctx, s.qdeg, 1, &d)) return rc;
                mf = d;
                mu -= d;
            }
            if (!bottom_up && static_cast<double>(mf) > static_cast<double>(mu) / alpha) bottom_up = true;
            else if (bottom_up && static_cast<double>(qlen) < static_cast<double>(n) / beta) bottom_up = false;
            // every level starts with zero counters, a clear nb and qdeg[qlen] = 0: level_turn
            // at the end of the previous level (the first: the level_prep before the loop)
            if (!bottom_up && !queued) {    // after bottom-up levels: queue the frontier bitmap
                HIP_TRY(k_bfs_queue(push, g.n_active, s.fb, s.q[cur], s.qdeg, s.cnt, st));
                HIP_TRY(k_level_prep(s.cnt, nullptr, 0, nullptr, st));   // the queue's counts out
            }
            queued = !bottom_up;
            DevSpan span(st, "bfs.level", {"level", L}, {"bottom_up", bottom_up ? 1 : 0});
            if (bottom_up) {
                // words past n_active hold only entry-less vertices: nothing to find there
                HIP_TRY(k_bu_step(pull, push, g.n_active, s.fb, s.vb, s.nb, s.level, s.cnt, L + 1, st));
            } else {
                HIP_TRY(scan_exclusive_i64(s.cub_tmp, s.cub_bytes, s.qdeg, s.qpre, qlen + 1, st));
                // qdeg is reused for the next queue's degrees after the scan consumed it
                HIP_TRY(k_td_expand(push, s.q[cur], s.qpre, qlen, s.level, s.vb, s.nb, s.q[cur ^ 1], s.qdeg, s.cnt, L + 1, st));
            }
            span.end();
            // the counters to the host, then the next level's prep (fb, consumed, is its nb)
            const unsigned long long seq = ++s.pub_seq;
            HIP_TRY(k_level_turn(s.cnt, s.hcnt_dev, seq, s.fb, words, s.qdeg, st));
            int rc = wait_publish(ctx, seq);
            if (rc) return rc;
            qlen = static_cast<int64_t>(s.hcnt->qlen);
            mf = static_cast<int64_t>(s.hcnt->mf);
            mu -= mf;
            if (trace) std::fprintf(stderr, "[tgo] level %d %s -> next frontier %lld vertices, %lld entries (unexplored %lld)\n",
                                    L, bottom_up ? "BU" : "TD", (long long)qlen, (long long)mf, (long long)mu);
            std::swap(s.fb, s.nb);
            cur ^= 1;
            ++levels;
        }
    }
    HIP_TRY(k_level_to_dist(s.level, s.dist, n, st));
    trace_resolve(st);
    ctx->st.levels = levels;
    ctx->st.iterations = max_depth;   // the reference always runs iterations 0..maxDepth
    return TGO_OK;
}

}  // namespace tgo

namespace {

int run_sssp(tgo_ctx* ctx, int64_t seed, int max_depth, int scope, bool weighted) {
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    const int64_t n = g.n, words = (n + 63) / 64 + 1;
    const View push = push_view(g, scope);
    HIP_TRY(k_fill_i64(s.dist, INT64_MAX, n, st));
    HIP_TRY(hipMemsetAsync(s.vb, 0, words * 8, st));
    int levels = 0;
    if (seed >= 0) {
        HIP_TRY(k_sssp_seed(push, s.dist, s.msg, s.vb, s.q[0], s.qdeg, seed, st));
        int64_t qlen = 1;
        int cur = 0;
        for (int L = 0; L < max_depth && qlen > 0; ++L) {
            // counters, "improved this level" marks, scan tail
            DevSpan span(st, "sssp.superstep", {"superstep", L}, {"queue", qlen});
            HIP_TRY(k_level_prep(s.cnt, s.vb, words, s.qdeg + qlen, st));
            HIP_TRY(scan_exclusive_i64(s.cub_tmp, s.cub_bytes, s.qdeg, s.qpre, qlen + 1, st));
            int rc;
            HIP_TRY(k_sssp_relax(push, s.q[cur], s.qpre, qlen, s.msg, s.dist, s.vb, s.q[cur ^ 1], s.qdeg, s.cnt, weighted ? 1 : 0, st));
            span.end();
            rc = read_counters(ctx);
            if (rc) return rc;
            if (s.hcnt->err) return fail(ctx, TGO_E_PROGRAM,
                "vertex program failed: a traversed edge has no value for the weight property");
            qlen = static_cast<int64_t>(s.hcnt->qlen);
            // snapshot the improved vertices' distances: these are their messages
            if (qlen > 0) HIP_TRY(k_sssp_commit(s.q[cur ^ 1], qlen, s.dist, s.msg, s.vb, st));
            cur ^= 1;
            ++levels;
        }
    }
    HIP_TRY(k_dist_finalize(s.dist, n, st));
    trace_resolve(st);
    ctx->st.levels = levels;
    ctx->st.iterations = max_depth;
    return TGO_OK;
}

}  // namespace

namespace tgo {

// Bucket width when the caller passes 0: TGO_DELTA, else a quarter of the mean edge weight
// (RMAT scale 24, weights 1..255: 39 ms at width 32 against 49 ms at 256 and 43 ms at one
// bucket per 2048 — profiles/r01_sssp_delta_sweep.log).
int64_t default_delta(const DevGraph& g, bool weighted) {
    const double env = env_double("TGO_DELTA", 0.0);
    if (env > 0) return static_cast<int64_t>(env);
    return std::max<int64_t>(1, static_cast<int64_t>(weighted ? 0.25 * g.mean_weight : 1.0));
}

}  // namespace tgo

namespace {

// The light/heavy loop driven from the device (delta_loop.hip): the host enqueues steps in
// batches and reads the loop state once per batch (dist, pending and member bitmaps are
// initialised by the caller).
int run_delta_device(tgo_ctx* ctx, int64_t seed, int64_t delta, bool force_scan) {
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    const int64_t n = g.n;
    static const bool trace = trace_on();
    static const int batch = static_cast<int>(std::max(1.0, env_double("TGO_DS_BATCH", 8.0)));
    // Piles (binned loop, TGO_DS_BINS=0 turns them off): a relaxation from bucket k reaches at
    // most bucket k + 1 + (max_weight - 1) / delta, so that many + 1 piles in a ring hold every
    // pending vertex; wider weight ranges keep the bitmap-scan loop.
    static const bool bins_env = env_double("TGO_DS_BINS", 1.0) != 0.0;
    const bool bins_on = tuned_on(ctx->tune.i64(TGO_TUNE_DS_BINS), bins_env);
    const int64_t reach = 2 + (std::max<int64_t>(g.max_weight, 1) - 1) / delta;
    const int nbins = (bins_on && !force_scan && reach <= kDsMaxBins) ? static_cast<int>(reach) : 0;
    // TGO_DS_DONE=1: the relax skips the distance read of done targets (measured neutral at
    // RMAT-24: the largest phases come before most vertices are done); TGO_DS_PILE_SCAN: piles
    // above this fraction of n are extracted by the bitmap scan
    static const bool done_env = env_double("TGO_DS_DONE", 0.0) != 0.0;
    const bool done_filter = tuned_on(ctx->tune.i64(TGO_TUNE_DS_DONE), done_env);
    static const double pile_scan = env_double("TGO_DS_PILE_SCAN", 1.0 / 16.0);
    const int64_t scan_above = static_cast<int64_t>(pile_scan * static_cast<double>(n));
    if (!s.ds_loop) {
        for (int b = 0; b < 2; ++b) {
            HIP_TRY(dev_alloc(ctx, s.ds_q[b], 2 * n + 2));
            HIP_TRY(dev_alloc(ctx, s.ds_qp[b], 2 * n + 2));
        }
        HIP_TRY(dev_alloc(ctx, s.ds_loop, 1));
        ctx->st.device_bytes = ctx->dev_bytes;
    }
    const int64_t cap_set = ctx->tune.i64(TGO_TUNE_DS_PILE_CAP);
    const int64_t cap = cap_set > 0 ? cap_set : std::max<int64_t>(n, 1024);
    if (nbins && s.ds_pile && s.ds_pile_cap != cap) {
        dev_free(ctx, s.ds_pile, kDsMaxBins * s.ds_pile_cap);
        s.ds_pile_cap = 0;
    }
    if (nbins && !s.ds_pile) {
        // a pile holds up to n appends per bucket (more drop to the bitmap scan of that bucket)
        s.ds_pile_cap = cap;
        HIP_TRY(dev_alloc(ctx, s.ds_pile, kDsMaxBins * s.ds_pile_cap));
        if (!s.ds_mlist) HIP_TRY(dev_alloc(ctx, s.ds_mlist, n + 1));
        if (!s.ds_done) HIP_TRY(dev_alloc(ctx, s.ds_done, (n + 63) / 64 + 1));
        ctx->st.device_bytes = ctx->dev_bytes;
    }
    if (nbins) HIP_TRY(hipMemsetAsync(s.ds_done, 0, ((n + 63) / 64 + 1) * 8, st));
    // Pull form (TGO_DS_PULL = members as a fraction of n, 0 = off): a finished bucket with at
    // least that many members has its heavy entries pulled by the vertices that can still
    // improve (delta_loop.hip ds_pull_heavy) instead of pushed entry by entry.
    static const double pull_env = env_double("TGO_DS_PULL", 0.0);
    const double pull_frac = tuned(ctx->tune.f64(TGO_TUNE_DS_PULL), pull_env);
    DsPull pull{};
    if (nbins && pull_frac > 0) {
        const int64_t words = (n + 63) / 64 + 1;
        for (int b = 0; b < 2; ++b) {
            if (!s.ds_pm[b]) HIP_TRY(dev_alloc(ctx, s.ds_pm[b], words));
            if (!s.ds_pl[b]) HIP_TRY(dev_alloc(ctx, s.ds_pl[b], n + 1));
            HIP_TRY(hipMemsetAsync(s.ds_pm[b], 0, words * 8, st));
            pull.pm[b] = s.ds_pm[b];
            pull.pl[b] = s.ds_pl[b];
        }
        ctx->st.device_bytes = ctx->dev_bytes;
        pull.view = pull_view(g, g.scope);
        pull.n_active = g.n_active > 0 ? std::min<int64_t>(g.n_active, n) : n;
        pull.min_members = std::max<int64_t>(1, static_cast<int64_t>(pull_frac * static_cast<double>(n)));
    }
    HIP_TRY(k_ds_loop_seed(g.push_ws, s.ds_light, s.dist, s.ds_q[0], s.ds_qp[0], s.ds_loop, seed, delta, st));
    DsLoop h{};
    int cur = 0;
    // Small steps (TGO_TUNE_DS_SMALL / TGO_DS_SMALL, default off; delta_loop.hip ds_small_steps):
    // the tiny steps run in one block inside one launch.  The binned loop without the done
    // filter or pulls.  Off by default: 12.6 -> 13.8 ms per RMAT-24 source
    // (profiles/r05ss1_sssp_small_ab.log) — a tiny step is a chain of dependent memory
    // round trips either way, and one block pays them with fewer loads in flight.
    static const bool small_env = env_double("TGO_DS_SMALL", 0.0) != 0.0;
    const bool small_on = tuned_on(ctx->tune.i64(TGO_TUNE_DS_SMALL), small_env);
    const bool small = small_on && nbins && !done_filter && pull.min_members == 0;
    // every step either relaxes a non-empty queue or extracts (at most one extraction in a row
    // takes nothing); a run needs far fewer than 4n + 64 steps — the bound only stops a bug
    const int64_t max_steps = 4 * n + 64;
    // Pipelined stop checks (TGO_DS_PIPE, default on): each batch ends with a publish of the
    // stop flags to host-mapped words, and the host checks batch k while batch k + 1 runs (a
    // batch after the stop only runs steps that find nothing to do).  The stream no longer
    // drains at every check: one SSSP run had ~12 drains of ~60 us (profiles/r04v_sssp_timeline.txt).
    static const bool pipe = env_double("TGO_DS_PIPE", 1.0) != 0.0;
    if (pipe) {
        unsigned long long pending = 0;                       // publish to check next (0: none)
        bool stop = false;
        for (int64_t steps = 0; !stop;) {
            DevSpan span(st, "sssp.delta_steps", {"first_step", steps}, {"steps", batch});
            for (int k = 0; k < batch; ++k) {
                if (small)
                    HIP_TRY(k_ds_loop_step_small(g.push_ws, s.ds_light, s.vb, s.ds_member, n, s.dist, s.msg, s.ds_q,
                                                 s.ds_qp, s.ds_loop, delta, nbins, s.ds_pile, s.ds_pile_cap,
                                                 s.ds_mlist, s.ds_done, scan_above, st));
                else if (nbins)
                    HIP_TRY(k_ds_loop_step_bins(g.push_ws, s.ds_light, s.vb, s.ds_member, n, s.dist, s.msg, s.ds_q,
                                                s.ds_qp, s.ds_loop, cur, delta, nbins, s.ds_pile, s.ds_pile_cap,
                                                s.ds_mlist, s.ds_done, done_filter, scan_above, pull, st));
                else
                    HIP_TRY(k_ds_loop_step(g.push_ws, s.ds_light, s.vb, s.ds_member, n, s.dist, s.msg, s.ds_q, s.ds_qp,
                                           s.ds_loop, cur, delta, st));
                cur ^= 1;
            }
            steps += batch;
            span.end();
            const unsigned long long seq = ++s.pub_seq;
            HIP_TRY(k_ds_publish(s.ds_loop, s.hcnt_dev, seq, st));
            if (pending) {
                if (int rc = wait_publish(ctx, pending, true)) return rc;
                const volatile unsigned long long* hw = host_words(ctx);
                if (hw[1]) return fail(ctx, TGO_E_PROGRAM, "vertex program failed: a traversed edge has no value for the weight property");
                stop = hw[0] != 0 || hw[2] != 0;
            }
            pending = seq;
            if (!stop && steps > max_steps) return fail(ctx, TGO_E_HIP, "delta-stepping: the device loop did not converge");
        }
        HIP_TRY(hipMemcpyAsync(&h, s.ds_loop, sizeof(DsLoop), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (h.err) return fail(ctx, TGO_E_PROGRAM, "vertex program failed: a traversed edge has no value for the weight property");
    }
    for (int64_t steps = 0; !pipe;) {
        DevSpan span(st, "sssp.delta_steps", {"first_step", steps}, {"steps", batch});
        for (int k = 0; k < batch; ++k) {
            if (small)
                HIP_TRY(k_ds_loop_step_small(g.push_ws, s.ds_light, s.vb, s.ds_member, n, s.dist, s.msg, s.ds_q,
                                             s.ds_qp, s.ds_loop, delta, nbins, s.ds_pile, s.ds_pile_cap, s.ds_mlist,
                                             s.ds_done, scan_above, st));
            else if (nbins)
                HIP_TRY(k_ds_loop_step_bins(g.push_ws, s.ds_light, s.vb, s.ds_member, n, s.dist, s.msg, s.ds_q, s.ds_qp,
                                            s.ds_loop, cur, delta, nbins, s.ds_pile, s.ds_pile_cap, s.ds_mlist,
                                            s.ds_done, done_filter, scan_above, pull, st));
            else
                HIP_TRY(k_ds_loop_step(g.push_ws, s.ds_light, s.vb, s.ds_member, n, s.dist, s.msg, s.ds_q, s.ds_qp,
                                       s.ds_loop, cur, delta, st));
            cur ^= 1;
        }
        steps += batch;
        span.end();
        HIP_TRY(hipMemcpyAsync(&h, s.ds_loop, sizeof(DsLoop), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (h.err) return fail(ctx, TGO_E_PROGRAM, "vertex program failed: a traversed edge has no value for the weight property");
        if (h.spill) break;
        if (h.done) break;
        if (steps > max_steps) return fail(ctx, TGO_E_HIP, "delta-stepping: the device loop did not converge");
    }
    if (h.spill) {
        // a relaxation reached past the piles (the weight bound was wrong): start again with
        // the bitmap-scan loop (dist, pending and member state re-initialised by the caller)
        trace_resolve(st);
        return TGO_E_STATE;
    }
    HIP_TRY(k_dist_finalize(s.dist, n, st));
    trace_resolve(st);
    if (trace)
        std::fprintf(stderr, "[tgo] delta %lld (device loop, %d piles): %llu phases, %llu buckets, %llu extractions "
                     "(%llu bitmap scans), %llu entries relaxed\n", (long long)delta, nbins, h.phases, h.buckets,
                     h.extractions, h.full_scans, h.relaxed);
    ctx->st.levels = static_cast<int32_t>(h.phases);
    ctx->st.relaxed_entries = static_cast<int64_t>(h.relaxed);
    return TGO_OK;
}

// Light/heavy delta-stepping (delta.hip, weighted one-GPU loads): a bucket's phases relax
// light entries only; when its near queue runs dry the bucket's members relax their heavy
// entries once; then the threshold moves to the next non-empty bucket.
int run_delta_split(tgo_ctx* ctx, int64_t seed, int64_t delta) {
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    const int64_t n = g.n, words = (n + 63) / 64 + 1;
    static const bool trace = trace_on();
    if (!s.ds_light) {
        HIP_TRY(dev_alloc(ctx, s.ds_light, n + 1));
        HIP_TRY(dev_alloc(ctx, s.ds_member, words));
        ctx->st.device_bytes = ctx->dev_bytes;
    }
    if (s.ds_light_delta != delta) {
        HIP_TRY(k_ds_light_end(g.push_ws, delta, n, s.ds_light, st));
        s.ds_light_delta = delta;
    }
    HIP_TRY(k_fill_i64(s.dist, INT64_MAX, n, st));
    HIP_TRY(hipMemsetAsync(s.vb, 0, words * 8, st));        // pending bitmap
    HIP_TRY(hipMemsetAsync(s.ds_member, 0, words * 8, st));
    // device-driven steps (delta_loop.hip) unless TGO_DS_HOSTLOOP=1 or the packed queue
    // counters could overflow: a queue holds up to 2n + 2 takes (a light and a heavy take per
    // vertex, ds_q / ds_qp are sized for that) in the count field above kDsCountShift, and up
    // to nnz entries below it
    static const bool host_loop = env_double("TGO_DS_HOSTLOOP", 0.0) != 0.0;
    constexpr int64_t kDsMaxCount = int64_t(1) << (64 - kDsCountShift);
    static_assert(kDsCountShift > 32 && kDsCountShift < 64, "queue counter layout");
    if (!host_loop && seed >= 0 && 2 * n + 2 < kDsMaxCount && g.push_ws.nnz < (int64_t(1) << kDsCountShift)) {
        const int rc = run_delta_device(ctx, seed, delta, false);
        if (rc != TGO_E_STATE) return rc;
        HIP_TRY(k_fill_i64(s.dist, INT64_MAX, n, st));
        HIP_TRY(hipMemsetAsync(s.vb, 0, words * 8, st));
        HIP_TRY(hipMemsetAsync(s.ds_member, 0, words * 8, st));
        return run_delta_device(ctx, seed, delta, true);
    }
    int phases = 0, buckets = 0;
    int64_t relaxed = 0;
    // TGO_DS_TRACE=1: one line per phase (queue, entries, wall time since the previous phase)
    static const bool phase_trace = env_double("TGO_DS_TRACE", 0.0) != 0.0;
    auto t_phase = std::chrono::steady_clock::now();
    if (seed >= 0) {
        HIP_TRY(k_ds_seed_ws(g.push_ws, s.ds_light, s.dist, s.q[0], s.qdeg, seed, st));
        int64_t qlen = 1, thr = delta;
        int cur = 0;
        for (;;) {
            if (qlen == 0) {
                // bucket settled: next near queue + the members' heavy entries, one extraction
                HIP_TRY(hipMemsetAsync(s.cnt, 0, sizeof(Counters), st));
                HIP_TRY(hipMemsetAsync(&s.cnt->red[0], 0x7F, sizeof(unsigned long long), st));   // ~INT64_MAX
                HIP_TRY(k_ds_pending_min_ws(s.vb, s.ds_member, words, s.dist, s.cnt, st));
                if (int rc = read_counters(ctx)) return rc;
                const int64_t pending = static_cast<int64_t>(s.hcnt->red[1]);
                const int64_t members = static_cast<int64_t>(s.hcnt->red2);
                if (pending == 0 && members == 0) break;        // converged
                if (pending > 0) {
                    const int64_t mn = static_cast<int64_t>(s.hcnt->red[0]);
                    if (mn >= thr) thr = (mn / delta + 1) * delta;
                    ++buckets;
                }
                HIP_TRY(hipMemsetAsync(s.cnt, 0, sizeof(Counters), st));
                HIP_TRY(k_ds_extract_ws(g.push_ws, s.ds_light, s.vb, s.ds_member, n, s.dist, thr, s.q[cur], s.qdeg, s.cnt,
                                        st));
                if (int rc = read_counters(ctx)) return rc;
                qlen = static_cast<int64_t>(s.hcnt->qlen);
                if (trace) std::fprintf(stderr, "[tgo] delta bucket thr %lld: %lld pending, %lld members, %lld queued\n",
                                        (long long)thr, (long long)pending, (long long)members, (long long)qlen);
                if (qlen == 0) {
                    if (pending > 0) return fail(ctx, TGO_E_HIP, "delta-stepping: extraction found no vertex below the threshold");
                    continue;                                   // members without heavy entries
                }
            }
            HIP_TRY(k_ds_commit_ws(s.q[cur], qlen, s.dist, s.msg, s.vb, s.ds_member, s.qdeg, s.cnt, st));
            HIP_TRY(scan_exclusive_i64(s.cub_tmp, s.cub_bytes, s.qdeg, s.qpre, qlen + 1, st));   // tail zeroed by commit
            HIP_TRY(k_ds_relax_ws(g.push_ws, s.ds_light, s.q[cur], s.qpre, qlen, s.msg, s.dist, s.vb, s.q[cur ^ 1], s.qdeg,
                                  s.cnt, thr, st));
            if (int rc = read_counters(ctx)) return rc;
            if (s.hcnt->err) return fail(ctx, TGO_E_PROGRAM,
                "vertex program failed: a traversed edge has no value for the weight property");
            relaxed += static_cast<int64_t>(s.hcnt->red[1]);
            if (phase_trace) {
                const auto now = std::chrono::steady_clock::now();
                std::fprintf(stderr, "[tgo] ds phase %d thr %lld: queue %lld, entries %llu, next %llu, %.1f us\n", phases,
                             (long long)thr, (long long)qlen, s.hcnt->red[1], s.hcnt->qlen,
                             std::chrono::duration<double, std::micro>(now - t_phase).count());
                t_phase = now;
            }
            qlen = static_cast<int64_t>(s.hcnt->qlen);
            cur ^= 1;
            ++phases;
        }
    }
    HIP_TRY(k_dist_finalize(s.dist, n, st));
    if (trace) std::fprintf(stderr, "[tgo] delta %lld (light/heavy): %d phases, %d buckets, %lld entries relaxed\n",
                            (long long)delta, phases, buckets, (long long)relaxed);
    ctx->st.levels = phases;
    ctx->st.relaxed_entries = relaxed;
    return TGO_OK;
}

// Delta-stepping (delta.hip): converged distances, near queue relaxed phase by phase,
// bucket threshold advanced from the minimum pending distance when the queue runs dry.
int run_delta(tgo_ctx* ctx, int64_t seed, int scope, bool weighted, int64_t delta) {
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    const int64_t n = g.n, words = (n + 63) / 64 + 1;
    const View push = push_view(g, scope);
    static const bool trace = trace_on();
    if (delta <= 0) delta = default_delta(g, weighted);
    if (weighted && g.push_ws_ready && scope == g.scope) return run_delta_split(ctx, seed, delta);
    HIP_TRY(k_fill_i64(s.dist, INT64_MAX, n, st));
    HIP_TRY(hipMemsetAsync(s.vb, 0, words * 8, st));        // pending bitmap
    int phases = 0, buckets = 0;
    int64_t relaxed = 0;
    if (seed >= 0) {
        HIP_TRY(k_ds_seed(push, s.dist, s.q[0], s.qdeg, seed, st));
        int64_t qlen = 1, thr = delta;
        int cur = 0;
        for (;;) {
            if (qlen == 0) {
                HIP_TRY(hipMemsetAsync(s.cnt, 0, sizeof(Counters), st));
                HIP_TRY(hipMemsetAsync(&s.cnt->red[0], 0x7F, sizeof(unsigned long long), st));   // ~INT64_MAX
                HIP_TRY(k_ds_pending_min(s.vb, words, s.dist, s.cnt, st));
                if (int rc = read_counters(ctx)) return rc;
                if (s.hcnt->red[1] == 0) break;                 // nothing pending: converged
                const int64_t mn = static_cast<int64_t>(s.hcnt->red[0]);
                if (mn >= thr) thr = (mn / delta + 1) * delta;
                ++buckets;
                HIP_TRY(hipMemsetAsync(s.cnt, 0, sizeof(Counters), st));
                HIP_TRY(k_ds_extract(push, s.vb, n, s.dist, thr, s.q[cur], s.qdeg, s.cnt, st));
                if (int rc = read_counters(ctx)) return rc;
                qlen = static_cast<int64_t>(s.hcnt->qlen);
                if (trace) std::fprintf(stderr, "[tgo] delta bucket thr %lld: min pending %lld, %llu pending, %lld queued\n",
                                        (long long)thr, (long long)mn, s.hcnt->red[1], (long long)qlen);
                if (qlen == 0) return fail(ctx, TGO_E_HIP, "delta-stepping: extraction found no vertex below the threshold");
            }
            HIP_TRY(k_ds_commit(s.q[cur], qlen, s.dist, s.msg, s.vb, st));
            if (int rc = scan_frontier(ctx, qlen)) return rc;
            HIP_TRY(hipMemsetAsync(s.cnt, 0, sizeof(Counters), st));
            HIP_TRY(k_ds_relax(push, s.q[cur], s.qpre, qlen, s.msg, s.dist, s.vb, s.q[cur ^ 1], s.qdeg, s.cnt,
                               weighted ? 1 : 0, thr, st));
            if (int rc = read_counters(ctx)) return rc;
            if (s.hcnt->err) return fail(ctx, TGO_E_PROGRAM,
                "vertex program failed: a traversed edge has no value for the weight property");
            relaxed += static_cast<int64_t>(s.hcnt->red[1]);      // qpre[qlen], set by ds_relax
            qlen = static_cast<int64_t>(s.hcnt->qlen);
            cur ^= 1;
            ++phases;
        }
    }
    HIP_TRY(k_dist_finalize(s.dist, n, st));
    if (trace) std::fprintf(stderr, "[tgo] delta %lld: %d phases, %d buckets, %lld entries relaxed\n",
                            (long long)delta, phases, buckets, (long long)relaxed);
    ctx->st.levels = phases;
    ctx->st.relaxed_entries = relaxed;
    return TGO_OK;
}

int finish_distance_program(tgo_ctx* ctx, int scope, int flags, int64_t* dist_out) {
    // not program_end: the loops set the iterations, and run_bfs, run_sssp and the device delta
    // loop resolve the trace themselves (run_delta's scan loop never does: the reason is unknown)
    HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
    HIP_TRY(hipEventSynchronize(ctx->ev1));
    int rc = program_elapsed(ctx);
    if (rc) return rc;
    if (flags & TGO_FLAG_STATS) {
        int64_t reached[2];
        if ((rc = reach_stats(ctx, scope, reached))) return rc;
        ctx->st.reached = reached[0];
        ctx->st.reached_entries = reached[1];
    }
    if (dist_out && (rc = rows_out(ctx, ctx->sc.dist, dist_out))) return rc;
    publish_result(ctx, TGO_RESULT_DISTANCE, ResultSource{ctx->sc.dist, nullptr});
    return TGO_OK;
}

}  // namespace

extern "C" {

int tgo_bfs(tgo_ctx* ctx, const tgo_bfs_args* a, int64_t* dist_out) {
    int rc = program_open(ctx, a);
    if (rc) return rc;
    if (a->max_depth < 0) return fail(ctx, TGO_E_INVALID, "max_depth < 0");
    (void)hipSetDevice(ctx->opts.device);
    int64_t seed;
    if ((rc = resolve_seed(ctx, a->seed, a->seed_is_dense, seed))) return rc;
    HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
    if ((rc = run_bfs(ctx, seed, a->max_depth, a->scope))) return rc;
    return finish_distance_program(ctx, a->scope, a->flags, dist_out);
}

int tgo_sssp(tgo_ctx* ctx, const tgo_sssp_args* a, int64_t* dist_out) {
    int rc = program_open(ctx, a);
    if (rc) return rc;
    if (a->max_depth < 0) return fail(ctx, TGO_E_INVALID, "max_depth < 0");
    if (a->mode != TGO_SSSP_HOP_BOUNDED && a->mode != TGO_SSSP_DELTA) return fail(ctx, TGO_E_INVALID, "invalid mode");
    if (ctx->g.has_weight && ctx->g.weight_dt != TGO_DT_INTEGER)
        return fail(ctx, TGO_E_UNSUPPORTED, "ShortestDistanceVertexProgram reads edge.<Integer>value(weight): the weight "
                                            "property is not an Integer key (ClassCastException in the reference)");
    (void)hipSetDevice(ctx->opts.device);
    int64_t seed;
    if ((rc = resolve_seed(ctx, a->seed, a->seed_is_dense, seed))) return rc;
    HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
    ctx->st.relaxed_entries = 0;
    if (a->mode == TGO_SSSP_DELTA) {
        // converged distances (== the reference's whenever maxDepth >= the hop count of
        // every shortest path); max_depth only sets the reported iteration count
        if (ctx->g.has_weight && ctx->g.min_weight < 0)
            return fail(ctx, TGO_E_INVALID, "DELTA mode needs non-negative weights");
        if ((rc = run_delta(ctx, seed, a->scope, ctx->g.has_weight, a->delta))) return rc;
        ctx->st.iterations = a->max_depth;
    } else {
        if ((rc = run_sssp(ctx, seed, a->max_depth, a->scope, ctx->g.has_weight))) return rc;
    }
    return finish_distance_program(ctx, a->scope, a->flags, dist_out);
}

// PageRank's ranks are fetched through this too, from the same scratch (the bits of the doubles).  Every
// other program that publishes through sc.dist (labels, counts, truss numbers) has a tgo_copy_* of its own.
int tgo_copy_distances(tgo_ctx* ctx, int64_t* dist_out) {
    if (!ctx || !dist_out) return TGO_E_INVALID;
    if (!ctx->loaded) return fail(ctx, TGO_E_STATE, "no graph loaded");
    if (ctx->res_kind != TGO_RESULT_DISTANCE && ctx->res_kind != TGO_RESULT_PAGERANK)
        return fail(ctx, TGO_E_STATE, "tgo_bfs / tgo_sssp / tgo_pagerank is not the last program run on this ctx");
    (void)hipSetDevice(ctx->opts.device);
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return rows_out(ctx, ctx->sc.dist, dist_out);
}

}  // extern "C"
