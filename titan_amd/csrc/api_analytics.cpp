// api_analytics.cpp — the analytics of a bothE load: connected components, triangles, k-core,
// strongly connected components, betweenness centrality, peer-pressure clustering; and of any load:
// closeness / harmonic centrality.
#include <climits>
#include "ctx.hpp"

using namespace tgo;

extern "C" {

// ------------------------------------------------------------------ connected components
// Weakly connected components (cc.hip).  Device arrays: parent = sc.level (int32), the per-root
// minimum = sc.vec[0] (as int64), labels in internal order = sc.dist, row-order staging = sc.msg.
// "changed" / "roots" words: Counters::qlen / red[0], read through the published mirror.
static int cc_word(tgo_ctx* ctx, bool roots, unsigned long long& out) {
    if (int rc = read_counters(ctx)) return rc;
    out = roots ? ctx->sc.hcnt->red[0] : ctx->sc.hcnt->qlen;
    return TGO_OK;
}

// Flatten the parent trees: pointer-jumping launches until one finds every vertex under a root.
static int cc_compress(tgo_ctx* ctx, int32_t& rounds) {
    Scratch& s = ctx->sc;
    for (;;) {
        HIP_TRY(k_level_prep(s.cnt, nullptr, 0, nullptr, ctx->stream));
        {
            DevSpan span(ctx->stream, "components.jump", {"round", rounds});
            HIP_TRY(k_cc_jump(s.level, ctx->g.n, &s.cnt->qlen, ctx->stream));
        }
        ++rounds;
        unsigned long long changed = 0;
        if (int rc = cc_word(ctx, false, changed)) return rc;
        if (!changed) return TGO_OK;
    }
}

// g.cc_tid = the Titan id of every internal index: once per graph (tgo_components and tgo_scc label with it).
static int titan_ids_by_index(tgo_ctx* ctx) {
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    const int64_t n = g.n;
    if (g.cc_tid) return TGO_OK;
    HIP_TRY(dev_alloc(ctx, g.cc_tid, n));
    ctx->st.device_bytes = ctx->dev_bytes;
    HIP_TRY(hipMemcpyAsync(s.msg, ctx->titan_id.data(), n * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(k_cc_scatter_ids(s.msg, g.perm, g.cc_tid, n, st));
    HIP_TRY(hipStreamSynchronize(st));
    return TGO_OK;
}

int tgo_components(tgo_ctx* ctx, const tgo_cc_args* a, int64_t* label_out, tgo_cc_info* info) {
    int rc = bothE_program_check(ctx, a, "tgo_cc_args", "connected components run", nullptr);
    if (rc) return rc;
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    const int64_t n = g.n;
    int64_t* const label = s.dist;
    if ((rc = titan_ids_by_index(ctx))) return rc;
    HIP_TRY(hipEventRecord(ctx->ev0, st));
    int32_t rounds = 0;
    const int path = g.has_transpose ? TGO_CC_PROPAGATE : TGO_CC_HOOK;
    unsigned long long components = 0;
    if (path == TGO_CC_HOOK) {
        // every edge sits once in the OUT lists; the first entries are hooked and flattened
        // first so that the bulk of the entries meets short trees
        int32_t* const parent = s.level;
        int64_t* const minid = reinterpret_cast<int64_t*>(s.vec[0]);
        HIP_TRY(k_cc_init(parent, n, st));
        {
            DevSpan span(st, "components.hook_sample");
            HIP_TRY(k_cc_hook(g.out, n, 0, 2, parent, st));
            HIP_TRY(k_cc_hook(g.in, n, 0, 1, parent, st));
        }
        rounds += 2;
        if ((rc = cc_compress(ctx, rounds))) return rc;
        {
            DevSpan span(st, "components.hook_rest");
            HIP_TRY(k_cc_hook(g.out, n, 2, -1, parent, st));
        }
        ++rounds;
        if ((rc = cc_compress(ctx, rounds))) return rc;
        DevSpan span(st, "components.label");
        HIP_TRY(k_fill_i64(minid, INT64_MAX, n, st));
        HIP_TRY(k_level_prep(s.cnt, nullptr, 0, nullptr, st));
        HIP_TRY(k_cc_min_id(parent, g.cc_tid, n, minid, st));
        HIP_TRY(k_cc_label(parent, minid, n, label, &s.cnt->red[0], st));
        span.end();
        if ((rc = cc_word(ctx, true, components))) return rc;
    } else {
        const View pull = pull_view(g, TGO_SCOPE_BOTH_E);
        HIP_TRY(hipMemcpyAsync(label, g.cc_tid, n * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
        for (;;) {
            HIP_TRY(k_level_prep(s.cnt, nullptr, 0, nullptr, st));
            {
                DevSpan span(st, "components.pull_round", {"round", rounds});
                HIP_TRY(k_cc_pull_round(pull, n, label, &s.cnt->qlen, st));
            }
            ++rounds;
            unsigned long long changed = 0;
            if ((rc = cc_word(ctx, false, changed))) return rc;
            if (!changed) break;
        }
        HIP_TRY(k_level_prep(s.cnt, nullptr, 0, nullptr, st));
        HIP_TRY(k_cc_count_own(label, g.cc_tid, n, &s.cnt->red[0], st));
        if ((rc = cc_word(ctx, true, components))) return rc;
    }
    if ((rc = program_end(ctx, rounds))) return rc;
    if (info) *info = tgo_cc_info{static_cast<int64_t>(components), rounds, path};
    if (label_out && (rc = rows_out(ctx, label, label_out))) return rc;
    publish_result(ctx, TGO_RESULT_COMPONENT, ResultSource{label, nullptr});
    return TGO_OK;
}

int tgo_copy_components(tgo_ctx* ctx, int64_t* label_out) {
    if (!ctx || !label_out) return TGO_E_INVALID;
    if (int rc = last_result_check(ctx, TGO_RESULT_COMPONENT, "tgo_components")) return rc;
    // (unlike tgo_copy_triangles / tgo_copy_cores, no hipSetDevice first: the reason is unknown)
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return rows_out(ctx, ctx->sc.dist, label_out);
}

// ------------------------------------------------------------------ triangles
// Triangle counting (tri.hip).  The forward lists, the degrees and the totals' words live with the
// graph (dev_alloc: released with it); per run: counts in internal order = sc.dist, coefficients =
// sc.vec[0], the block and wave kernels' row queues = sc.level and sc.q[0], row-order staging = sc.msg.
// Defaults of TGO_TUNE_TRI_WAVE_ROW / _BLOCK_ROW (DESIGN.md 4.5 has the sweep).
constexpr int64_t kTriWaveRow = 8, kTriBlockRow = 8;

static int tri_forward_lists(tgo_ctx* ctx) {
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    const int64_t n = g.n;
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
    ctx->st.device_bytes = ctx->dev_bytes;
    return TGO_OK;
}

int tgo_triangles(tgo_ctx* ctx, const tgo_tri_args* a, int64_t* tri_out, tgo_tri_info* info) {
    int rc = bothE_program_check(ctx, a, "tgo_tri_args", "triangles are counted", "triangles");
    if (rc) return rc;
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    const int64_t n = g.n;
    if (!g.tri_fadj && (rc = tri_forward_lists(ctx))) return rc;
    int64_t* const tri = s.dist;
    double* const lcc = s.vec[0];
    HIP_TRY(hipEventRecord(ctx->ev0, st));
    HIP_TRY(k_fill_i64(tri, 0, n, st));
    HIP_TRY(hipMemsetAsync(g.tri_tot + 1, 0, 15 * sizeof(unsigned long long), st));
    {
        DevSpan span(st, "triangles.count", {"forward_entries", g.tri_fnnz}, {"max_forward", g.tri_max_fwd});
        HIP_TRY(k_tri_count(g.tri_foff, g.tri_fadj, n, tuned(ctx->tri_wave_row, kTriWaveRow),
                            tuned(ctx->tri_block_row, kTriBlockRow), g.tri_max_fwd, tri, s.level,
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
    int rc = last_result_check(ctx, TGO_RESULT_TRIANGLES, "tgo_triangles");
    if (rc) return rc;
    (void)hipSetDevice(ctx->opts.device);
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    // each copy-out finishes before the next reuses sc.msg
    if (tri_out && (rc = rows_out(ctx, ctx->sc.dist, tri_out))) return rc;
    if (deg_out && (rc = rows_out(ctx, ctx->g.tri_deg, deg_out))) return rc;
    if (lcc_out && (rc = rows_out(ctx, ctx->sc.vec[0], lcc_out))) return rc;
    return TGO_OK;
}

// ------------------------------------------------------------------ k-core decomposition
// k-core (core.hip).  The backward lists and the totals' words live with the graph (dev_alloc:
// released with it), beside the forward lists and degrees they share with tgo_triangles.  Per run:
// working degrees (int32, the core numbers at the end) = sc.level, cores in internal order =
// sc.dist, the alive lists = sc.q[0] / sc.q[1], the level queues = sc.vec[0] / sc.vec[1] (as
// int32), row-order staging = sc.msg.  Level control: Counters through publish_turn / wait_publish.
// Defaults of TGO_TUNE_CORE_WAVE_ROW / _TAIL / _LDS_QUEUE: DESIGN.md 4.6 has the sweep they come from.
constexpr int64_t kCoreWaveRow = 64, kCoreTail = 1024, kCoreLdsQueue = 256;

static int core_backward_lists(tgo_ctx* ctx) {
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    const int64_t n = g.n;
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
    ctx->st.device_bytes = ctx->dev_bytes;
    return TGO_OK;
}

// One publish of the level counters, which are zero again afterwards.
static int core_turn(tgo_ctx* ctx) {
    Scratch& s = ctx->sc;
    const unsigned long long seq = ++s.pub_seq;
    HIP_TRY(k_publish_turn(s.cnt, s.hcnt_dev, seq, nullptr, ctx->stream));
    int rc = wait_publish(ctx, seq);
    if (rc) return rc;
    if (s.hcnt->err) return fail(ctx, TGO_E_HIP, "k-core peel: a queue overflowed (inconsistent lists)");
    return TGO_OK;
}

// The peel: deg (a copy of d(v)) ends as the core numbers.  Out: levels, peel launches, the largest
// core number and the vertices peeled at it.
static int core_peel_levels(tgo_ctx* ctx, int32_t* deg, int32_t& levels, int32_t& rounds, int64_t& top,
                            int64_t& innermost) {
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    const int64_t n = g.n;
    const CoreView lists{g.tri_foff, g.tri_fadj, g.core_boff, g.core_badj};
    const int64_t wave_row = tuned(ctx->core_wave_row, kCoreWaveRow);
    const int64_t tail = std::min<int64_t>(tuned(ctx->core_tail, kCoreTail), kCoreQueue);
    const int64_t lds_cap = tuned(ctx->core_lds_queue, kCoreLdsQueue);
    int32_t* const alive_list[2] = {s.q[0], s.q[1]};
    int32_t* const queue[2] = {reinterpret_cast<int32_t*>(s.vec[0]), reinterpret_cast<int32_t*>(s.vec[1])};
    auto min_of = [](unsigned long long word) {        // Counters::red[0] of core_scan / core_peel
        return word ? static_cast<int64_t>(INT32_MAX) - static_cast<int64_t>(word) : INT64_MAX;
    };
    int rc = TGO_OK;
    HIP_TRY(k_core_deg_init(g.tri_deg, n, deg, st));
    HIP_TRY(k_level_prep(s.cnt, nullptr, 0, nullptr, st));
    // the smallest degree: a scan that queues nothing
    HIP_TRY(k_core_scan(nullptr, n, deg, -1, nullptr, nullptr, s.cnt, st));
    if ((rc = core_turn(ctx))) return rc;
    int64_t next_k = min_of(s.hcnt->red[0]);
    int64_t alive = n, len = n, k = -1;
    const int32_t* list = nullptr;      // the alive list in use (null: every vertex)
    int spare = 0;                      // the alive_list buffer it is not in
    while (alive > 0) {
        if (next_k == INT64_MAX) return fail(ctx, TGO_E_HIP, "k-core peel: alive vertices without a degree");
        if (tail > 0 && alive <= tail) {
            if (len > 2 * alive) {      // the one workgroup scans the list once per level: compact it first
                HIP_TRY(k_core_scan(list, len, deg, static_cast<int32_t>(k), nullptr, alive_list[spare], s.cnt, st));
                if ((rc = core_turn(ctx))) return rc;
                list = alive_list[spare];
                spare ^= 1;
                len = static_cast<int64_t>(s.hcnt->mf);
                if (len != alive) return fail(ctx, TGO_E_HIP, "k-core peel: inconsistent alive count");
            }
            HIP_TRY(k_core_tail(list, len, lists, deg, static_cast<int32_t>(k), wave_row, s.cnt, st));
            if ((rc = core_turn(ctx))) return rc;
            ++rounds;
            levels += static_cast<int32_t>(s.hcnt->qlen);
            innermost = static_cast<int64_t>(s.hcnt->mf);
            top = static_cast<int64_t>(s.hcnt->red[0]);
            return TGO_OK;
        }
        k = next_k;
        const bool rebuild = 2 * alive <= len;      // the list has at least halved
        HIP_TRY(k_core_scan(list, len, deg, static_cast<int32_t>(k), queue[0], rebuild ? alive_list[spare] : nullptr,
                            s.cnt, st));
        if ((rc = core_turn(ctx))) return rc;
        int64_t qlen = static_cast<int64_t>(s.hcnt->qlen);
        next_k = min_of(s.hcnt->red[0]);
        if (rebuild) {
            list = alive_list[spare];
            spare ^= 1;
            len = static_cast<int64_t>(s.hcnt->mf);
        }
        // the minimum named a vertex that the level before went on to drop and peel: nobody is
        // left at k, and this scan's minimum is exact (nothing has changed since it ran)
        if (qlen == 0) continue;
        if (qlen > alive) return fail(ctx, TGO_E_HIP, "k-core peel: inconsistent level queue");
        ++levels;
        top = k;
        innermost = qlen;
        alive -= qlen;
        for (int cur = 0; qlen > 0 && k > 0; cur ^= 1) {    // (a vertex of level 0 has no neighbour)
            HIP_TRY(k_core_peel(queue[cur], qlen, lists, deg, static_cast<int32_t>(k), wave_row, lds_cap, queue[cur ^ 1],
                                n, s.cnt, st));
            if ((rc = core_turn(ctx))) return rc;
            ++rounds;
            const int64_t drops = static_cast<int64_t>(s.hcnt->mf);     // queued for the next launch or not
            qlen = static_cast<int64_t>(s.hcnt->qlen);
            if (drops > alive || qlen > drops) return fail(ctx, TGO_E_HIP, "k-core peel: inconsistent drop count");
            innermost += drops;
            alive -= drops;
            next_k = std::min(next_k, min_of(s.hcnt->red[0]));
        }
    }
    return TGO_OK;
}

int tgo_kcore(tgo_ctx* ctx, const tgo_core_args* a, int64_t* core_out, tgo_core_info* info) {
    int rc = bothE_program_check(ctx, a, "tgo_core_args", "core numbers are computed", "core numbers");
    if (rc) return rc;
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    const int64_t n = g.n;
    if (!g.tri_fadj && (rc = tri_forward_lists(ctx))) return rc;
    if (!g.core_badj && (rc = core_backward_lists(ctx))) return rc;
    int32_t* const deg = s.level;
    int64_t* const core = s.dist;
    HIP_TRY(hipEventRecord(ctx->ev0, st));
    int32_t levels = 0, rounds = 0;
    int64_t top = 0, innermost = 0;
    unsigned long long tot[2] = {0, 0};
    if (g.tri_fnnz == 0) {
        // no simple edge: nothing is peeled, every core number is 0 and the info stays zero
        HIP_TRY(k_fill_i64(core, 0, n, st));
    } else {
        {
            DevSpan span(st, "kcore.peel", {"simple_edges", g.tri_fnnz});
            if ((rc = core_peel_levels(ctx, deg, levels, rounds, top, innermost))) return rc;
        }
        DevSpan span(st, "kcore.finish");
        HIP_TRY(hipMemsetAsync(g.core_tot, 0, 2 * sizeof(unsigned long long), st));
        HIP_TRY(k_core_finish(deg, n, static_cast<int32_t>(top), core, g.core_tot, st));
        span.end();
        HIP_TRY(hipMemcpyAsync(tot, g.core_tot, sizeof tot, hipMemcpyDeviceToHost, st));
    }
    if ((rc = program_end(ctx, levels))) return rc;
    // the device's own count of the result against the level loop's bookkeeping
    if (static_cast<int64_t>(tot[1]) != top || static_cast<int64_t>(tot[0]) != innermost)
        return fail(ctx, TGO_E_HIP, "k-core: the core numbers disagree with the peel's level counts");
    if (info) *info = tgo_core_info{top, innermost, g.tri_fnnz, levels, rounds};
    if (core_out && (rc = rows_out(ctx, core, core_out))) return rc;
    publish_result(ctx, TGO_RESULT_CORE, ResultSource{core, nullptr});
    return TGO_OK;
}

int tgo_copy_cores(tgo_ctx* ctx, int64_t* core_out) {
    if (!ctx || !core_out) return TGO_E_INVALID;
    if (int rc = last_result_check(ctx, TGO_RESULT_CORE, "tgo_kcore")) return rc;
    (void)hipSetDevice(ctx->opts.device);
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return rows_out(ctx, ctx->sc.dist, core_out);
}

// ------------------------------------------------------------------ strongly connected components
// SCC (scc.hip).  Nothing is cached with the graph but the Titan ids it shares with tgo_components.
// Per run: comp (int32; -1 = live, else the representative) = sc.level, the live in- and
// out-degrees = the halves of sc.vec[0] (as int32; the first half ends as the components' sizes),
// colour and mark = the halves of sc.vec[1], the walks' queues = sc.q[0] / sc.q[1], the live lists
// = sc.qdeg / sc.qpre (as int32), a live vertex's place in its list = sc.vec[2] (as int32), which
// ends as the per-representative minimum (as int64), labels in internal order = sc.dist, row-order
// staging = sc.msg.  Level control: Counters through publish_turn / wait_publish.
// Defaults of TGO_TUNE_SCC_WAVE_ROW / _TAIL.
constexpr int64_t kSccWaveRow = 64, kSccTailDefault = kSccTail;
enum : int { kSccTrimWalk = 0, kSccForward = 1, kSccBackward = 2, kSccColourBack = 3 };

struct SccRun {
    SccGraph G;
    SccState S;
    int64_t n, wave_row;
    bool trim;
    int32_t* queue[2];
    int64_t live;           // vertices without a component yet
    int32_t rounds = 0;
};

// One publish of the level counters, which are zero again afterwards.
static int scc_turn(tgo_ctx* ctx) {
    Scratch& s = ctx->sc;
    const unsigned long long seq = ++s.pub_seq;
    HIP_TRY(k_publish_turn(s.cnt, s.hcnt_dev, seq, nullptr, ctx->stream));
    int rc = wait_publish(ctx, seq);
    if (rc) return rc;
    if (s.hcnt->err) return fail(ctx, TGO_E_HIP, "strongly connected components: a queue overflowed (inconsistent lists)");
    return TGO_OK;
}

// Walks queue[0][0, qlen) and whatever the walks discover, launch after launch, until a launch leaves
// nothing queued.  A vertex is discovered at most once per walk: the loop ends within n discoveries.
static int scc_walk_all(tgo_ctx* ctx, SccRun& r, int mode, int64_t qlen, int64_t& found) {
    Scratch& s = ctx->sc;
    found = 0;
    for (int cur = 0; qlen > 0; cur ^= 1) {
        HIP_TRY(k_scc_walk(mode, r.queue[cur], qlen, r.G, r.S, r.wave_row, r.queue[cur ^ 1], r.n, s.cnt, ctx->stream));
        if (int rc = scc_turn(ctx)) return rc;
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
static int scc_trim(tgo_ctx* ctx, SccRun& r, int64_t qlen) {
    if (!r.trim || qlen == 0) return TGO_OK;
    DevSpan span(ctx->stream, "scc.trim", {"queued", qlen}, {"live", r.live});
    int64_t found = 0;
    if (int rc = scc_walk_all(ctx, r, kSccTrimWalk, qlen, found)) return rc;
    if (found > r.live) return fail(ctx, TGO_E_HIP, "strongly connected components: inconsistent trim count");
    r.live -= found;
    return TGO_OK;
}

// The vertices of list (null: all) whose mark holds `bits` retire under rep (< 0: their colour), then the trim.
static int scc_retire(tgo_ctx* ctx, SccRun& r, const int32_t* list, int64_t len, int32_t bits, int32_t rep) {
    Scratch& s = ctx->sc;
    HIP_TRY(k_scc_retire(list, len, r.S, bits, rep, r.trim ? r.queue[0] : nullptr, r.n, s.cnt, ctx->stream));
    if (int rc = scc_turn(ctx)) return rc;
    const int64_t got = static_cast<int64_t>(s.hcnt->mf), qlen = static_cast<int64_t>(s.hcnt->qlen);
    if (got < 1 || got > r.live) return fail(ctx, TGO_E_HIP, "strongly connected components: no progress (a pass retired no vertex)");
    r.live -= got;
    return scc_trim(ctx, r, qlen);
}

// Forward-backward from the live vertex with the largest din * dout (the smallest id among equals).
static int scc_pivot(tgo_ctx* ctx, SccRun& r) {
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    HIP_TRY(k_scc_pivot_pick(r.S, r.n, 0, 0, s.cnt, st));
    int rc = scc_turn(ctx);
    if (rc) return rc;
    const unsigned long long product = s.hcnt->red[0];
    if (!product) return fail(ctx, TGO_E_HIP, "strongly connected components: live vertices without a pivot");
    HIP_TRY(k_scc_pivot_pick(r.S, r.n, 1, product, s.cnt, st));
    if ((rc = scc_turn(ctx))) return rc;
    const int64_t pivot = static_cast<int64_t>(0xFFFFFFFFULL - s.hcnt->red[0]);
    if (pivot < 0 || pivot >= r.n) return fail(ctx, TGO_E_HIP, "strongly connected components: inconsistent pivot");
    HIP_TRY(k_fill_i32(r.S.mark, 0, r.n, st));
    int64_t found = 0;
    {
        DevSpan span(st, "scc.pivot_forward", {"pivot", pivot}, {"live", r.live});
        HIP_TRY(k_scc_seed(r.S, static_cast<int32_t>(pivot), 3, r.queue[0], st));
        if ((rc = scc_walk_all(ctx, r, kSccForward, 1, found))) return rc;
    }
    {
        DevSpan span(st, "scc.pivot_backward", {"pivot", pivot}, {"forward", found + 1});
        HIP_TRY(k_scc_seed(r.S, static_cast<int32_t>(pivot), 3, r.queue[0], st));
        if ((rc = scc_walk_all(ctx, r, kSccBackward, 1, found))) return rc;
    }
    return scc_retire(ctx, r, nullptr, r.n, 3, static_cast<int32_t>(pivot));
}

// Colouring passes (on the grid, or all that remain in one workgroup) until no vertex is live.
static int scc_colour_passes(tgo_ctx* ctx, SccRun& r, int64_t tail, int32_t& passes) {
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    int32_t* const lists[2] = {reinterpret_cast<int32_t*>(s.qdeg), reinterpret_cast<int32_t*>(s.qpre)};
    int32_t* const pos = reinterpret_cast<int32_t*>(s.vec[2]);
    const int32_t* list = nullptr;      // the live list in use (null: every vertex)
    int64_t len = r.n;
    int spare = 0, rc = TGO_OK;
    while (r.live > 0) {
        HIP_TRY(k_scc_live_list(list, len, r.S, lists[spare], pos, r.n, s.cnt, st));
        if ((rc = scc_turn(ctx))) return rc;
        list = lists[spare];
        spare ^= 1;
        len = static_cast<int64_t>(s.hcnt->qlen);
        if (len != r.live) return fail(ctx, TGO_E_HIP, "strongly connected components: inconsistent live count");
        if (tail > 0 && r.live <= tail) {
            DevSpan span(st, "scc.tail", {"live", r.live});
            HIP_TRY(k_scc_tail(list, len, r.G, r.S.comp, pos, r.trim, r.wave_row, s.cnt, st));
            if ((rc = scc_turn(ctx))) return rc;
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
            HIP_TRY(k_scc_colour_init(list, len, r.S, st));
            // a colour travels at least one arc per launch and no simple path has more than live - 1
            for (int64_t launches = 1;; ++launches) {
                HIP_TRY(k_scc_colour_round(list, len, r.G, r.S, r.wave_row, s.cnt, st));
                if ((rc = scc_turn(ctx))) return rc;
                ++r.rounds;
                if (!s.hcnt->qlen) break;
                if (launches > r.live)
                    return fail(ctx, TGO_E_HIP, "strongly connected components: no progress (the colours do not settle)");
            }
        }
        {
            DevSpan span(st, "scc.colour_backward", {"pass", passes});
            HIP_TRY(k_scc_roots(list, len, r.S, r.queue[0], r.n, s.cnt, st));
            if ((rc = scc_turn(ctx))) return rc;
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
        int32_t* const half0 = reinterpret_cast<int32_t*>(s.vec[0]);
        int32_t* const half1 = reinterpret_cast<int32_t*>(s.vec[1]);
        r.G = SccGraph{g.out.off, g.out.adj, g.in.off, g.in.adj};
        r.S = SccState{s.level, half0, half0 + n, half1, half1 + n};
        r.n = n;
        r.wave_row = tuned(ctx->scc_wave_row, kSccWaveRow);
        r.trim = ctx->scc_trim != 0;
        r.queue[0] = s.q[0];
        r.queue[1] = s.q[1];
        r.live = n;
        const int64_t tail = std::min<int64_t>(tuned(ctx->scc_tail, kSccTailDefault), kSccTail);
        HIP_TRY(k_level_prep(s.cnt, nullptr, 0, nullptr, st));
        {
            DevSpan span(st, "scc.trim", {"live", n});
            HIP_TRY(k_scc_init(r.G, n, r.S, r.trim, r.wave_row, r.queue[0], s.cnt, st));
            if ((rc = scc_turn(ctx))) return rc;
            ++r.rounds;
        }
        const int64_t first = static_cast<int64_t>(s.hcnt->qlen);
        if (first > n) return fail(ctx, TGO_E_HIP, "strongly connected components: inconsistent trim count");
        r.live -= first;
        if ((rc = scc_trim(ctx, r, first))) return rc;
        if (ctx->scc_pivot != 0 && r.live > tail && (rc = scc_pivot(ctx, r))) return rc;
        if ((rc = scc_colour_passes(ctx, r, tail, out.passes))) return rc;
        // labels, and the device's own count of the vertices that have a component
        int64_t* const minid = reinterpret_cast<int64_t*>(s.vec[2]);
        int32_t* const size = r.S.din;
        {
            DevSpan span(st, "scc.label");
            HIP_TRY(k_fill_i64(minid, INT64_MAX, n, st));
            HIP_TRY(k_fill_i32(size, 0, n, st));
            HIP_TRY(k_scc_fold(r.S.comp, g.cc_tid, n, minid, size, st));
            HIP_TRY(k_scc_label(r.S.comp, minid, size, n, label, s.cnt, st));
        }
        if ((rc = scc_turn(ctx))) return rc;
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
    if (int rc = last_result_check(ctx, TGO_RESULT_SCC, "tgo_scc")) return rc;
    (void)hipSetDevice(ctx->opts.device);
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return rows_out(ctx, ctx->sc.dist, label_out);
}

// ------------------------------------------------------------------ betweenness centrality
// Brandes' betweenness (bc.hip).  The simple adjacency of the undirected reading lives with the graph
// (dev_alloc: released with it).  Per run: the running sum bc in internal order = sc.vec[2] (it is
// the published result: nothing else writes it before the next program); per seed: the BFS levels =
// sc.level (run_bfs, which also uses sc.q[*], sc.qdeg, sc.qpre, the bitmaps and sc.dist while it
// runs), then the level histogram and the scatter's cursors = sc.qdeg, the level offsets = sc.qpre
// (depth + 2 <= n + 1 words; once the host has them, word L of sc.qdeg / sc.qpre counts the long rows
// that level L of the forward / backward sweep queues), the level-ordered list = sc.q[0], the long
// rows' queue = sc.q[1], sigma = sc.vec[0], delta = sc.vec[1]; row-order staging = sc.msg.  The level offsets reach the host kCounterWords words a publish; the
// overflow flag is Counters::err through publish_turn / wait_publish.
// Default of TGO_TUNE_BC_WAVE_ROW.
constexpr int64_t kBcWaveRow = 64;

static int bc_simple_adjacency(tgo_ctx* ctx) {
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
    ctx->st.device_bytes = ctx->dev_bytes;
    return TGO_OK;
}

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

// One publish of the level counters, which are zero again afterwards; overflow = Counters::err.
static int bc_turn(tgo_ctx* ctx, bool& overflow) {
    Scratch& s = ctx->sc;
    const unsigned long long seq = ++s.pub_seq;
    HIP_TRY(k_publish_turn(s.cnt, s.hcnt_dev, seq, nullptr, ctx->stream));
    int rc = wait_publish(ctx, seq);
    if (rc) return rc;
    overflow = s.hcnt->err != 0;
    return TGO_OK;
}

// delta_seed added to r.bc; depth and reached: the deepest level and the vertices reached (seed included).
static int bc_one_seed(tgo_ctx* ctx, BcRun& r, int64_t seed, int64_t shown, std::vector<int64_t>& loff, int32_t& depth,
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
    for (int64_t w0 = 0; w0 < words; w0 += kCounterWords) {
        const int count = static_cast<int>(std::min<int64_t>(kCounterWords, words - w0));
        const unsigned long long seq = ++s.pub_seq;
        HIP_TRY(k_publish_words(s.qpre + w0, count, s.hcnt_dev, seq, st));
        if ((rc = wait_publish(ctx, seq))) return rc;
        const volatile unsigned long long* host = reinterpret_cast<volatile unsigned long long*>(s.hcnt);
        for (int i = 0; i < count; ++i) loff[static_cast<size_t>(w0 + i)] = static_cast<int64_t>(host[i]);
    }
    bool overflow = false;
    if ((rc = bc_turn(ctx, overflow))) return rc;
    bool sane = !overflow && loff[0] == 0 && loff[1] == 1 && loff[static_cast<size_t>(depth) + 1] <= n;
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
    if ((rc = bc_turn(ctx, overflow))) return rc;
    if (overflow)
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

int tgo_betweenness(tgo_ctx* ctx, const tgo_bc_args* a, const int64_t* seeds, int64_t nseeds, double* bc_out,
                    tgo_bc_info* info) {
    int rc = bothE_program_check(ctx, a, "tgo_bc_args", "betweenness centrality runs", "shortest paths");
    if (rc) return rc;
    if (a->directed != 0 && a->directed != 1) return fail(ctx, TGO_E_INVALID, "tgo_bc_args.directed must be 0 or 1");
    if (nseeds < -1) return fail(ctx, TGO_E_INVALID, "nseeds must be >= 0, or -1 for every vertex");
    if (nseeds > 0 && !seeds) return fail(ctx, TGO_E_INVALID, "null seeds");
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    const int64_t n = g.n;
    // the seeds as internal ids, in the order given (an unknown Titan id: -1, nothing runs for it)
    const int64_t count = nseeds < 0 ? n : nseeds;
    std::vector<int64_t> internal(static_cast<size_t>(count));
    for (int64_t i = 0; i < count; ++i) {
        if (nseeds < 0) internal[i] = ctx->perm[i];
        else if ((rc = resolve_seed(ctx, seeds[i], a->seed_is_dense, internal[i]))) return rc;
    }
    BcRun r{};
    if (a->directed) {
        r = BcRun{g.in.off, g.out.off, g.in.adj, g.out.adj, true, TGO_SCOPE_OUT_E};
    } else {
        if (n > 0 && !g.bc_sadj && (rc = bc_simple_adjacency(ctx))) return rc;
        r = BcRun{g.bc_soff, g.bc_soff, g.bc_sadj, g.bc_sadj, false, TGO_SCOPE_BOTH_E};
    }
    r.wave_row = tuned(ctx->bc_wave_row, kBcWaveRow);
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
    if (int rc = last_result_check(ctx, TGO_RESULT_BETWEENNESS, "tgo_betweenness")) return rc;
    (void)hipSetDevice(ctx->opts.device);
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return rows_out(ctx, ctx->sc.vec[2], bc_out);
}

// ------------------------------------------------------------------ peer-pressure clustering
// Peer pressure (pp.hip).  The ranks of the Titan ids (and their inverse) live with the graph beside
// cc_tid (dev_alloc: released with it).  Per run: the two vote arrays = sc.level and sc.vec[0] (as
// int32 labels, distribute = 0) or sc.vec[1] and sc.vec[2] (as 8-byte words, distribute = 1), the wave
// and block queues = sc.q[0] / sc.q[1], the clusters' populations = sc.qdeg (as int32), labels in
// internal order = sc.dist, row-order staging = sc.msg.  Round control: Counters through
// k_publish_turn / wait_publish, one publish per round.
// Defaults of TGO_TUNE_PP_WAVE_ROW / _BLOCK_ROW / _SLOTS.
constexpr int64_t kPpWaveRow = 16, kPpBlockRow = 2048, kPpSlots = 512;

// g.pp_rank / g.pp_inv: once per graph.
static int pp_ranks(tgo_ctx* ctx) {
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
    ctx->st.device_bytes = ctx->dev_bytes;
    return TGO_OK;
}

// One publish of the round's counters, which are zero again afterwards.
static int pp_turn(tgo_ctx* ctx) {
    Scratch& s = ctx->sc;
    const unsigned long long seq = ++s.pub_seq;
    HIP_TRY(k_publish_turn(s.cnt, s.hcnt_dev, seq, nullptr, ctx->stream));
    return wait_publish(ctx, seq);
}

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
    int64_t* const label = s.dist;
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
        r.wave_row = tuned(ctx->pp_wave_row, kPpWaveRow);
        r.block_row = tuned(ctx->pp_block_row, kPpBlockRow);
        r.slots = static_cast<int32_t>(tuned(ctx->pp_slots, kPpSlots));
        r.distribute = a->distribute != 0;
        r.wq = s.q[0];
        r.bq = s.q[1];
        void* votes[2] = {s.level, s.vec[0]};
        if (r.distribute) { votes[0] = s.vec[1]; votes[1] = s.vec[2]; }
        int cur = 0;
        HIP_TRY(k_level_prep(s.cnt, nullptr, 0, nullptr, st));
        HIP_TRY(k_pp_init(r, send, g.pp_rank, votes[cur], s.cnt, st));
        if ((rc = pp_turn(ctx))) return rc;
        r.nwave = static_cast<int64_t>(s.hcnt->qlen);
        r.nblock = static_cast<int64_t>(s.hcnt->mf);
        if (r.nwave + r.nblock > n) return fail(ctx, TGO_E_HIP, "peer pressure: inconsistent row queues");
        while (out.rounds < a->max_rounds) {
            const bool first = out.rounds == 0;
            {
                DevSpan span(st, first ? "peer_pressure.first" : "peer_pressure.vote", {"round", out.rounds + 1});
                HIP_TRY(k_pp_round(r, first, 0, votes[cur], votes[cur ^ 1], s.cnt, st));
            }
            if (r.nwave > 0) {
                DevSpan span(st, "peer_pressure.queue", {"round", out.rounds + 1}, {"wave_rows", r.nwave});
                HIP_TRY(k_pp_round(r, first, 1, votes[cur], votes[cur ^ 1], s.cnt, st));
            }
            if (r.nblock > 0) {
                DevSpan span(st, "peer_pressure.queue", {"round", out.rounds + 1}, {"block_rows", r.nblock});
                HIP_TRY(k_pp_round(r, first, 2, votes[cur], votes[cur ^ 1], s.cnt, st));
            }
            if ((rc = pp_turn(ctx))) return rc;
            cur ^= 1;
            ++out.rounds;
            out.changed_last = static_cast<int64_t>(s.hcnt->red[0]);
            if (out.changed_last > n) return fail(ctx, TGO_E_HIP, "peer pressure: inconsistent change count");
            if (out.changed_last == 0) break;
        }
        out.converged = out.rounds > 0 && out.changed_last == 0;
        {
            DevSpan span(st, "peer_pressure.label");
            int32_t* const hist = reinterpret_cast<int32_t*>(s.qdeg);
            HIP_TRY(k_fill_i32(hist, 0, n, st));
            HIP_TRY(k_pp_finish(r, votes[cur], g.pp_inv, g.cc_tid, label, hist, s.cnt, st));
        }
        if ((rc = pp_turn(ctx))) return rc;
        out.clusters = static_cast<int64_t>(s.hcnt->qlen);
        out.largest = static_cast<int64_t>(s.hcnt->red[0]);
    }
    if ((rc = program_end(ctx, out.rounds))) return rc;
    if (info) *info = out;
    if (cluster_out && n > 0 && (rc = rows_out(ctx, label, cluster_out))) return rc;
    publish_result(ctx, TGO_RESULT_PEER_PRESSURE, ResultSource{label, nullptr});
    return TGO_OK;
}

int tgo_copy_peer_pressure(tgo_ctx* ctx, int64_t* cluster_out) {
    if (!ctx || !cluster_out) return TGO_E_INVALID;
    if (int rc = last_result_check(ctx, TGO_RESULT_PEER_PRESSURE, "tgo_peer_pressure")) return rc;
    (void)hipSetDevice(ctx->opts.device);
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return rows_out(ctx, ctx->sc.dist, cluster_out);
}

// ------------------------------------------------------------------ closeness / harmonic centrality
// The distance-based centralities (cl.hip) out of the multi-source sweep (run_ms_sweep, api_msbfs.cpp).
// Device arrays, internal order, kept across the batches of one run and published as its result:
// sc.cl_far / cl_reach (u64), sc.cl_ecc (int32), sc.cl_harm, sc.cl_close (fp64; the result source of
// tgo_result_rows); the sweep's own state is sc.ms_*; row-order staging = sc.msg; the two reductions of the
// finish = Counters::red[0..1] through publish_turn / wait_publish.
static int cl_alloc(tgo_ctx* ctx) {
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
    ctx->st.device_bytes = ctx->dev_bytes;
    return TGO_OK;
}

namespace {
// The whole run's device time: the sweeps record ctx->ev0 / ev1 for themselves.
struct ClTimer {
    hipEvent_t t0 = nullptr, t1 = nullptr;
    ~ClTimer() {
        if (t0) (void)hipEventDestroy(t0);
        if (t1) (void)hipEventDestroy(t1);
    }
};
}  // namespace

int tgo_closeness(tgo_ctx* ctx, const tgo_cl_args* a, const int64_t* seeds, int64_t nseeds, double* closeness_out,
                  double* harmonic_out, tgo_cl_info* info) {
    if (!ctx) return TGO_E_INVALID;
    ctx->res_kind = -1;
    if (!a) return fail(ctx, TGO_E_INVALID, "null args");
    int rc = check_program(ctx, a->scope);
    if (rc) return rc;
    if (a->flags != 0) return fail(ctx, TGO_E_INVALID, "tgo_cl_args.flags must be 0");
    if (a->max_depth < 0) return fail(ctx, TGO_E_INVALID, "max_depth < 0");
    if (nseeds < -1) return fail(ctx, TGO_E_INVALID, "nseeds must be >= 0, or -1 for every vertex");
    if (nseeds > 0 && !seeds) return fail(ctx, TGO_E_INVALID, "null seeds");
    if (ctx->g.partitioned) return fail(ctx, TGO_E_UNSUPPORTED, "closeness centrality runs on a one-GPU load");
    (void)hipSetDevice(ctx->opts.device);
    if ((rc = ms_alloc(ctx))) return rc;
    if ((rc = cl_alloc(ctx))) return rc;
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    const int64_t n = g.n;
    // the seeds that are executed vertices as internal ids, in the order given
    const int64_t count = nseeds < 0 ? n : nseeds;
    std::vector<int64_t> internal;
    internal.reserve(static_cast<size_t>(count));
    for (int64_t i = 0; i < count; ++i) {
        int64_t v = -1;
        if (nseeds < 0) v = ctx->perm[i];
        else if ((rc = resolve_seed(ctx, seeds[i], a->seed_is_dense, v))) return rc;
        if (v >= 0) internal.push_back(v);
    }
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
        const unsigned long long seq = ++s.pub_seq;
        HIP_TRY(k_publish_turn(s.cnt, s.hcnt_dev, seq, nullptr, st));
        if ((rc = wait_publish(ctx, seq))) return rc;
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
    if (int rc = last_result_check(ctx, TGO_RESULT_CLOSENESS, "tgo_closeness")) return rc;
    (void)hipSetDevice(ctx->opts.device);
    Scratch& s = ctx->sc;
    const int64_t n = ctx->g.n;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (n <= 0) return TGO_OK;
    int rc = TGO_OK;
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
