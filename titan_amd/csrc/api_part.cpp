// api_part.cpp — the 1-D partitioned (multi-GPU) primitives (include/titan_gpu_olap_part.h): one rank's
// share of a program's step between two exchanges, and what part_driver.cpp's native loops call.
// The multi-source steps take what the native sweep chooses per call as arguments (ctx.hpp MsRecv /
// MsOwn); nothing about one call is kept in the context for the next.
#include "ctx.hpp"

using namespace tgo;

extern "C" {

static int part_qlen_now(tgo_ctx* ctx, int64_t& q) {
    if (ctx->part_qlen_stale) {
        HIP_TRY(hipMemcpyAsync(&ctx->part_qlen, ctx->part_qlen_dev, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        ctx->part_qlen_stale = false;
    }
    q = ctx->part_qlen;
    return TGO_OK;
}

int tgo_part_device_counts(tgo_ctx* ctx, int64_t* dev_counts) {
    int rc = part_check(ctx);
    if (rc) return rc;
    if (dev_counts) ctx->part_qlen_dev = dev_counts + 2;        // [2]: this rank's queue length
    if (!dev_counts && ctx->part_qlen_stale) {
        int64_t q;
        if ((rc = part_qlen_now(ctx, q))) return rc;
    }
    ctx->part_dcounts = dev_counts;
    return TGO_OK;
}

int tgo_part_set_local_qlen(tgo_ctx* ctx, int64_t qlen) {
    int rc = part_check(ctx);
    if (rc) return rc;
    if (!ctx->part_qlen_stale) return TGO_OK;               // nothing pending
    if (qlen < 0 || qlen > ctx->g.n) return fail(ctx, TGO_E_INVALID, "local queue length out of range");
    ctx->part_qlen = qlen;
    ctx->part_qlen_stale = false;
    return TGO_OK;
}

int tgo_part_bfs_begin(tgo_ctx* ctx, int64_t seed_global, uint64_t* nb_local, int64_t* counts) {
    int rc = part_check(ctx);
    if (rc) return rc;
    if (ctx->g.scope != TGO_SCOPE_BOTH_E) return fail(ctx, TGO_E_UNSUPPORTED, "partitioned BFS runs over bothE");
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    const int64_t n = g.n, words = n / 64;
    const View push = push_view(g, TGO_SCOPE_BOTH_E);
    HIP_TRY(hipEventRecord(ctx->ev0, st));
    HIP_TRY(k_fill_i32(s.level, -1, n, st));
    HIP_TRY(hipMemsetAsync(s.vb, 0, (words + 1) * 8, st));
    HIP_TRY(hipMemsetAsync(nb_local, 0, words * 8, st));
    HIP_TRY(hipMemsetAsync(s.cnt, 0, sizeof(Counters), st));
    ctx->part_cur = 0;
    ctx->part_queued = true;
    ctx->part_qlen = 0;
    ctx->part_qlen_stale = false;
    int64_t deg = 0;
    int64_t seed = seed_global - g.lo;
    if (seed >= 0 && seed < n) {
        seed = ctx->perm[seed];
        // the owner seeds: level 0, visited, in the frontier bitmap slice and the queue
        HIP_TRY(k_bfs_seed(push, s.level, s.vb, nb_local, s.q[0], s.qdeg, seed, st));
        HIP_TRY(hipMemcpyAsync(&deg, s.qdeg, sizeof(int64_t), hipMemcpyDeviceToHost, st));
        ctx->part_qlen = 1;
    }
    HIP_TRY(hipStreamSynchronize(st));
    if (counts) { counts[0] = ctx->part_qlen; counts[1] = deg; }
    return TGO_OK;
}

int tgo_part_bfs_td(tgo_ctx* ctx, int32_t level, uint64_t* disc_global) {
    int rc = part_check(ctx);
    if (rc) return rc;
    (void)level;
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    const View push = push_view(g, TGO_SCOPE_BOTH_E);
    int64_t qlen = 0;
    if ((rc = part_qlen_now(ctx, qlen))) return rc;
    if (qlen > 0 && !ctx->part_queued) {
        HIP_TRY(hipMemsetAsync(s.cnt, 0, sizeof(Counters), st));
        HIP_TRY(k_bfs_queue(push, g.n_active, ctx->part_frontier, s.q[ctx->part_cur], s.qdeg, s.cnt, st));
        ctx->part_queued = true;
    }
    if (qlen > 0) {
        if ((rc = scan_frontier(ctx, ctx->part_qlen))) return rc;
        HIP_TRY(k_part_td_mark(push, s.q[ctx->part_cur], s.qpre, ctx->part_qlen, disc_global, s.vb, g.lo, g.n, st));
    }
    return part_done(ctx);
}

int tgo_part_bfs_claim(tgo_ctx* ctx, int32_t level, const uint64_t* recv, int32_t nslices,
                       uint64_t* nb_local, int64_t* counts) {
    int rc = part_check(ctx);
    if (rc) return rc;
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    const View push = push_view(g, TGO_SCOPE_BOTH_E);
    HIP_TRY(hipMemsetAsync(s.cnt, 0, sizeof(Counters), st));
    const int nxt = ctx->part_cur ^ 1;
    HIP_TRY(k_part_claim(push, recv, nslices, g.n / 64, g.n, s.vb, nb_local, s.level, s.q[nxt], s.qdeg, s.cnt,
                         level + 1, st));
    ctx->part_cur = nxt;
    ctx->part_queued = true;
    return part_counts(ctx, counts);
}

}  // extern "C" (the fused level helpers below are C++, used by part_driver.cpp)
namespace tgo {
// tgo_part_bfs_run's top-down level, fused: the current queue (built from the frontier bitmap
// when the last level was bottom-up), then ONE expansion that claims owned targets in place —
// the one-GPU td_expand — and marks only remote ones in disc; nb_local is zeroed first.  With
// world 1 nothing is remote, and the level needs no exchange and no claim pass over the whole
// bitmap (the C-ABI's td / all-to-all / claim protocol makes two passes over every word).
int part_bfs_td_fused(tgo_ctx* ctx, int32_t level, uint64_t* disc, uint64_t* nb_local) {
    int rc = part_check(ctx);
    if (rc) return rc;
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    const View push = push_view(g, TGO_SCOPE_BOTH_E);
    int64_t qlen = 0;
    if ((rc = part_qlen_now(ctx, qlen))) return rc;
    if (qlen > 0 && !ctx->part_queued) {
        HIP_TRY(hipMemsetAsync(s.cnt, 0, sizeof(Counters), st));
        HIP_TRY(k_bfs_queue(push, g.n_active, ctx->part_frontier, s.q[ctx->part_cur], s.qdeg, s.cnt, st));
        ctx->part_queued = true;
    }
    if (qlen > 0 && (rc = scan_frontier(ctx, qlen))) return rc;
    HIP_TRY(hipMemsetAsync(s.cnt, 0, sizeof(Counters), st));
    HIP_TRY(hipMemsetAsync(nb_local, 0, (g.n / 64) * 8, st));
    const int nxt = ctx->part_cur ^ 1;
    if (qlen > 0)
        HIP_TRY(k_part_td_claim(push, s.q[ctx->part_cur], s.qpre, qlen, disc, s.vb, nb_local, s.level, s.q[nxt], s.qdeg,
                                s.cnt, level + 1, g.lo, g.n, st));
    ctx->part_cur = nxt;
    ctx->part_queued = true;
    return part_done(ctx);
}
// The remote discoveries (received slices) into the queue part_bfs_td_fused started.
int part_bfs_claim_remote(tgo_ctx* ctx, int32_t level, const uint64_t* recv, int32_t nslices, uint64_t* nb_local) {
    int rc = part_check(ctx);
    if (rc) return rc;
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    const View push = push_view(g, TGO_SCOPE_BOTH_E);
    HIP_TRY(k_part_claim(push, recv, nslices, g.n / 64, g.n, s.vb, nb_local, s.level, s.q[ctx->part_cur], s.qdeg, s.cnt,
                         level + 1, ctx->stream, true));
    return part_done(ctx);
}
// The level's counts (device counts when set, as tgo_part_bfs_claim).
int part_bfs_level_done(tgo_ctx* ctx) { return part_counts(ctx, nullptr); }
}  // namespace tgo
extern "C" {

int tgo_part_bfs_bu(tgo_ctx* ctx, int32_t level, const uint64_t* fb_global, uint64_t* nb_local, int64_t* counts) {
    int rc = part_check(ctx);
    if (rc) return rc;
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    const View pull = pull_view(g, TGO_SCOPE_BOTH_E), push = push_view(g, TGO_SCOPE_BOTH_E);
    HIP_TRY(hipMemsetAsync(s.cnt, 0, sizeof(Counters), st));
    HIP_TRY(hipMemsetAsync(nb_local, 0, (g.n / 64) * 8, st));
    const int nxt = ctx->part_cur ^ 1;
    HIP_TRY(k_bu_step(pull, push, g.n_active, fb_global, s.vb, nb_local, s.level, s.cnt, level + 1, st));
    ctx->part_cur = nxt;
    ctx->part_queued = false;       // counted only: bfs_td queues nb_local if it runs next
    ctx->part_frontier = nb_local;
    return part_counts(ctx, counts);
}

int tgo_part_bfs_end(tgo_ctx* ctx, int64_t* dist_local, int64_t* reached) {
    int rc = part_check(ctx);
    if (rc) return rc;
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    HIP_TRY(k_level_to_dist(s.level, s.dist, g.n, st));
    HIP_TRY(hipEventRecord(ctx->ev1, st));
    if (reached && (rc = reach_stats(ctx, TGO_SCOPE_BOTH_E, reached))) return rc;
    if (dist_local && (rc = rows_out_async(ctx, s.dist, dist_local))) return rc;
    // the partitioned ends wait once, for the whole stream (the copy-out included), not for ev1,
    // and resolve no trace: the native drivers (part_driver.cpp) do that before they call the end
    HIP_TRY(hipStreamSynchronize(st));
    return program_elapsed(ctx);
}

// ---- partitioned multi-source BFS
int tgo_part_ms_begin(tgo_ctx* ctx, const int64_t* seeds, int32_t nseeds, uint64_t* fr_local, int64_t* counts) {
    int rc = part_check(ctx);
    if (rc) return rc;
    if (!seeds || nseeds < 1 || nseeds > TGO_MAX_SOURCES) return fail(ctx, TGO_E_INVALID, "nseeds must be in [1, 64]");
    if (ctx->g.scope != TGO_SCOPE_BOTH_E) return fail(ctx, TGO_E_UNSUPPORTED, "partitioned BFS runs over bothE");
    if ((rc = ms_alloc(ctx))) return rc;
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    const int64_t n = g.n;
    const View push = push_view(g, TGO_SCOPE_BOTH_E);
    // owned seeds, as local ids; sources keep their global bit position r
    std::vector<int64_t> local(nseeds, -1);
    std::vector<int32_t> uniq;
    for (int r = 0; r < nseeds; ++r) {
        int64_t l = seeds[r] - g.lo;
        if (l >= 0 && l < n) {
            l = ctx->perm[l];
            local[r] = l;
            if (std::find(uniq.begin(), uniq.end(), static_cast<int32_t>(l)) == uniq.end()) uniq.push_back(static_cast<int32_t>(l));
        }
    }
    s.ms_nsrc = nseeds;
    HIP_TRY(hipEventRecord(ctx->ev0, st));
    HIP_TRY(hipMemsetAsync(s.ms_vis, 0, n * 8, st));
    HIP_TRY(hipMemsetAsync(fr_local, 0, n * 8, st));
    if (!s.pk_ovf) HIP_TRY(dev_alloc(ctx, s.pk_ovf, 1));
    HIP_TRY(hipMemsetAsync(s.pk_ovf, 0, sizeof(int), st));
    const int64_t touch_n = g.n_global / kPackChunk + kMaxRanks + 1;
    if (!s.pk_touch) HIP_TRY(dev_alloc(ctx, s.pk_touch, touch_n));
    HIP_TRY(hipMemsetAsync(s.pk_touch, 0, touch_n, st));
    s.ms_nplanes = 0;
    // seeds owned elsewhere stay -1 (skipped by the seed kernel; their bit is set by the owner)
    HIP_TRY(hipMemcpyAsync(s.ms_seeds, local.data(), nseeds * sizeof(int64_t), hipMemcpyHostToDevice, st));
    // entry-less seeds stay out of the masks: the pull levels never write the masks' tail
    // [n_active, n), which therefore stays zero in both alternating buffers
    HIP_TRY(k_ms_seed(s.ms_seeds, nseeds, s.ms_vis, fr_local, g.n_active, st));
    ctx->part_cur = 0;
    ctx->part_queued = true;
    ctx->part_qlen = static_cast<int64_t>(uniq.size());
    ctx->part_qlen_stale = false;
    int64_t mf = 0;
    if (!uniq.empty()) {
        HIP_TRY(hipMemcpyAsync(s.q[0], uniq.data(), uniq.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(k_degree_i64(push, s.q[0], static_cast<int64_t>(uniq.size()), s.qdeg, st));
        std::vector<int64_t> d(uniq.size());
        HIP_TRY(hipMemcpyAsync(d.data(), s.qdeg, d.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (int64_t x : d) mf += x;
    }
    HIP_TRY(hipStreamSynchronize(st));
    if (counts) { counts[0] = ctx->part_qlen; counts[1] = mf; }
    return TGO_OK;
}

// ---- source split of a dense level (tgo_bfs_multi's split, partitioned; titan_gpu_olap_part.h)
int tgo_part_ms_source_counts(tgo_ctx* ctx, const uint64_t* fr_local, int64_t* counts_dev) {
    int rc = part_check(ctx);
    if (rc) return rc;
    if (!fr_local || !counts_dev) return fail(ctx, TGO_E_INVALID, "null argument");
    HIP_TRY(k_ms_source_counts(fr_local, ctx->g.n_active, reinterpret_cast<unsigned long long*>(counts_dev), ctx->stream));
    return part_done(ctx);
}

int tgo_part_ms_source_entries(tgo_ctx* ctx, const uint64_t* fr_local, uint64_t cand, int64_t* entries_dev) {
    int rc = part_check(ctx);
    if (rc) return rc;
    if (!fr_local || !entries_dev) return fail(ctx, TGO_E_INVALID, "null argument");
    HIP_TRY(k_ms_source_entries(push_view(ctx->g, TGO_SCOPE_BOTH_E), fr_local, ctx->g.n_active, cand,
                                reinterpret_cast<unsigned long long*>(entries_dev), ctx->stream));
    return part_done(ctx);
}

// The sparse sources' frontiers pushed into cand_global: a masked queue of this rank's
// frontier in the idle queue buffer (a dense level builds no queue), the pack's touch flags.
int tgo_part_ms_push_masked(tgo_ctx* ctx, const uint64_t* fr_local, uint64_t* cand_global, uint64_t mask) {
    int rc = part_check(ctx);
    if (rc) return rc;
    if (!fr_local || !cand_global) return fail(ctx, TGO_E_INVALID, "null argument");
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    const View push = push_view(g, TGO_SCOPE_BOTH_E);
    int32_t* q = s.q[ctx->part_cur ^ 1];
    HIP_TRY(hipMemsetAsync(s.cnt, 0, sizeof(Counters), st));
    HIP_TRY(k_ms_queue(push, g.n_active, fr_local, q, s.qdeg, s.cnt, st, mask));
    if ((rc = read_counters(ctx))) return rc;
    const int64_t qlen = static_cast<int64_t>(s.hcnt->qlen);
    if (qlen > 0) {
        if ((rc = scan_frontier(ctx, qlen))) return rc;
        const PackTouch touch{s.pk_touch, g.n, (g.n + kPackChunk - 1) / kPackChunk};
        HIP_TRY(k_ms_push(push, q, s.qpre, qlen, fr_local, nullptr, cand_global, st, touch, mask));
    }
    return part_done(ctx);
}

}  // extern "C" (the step forms tgo_part_msbfs_run calls, ctx.hpp; their C entry points follow)
namespace tgo {

int part_ms_push(tgo_ctx* ctx, const uint64_t* fr_local, uint64_t* cand_global, uint64_t* own_next, int self) {
    int rc = part_check(ctx);
    if (rc) return rc;
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    int64_t qlen = 0;
    if ((rc = part_qlen_now(ctx, qlen))) return rc;
    if (qlen > 0 && !ctx->part_queued) {
        HIP_TRY(hipMemsetAsync(s.cnt, 0, sizeof(Counters), ctx->stream));
        HIP_TRY(k_ms_queue(push_view(g, TGO_SCOPE_BOTH_E), g.n_active, fr_local, s.q[ctx->part_cur], s.qdeg, s.cnt,
                           ctx->stream));
        ctx->part_queued = true;
    }
    // the owned targets' candidates go straight into own_next (zeroed here), so the settle
    // neither zeroes those masks nor ORs the own slice (MsOwn::direct)
    uint64_t* own = self >= 0 ? own_next : nullptr;
    const int64_t own_lo = own ? static_cast<int64_t>(self) * g.n : 0;
    if (own) HIP_TRY(k_level_prep(nullptr, own, g.n_active, nullptr, ctx->stream));   // the tail stays zero
    if (qlen > 0) {
        if ((rc = scan_frontier(ctx, ctx->part_qlen))) return rc;
        const PackTouch touch{s.pk_touch, g.n, (g.n + kPackChunk - 1) / kPackChunk};
        HIP_TRY(k_ms_push(push_view(g, TGO_SCOPE_BOTH_E), s.q[ctx->part_cur], s.qpre, ctx->part_qlen, fr_local,
                          nullptr, cand_global, ctx->stream, touch, ~0ULL, true, own, own_lo));
    }
    return part_done(ctx);
}

// What the settles and the ORs share: the checks of the received pairs (`name`: the entry
// point's, for its messages), then the pairs and the rank's own slice OR-ed into fr_next.
static int ms_recv_check(tgo_ctx* ctx, const char* name, const MsRecv& in, const uint64_t* fr_next, int64_t& npairs) {
    auto bad = [&](const char* what) {
        return fail(ctx, TGO_E_INVALID, std::string(name) + (in.sized ? "_pairs: bad " : "_fixed: bad ") + what);
    };
    if (!in.recv || !fr_next || in.nslices < 1 || in.nslices > kMaxRanks ||
        (in.sized ? !in.counts : in.cap < 1 || in.cap > ctx->g.n))
        return bad("arguments");
    npairs = 0;
    for (int r = 0; in.sized && r < in.nslices; ++r) {
        if (in.counts[r] < 0 || in.counts[r] > ctx->g.n) return bad("count");
        npairs += in.counts[r];
    }
    return TGO_OK;
}

static int ms_or_received(tgo_ctx* ctx, const MsRecv& in, int64_t npairs, uint64_t* fr_next, const MsOwn& own) {
    if (in.sized) HIP_TRY(k_ms_or_pairs(in.recv, npairs, fr_next, ctx->stream));
    else HIP_TRY(k_ms_or_fixed(in.recv, in.nslices, in.cap, fr_next, ctx->stream));
    if (own.direct || own.self < 0 || !own.cand) return TGO_OK;
    const int64_t nl = ctx->g.n, cps = (nl + kPackChunk - 1) / kPackChunk;
    uint8_t* touched = ctx->sc.pk_touch ? ctx->sc.pk_touch + static_cast<int64_t>(own.self) * cps : nullptr;
    HIP_TRY(k_ms_or_local(own.cand + static_cast<int64_t>(own.self) * nl, nl, cps, touched, fr_next, ctx->stream));
    return TGO_OK;
}

// The received candidate pairs OR-ed into fr_next (zeroed first), no settle: the pull of the
// same level reads them (tgo_part_ms_pull_split).
int part_ms_or(tgo_ctx* ctx, const MsRecv& in, uint64_t* fr_next, const MsOwn& own) {
    int rc = part_check(ctx);
    if (rc) return rc;
    int64_t npairs = 0;
    if ((rc = ms_recv_check(ctx, "ms_or", in, fr_next, npairs))) return rc;
    HIP_TRY(hipMemsetAsync(fr_next, 0, ctx->g.n_active * 8, ctx->stream));
    if ((rc = ms_or_received(ctx, in, npairs, fr_next, own))) return rc;
    return part_done(ctx);
}

// The planes a discovery at level + 1 writes; a sweep is at most 65535 levels deep.
static int ms_level_planes(tgo_ctx* ctx, int32_t level) {
    if (level + 1 >= (1 << kLevelPlanes)) return fail(ctx, TGO_E_UNSUPPORTED, "multi-source BFS levels are < 65536");
    return ms_planes_for(ctx, level + 1);
}

// The candidates in fr_next settled: the bits not visited yet become level + 1 and the next
// frontier, queued in the other queue buffer (count_only: counted only), and the level's counts.
static int ms_settle_tail(tgo_ctx* ctx, int32_t level, uint64_t* fr_next, int64_t* sums, bool count_only, int64_t* counts) {
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    unsigned long long* srcent = reinterpret_cast<unsigned long long*>(sums);
    const int nxt = ctx->part_cur ^ 1;
    if (count_only) {
        HIP_TRY(k_ms_settle_count(push_view(g, TGO_SCOPE_BOTH_E), g.n_active, s.ms_vis, fr_next, ms_planes(ctx), s.cnt,
                                  level + 1, st, srcent));
    } else {
        HIP_TRY(k_ms_settle(push_view(g, TGO_SCOPE_BOTH_E), g.n_active, s.ms_vis, fr_next, ms_planes(ctx), s.q[nxt], s.qdeg,
                            s.cnt, level + 1, st, srcent));
    }
    ctx->part_queued = !count_only;
    ctx->part_cur = nxt;
    return part_counts(ctx, counts);
}

int part_ms_settle(tgo_ctx* ctx, int32_t level, const MsRecv& in, uint64_t* fr_next, const MsOwn& own, int64_t* counts) {
    int rc = part_check(ctx);
    if (rc) return rc;
    int64_t npairs = 0;
    if ((rc = ms_recv_check(ctx, "ms_settle", in, fr_next, npairs)) || (rc = ms_level_planes(ctx, level))) return rc;
    HIP_TRY(k_level_prep(ctx->sc.cnt, own.direct ? nullptr : fr_next, own.direct ? 0 : ctx->g.n_active, nullptr,
                         ctx->stream));   // tail stays zero
    if ((rc = ms_or_received(ctx, in, npairs, fr_next, own))) return rc;
    return ms_settle_tail(ctx, level, fr_next, own.sums, own.count_only, counts);
}

// The head of the three packs: the count pass over the candidate masks (slice `self` skipped)
// and the scan of the chunk counts into pk_off.  cps: chunks per slice.
static int ms_pack_head(tgo_ctx* ctx, uint64_t* cand_global, int32_t nranks, int64_t* send, int self, int64_t& cps,
                        int64_t& nchunks) {
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    cps = (g.n + kPackChunk - 1) / kPackChunk;
    nchunks = cps * nranks;
    if (!s.pk_cnt) {
        HIP_TRY(dev_alloc(ctx, s.pk_cnt, g.n_global / kPackChunk + kMaxRanks + 1));
        HIP_TRY(dev_alloc(ctx, s.pk_off, g.n_global / kPackChunk + kMaxRanks + 1));
    }
    HIP_TRY(hipMemsetAsync(s.pk_cnt + nchunks, 0, sizeof(int64_t), st));
    HIP_TRY(k_ms_pack(false, cand_global, g.n, cps, nchunks, s.pk_cnt, s.pk_off, send, st, s.pk_touch, self));
    HIP_TRY(scan_exclusive_i64(s.cub_tmp, s.cub_bytes, s.pk_cnt, s.pk_off, nchunks + 1, st));
    return TGO_OK;
}

// Device form of tgo_part_ms_pack: no host synchronisation — the split sizes (int64
// elements, 2 per pair) go to send_elems_dev for the caller's device all-to-all.
int part_ms_pack_dev(tgo_ctx* ctx, uint64_t* cand_global, int32_t nranks, int64_t* send, int64_t* send_elems_dev, int self) {
    int rc = part_check(ctx);
    if (rc) return rc;
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    if (!cand_global || !send || !send_elems_dev || nranks < 1 || nranks > kMaxRanks ||
        static_cast<int64_t>(nranks) * g.n != g.n_global)
        return fail(ctx, TGO_E_INVALID, "ms_pack_dev: bad arguments (nranks * n_local must equal n_global)");
    hipStream_t st = ctx->stream;
    int64_t cps = 0, nchunks = 0;
    if ((rc = ms_pack_head(ctx, cand_global, nranks, send, self, cps, nchunks))) return rc;
    HIP_TRY(k_slice_elems(s.pk_off, cps, nranks, send_elems_dev, st));
    HIP_TRY(k_ms_pack(true, cand_global, g.n, cps, nchunks, s.pk_cnt, s.pk_off, send, st, s.pk_touch, self));
    return part_done(ctx);
}

// Fixed-capacity sparse exchange (msbfs.hip ms_pack_fixed): owner r's slot of `send` is
// 2 * (cap + 1) int64 (header + pairs), so the caller's all-to-all has equal splits.
int part_ms_pack_fixed(tgo_ctx* ctx, uint64_t* cand_global, int32_t nranks, int64_t cap, int64_t* send, int self) {
    int rc = part_check(ctx);
    if (rc) return rc;
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    if (!cand_global || !send || nranks < 1 || nranks > kMaxRanks || cap < 1 || cap > g.n ||
        static_cast<int64_t>(nranks) * g.n != g.n_global)
        return fail(ctx, TGO_E_INVALID, "ms_pack_fixed: bad arguments (1 <= cap <= n_local, nranks * n_local == n_global)");
    if (!s.pk_ovf) return fail(ctx, TGO_E_STATE, "ms_pack_fixed before ms_begin");
    int64_t cps = 0, nchunks = 0;
    if ((rc = ms_pack_head(ctx, cand_global, nranks, send, self, cps, nchunks))) return rc;
    HIP_TRY(k_ms_pack_fixed(cand_global, g.n, cps, nchunks, s.pk_off, nranks, cap, send, s.pk_ovf, s.pk_touch, ctx->stream,
                            self));
    return part_done(ctx);
}

}  // namespace tgo
extern "C" {

int tgo_part_ms_or_fixed(tgo_ctx* ctx, const int64_t* recv, int32_t nslices, int64_t cap, uint64_t* fr_next) {
    return part_ms_or(ctx, MsRecv::fixed(recv, nslices, cap), fr_next, MsOwn{});
}

int tgo_part_ms_or_pairs(tgo_ctx* ctx, const int64_t* recv, const int64_t* recv_counts, int32_t nslices,
                         uint64_t* fr_next) {
    return part_ms_or(ctx, MsRecv::pairs(recv, recv_counts, nslices), fr_next, MsOwn{});
}

// One pull level over the gathered frontier masks.  sparse (null: none): the sources a split
// level pushed instead — they stay out of the pull, and with cand_in_next their candidates are
// in fr_next already (tgo_part_ms_or_*).
static int ms_pull(tgo_ctx* ctx, int32_t level, const uint64_t* fr_global, uint64_t* fr_next, const uint64_t* sparse,
                   int32_t cand_in_next, int64_t* counts) {
    int rc = part_check(ctx);
    if (rc) return rc;
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    const View pull = pull_view(g, TGO_SCOPE_BOTH_E), push = push_view(g, TGO_SCOPE_BOTH_E);
    const uint64_t full = s.ms_nsrc == 64 ? ~0ULL : ((1ULL << s.ms_nsrc) - 1ULL);
    if ((rc = ms_level_planes(ctx, level))) return rc;
    HIP_TRY(hipMemsetAsync(s.cnt, 0, sizeof(Counters), st));
    // the pull writes every active row's mask; the entry-less tail is zero already (no
    // entry-less seed enters a mask, tgo_part_ms_begin)
    const int nxt = ctx->part_cur ^ 1;
    HIP_TRY(k_ms_pull(pull, push, g.n_active, full, fr_global, nullptr, s.ms_vis, fr_next, ms_planes(ctx), s.cnt,
                      level + 1, st, 0, sparse ? full & ~*sparse : ~0ULL, cand_in_next ? fr_next : nullptr));
    ctx->part_cur = nxt;
    ctx->part_queued = false;       // counted only: ms_push builds the queue if it needs one
    return part_counts(ctx, counts);
}

int tgo_part_ms_pull_split(tgo_ctx* ctx, int32_t level, const uint64_t* fr_global, uint64_t* fr_next, uint64_t sparse,
                           int32_t cand_in_next, int64_t* counts) {
    return ms_pull(ctx, level, fr_global, fr_next, &sparse, cand_in_next, counts);
}

int tgo_part_ms_pull(tgo_ctx* ctx, int32_t level, const uint64_t* fr_global, uint64_t* fr_next, int64_t* counts) {
    return ms_pull(ctx, level, fr_global, fr_next, nullptr, 0, counts);
}

int tgo_part_ms_push(tgo_ctx* ctx, int32_t level, const uint64_t* fr_local, uint64_t* cand_global) {
    (void)level;
    return part_ms_push(ctx, fr_local, cand_global, nullptr, -1);
}

int tgo_part_ms_settle(tgo_ctx* ctx, int32_t level, const uint64_t* recv, int32_t nslices, uint64_t* fr_next,
                       int64_t* counts) {
    int rc = part_check(ctx);
    if (rc) return rc;
    if ((rc = ms_level_planes(ctx, level))) return rc;
    HIP_TRY(hipMemsetAsync(ctx->sc.cnt, 0, sizeof(Counters), ctx->stream));
    HIP_TRY(k_or_slices(recv, nslices, ctx->g.n, fr_next, ctx->stream));
    return ms_settle_tail(ctx, level, fr_next, nullptr, false, counts);
}

int tgo_part_ms_pack(tgo_ctx* ctx, uint64_t* cand_global, int32_t nranks, int64_t* send, int64_t* send_counts) {
    int rc = part_check(ctx);
    if (rc) return rc;
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    if (!cand_global || !send || !send_counts || nranks < 1 || nranks > kMaxRanks ||
        static_cast<int64_t>(nranks) * g.n != g.n_global)
        return fail(ctx, TGO_E_INVALID, "ms_pack: bad arguments (nranks * n_local must equal n_global)");
    hipStream_t st = ctx->stream;
    int64_t cps = 0, nchunks = 0;
    if ((rc = ms_pack_head(ctx, cand_global, nranks, send, -1, cps, nchunks))) return rc;
    std::vector<int64_t> off(nranks + 1);
    for (int r = 0; r <= nranks; ++r)     // offsets at the slice boundaries (pk_cnt[nchunks] is 0)
        HIP_TRY(hipMemcpyAsync(&off[r], s.pk_off + r * cps, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int r = 0; r < nranks; ++r) send_counts[r] = off[r + 1] - off[r];
    if (off[nranks] > 0) HIP_TRY(k_ms_pack(true, cand_global, g.n, cps, nchunks, s.pk_cnt, s.pk_off, send, st, s.pk_touch));
    return part_done(ctx);
}

int tgo_part_ms_pack_dev(tgo_ctx* ctx, uint64_t* cand_global, int32_t nranks, int64_t* send, int64_t* send_elems_dev) {
    return part_ms_pack_dev(ctx, cand_global, nranks, send, send_elems_dev, -1);
}

int tgo_part_ms_pack_fixed(tgo_ctx* ctx, uint64_t* cand_global, int32_t nranks, int64_t cap, int64_t* send) {
    return part_ms_pack_fixed(ctx, cand_global, nranks, cap, send, -1);
}

int tgo_part_ms_settle_fixed(tgo_ctx* ctx, int32_t level, const int64_t* recv, int32_t nslices, int64_t cap,
                             uint64_t* fr_next, int64_t* counts) {
    return part_ms_settle(ctx, level, MsRecv::fixed(recv, nslices, cap), fr_next, MsOwn{}, counts);
}

int tgo_part_ms_settle_pairs(tgo_ctx* ctx, int32_t level, const int64_t* recv, const int64_t* recv_counts,
                             int32_t nslices, uint64_t* fr_next, int64_t* counts) {
    return part_ms_settle(ctx, level, MsRecv::pairs(recv, recv_counts, nslices), fr_next, MsOwn{}, counts);
}

int tgo_part_ms_end(tgo_ctx* ctx, int64_t* reached, int64_t* entries) {
    int rc = part_check(ctx);
    if (rc) return rc;
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    HIP_TRY(hipEventRecord(ctx->ev1, st));
    if (reached || entries) {
        HIP_TRY(hipMemsetAsync(s.ms_stat, 0, 2 * TGO_MAX_SOURCES * sizeof(unsigned long long), st));
        HIP_TRY(k_ms_reach(pull_view(ctx->g, TGO_SCOPE_BOTH_E), s.ms_vis, ctx->g.n, s.ms_nsrc, s.ms_stat,
                           s.ms_stat + TGO_MAX_SOURCES, st));
        std::vector<unsigned long long> h(2 * TGO_MAX_SOURCES);
        HIP_TRY(hipMemcpyAsync(h.data(), s.ms_stat, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (int r = 0; r < s.ms_nsrc; ++r) {
            if (reached) reached[r] = static_cast<int64_t>(h[r]);
            if (entries) entries[r] = static_cast<int64_t>(h[TGO_MAX_SOURCES + r]);
        }
    }
    // the fixed-capacity exchange (tgo_part_ms_pack_fixed) drops the pairs past an owner's
    // capacity: a sweep that overflowed has wrong levels and fails here
    int ovf = 0;
    if (s.pk_ovf) HIP_TRY(hipMemcpyAsync(&ovf, s.pk_ovf, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (ovf) return fail(ctx, TGO_E_STATE, "ms_pack_fixed: an owner's pairs exceeded the capacity (cap below the level's frontier entries)");
    return program_elapsed(ctx);        // (one stream wait, as tgo_part_bfs_end)
}

int tgo_part_ms_levels(tgo_ctx* ctx, int32_t source, int64_t* dist_local) {
    int rc = part_check(ctx);
    if (rc) return rc;
    Scratch& s = ctx->sc;
    if (!s.ms_vis || source < 0 || source >= s.ms_nsrc || !dist_local) return fail(ctx, TGO_E_INVALID, "bad source");
    HIP_TRY(k_ms_extract(ms_planes(ctx), s.ms_nplanes, s.ms_vis, ctx->g.perm, source, s.msg, ctx->g.n, ctx->stream));
    HIP_TRY(hipMemcpyAsync(dist_local, s.msg, ctx->g.n * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return TGO_OK;
}

int tgo_part_active_rows(tgo_ctx* ctx, int64_t* n_active) {
    int rc = part_check(ctx);
    if (rc) return rc;
    if (!n_active) return fail(ctx, TGO_E_INVALID, "null argument");
    *n_active = ctx->g.n_active;
    return TGO_OK;
}

// The longest in-row of this rank's rows, and the longest of any rank as the driver agreed it
// (all-reduce MAX) before tgo_part_pr_blocked: the blocked layout's fixed-point range comes from it.
int tgo_part_pr_longest_row(tgo_ctx* ctx, int64_t* longest_row) {
    int rc = part_check(ctx);
    if (rc) return rc;
    if (!longest_row) return fail(ctx, TGO_E_INVALID, "null argument");
    *longest_row = ctx->part_max_in_row;
    return TGO_OK;
}

int tgo_part_pr_set_longest_row(tgo_ctx* ctx, int64_t longest_row) {
    int rc = part_check(ctx);
    if (rc) return rc;
    if (longest_row < ctx->part_max_in_row)
        return fail(ctx, TGO_E_INVALID, "tgo_part_pr_set_longest_row: shorter than this rank's longest in-row");
    ctx->part_pr_job_row = longest_row;
    return TGO_OK;
}

// Cache-blocked partitioned PageRank.  The gathered contribution vector is laid out hot-first
// across ranks: [rank 0 rows 0..H) ... [rank W-1 rows 0..H) | [rank 0 rows H..A) ... — the
// degree-grouped layout puts each rank's hottest rows first and its entry-less rows last, so
// the first W*H sources are the job's hot set and rows >= A are never anyone's source.  The
// owned in-lists are re-expressed in that index space and cache-blocked as on one GPU.
int tgo_part_pr_blocked(tgo_ctx* ctx, int32_t world, int64_t active_span, int64_t* hot_per_rank) {
    int rc = part_check(ctx);
    if (rc) return rc;
    DevGraph& g = ctx->g;
    const int64_t nl = g.n;
    if (!hot_per_rank || world < 1 || g.n_global != static_cast<int64_t>(world) * nl)
        return fail(ctx, TGO_E_INVALID, "tgo_part_pr_blocked: world must equal n_global / n_local");
    if (active_span < g.n_active || active_span > nl)
        return fail(ctx, TGO_E_INVALID, "tgo_part_pr_blocked: active_span must cover every rank's active rows");
    *hot_per_rank = 0;
    if (g.scope == TGO_SCOPE_BOTH_E || env_i64("TGO_PR_BLOCKED", 1) == 0) {
        ctx->part_pr_world = 0;
        return TGO_OK;                                  // plain layout: one rank-major all-gather
    }
    int64_t H = env_i64("TGO_PR_HOT", pr_hot_default()) / world;
    H = std::min(active_span, std::max<int64_t>(64, H / 64 * 64));
    // the fixed-point range is the job's: from the longest in-row of ANY rank (agreed by the
    // driver, tgo_part_pr_set_longest_row), so what a rank with short rows emits is checked
    // against the range of the peer that sums the longest row
    const int64_t job_row = std::max(ctx->part_pr_job_row, ctx->part_max_in_row);
    if (ctx->part_pr_world == world && ctx->part_pr_hot == H && ctx->part_pr_span == active_span &&
        ctx->part_pr_built_row == job_row) {
        *hot_per_rank = H;
        return TGO_OK;                                  // already built for this layout
    }
    TrimTemps trim_temps;
    const int64_t A = active_span, W = world;
    std::vector<int64_t> off(nl + 1);
    HIP_TRY(hipMemcpy(off.data(), g.in.off, (nl + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
    // the in-lists' sources as positions in the blocked gathered vector, mapped on the device;
    // the cold layout is built from that device copy (pr_layout.hip), as on one GPU
    const int64_t nnz = g.in.nnz;
    int32_t* gidx = nullptr;
    int* bad = nullptr;
    HIP_TRY(hipMalloc(&gidx, std::max<int64_t>(nnz, 1) * sizeof(int32_t)));
    struct Free { void* p; ~Free() { if (p) (void)hipFree(p); } } free_gidx{gidx};
    HIP_TRY(hipMalloc(&bad, sizeof(int)));
    Free free_bad{bad};
    HIP_TRY(hipMemsetAsync(bad, 0, sizeof(int), ctx->stream));
    HIP_TRY(k_part_gathered_index(g.in.adj, nnz, nl, A, H, W, gidx, bad, ctx->stream));
    int hbad = 0;
    HIP_TRY(hipMemcpyAsync(&hbad, bad, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (hbad) return fail(ctx, TGO_E_INVALID, "tgo_part_pr_blocked: a source row lies beyond active_span");
    // the mapping is not monotone in the global id: re-sort each row so the device build applies
    if (!host_assembly()) {
        std::string err;
        if (int r = sort_rows_device(g.in.off, nl, gidx, nnz, ctx->stream, err)) return fail(ctx, r, err);
    }
    bool ready = false;
    const std::vector<int32_t> no_host_adj;
    if ((rc = upload_cold_blocks(ctx, off, no_host_adj, W * A, W * H, g.n_active, g.cold_in, ready, g.in.off, gidx, nnz, 0,
                                 job_row)))
        return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    g.cold_in_ready = ready;
    if (!ready) { ctx->part_pr_world = 0; return TGO_OK; }
    Scratch& s = ctx->sc;
    if (g.cold_in.rb_hot.nchunks > s.partial_cap) {
        s.partial_cap = g.cold_in.rb_hot.nchunks;
        HIP_TRY(dev_alloc(ctx, s.partial, s.partial_cap));
    }
    ctx->part_pr_world = world;
    ctx->part_pr_hot = H;
    ctx->part_pr_span = A;
    ctx->part_pr_built_row = job_row;
    ctx->st.device_bytes = ctx->dev_bytes;
    *hot_per_rank = H;
    return TGO_OK;
}

int tgo_part_pr_begin(tgo_ctx* ctx, const tgo_pr_args* a, double* contrib_local) {
    int rc = part_check(ctx);
    if (rc) return rc;
    if (!a || a->max_iterations < 1) return fail(ctx, TGO_E_INVALID, "partitioned PageRank needs max_iterations >= 1");
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    const double N = static_cast<double>(a->vertex_count);
    ctx->part_alpha = a->alpha;
    ctx->part_base = (1.0 - a->alpha) / N;
    ctx->part_pr_iter = 1;
    ctx->part_pr_iters = a->max_iterations;
    if (!ctx->part_pr_plain) ctx->st.exact_reruns = 0;
    HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
    // iteration 1 (PageRankVertexProgram.java:78-83) on the owned rows
    HIP_TRY(k_pr_init(g.out, s.vec[0], contrib_local, reinterpret_cast<double*>(s.dist), 1.0 / N, g.n, ctx->stream));
    return part_done(ctx);
}

static bool part_pr_blocked_ready(const tgo_ctx* ctx) {
    return ctx->part_pr_world > 0 && ctx->g.cold_in_ready && !ctx->part_pr_plain;
}

// The fixed-point passes' range flag of the last partitioned PageRank (read and cleared).
int tgo_part_pr_exact_check(tgo_ctx* ctx, int32_t* bad) {
    int rc = part_check(ctx);
    if (rc) return rc;
    if (!bad) return fail(ctx, TGO_E_INVALID, "null argument");
    bool b = false;
    if (part_pr_blocked_ready(ctx) && (rc = fx_take_bad(ctx, ctx->g.cold_in, &b))) return rc;
    *bad = b ? 1 : 0;
    return TGO_OK;
}

// Run the next partitioned PageRank programs on the plain layout (rank-major n_local slices,
// fp64 gather) while on = 1, keeping the blocked layout for later ones.
int tgo_part_pr_plain(tgo_ctx* ctx, int32_t on) {
    int rc = part_check(ctx);
    if (rc) return rc;
    ctx->part_pr_plain = on != 0;
    if (on) ctx->st.exact_reruns = 1;                // the stats of the program that re-runs
    return TGO_OK;
}

// the PAGE_RANK property is only read after the last superstep: write it there
static double* part_pr_out(tgo_ctx* ctx) {
    return ctx->part_pr_iter + 1 == ctx->part_pr_iters ? reinterpret_cast<double*>(ctx->sc.dist) : nullptr;
}

int tgo_part_pr_step_cold(tgo_ctx* ctx, const double* gathered) {
    int rc = part_check(ctx);
    if (rc) return rc;
    if (!part_pr_blocked_ready(ctx)) return fail(ctx, TGO_E_STATE, "tgo_part_pr_step_cold needs tgo_part_pr_blocked");
    HIP_TRY(k_pr_cold_phase(ctx->g.cold_in, gathered, ctx->stream, ctx->part_pr_iter == 1));
    return part_done(ctx);
}

int tgo_part_pr_step_hot(tgo_ctx* ctx, const double* gathered, double* contrib_local) {
    int rc = part_check(ctx);
    if (rc) return rc;
    if (!part_pr_blocked_ready(ctx)) return fail(ctx, TGO_E_STATE, "tgo_part_pr_step_hot needs tgo_part_pr_blocked");
    if (ctx->part_pr_iter >= ctx->part_pr_iters) return fail(ctx, TGO_E_STATE, "PageRank program already complete");
    Scratch& s = ctx->sc;
    HIP_TRY(k_pr_hot_phase(ctx->g.cold_in, gathered, s.vec[0], part_pr_out(ctx), contrib_local, s.partial,
                           ctx->part_alpha, ctx->part_base, ctx->stream, ctx->part_pr_iter == 1));
    ++ctx->part_pr_iter;
    return part_done(ctx);
}

int tgo_part_pr_step(tgo_ctx* ctx, const double* contrib_global, double* contrib_local) {
    int rc = part_check(ctx);
    if (rc) return rc;
    if (part_pr_blocked_ready(ctx)) {
        if ((rc = tgo_part_pr_step_cold(ctx, contrib_global))) return rc;
        return tgo_part_pr_step_hot(ctx, contrib_global, contrib_local);
    }
    if (ctx->part_pr_iter >= ctx->part_pr_iters) return fail(ctx, TGO_E_STATE, "PageRank program already complete");
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    // owned rows gather over their IN lists (global source ids) from the gathered vector
    HIP_TRY(k_pr_iter(g.in, g.rb_in, contrib_global, s.vec[0], part_pr_out(ctx), contrib_local, s.partial,
                      ctx->part_alpha, ctx->part_base, g.n, PrTuning{}, ctx->stream));
    ++ctx->part_pr_iter;
    return part_done(ctx);
}

int tgo_part_pr_end(tgo_ctx* ctx, double* pr_local) {
    int rc = part_check(ctx);
    if (rc) return rc;
    if (ctx->part_pr_iter != ctx->part_pr_iters)
        return fail(ctx, TGO_E_STATE, "partitioned PageRank ended before its last iteration");
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    double* pr = reinterpret_cast<double*>(s.dist);
    // blocked updates skip the entry-less rows: their rank after any update is (1-a)/N
    if (part_pr_blocked_ready(ctx) && ctx->part_pr_iters >= 2 && g.cold_in.n_rows < g.n)
        HIP_TRY(k_fill_f64(pr + g.cold_in.n_rows, ctx->part_base, g.n - g.cold_in.n_rows, ctx->stream));
    HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
    if (pr_local && (rc = rows_out_async(ctx, s.dist, pr_local))) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return program_elapsed(ctx);        // (one stream wait, as tgo_part_bfs_end)
}

// ---- partitioned delta-stepping SSSP (delta.hip; exchange protocol: titan_amd/distributed.py)
static int ds_part_alloc(tgo_ctx* ctx) {
    Scratch& s = ctx->sc;
    if (s.ds_rbest) return TGO_OK;
    HIP_TRY(dev_alloc(ctx, s.ds_rbest, ctx->g.n_global));
    HIP_TRY(dev_alloc(ctx, s.ds_rmark, ctx->g.n_global / 64 + 1));
    HIP_TRY(dev_alloc(ctx, s.ds_pack, 3 * kMaxRanks + 2));
    return TGO_OK;
}
// the loop state words after the pack counters (delta.hip ds_track_reset)
static long long* ds_track(Scratch& s) { return reinterpret_cast<long long*>(s.ds_pack + 3 * kMaxRanks); }

int tgo_part_sssp_begin(tgo_ctx* ctx, int64_t seed_global, int64_t delta, int64_t* out) {
    int rc = part_check(ctx);
    if (rc) return rc;
    DevGraph& g = ctx->g;
    if (g.has_weight && g.min_weight < 0) return fail(ctx, TGO_E_INVALID, "delta-stepping needs non-negative weights");
    if ((rc = ds_part_alloc(ctx))) return rc;
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    const int64_t n = g.n;
    const View push = push_view(g, g.scope);
    HIP_TRY(hipEventRecord(ctx->ev0, st));
    HIP_TRY(k_fill_i64(s.dist, INT64_MAX, n, st));
    HIP_TRY(hipMemsetAsync(s.vb, 0, ((n + 63) / 64 + 1) * 8, st));
    HIP_TRY(k_fill_i64(s.ds_rbest, INT64_MAX, g.n_global, st));
    HIP_TRY(hipMemsetAsync(s.ds_rmark, 0, (g.n_global / 64 + 1) * 8, st));
    HIP_TRY(hipMemsetAsync(s.ds_pack, 0, 3 * kMaxRanks * sizeof(unsigned long long), st));
    HIP_TRY(k_ds_track_reset(ds_track(s), st));
    ctx->part_cur = 0;
    ctx->part_qlen = 0;
    ctx->part_qlen_stale = false;
    ctx->part_relaxed = 0;
    ctx->part_phases = 0;
    ctx->part_seed = -1;
    ctx->part_split = false;
    ctx->part_devloop = false;
    int64_t seed = seed_global - g.lo;
    if (seed >= 0 && seed < n) {
        seed = ctx->perm[seed];
        HIP_TRY(k_ds_seed(push, s.dist, s.q[0], s.qdeg, seed, st));
        ctx->part_qlen = 1;
        ctx->part_seed = seed;
    }
    HIP_TRY(hipStreamSynchronize(st));
    if (out) {
        out[0] = ctx->part_qlen;
        out[1] = delta > 0 ? delta : default_delta(g, g.has_weight);
    }
    return TGO_OK;
}

// The smallest weight of the rank's load (0 without weights).  Delta-stepping refuses negative
// weights; the drivers agree on the global minimum BEFORE the first collective, so every rank
// fails together instead of one rank failing while its peers wait in an exchange.
int tgo_part_weight_min(tgo_ctx* ctx, int64_t* min_weight) {
    int rc = part_check(ctx);
    if (rc) return rc;
    if (!min_weight) return fail(ctx, TGO_E_INVALID, "null argument");
    *min_weight = ctx->g.has_weight ? ctx->g.min_weight : 0;
    return TGO_OK;
}

// The relax half of a phase.  send_counts (host) set: the pair counts come back to the host
// (one stream synchronisation); sizes (device) set instead: the exchange header is written on
// the device (ds_mark_sizes) and nothing waits.
static int part_sssp_relax_impl(tgo_ctx* ctx, int64_t thr, int32_t nranks, int64_t* send, int64_t* send_counts,
                                int64_t* sizes) {
    int rc = part_check(ctx);
    if (rc) return rc;
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    if (!s.ds_rbest) return fail(ctx, TGO_E_STATE, "tgo_part_sssp_begin has not run");
    if (nranks < 1 || nranks > kMaxRanks || g.n * nranks != g.n_global || !send || (!send_counts && !sizes))
        return fail(ctx, TGO_E_INVALID, "nranks * n_local must equal n_global (equal partitions, <= 64 ranks)");
    hipStream_t st = ctx->stream;
    const View push = push_view(g, g.scope);
    const int cur = ctx->part_cur;
    if (ctx->part_split && ctx->part_qlen > 0) {      // commit_ws zeroes the counters and the scan's tail
        const int64_t ql = ctx->part_qlen;
        HIP_TRY(k_ds_commit_ws(s.q[cur], ql, s.dist, s.msg, s.vb, s.ds_member, s.qdeg, s.cnt, st, ds_track(s)));
        HIP_TRY(scan_exclusive_i64(s.cub_tmp, s.cub_bytes, s.qdeg, s.qpre, ql + 1, st));
        HIP_TRY(k_ds_relax_ws_part(s.ds_pws, s.ds_light, s.q[cur], s.qpre, ql, s.msg, s.dist, s.vb, s.q[cur ^ 1], s.qdeg,
                                   s.cnt, thr, g.lo, g.n, s.ds_rbest, s.ds_rmark, ds_track(s), st));
    } else {
        HIP_TRY(hipMemsetAsync(s.cnt, 0, sizeof(Counters), st));
    }
    if (!ctx->part_split && ctx->part_qlen > 0) {
        HIP_TRY(k_ds_commit(s.q[cur], ctx->part_qlen, s.dist, s.msg, s.vb, st));
        if ((rc = scan_frontier(ctx, ctx->part_qlen))) return rc;
        HIP_TRY(k_ds_relax_part(push, s.q[cur], s.qpre, ctx->part_qlen, s.msg, s.dist, s.vb, s.q[cur ^ 1], s.qdeg,
                                s.cnt, g.has_weight ? 1 : 0, thr, g.lo, g.n, s.ds_rbest, s.ds_rmark, ds_track(s), st));
    }
    unsigned long long* counts = s.ds_pack;
    unsigned long long* offs = counts + kMaxRanks;
    unsigned long long* cursor = offs + kMaxRanks;
    // device header: the counts / cursors are zero here (begin, then every ds_mark_sizes)
    if (send_counts) HIP_TRY(hipMemsetAsync(counts, 0, 3 * kMaxRanks * sizeof(unsigned long long), st));
    const int64_t words = g.n_global / 64, wpr = g.n / 64;
    if (!send_counts && nranks == 1) {      // one rank owns every target: nothing is ever marked
        HIP_TRY(k_ds_mark_sizes(counts, nranks, ctx->part_qlen, offs, cursor, ds_track(s), sizes, st));
        return part_done(ctx);
    }
    HIP_TRY(k_ds_mark_count(s.ds_rmark, words, wpr, counts, st));
    if (!send_counts) {
        HIP_TRY(k_ds_mark_sizes(counts, nranks, ctx->part_qlen, offs, cursor, ds_track(s), sizes, st));
        HIP_TRY(k_ds_mark_pack(s.ds_rmark, words, wpr, g.n, s.ds_rbest, offs, cursor, send, st));
        return part_done(ctx);
    }
    unsigned long long h[kMaxRanks], ho[kMaxRanks];
    HIP_TRY(hipMemcpyAsync(h, counts, nranks * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    unsigned long long acc = 0;
    for (int r = 0; r < nranks; ++r) {
        ho[r] = acc;
        acc += h[r];
        send_counts[r] = static_cast<int64_t>(h[r]);
    }
    HIP_TRY(hipMemcpyAsync(offs, ho, nranks * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
    HIP_TRY(k_ds_mark_pack(s.ds_rmark, words, wpr, g.n, s.ds_rbest, offs, cursor, send, st));
    return part_done(ctx);          // the caller's exchange follows on the same stream
}

int tgo_part_sssp_relax(tgo_ctx* ctx, int64_t thr, int32_t nranks, int64_t* send, int64_t* send_counts) {
    if (ctx && !send_counts) return fail(ctx, TGO_E_INVALID, "null send_counts");
    return part_sssp_relax_impl(ctx, thr, nranks, send, send_counts, nullptr);
}

int tgo_part_sssp_apply(tgo_ctx* ctx, int64_t thr, const int64_t* recv, int64_t npairs, int64_t* counts) {
    int rc = part_check(ctx);
    if (rc) return rc;
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    if (!s.ds_rbest) return fail(ctx, TGO_E_STATE, "tgo_part_sssp_begin has not run");
    if (npairs < 0 || (npairs > 0 && !recv)) return fail(ctx, TGO_E_INVALID, "bad received pairs");
    hipStream_t st = ctx->stream;
    if (npairs > 0)
        HIP_TRY(k_ds_apply(push_view(g, g.scope), recv, npairs, s.dist, s.vb, s.q[ctx->part_cur ^ 1], s.qdeg, s.cnt,
                           thr, ctx->part_split ? s.ds_pws.off : nullptr, ctx->part_split ? s.ds_light : nullptr,
                           ds_track(s), st));
    if ((rc = read_counters(ctx))) return rc;
    if (s.hcnt->err) return fail(ctx, TGO_E_PROGRAM,
        "vertex program failed: a traversed edge has no value for the weight property");
    if (ctx->part_qlen > 0) ctx->part_relaxed += static_cast<int64_t>(s.hcnt->red[1]);
    ctx->part_cur ^= 1;
    ctx->part_qlen = static_cast<int64_t>(s.hcnt->qlen);
    ctx->part_qlen_stale = false;
    ++ctx->part_phases;
    if (counts) {
        counts[0] = ctx->part_qlen;
        counts[1] = static_cast<int64_t>(s.hcnt->mf);
    }
    return TGO_OK;
}

int tgo_part_sssp_pending_min(tgo_ctx* ctx, int64_t* out) {
    int rc = part_check(ctx);
    if (rc) return rc;
    Scratch& s = ctx->sc;
    if (!out) return fail(ctx, TGO_E_INVALID, "null output");
    hipStream_t st = ctx->stream;
    HIP_TRY(hipMemsetAsync(s.cnt, 0, sizeof(Counters), st));
    HIP_TRY(hipMemsetAsync(&s.cnt->red[0], 0x7F, sizeof(unsigned long long), st));
    HIP_TRY(k_ds_pending_min(s.vb, (ctx->g.n + 63) / 64, s.dist, s.cnt, st));
    if ((rc = read_counters(ctx))) return rc;
    out[1] = static_cast<int64_t>(s.hcnt->red[1]);
    out[0] = out[1] ? static_cast<int64_t>(s.hcnt->red[0]) : INT64_MAX;
    return TGO_OK;
}

int tgo_part_sssp_extract(tgo_ctx* ctx, int64_t thr, int64_t* counts) {
    int rc = part_check(ctx);
    if (rc) return rc;
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    HIP_TRY(hipMemsetAsync(s.cnt, 0, sizeof(Counters), st));
    if (!s.ds_rbest) return fail(ctx, TGO_E_STATE, "tgo_part_sssp_begin has not run");
    HIP_TRY(k_ds_track_reset(ds_track(s), st));     // the extraction sets the pending minimum afresh
    if (ctx->part_split)            // the new near queue (light) and the settled members' heavy entries
        HIP_TRY(k_ds_extract_ws(s.ds_pws, s.ds_light, s.vb, s.ds_member, g.n, s.dist, thr, s.q[ctx->part_cur], s.qdeg,
                                s.cnt, st, ds_track(s)));
    else
        HIP_TRY(k_ds_extract(push_view(g, g.scope), s.vb, g.n, s.dist, thr, s.q[ctx->part_cur], s.qdeg, s.cnt, st,
                             ds_track(s)));
    return part_counts(ctx, counts, false);   // the SSSP driver reads counts on the host
}

int tgo_part_sssp_end(tgo_ctx* ctx, int64_t* dist_local, int64_t* reached) {
    int rc = part_check(ctx);
    if (rc) return rc;
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    if (ctx->part_devloop) {            // the device loop's counts and failure flag
        DsLoop h{};
        HIP_TRY(hipMemcpyAsync(&h, s.ds_loop, sizeof(DsLoop), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        ctx->part_devloop = false;
        if (h.err) return fail(ctx, TGO_E_PROGRAM,
            "vertex program failed: a traversed edge has no value for the weight property");
        ctx->part_relaxed = static_cast<int64_t>(h.relaxed);
        ctx->part_phases = static_cast<int32_t>(h.phases);
    }
    HIP_TRY(k_dist_finalize(s.dist, g.n, st));
    HIP_TRY(hipEventRecord(ctx->ev1, st));
    if (reached && (rc = reach_stats(ctx, g.scope, reached))) return rc;
    if (dist_local && (rc = rows_out_async(ctx, s.dist, dist_local))) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    if ((rc = program_elapsed(ctx))) return rc;     // (one stream wait, as tgo_part_bfs_end)
    ctx->st.relaxed_entries = ctx->part_relaxed;
    ctx->st.levels = ctx->part_phases;
    return TGO_OK;
}

}  // extern "C"

// accessors for the C++ partitioned driver (part_driver.cpp)
namespace tgo {
// tgo_part_sssp_relax with the exchange header (sizes, 2 * nranks words) written on the device
int part_sssp_relax_dev(tgo_ctx* ctx, int64_t thr, int32_t nranks, int64_t* send, int64_t* sizes) {
    if (!sizes) return fail(ctx, TGO_E_INVALID, "null sizes");
    return part_sssp_relax_impl(ctx, thr, nranks, send, nullptr, sizes);
}
// The header fold after the driver's header all-to-all (delta.hip ds_header_fold).
int part_sssp_header_fold(tgo_ctx* ctx, const int64_t* own, const int64_t* recv, int nranks, int64_t* out) {
    HIP_TRY(k_ds_header_fold(own, recv, nranks, out, ctx->stream));
    return TGO_OK;
}
// ... and its 2 * nranks + 3 words to the host in the same launch (through the mapped counter
// page: part_read_words without its own publish kernel).
int part_sssp_header_read(tgo_ctx* ctx, const int64_t* own, const int64_t* recv, int nranks, int64_t* out,
                          int64_t* words) {
    Scratch& s = ctx->sc;
    const int count = 2 * nranks + 3;
    if (!s.hcnt || count > kCounterWords) return fail(ctx, TGO_E_STATE, "part_sssp_header_read");
    const unsigned long long seq = ++s.pub_seq;
    HIP_TRY(k_ds_header_fold(own, recv, nranks, out, ctx->stream, s.hcnt_dev, seq));
    if (int rc = wait_publish(ctx, seq)) return rc;
    for (int i = 0; i < count; ++i) words[i] = static_cast<int64_t>(host_words(ctx)[i]);
    return TGO_OK;
}
// Switch the run tgo_part_sssp_begin started onto the light/heavy split at bucket width delta
// (weighted loads; TGO_DS_SPLIT=0 keeps the plain form): the push view is split on the device
// (once per width), and the seed re-queued with its light degree.  Returns whether it did.
int part_sssp_split(tgo_ctx* ctx, int64_t delta, bool* on) {
    int rc = part_check(ctx);
    if (rc) return rc;
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    *on = false;
    static const bool enabled = env_i64("TGO_DS_SPLIT", 1) != 0;
    if (!enabled || !g.has_weight || delta <= 0 || !s.ds_rbest) return TGO_OK;
    hipStream_t st = ctx->stream;
    const View push = push_view(g, g.scope);
    const int64_t n = g.n, words = (n + 63) / 64 + 1;
    if (!s.ds_light) {
        HIP_TRY(dev_alloc(ctx, s.ds_light, n + 1));
        HIP_TRY(dev_alloc(ctx, s.ds_member, words));
    }
    if (!s.ds_pws.off) {
        const int64_t nnz = (g.has_transpose ? g.push_t.nnz
                             : g.scope == TGO_SCOPE_IN_E ? g.in.nnz
                             : g.scope == TGO_SCOPE_OUT_E ? g.out.nnz : g.in.nnz + g.out.nnz);
        HIP_TRY(dev_alloc(ctx, s.ds_pws.off, n + 1));
        HIP_TRY(dev_alloc(ctx, s.ds_pws.adj, std::max<int64_t>(nnz, 1)));
        HIP_TRY(dev_alloc(ctx, s.ds_pws.w, std::max<int64_t>(nnz, 1)));
        s.ds_pws.nnz = nnz;
        s.ds_light_delta = -1;
        ctx->st.device_bytes = ctx->dev_bytes;
    }
    if (s.ds_light_delta != delta) {
        HIP_TRY(k_ds_split_rows(push, n, delta, s.ds_pws, s.ds_light, st));
        s.ds_light_delta = delta;
    }
    HIP_TRY(hipMemsetAsync(s.ds_member, 0, words * 8, st));
    if (ctx->part_seed >= 0) HIP_TRY(k_ds_seed_ws(s.ds_pws, s.ds_light, s.dist, s.q[0], s.qdeg, ctx->part_seed, st));
    ctx->part_split = true;
    *on = true;
    // the device-sized loop (TGO_DS_PART_DEVLOOP=0: the host-sized phases above) when the
    // packed queue counters hold a queue (2n + 2 takes, nnz entries), as on one GPU
    static const bool devloop = env_i64("TGO_DS_PART_DEVLOOP", 1) != 0;
    constexpr int64_t kDsMaxCount = int64_t(1) << (64 - kDsCountShift);
    if (devloop && 2 * n + 2 < kDsMaxCount && s.ds_pws.nnz < (int64_t(1) << kDsCountShift)) {
        if (!s.ds_loop) {
            for (int b = 0; b < 2; ++b) {
                HIP_TRY(dev_alloc(ctx, s.ds_q[b], 2 * n + 2));
                HIP_TRY(dev_alloc(ctx, s.ds_qp[b], 2 * n + 2));
            }
            HIP_TRY(dev_alloc(ctx, s.ds_loop, 1));
            ctx->st.device_bytes = ctx->dev_bytes;
        }
        HIP_TRY(k_ds_loop_seed(s.ds_pws, s.ds_light, s.dist, s.ds_q[0], s.ds_qp[0], s.ds_loop, ctx->part_seed, delta, st));
        ctx->part_devloop = true;
        ctx->part_cur = 0;
    }
    return part_done(ctx);
}
// One phase of the device-sized loop, relax half: commit + relax of the current queue (remote
// targets marked), then the exchange header (sizes, 4 words per rank) and the pack.
// fold (one rank only, may be null): the header's fold (part_sssp_header_read's 5 words) read
// here — one rank's header all-to-all is the identity, so the header kernel publishes it.
int part_sssp_dev_relax(tgo_ctx* ctx, int32_t nranks, int64_t* send, int64_t* sizes, int64_t* fold) {
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    if (!ctx->part_devloop || nranks < 1 || nranks > kMaxRanks || g.n * nranks != g.n_global)
        return fail(ctx, TGO_E_STATE, "part_sssp_dev_relax");
    HIP_TRY(k_ds_part_relax(s.ds_pws, s.ds_light, s.vb, s.ds_member, s.dist, s.msg, s.ds_q, s.ds_qp, s.ds_loop,
                            ctx->part_cur, s.ds_light_delta, g.lo, g.n, s.ds_rbest, s.ds_rmark, st));
    unsigned long long* counts = s.ds_pack;
    unsigned long long* offs = counts + kMaxRanks;
    unsigned long long* cursor = offs + kMaxRanks;
    const int64_t words = g.n_global / 64, wpr = g.n / 64;
    if (nranks > 1) HIP_TRY(k_ds_mark_count(s.ds_rmark, words, wpr, counts, st));   // one rank marks nothing
    if (fold) {
        if (nranks != 1 || !s.hcnt) return fail(ctx, TGO_E_STATE, "part_sssp_dev_relax: fold");
        const unsigned long long seq = ++s.pub_seq;
        HIP_TRY(k_ds_part_header(counts, nranks, s.ds_loop, ctx->part_cur, offs, cursor, sizes, st, s.hcnt_dev, seq));
        if (int rc = wait_publish(ctx, seq)) return rc;
        for (int i = 0; i < 5; ++i) fold[i] = static_cast<int64_t>(host_words(ctx)[i]);
        return TGO_OK;
    }
    HIP_TRY(k_ds_part_header(counts, nranks, s.ds_loop, ctx->part_cur, offs, cursor, sizes, st));
    if (nranks > 1) HIP_TRY(k_ds_mark_pack(s.ds_rmark, words, wpr, g.n, s.ds_rbest, offs, cursor, send, st));
    return TGO_OK;
}
// ... apply half: the received pairs into the next queue, which becomes current
int part_sssp_dev_apply(tgo_ctx* ctx, const int64_t* recv, int64_t npairs) {
    Scratch& s = ctx->sc;
    if (!ctx->part_devloop) return fail(ctx, TGO_E_STATE, "part_sssp_dev_apply");
    HIP_TRY(k_ds_part_apply(recv, npairs, s.ds_pws, s.ds_light, s.dist, s.vb, s.ds_q, s.ds_qp, s.ds_loop, ctx->part_cur,
                            ctx->stream));
    ctx->part_cur ^= 1;
    return TGO_OK;
}
// ... after an empty global phase: the next near queue (and the members' heavy entries) below thr
int part_sssp_dev_extract(tgo_ctx* ctx, int64_t thr) {
    Scratch& s = ctx->sc;
    if (!ctx->part_devloop) return fail(ctx, TGO_E_STATE, "part_sssp_dev_extract");
    HIP_TRY(k_ds_part_extract(s.ds_pws, s.ds_light, s.vb, s.ds_member, ctx->g.n, s.dist, s.ds_q, s.ds_qp, s.ds_loop,
                              ctx->part_cur, thr, ctx->stream));
    return TGO_OK;
}
// read_words (ctx.hpp) for part_driver.cpp's loops: at most one publish of words.
int part_read_words(tgo_ctx* ctx, const int64_t* dev, int count, int64_t* out) {
    if (!ctx->sc.hcnt || count < 0 || count > kCounterWords) return fail(ctx, TGO_E_STATE, "part_read_words");
    return read_words(ctx, dev, count, out);
}
int part_in_list(tgo_ctx* ctx, const int32_t** adj, int64_t* nnz) {
    if (int rc = part_check(ctx)) return rc;
    *adj = ctx->g.in.adj;
    *nnz = ctx->g.in.nnz;
    return TGO_OK;
}
int part_out_list(tgo_ctx* ctx, const int32_t** adj, int64_t* nnz) {
    if (int rc = part_check(ctx)) return rc;
    *adj = ctx->g.out.adj;
    *nnz = ctx->g.out.nnz;
    return TGO_OK;
}
// the blocked gathered layout of the last tgo_part_pr_blocked (world 0: plain layout)
int part_pr_layout_of(tgo_ctx* ctx, int32_t* world, int64_t* hot, int64_t* span) {
    if (int rc = part_check(ctx)) return rc;
    const bool blocked = part_pr_blocked_ready(ctx);
    *world = blocked ? ctx->part_pr_world : 0;
    *hot = blocked ? ctx->part_pr_hot : 0;
    *span = blocked ? ctx->part_pr_span : ctx->g.n;
    return TGO_OK;
}
int part_dims(tgo_ctx* ctx, int64_t* n_local, int64_t* lo, int64_t* n_global, int64_t* entries) {
    if (int rc = part_check(ctx)) return rc;
    *n_local = ctx->g.n;
    *lo = ctx->g.lo;
    *n_global = ctx->g.n_global;
    *entries = ctx->g.out.nnz + ctx->g.in.nnz;
    return TGO_OK;
}
int part_scratch(tgo_ctx* ctx, void** p, int64_t bytes, Scratch::DrvSlot slot) {
    Scratch& s = ctx->sc;
    if (slot < 0 || slot >= Scratch::kDrvSlots) return fail(ctx, TGO_E_INVALID, "driver scratch slot");
    if (s.drv_bytes[slot] < bytes) {                // fresh buffers start zero
        uint8_t* q = nullptr;
        HIP_TRY(dev_alloc(ctx, q, bytes));
        HIP_TRY(hipMemsetAsync(q, 0, static_cast<size_t>(bytes), ctx->stream));
        s.drv[slot] = q;
        s.drv_bytes[slot] = bytes;
    }
    *p = s.drv[slot];
    return TGO_OK;
}

}  // namespace tgo
