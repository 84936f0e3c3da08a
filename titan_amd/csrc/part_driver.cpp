// part_driver.cpp — the partitioned (multi-GPU) programs driven from C++: the multi-source BFS
// sweep, single-source BFS, delta-stepping SSSP and PageRank.
//
// titan_amd/distributed.py drives the partitioned programs from Python: every level is a local
// step through the C-ABI plus an RCCL collective through torch.distributed, and each level pays
// Python dispatch and several host round trips.  Each tgo_part_*_run here runs the same protocol
// as one C++ loop over an exchange object (part_exchange.hpp: RCCL in production, an in-process
// group of thread ranks in the tests); the local steps are api_part.cpp's.  The multi-source sweep
// (dense level: in-place all-gather of the owned frontier masks, or the ghost masks only, + pull;
// sparse level: push into candidate masks, packed (owner-local id, mask) pairs in a fixed-
// capacity or sized all-to-all, settle; level counts all-reduced on the device) passes what it
// chooses per level to the steps as arguments (ctx.hpp MsRecv / MsOwn).
// The reference has no multi-process OLAP executor (FulgoraGraphComputer.java:117-311 is one
// JVM); the sweep is the multi-GPU form of ShortestDistanceVertexProgram with unit weights
// (ShortestDistanceVertexProgram.java:96-130) over bothE.
#include <algorithm>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "part_exchange.hpp"

using namespace tgo;

namespace {

using Slot = Scratch::DrvSlot;

// part_scratch (api_part.cpp) for an array of `count` T
template <class T>
int scratch(tgo_ctx* ctx, T*& p, int64_t count, Slot slot) {
    void* q = nullptr;
    const int rc = part_scratch(ctx, &q, count * static_cast<int64_t>(sizeof(T)), slot);
    p = static_cast<T*>(q);
    return rc;
}

// Every loop opens with this: the partition's dimensions checked against the exchange, and the
// driver's `words` device scalars (in `slot`) and pinned host words.
int driver_open(tgo_ctx* ctx, tgo_exchange* x, const char* name, Slot slot, int64_t words, Driver& d, int64_t& nl,
                int64_t& lo, int64_t& ng, int64_t& ent) {
    int rc = part_dims(ctx, &nl, &lo, &ng, &ent);
    if (rc) return rc;
    if (static_cast<int64_t>(x->world) * nl != ng || lo != static_cast<int64_t>(x->rank) * nl)
        return fail(ctx, TGO_E_INVALID, std::string(name) + ": the exchange's world / rank do not match the partition");
    d.ctx = ctx;
    d.x = x;
    d.st = ctx->stream;
    if ((rc = scratch(ctx, d.dbuf, words, slot))) return rc;
    d.hc = x->host_counts();
    if (!d.hc) return fail(ctx, TGO_E_HIP, std::string(name) + ": pinned counts");
    return TGO_OK;
}

// Ghost lists (part_ghost.hip), kept with the graph: which of this rank's rows every peer
// reads (send_row) and where each value received from a peer goes (recv_pos).  PageRank reads
// over its in-lists into the blocked gathered vector; the multi-source sweep over both lists
// into the global mask vector (position = global id).
struct PrGhost {
    int world = 0, rank = -1;
    int64_t nl = 0, hot = 0, span = 0;
    int32_t* send_row = nullptr;    // local rows this rank sends, peer-major
    int32_t* recv_pos = nullptr;    // gathered-vector position of every received value
    double* sbuf = nullptr;
    double* rbuf = nullptr;
    int64_t nsend = 0, nrecv = 0;
    std::vector<size_t> sb, so, rb, ro;   // byte counts / offsets per peer (doubles)
    ~PrGhost() {
        for (void* p : {static_cast<void*>(send_row), static_cast<void*>(recv_pos), static_cast<void*>(sbuf),
                        static_cast<void*>(rbuf)})
            if (p) (void)hipFree(p);
    }
};

int build_ghost(tgo_ctx* ctx, tgo_exchange* x, Driver& d, int64_t nl, int64_t hot, int64_t span, bool both_lists,
                PrGhost& gh) {
    const int W = x->world, R = x->rank;
    hipStream_t st = d.st;
    const int32_t *adj = nullptr, *adj2 = nullptr;
    int64_t nnz = 0, nnz2 = 0;
    int rc = part_in_list(ctx, &adj, &nnz);
    if (!rc && both_lists) rc = part_out_list(ctx, &adj2, &nnz2);
    if (rc) return rc;
    std::string err;
    int32_t* need = nullptr;
    std::vector<int64_t> need_count;
    if ((rc = ghost_needs(adj, nnz, adj2, nnz2, nl, R, W, &need, need_count, st, err))) return fail(ctx, rc, err);
    struct Free { void* p; ~Free() { if (p) (void)hipFree(p); } } free_need{need};
    int64_t nneed = 0;
    for (int64_t c : need_count) nneed += c;
    // counts to the owners, then the ids (as int32 bytes)
    int64_t* sizes = nullptr;
    if ((rc = scratch(ctx, sizes, 2 * W, both_lists ? Slot::kMsGhostSizes : Slot::kPrGhostSizes))) return rc;
    if ((rc = d.upload(sizes, need_count.data(), W * sizeof(int64_t), "ghost counts upload"))) return rc;
    if (int r = x->all_to_all(sizes, sizes + W, 8, st)) return d.xfail(r);
    std::vector<int64_t> gives(W);
    if ((rc = d.download(gives.data(), sizes + W, W * sizeof(int64_t), "ghost counts read"))) return rc;
    int64_t ngive = 0;
    for (int64_t c : gives) ngive += c;
    gh.world = W; gh.rank = R; gh.nl = nl; gh.hot = hot; gh.span = span;
    gh.nsend = ngive;
    gh.nrecv = nneed;
    if (hipMalloc(&gh.send_row, std::max<int64_t>(ngive, 1) * 4) != hipSuccess ||
        hipMalloc(&gh.recv_pos, std::max<int64_t>(nneed, 1) * 4) != hipSuccess ||
        hipMalloc(&gh.sbuf, std::max<int64_t>(ngive, 1) * 8) != hipSuccess ||
        hipMalloc(&gh.rbuf, std::max<int64_t>(nneed, 1) * 8) != hipSuccess)
        return fail(ctx, TGO_E_OOM, "ghost buffers");
    std::vector<size_t> ib, io, gb, go;
    peer_splits(need_count.data(), W, 4, ib, io);           // my needs (ids), to owner p
    peer_splits(gives.data(), W, 4, gb, go);                // p's needs of my rows
    peer_splits(need_count.data(), W, 8, gh.rb, gh.ro);     // values received from p
    peer_splits(gives.data(), W, 8, gh.sb, gh.so);          // values sent to p
    if (int r = x->all_to_allv(need, ib.data(), io.data(), gh.send_row, gb.data(), go.data(), st)) return d.xfail(r);
    if (hipError_t e = k_sub_i32(gh.send_row, ngive, static_cast<int32_t>(static_cast<int64_t>(R) * nl), st))
        return fail(ctx, TGO_E_HIP, hipGetErrorString(e));
    if (hipError_t e = k_gathered_pos(need, nneed, nl, span, hot, W, gh.recv_pos, st))
        return fail(ctx, TGO_E_HIP, hipGetErrorString(e));
    if (hipStreamSynchronize(st) != hipSuccess) return d.hip("ghost lists");
    return TGO_OK;
}

// the ghost lists a driver keeps with the graph (tgo_ctx::part_state): PageRank's and the sweep's
struct GhostCache {
    std::shared_ptr<PrGhost> pr, ms;
};
GhostCache& ghost_cache(tgo_ctx* ctx) {
    std::shared_ptr<void>& st = ctx->part_state;
    if (!st) st = std::make_shared<GhostCache>();
    return *static_cast<GhostCache*>(st.get());
}

// The cached lists when they were built for this exchange and layout, else fresh ones in their
// place; a failed build releases the peers.
int acquire_ghost(Driver& d, std::shared_ptr<PrGhost>& cached, int64_t nl, int64_t hot, int64_t span, bool both_lists,
                  PrGhost*& gh) {
    gh = cached.get();
    if (gh && gh->world == d.x->world && gh->rank == d.x->rank && gh->nl == nl && gh->hot == hot && gh->span == span)
        return TGO_OK;
    gh = nullptr;
    auto fresh = std::make_shared<PrGhost>();
    if (int rc = build_ghost(d.ctx, d.x, d, nl, hot, span, both_lists, *fresh)) {
        d.x->abort();
        return rc;
    }
    cached = fresh;
    gh = fresh.get();
    return TGO_OK;
}

}  // namespace

extern "C" int tgo_part_msbfs_run(tgo_ctx* ctx, tgo_exchange* x, const int64_t* seeds, int32_t nseeds, int32_t max_depth,
                                  double ms_alpha, int64_t fixed_bytes, int64_t* reached, int64_t* entries,
                                  int32_t* levels_out) {
    if (!ctx) return TGO_E_INVALID;
    if (!x || !seeds || nseeds < 1 || nseeds > TGO_MAX_SOURCES || max_depth < 0)
        return fail(ctx, TGO_E_INVALID, "tgo_part_msbfs_run: bad arguments");
    // the driver's device words: the level counts {next queue, its entries, own queue}, then 2 x 64
    // words for the per-source sums of a split and the per-seed statistics
    Driver d{};
    int64_t nl = 0, lo = 0, ng = 0, ent = 0;
    int rc = driver_open(ctx, x, "tgo_part_msbfs_run", Slot::kMsWords, 3 + 2 * TGO_MAX_SOURCES, d, nl, lo, ng, ent);
    if (rc) return rc;
    const int W = x->world;
    hipStream_t st = d.st;
    int64_t* const dc = d.dbuf;
    int64_t* const hc = d.hc;
    // scratch (ctx-owned, reused): two alternating global mask buffers, the candidate masks,
    // the pair buffers and the split sizes
    uint64_t *g0 = nullptr, *g1 = nullptr, *cand = nullptr;
    int64_t *send = nullptr, *recv = nullptr, *sizes = nullptr;
    const int64_t pairs_cap = 2 * ng + 2 * W;
    if ((rc = scratch(ctx, g0, ng, Slot::kMsMask0)) || (rc = scratch(ctx, g1, ng, Slot::kMsMask1)) ||
        (rc = scratch(ctx, cand, ng, Slot::kMsCand)) || (rc = scratch(ctx, send, pairs_cap, Slot::kMsSend)) ||
        (rc = scratch(ctx, recv, pairs_cap, Slot::kMsRecv)) || (rc = scratch(ctx, sizes, 2 * W, Slot::kMsSizes)))
        return rc;
    int64_t* const caller_dc = ctx->part_dcounts;       // restored at the end
    // the rank's own candidate words never travel: the packs skip its slice (self) and the ORs
    // take it from the candidate masks (own_slice); a push writes the owned targets straight into
    // the next masks (the Python reference driver keeps packing every slice)
    const int self = x->rank;
    MsOwn own_slice;
    own_slice.cand = cand;
    own_slice.self = self;
    uint64_t* glob[2] = {g0, g1};
    // no clearing per sweep (as the Python driver): the buffers start zero (part_scratch), a
    // level rewrites the active rows of the next mask and the entry-less tail stays zero, the
    // pack clears the candidate masks it reads, and a dense level's all-gather overwrites the
    // peers' slices before the pull reads them.  A failed sweep re-zeroes all three.
    auto rezero = [&]() {
        (void)hipMemsetAsync(g0, 0, ng * 8, st);
        (void)hipMemsetAsync(g1, 0, ng * 8, st);
        (void)hipMemsetAsync(cand, 0, ng * 8, st);
    };
    // dense levels: the ghost exchange (only the masks this rank's lists read, lists built once
    // per graph) unless TGO_TUNE_MS_GHOST = 0 or a single rank
    PrGhost* gh = nullptr;
    if (W > 1 && ctx->tune.i64(TGO_TUNE_MS_GHOST) != 0 &&
        (rc = acquire_ghost(d, ghost_cache(ctx).ms, nl, 0, nl, true, gh)))
        return rc;
    // global counts: local {a, b} through the pinned words, all-reduced in dc (one stream wait)
    auto global2 = [&](int64_t a, int64_t b) -> int {
        hc[0] = a; hc[1] = b;
        return d.reduce_copy(dc, hc, 2, tgo_exchange::kRedSum, "counts");
    };
    if ((rc = global2(ent, 0))) return rc;
    const int64_t total = hc[0];
    uint64_t* fr = glob[0] + lo;
    uint64_t* frn = glob[1] + lo;
    int64_t c[2];
    if ((rc = tgo_part_ms_begin(ctx, seeds, nseeds, fr, c))) return rc;
    if ((rc = global2(c[0], c[1]))) return rc;
    int64_t nf = hc[0], mf = hc[1];
    // level counts stay on the device: the steps publish {next queue, its entries, own queue}
    if ((rc = tgo_part_device_counts(ctx, dc))) return rc;
    int levels = 0;
    // source split of the first dense level of a run (tgo_bfs_multi's rule and budget)
    const double split_frac = ms_split_of(ctx);
    const uint64_t full = nseeds == 64 ? ~0ULL : ((1ULL << nseeds) - 1ULL);
    int64_t* sc64 = dc + 3;                                 // 64 per-source sums (free during the sweep)
    // pack + exchange the candidate masks of a push (fixed slots when cap bounds them), then
    // hand the received pairs to `then`.  The own slice never travels: its slot / split is
    // empty; with one rank nothing is exchanged at all.
    auto exchange = [&](int64_t entries, auto&& then) -> int {
        const int64_t cap = std::min<int64_t>(entries, nl);
        if (W == 1) {
            const int64_t none = 0;
            return then(MsRecv::pairs(recv, &none, W));
        }
        if (cap > 0 && static_cast<int64_t>(W) * (cap + 1) * 16 <= fixed_bytes) {
            if (int r = part_ms_pack_fixed(ctx, cand, W, cap, send, self)) return r;
            // equal slots known on the host; the own slot is neither sent nor received (its
            // header in recv zeroed so the settle reads no pairs from it)
            const size_t slot = static_cast<size_t>(cap + 1) * 16;
            std::vector<size_t> sb(W, slot), so(W);
            for (int p = 0; p < W; ++p) so[p] = static_cast<size_t>(p) * slot;
            sb[self] = 0;
            if (hipMemsetAsync(reinterpret_cast<char*>(recv) + so[self], 0, 16, st) != hipSuccess)
                return d.hip("own slot header");
            if (int r = x->all_to_allv(send, sb.data(), so.data(), recv, sb.data(), so.data(), st)) return d.xfail(r);
            return then(MsRecv::fixed(recv, W, cap));
        }
        // sized pairs: split sizes on the device, one all-to-all of them, one host read
        if (int r = part_ms_pack_dev(ctx, cand, W, send, sizes, self)) return r;
        if (int r = x->all_to_all(sizes, sizes + W, 8, st)) return d.xfail(r);
        std::vector<int64_t> both(2 * W);
        if (int r = d.download(both.data(), sizes, 2 * W * sizeof(int64_t), "split sizes read")) return r;
        std::vector<size_t> sb, so, rb, ro;
        peer_splits(both.data(), W, 8, sb, so);
        peer_splits(both.data() + W, W, 8, rb, ro);
        std::vector<int64_t> rpairs(W);
        for (int p = 0; p < W; ++p) rpairs[p] = both[W + p] / 2;
        if (int r = x->all_to_allv(send, sb.data(), so.data(), recv, rb.data(), ro.data(), st)) return d.xfail(r);
        return then(MsRecv::pairs(recv, rpairs.data(), W));
    };
    bool prev_dense = false;
    bool sums = false;
    for (int level = 0; level < max_depth && nf > 0; ++level) {
        const bool dense = static_cast<double>(mf) * ms_alpha > static_cast<double>(total);
        DevSpan span(st, "part.msbfs.level", {"level", level}, {"dense", dense ? 1 : 0});
        const bool first_dense = dense && !prev_dense;
        prev_dense = dense;
        const bool sums_ready = sums;   // the previous level's settle summed the per-source entries
        sums = false;
        if (dense) {
            uint64_t sparse = 0;
            int32_t with_cand = 0;
            if (first_dense && split_frac > 0.0) {
                // every source's exact push entries (all-reduced), the smallest within the budget;
                // after a push level its settle summed them (MsOwn::sums)
                int64_t se[64];
                if (!sums_ready && (rc = tgo_part_ms_source_entries(ctx, fr, full, sc64))) break;
                if ((rc = d.reduce_device(sc64, 64)) || (rc = d.download(se, sc64, sizeof(se), "per-source sums read"))) break;
                int order[64];
                for (int r = 0; r < nseeds; ++r) order[r] = r;
                std::sort(order, order + nseeds, [&](int a, int b) { return se[a] < se[b]; });
                int64_t used = 0;
                for (int i = 0; i < nseeds; ++i) {
                    const int r = order[i];
                    if (static_cast<double>(used + se[r]) > split_frac * static_cast<double>(total)) break;
                    used += se[r];
                    sparse |= 1ULL << r;
                }
                if (sparse == full) sparse = 0;
                if (sparse && used > 0) {               // push the sparse sources' frontiers
                    if ((rc = tgo_part_ms_push_masked(ctx, fr, cand, sparse))) break;
                    if ((rc = exchange(used, [&](const MsRecv& in) { return part_ms_or(ctx, in, frn, own_slice); }))) break;
                    with_cand = 1;
                }
            }
            if (gh) {                                   // ghosts: pack -> all-to-allv -> unpack into glob[0]
                const uint64_t* own = glob[0] + lo;
                if (k_pack_u64(own, gh->send_row, gh->nsend, reinterpret_cast<uint64_t*>(gh->sbuf), st) != hipSuccess) {
                    rc = d.hip("ghost pack");
                    break;
                }
                if (int r = x->all_to_allv(gh->sbuf, gh->sb.data(), gh->so.data(), gh->rbuf, gh->rb.data(), gh->ro.data(), st)) {
                    rc = d.xfail(r);
                    break;
                }
                if (k_unpack_u64(reinterpret_cast<const uint64_t*>(gh->rbuf), gh->recv_pos, gh->nrecv, glob[0], st) !=
                    hipSuccess) {
                    rc = d.hip("ghost unpack");
                    break;
                }
            } else if (int r = x->all_gather(glob[0], static_cast<size_t>(nl) * 8, st)) {
                rc = d.xfail(r);
                break;
            }
            if ((rc = tgo_part_ms_pull_split(ctx, level, glob[0], frn, sparse, with_cand, nullptr))) break;
        } else {
            // owned candidates straight into frn: the settle below neither zeroes nor ORs them
            if ((rc = part_ms_push(ctx, fr, cand, frn, self))) break;
            MsOwn settle;
            settle.direct = true;
            // the settle sums the per-source entries when the next level may pull (this
            // frontier's entries within 64x of the pull threshold), as the one-GPU sweep
            sums = split_frac > 0.0 && static_cast<double>(mf) * ms_alpha * 64.0 > static_cast<double>(total);
            if (sums) {
                if (hipMemsetAsync(sc64, 0, 64 * sizeof(int64_t), st) != hipSuccess) { rc = d.hip("per-source sums clear"); break; }
                settle.sums = sc64;
            }
            // and builds no queue when the next level will likely pull (within 8x of the threshold)
            settle.count_only = static_cast<double>(mf) * ms_alpha * 8.0 > static_cast<double>(total);
            if ((rc = exchange(mf, [&](const MsRecv& in) { return part_ms_settle(ctx, level, in, frn, settle, nullptr); })))
                break;
        }
        std::swap(fr, frn);
        std::swap(glob[0], glob[1]);
        // global {next frontier, its entries}; this rank's queue length back to the engine
        if ((rc = d.reduce_device(dc, 2)) || (rc = part_read_words(ctx, dc, 3, hc))) break;
        nf = hc[0];
        mf = hc[1];
        if ((rc = tgo_part_set_local_qlen(ctx, hc[2]))) break;
        ++levels;
    }
    const int rc_off = tgo_part_device_counts(ctx, caller_dc);
    trace_resolve(st);
    if (rc) {
        x->abort();
        rezero();
        return rc;
    }
    if (rc_off) return rc_off;
    const bool stats = reached || entries;           // the per-seed counts cost a pass over the masks
    std::vector<int64_t> both(2 * nseeds);           // reached, then entries
    if ((rc = tgo_part_ms_end(ctx, stats ? both.data() : nullptr, stats ? both.data() + nseeds : nullptr))) return rc;
    if (stats) {
        if ((rc = d.reduce_copy(dc + 3, both.data(), both.size(), tgo_exchange::kRedSum, "stats"))) return rc;
        for (int i = 0; i < nseeds; ++i) {
            if (reached) reached[i] = both[i];
            if (entries) entries[i] = both[nseeds + i];
        }
    }
    if (levels_out) *levels_out = levels;
    return TGO_OK;
}

// ======================================================================================
// Native loops of the other partitioned programs: single-source BFS, delta-stepping SSSP and
// PageRank, each ONE C-ABI call whose C++ loop issues its collectives through the exchange on
// the ctx stream (the protocols of titan_amd/distributed.py distributed_bfs / _sssp /
// _pagerank, which stay as the Python reference drivers).  They replace the per-superstep
// Python round trips of FulgoraGraphComputer's superstep loop (FulgoraGraphComputer.java:
// 151-189) in its multi-GPU form.


extern "C" int tgo_part_bfs_run(tgo_ctx* ctx, tgo_exchange* x, int64_t seed_global, int32_t max_depth, double alpha,
                                double beta, int64_t* dist_local, int64_t* reached, int32_t* levels_out) {
    if (!ctx) return TGO_E_INVALID;
    if (!x || max_depth < 0 || !(alpha > 0.0) || !(beta > 0.0))
        return fail(ctx, TGO_E_INVALID, "tgo_part_bfs_run: bad arguments");
    Driver d{};
    int64_t nl = 0, lo = 0, ng = 0, ent = 0;
    int rc = driver_open(ctx, x, "tgo_part_bfs_run", Slot::kBfsWords, 8, d, nl, lo, ng, ent);
    if (rc) return rc;
    const int W = x->world;
    const int64_t nwl = nl / 64, nwg = ng / 64;
    hipStream_t st = d.st;
    // two alternating global frontier bitmaps (the owned next frontier is the rank's slice of
    // the other one, so the all-gather is in place), the discovered bitmap and its received
    // slices, the device level counts
    uint64_t *f0 = nullptr, *f1 = nullptr, *disc = nullptr, *recv = nullptr;
    int64_t* dc = nullptr;
    if ((rc = scratch(ctx, f0, nwg, Slot::kBfsFront0)) || (rc = scratch(ctx, f1, nwg, Slot::kBfsFront1)) ||
        (rc = scratch(ctx, disc, nwg, Slot::kBfsDisc)) || (rc = scratch(ctx, recv, nwg, Slot::kBfsRecv)) ||
        (rc = scratch(ctx, dc, 4, Slot::kBfsCounts)))
        return rc;
    int64_t* const caller_dc = ctx->part_dcounts;
    uint64_t* glob[2] = {f0, f1};
    int64_t c[2] = {0, 0};
    if ((rc = tgo_part_bfs_begin(ctx, seed_global, glob[0] + x->rank * nwl, c))) return rc;
    if (int r = x->all_gather(glob[0], static_cast<size_t>(nwl) * 8, st)) return d.xfail(r);
    // the seed level's counts and the graph's total entries in one reduction (one host round trip)
    int64_t v3[3] = {c[0], c[1], ent}, g[3] = {0, 0, 0};
    if ((rc = d.reduce(v3, 3, tgo_exchange::kRedSum, g))) return rc;
    int64_t nf = g[0], mf = g[1], mu = g[2] - mf;
    if ((rc = tgo_part_device_counts(ctx, dc))) return rc;
    bool bottom_up = false;
    int levels = 0;
    for (int level = 0; level < max_depth && nf > 0; ++level) {
        // direction-optimizing switch (Beamer et al.; the one-GPU rule, tgo_bfs)
        if (!bottom_up && static_cast<double>(mf) > static_cast<double>(mu) / alpha) bottom_up = true;
        else if (bottom_up && static_cast<double>(nf) < static_cast<double>(ng) / beta) bottom_up = false;
        uint64_t* nb = glob[1] + x->rank * nwl;
        DevSpan span(st, "part.bfs.level", {"level", level}, {"bottom_up", bottom_up ? 1 : 0});
        if (bottom_up) {
            if ((rc = tgo_part_bfs_bu(ctx, level, glob[0], nb, nullptr))) break;
        } else {
            // owned targets claimed during the expansion (tgo::part_bfs_td_fused); the remote
            // ones travel as discovered-bitmap slices and are claimed by their owners
            if (W > 1 && hipMemsetAsync(disc, 0, nwg * 8, st) != hipSuccess) { rc = d.hip("disc clear"); break; }
            if ((rc = tgo::part_bfs_td_fused(ctx, level, disc, nb))) break;
            if (W > 1) {
                if (int r = x->all_to_all(disc, recv, static_cast<size_t>(nwl) * 8, st)) { rc = d.xfail(r); break; }
                if ((rc = tgo::part_bfs_claim_remote(ctx, level, recv, W, nb))) break;
            }
            if ((rc = tgo::part_bfs_level_done(ctx))) break;
        }
        if (int r = x->all_gather(glob[1], static_cast<size_t>(nwl) * 8, st)) { rc = d.xfail(r); break; }
        std::swap(glob[0], glob[1]);
        if ((rc = d.reduce_device(dc, 2)) || (rc = part_read_words(ctx, dc, 3, d.hc))) break;
        nf = d.hc[0];
        mf = d.hc[1];
        mu -= mf;
        if ((rc = tgo_part_set_local_qlen(ctx, d.hc[2]))) break;
        ++levels;
    }
    const int rc_off = tgo_part_device_counts(ctx, caller_dc);
    trace_resolve(st);
    if (rc) { x->abort(); return rc; }
    if (rc_off) return rc_off;
    int64_t rl[2] = {0, 0};
    // the reach statistics (a pass over every list) only when asked for
    if ((rc = tgo_part_bfs_end(ctx, dist_local, reached ? rl : nullptr))) return rc;
    if (reached && (rc = d.reduce(rl, 2, tgo_exchange::kRedSum, reached))) return rc;
    if (levels_out) *levels_out = levels;
    return TGO_OK;
}

extern "C" int tgo_part_sssp_run(tgo_ctx* ctx, tgo_exchange* x, int64_t seed_global, int64_t delta, int64_t* dist_local,
                                 int64_t* reached, int32_t* phases_out) {
    if (!ctx) return TGO_E_INVALID;
    if (!x) return fail(ctx, TGO_E_INVALID, "tgo_part_sssp_run: bad arguments");
    Driver d{};
    int64_t nl = 0, lo = 0, ng = 0, ent = 0;
    int rc = driver_open(ctx, x, "tgo_part_sssp_run", Slot::kSsspWords, 8, d, nl, lo, ng, ent);
    if (rc) return rc;
    const int W = x->world;
    hipStream_t st = d.st;
    int64_t *send = nullptr, *recv = nullptr, *sizes = nullptr;
    if ((rc = scratch(ctx, send, 2 * ng + 2, Slot::kSsspSend)) || (rc = scratch(ctx, recv, 2 * ng + 2, Slot::kSsspRecv)) ||
        (rc = scratch(ctx, sizes, 11 * W + 3, Slot::kSsspSizes)))
        return rc;
    // negative weights: every rank fails here, before any collective a peer could wait in
    int64_t wmin = 0, gmin = 0;
    if ((rc = tgo_part_weight_min(ctx, &wmin))) return rc;
    if ((rc = d.reduce(&wmin, 1, tgo_exchange::kRedMin, &gmin))) return rc;
    if (gmin < 0) return fail(ctx, TGO_E_INVALID, "delta-stepping needs non-negative weights (a rank holds a negative weight)");
    int64_t out[2] = {0, 0};
    if ((rc = tgo_part_sssp_begin(ctx, seed_global, delta, out))) return rc;
    if (delta <= 0) {           // the ranks' default widths follow their local mean weight: agree on one
        if ((rc = d.reduce(&out[1], 1, tgo_exchange::kRedMax, &delta))) return rc;
    }
    if (delta <= 0) return fail(ctx, TGO_E_INVALID, "tgo_part_sssp_run: bucket width");
    // light/heavy split (weighted loads): the same decision on every rank (the load's weights
    // and the agreed width); the loop below is the same either way
    bool split = false;
    if ((rc = part_sssp_split(ctx, delta, &split))) return rc;
    (void)split;
    // on the device-sized loop (delta_loop.hip) nothing but the header comes to the host
    const bool dev = ctx->part_devloop;
    int64_t thr = delta;
    int phases = 0;
    // per phase, ONE host read: the relax writes a 4-word header per peer on the device
    // {pair elements for it, near-queue length, pending minimum, members flag}; one all-to-all
    // moves the headers and a fold (2W + 3 words: sent / received sizes, global queue length,
    // pending minimum, members) comes back through the mapped counter page.  An empty global
    // near queue then moves straight to the next bucket: the pending minimum is kept on the
    // fly (delta.hip ds_track_reset), so no bitmap scan and no second collective.
    int64_t* hdr_recv = sizes + 4 * W;
    int64_t* fold = sizes + 8 * W;
    const int nf = 2 * W + 3;
    std::vector<int64_t> hf(nf);
    std::vector<size_t> sb, so, rb, ro;
    // One rank on the device loop: its header all-to-all is the identity, so the header kernel
    // folds and publishes it in one launch (3 launches and a copy fewer per phase).  Up to 14
    // ranks the fold publishes its own words (nf <= 32 counter-page words).
    const bool solo = dev && W == 1;
    for (;;) {
        DevSpan span(st, "part.sssp.phase", {"phase", phases}, {"threshold", thr});
        if (solo) {
            if ((rc = part_sssp_dev_relax(ctx, W, send, sizes, hf.data()))) break;
        } else {
            if ((rc = dev ? part_sssp_dev_relax(ctx, W, send, sizes, nullptr) : part_sssp_relax_dev(ctx, thr, W, send, sizes)))
                break;
            if (int r = x->all_to_all(sizes, hdr_recv, 32, st)) { rc = d.xfail(r); break; }
            if (nf <= 32) {                // through the mapped counter page (up to 14 ranks)
                if ((rc = part_sssp_header_read(ctx, sizes, hdr_recv, W, fold, hf.data()))) break;
            } else if ((rc = part_sssp_header_fold(ctx, sizes, hdr_recv, W, fold)) ||
                       (rc = d.download(hf.data(), fold, nf * sizeof(int64_t), "header read"))) break;
        }
        if (hf[2 * W] == 0) {   // every near queue was empty (nothing was relaxed): the next non-empty bucket
            span.end();
            const int64_t mn = hf[2 * W + 1];
            if (mn == INT64_MAX && hf[2 * W + 2] == 0) break;   // converged: nothing pending, no members left
            if (mn != INT64_MAX && mn >= thr) thr = (mn / delta + 1) * delta;
            if ((rc = dev ? part_sssp_dev_extract(ctx, thr) : tgo_part_sssp_extract(ctx, thr, nullptr))) break;
            continue;
        }
        peer_splits(hf.data(), W, 8, sb, so);
        const size_t b = peer_splits(hf.data() + W, W, 8, rb, ro);
        if (int r = x->all_to_allv(send, sb.data(), so.data(), recv, rb.data(), ro.data(), st)) { rc = d.xfail(r); break; }
        const int64_t np = static_cast<int64_t>(b / 16);
        if ((rc = dev ? part_sssp_dev_apply(ctx, recv, np) : tgo_part_sssp_apply(ctx, thr, recv, np, nullptr))) break;
        ++phases;
    }
    trace_resolve(st);
    if (rc) { x->abort(); return rc; }
    int64_t rl[2] = {0, 0};
    if ((rc = tgo_part_sssp_end(ctx, dist_local, rl))) return rc;
    if (reached && (rc = d.reduce(rl, 2, tgo_exchange::kRedSum, reached))) return rc;
    if (phases_out) *phases_out = phases;
    return TGO_OK;
}


extern "C" int tgo_part_pagerank_run(tgo_ctx* ctx, tgo_exchange* x, const tgo_pr_args* args, int32_t exchange_mode,
                                     double* pr_local, int64_t* exchanged_bytes) {
    if (!ctx) return TGO_E_INVALID;
    if (!x || !args || args->max_iterations < 1 || exchange_mode < 0 || exchange_mode > 1)
        return fail(ctx, TGO_E_INVALID, "tgo_part_pagerank_run: bad arguments");
    Driver d{};
    int64_t nl = 0, lo = 0, ng = 0, ent = 0;
    int rc = driver_open(ctx, x, "tgo_part_pagerank_run", Slot::kPrWords, 8, d, nl, lo, ng, ent);
    if (rc) return rc;
    const int W = x->world, R = x->rank;
    hipStream_t st = d.st;
    // layout: active span A = max active rows (every rank), the blocked hot-first layout
    // and the longest in-row of any rank: the fixed-point range is one per job, not per rank
    int64_t own[2] = {0, 0}, all[2] = {0, 0}, hot = 0;
    if ((rc = tgo_part_active_rows(ctx, &own[0])) || (rc = tgo_part_pr_longest_row(ctx, &own[1]))) return rc;
    if ((rc = d.reduce(own, 2, tgo_exchange::kRedMax, all))) return rc;
    int64_t span = all[0];
    if ((rc = tgo_part_pr_set_longest_row(ctx, all[1])) || (rc = tgo_part_pr_blocked(ctx, W, span, &hot))) return rc;
    if (hot == 0) span = nl;                     // plain layout: rank-major n_local slices
    double *contrib = nullptr, *gath = nullptr;
    if ((rc = scratch(ctx, contrib, nl, Slot::kPrContrib)) ||
        (rc = scratch(ctx, gath, static_cast<int64_t>(W) * span, Slot::kPrGathered)))
        return rc;
    PrGhost* gh = nullptr;
    if (exchange_mode == 1 && W > 1 && (rc = acquire_ghost(d, ghost_cache(ctx).pr, nl, hot, span, false, gh))) return rc;
    int64_t moved = 0;
    // the program on the blocked layout, and once more on the plain one if that run left the exact range
    for (;;) {
        if ((rc = tgo_part_pr_begin(ctx, args, contrib))) return rc;
        for (int it = 2; it <= args->max_iterations; ++it) {
            DevSpan upd(st, "part.pagerank.update", {"iteration", it}, {"ghost", gh ? 1 : 0});
            // the rank's own slice into the gathered vector
            hipError_t e = hot == 0
                ? hipMemcpyAsync(gath + static_cast<int64_t>(R) * nl, contrib, nl * 8, hipMemcpyDeviceToDevice, st)
                : hipMemcpyAsync(gath + static_cast<int64_t>(R) * hot, contrib, hot * 8, hipMemcpyDeviceToDevice, st);
            if (e == hipSuccess && hot > 0 && span > hot)
                e = hipMemcpyAsync(gath + static_cast<int64_t>(W) * hot + static_cast<int64_t>(R) * (span - hot), contrib + hot,
                                   (span - hot) * 8, hipMemcpyDeviceToDevice, st);
            if (e != hipSuccess) { rc = d.hip("own slice"); break; }
            if (W > 1 && gh) {                       // ghosts: exactly the remote values this rank reads
                if ((e = k_pack_f64(contrib, gh->send_row, gh->nsend, gh->sbuf, st)) != hipSuccess) { rc = d.hip("pack"); break; }
                if (int r = x->all_to_allv(gh->sbuf, gh->sb.data(), gh->so.data(), gh->rbuf, gh->rb.data(), gh->ro.data(), st)) {
                    rc = d.xfail(r);
                    break;
                }
                if ((e = k_unpack_f64(gh->rbuf, gh->recv_pos, gh->nrecv, gath, st)) != hipSuccess) { rc = d.hip("unpack"); break; }
                moved += gh->nrecv * 8;
            } else if (W > 1) {                      // all-gather of every rank's slices (in place)
                int r = hot == 0 ? x->all_gather(gath, static_cast<size_t>(nl) * 8, st)
                                 : x->all_gather(gath, static_cast<size_t>(hot) * 8, st);
                if (!r && hot > 0 && span > hot)
                    r = x->all_gather(gath + static_cast<int64_t>(W) * hot, static_cast<size_t>(span - hot) * 8, st);
                if (r) { rc = d.xfail(r); break; }
                moved += static_cast<int64_t>(W - 1) * (hot == 0 ? nl : span) * 8;
            }
            if ((rc = tgo_part_pr_step(ctx, gath, contrib))) break;
        }
        trace_resolve(st);
        if (rc) { x->abort(); tgo_part_pr_plain(ctx, 0); return rc; }
        if (hot == 0) break;
        // a message outside the fixed-point passes' exact range on ANY rank (+inf from a vertex
        // whose row cut left it no OUT entry, NaN, ...): every rank re-runs the program on the
        // plain fp64 gather (rank-major all-gather layout), whose sums are Java double sums
        int32_t bad = 0;
        if ((rc = tgo_part_pr_exact_check(ctx, &bad))) { x->abort(); return rc; }
        int64_t b = bad, any = 0;
        if ((rc = d.reduce(&b, 1, tgo_exchange::kRedMax, &any))) return rc;
        if (!any) break;
        if ((rc = tgo_part_pr_plain(ctx, 1))) return rc;
        hot = 0;
        span = nl;
        gh = nullptr;
        moved = 0;                           // the discarded blocked run's traffic is not the job's
        if ((rc = scratch(ctx, gath, static_cast<int64_t>(W) * span, Slot::kPrGathered))) { tgo_part_pr_plain(ctx, 0); return rc; }
    }
    rc = tgo_part_pr_end(ctx, pr_local);
    tgo_part_pr_plain(ctx, 0);
    if (rc) return rc;
    if (exchanged_bytes) *exchanged_bytes = moved;
    return TGO_OK;
}
