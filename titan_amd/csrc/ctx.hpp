// ctx.hpp — the context behind the C-ABI's opaque tgo_ctx, and the helpers that the driver
// files (api*.cpp, part_driver.cpp, part_load.cpp) share: a function used by more than one of them is declared here,
// once, under its file's heading; program.hpp (included last) is the frame of a program driver.  Private.
#pragma once
#include <algorithm>
#include <atomic>
#include <memory>
#include <string>
#include <utility>
#include <vector>
#include <hip/hip_runtime_api.h>
#include "engine.hpp"
#include "trace.hpp"
#include "tuning.hpp"
#include "../../include/titan_gpu_olap_part.h"

struct tgo_ctx {
    tgo_options opts{};
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string err;
    tgo::RowStaging staging;
    tgo::DevGraph g;
    bool loaded = false;
    std::vector<int64_t> titan_id;
    std::vector<int32_t> perm;                       // row-order dense -> internal
    // Titan id -> dense (seed lookups, tgo_dense_ids): binary search over titan_id when it is
    // strictly increasing (edge loads; row loads of an ordered scan usually), else over a
    // sorted copy built on the first lookup — no per-load hash map (16.8 M inserts at RMAT-24)
    bool id_sorted = false;
    std::vector<std::pair<int64_t, int32_t>> id_index;
    tgo::Scratch sc;
    tgo_stats st{};
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    int64_t dev_bytes = 0;
    std::vector<void*> allocs;
    int part_cur = 0;           // partitioned BFS: queue buffer holding the frontier
    int64_t part_qlen = 0;      // its length
    bool part_queued = true;    // q[part_cur] holds the frontier (pull / bottom-up levels only count it)
    const uint64_t* part_frontier = nullptr;   // after bottom-up: the caller's nb_local (queued lazily)
    int64_t* part_dcounts = nullptr;    // caller's device counts (tgo_part_device_counts)
    int64_t* part_qlen_dev = nullptr;   // device copy of the queue length (lazy host read)
    bool part_qlen_stale = false;       // part_qlen must be read from part_qlen_dev
    double part_alpha = 0.85, part_base = 0.0;
    int32_t part_pr_iter = 0;   // partitioned PageRank: iteration reached / program length
    int32_t part_pr_iters = 0;
    int32_t part_pr_world = 0;  // blocked gathered layout (tgo_part_pr_blocked): world, H, A
    bool part_pr_plain = false; // tgo_part_pr_plain: the plain layout although the blocked one is built
    int64_t part_pr_hot = 0, part_pr_span = 0;
    // the fixed-point range of the blocked layout is the job's (DESIGN.md FxGuard): the longest
    // in-row of this rank, the longest of any rank as the driver agreed it (0 = not told), and
    // the length the layout in g.cold_in was built for
    int64_t part_max_in_row = 0, part_pr_job_row = 0, part_pr_built_row = 0;
    int64_t part_relaxed = 0;   // partitioned SSSP: entries relaxed, phases
    int32_t part_phases = 0;
    int64_t part_seed = -1;     // partitioned SSSP: the seed's internal id when owned here
    bool part_split = false;    // partitioned SSSP run on the light/heavy split (part_sssp_split)
    bool part_devloop = false;  // ... and on the device-sized loop (delta_loop.hip, part_sssp_dev_*)
    tgo::EdgeProg edge_prog;        // tgo_set_edge_program (TGO_EDGE_PROGRAM gathers)
    int64_t pv_max_out = 0, pv_max_in = 0;   // largest OUT / IN list of a vertex cut
    std::vector<int64_t> pv_rows;            // row ids of the vertex cuts
    // last finished program whose compute keys tgo_result_rows can encode (-1 = none)
    int res_kind = -1;
    bool host_decode = false;                // TGO_HOST_DECODE latched for the load in progress
    tgo::DecodeScratch dec;                  // device row decoder buffers (decode.hip)
    bool res_empty = false;                  // it set no property (PageRank iterations(0))
    tgo::ResultSource res_src;
    int num_cus = 256;          // compute units of the device (persistent launches)
    tgo::Tuning tune;           // tgo_set_tuning (tuning.hpp): one value per TGO_TUNE_* key
    int64_t tri_max = 0;        // largest count of the last tgo_triangles (an Integer key's range check)
    // state a native partitioned driver keeps between runs on this graph (part_driver.cpp:
    // the PageRank ghost lists); dropped with the graph
    std::shared_ptr<void> part_state;
};

namespace tgo {

inline int fail(tgo_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    return code;
}

#define HIP_TRY(call)                                                              \
    do {                                                                           \
        hipError_t e__ = (call);                                                   \
        if (e__ != hipSuccess)                                                     \
            return fail(ctx, e__ == hipErrorOutOfMemory ? TGO_E_OOM : TGO_E_HIP,   \
                        std::string(#call) + ": " + hipGetErrorString(e__));       \
    } while (0)

template <class T>
hipError_t dev_alloc(tgo_ctx* ctx, T*& p, int64_t count) {
    void* q = nullptr;
    const size_t bytes = static_cast<size_t>(std::max<int64_t>(count, 1)) * sizeof(T);
    hipError_t e = hipMalloc(&q, bytes);
    if (e != hipSuccess) return e;
    ctx->allocs.push_back(q);
    ctx->dev_bytes += static_cast<int64_t>(bytes);
    p = static_cast<T*>(q);
    return hipSuccess;
}

// Release one dev_alloc array of `count` elements before the graph goes (the stream is
// synchronised first: queued kernels may still use it).
template <class T>
void dev_free(tgo_ctx* ctx, T*& p, int64_t count) {
    if (!p) return;
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    auto it = std::find(ctx->allocs.begin(), ctx->allocs.end(), static_cast<void*>(p));
    if (it != ctx->allocs.end()) {
        ctx->allocs.erase(it);
        ctx->dev_bytes -= static_cast<int64_t>(std::max<int64_t>(count, 1) * sizeof(T));
        (void)hipFree(p);
    }
    p = nullptr;
}

// Adopt a device array built on the device (DevArray): no copy, freed with the graph.
template <class T>
void adopt(tgo_ctx* ctx, T*& p, DevArray<T>& a) {
    p = a.p;
    if (a.p) {
        ctx->allocs.push_back(a.p);
        ctx->dev_bytes += static_cast<int64_t>(std::max<int64_t>(a.n, 1) * sizeof(T));
    }
    a.p = nullptr;
    a.n = -1;
}

template <class T>
hipError_t upload(tgo_ctx* ctx, T*& p, const std::vector<T>& h) {
    hipError_t e = dev_alloc(ctx, p, static_cast<int64_t>(h.size()));
    if (e != hipSuccess || h.empty()) return e;
    return copy_chunked(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
}

// ------------------------------------------------------------------ api.cpp
void free_graph(tgo_ctx* ctx);
int threads_of(const tgo_ctx* ctx);
int resolve_seed(tgo_ctx* ctx, int64_t seed, int is_dense, int64_t& out);
int check_program(tgo_ctx* ctx, int scope);

// The helpers of the per-level path (wait_publish, read_counters, the turns, read_words,
// scan_frontier) are inline: a level loop calls nothing across files for them.

// The host-mapped counter page as words: [0, kCounterWords) what the last publish stored (a Counters,
// or the words of read_words), then the publish sequence number.
inline const volatile unsigned long long* host_words(const tgo_ctx* ctx) {
    return reinterpret_cast<const volatile unsigned long long*>(ctx->sc.hcnt);
}

// Counters of the work queued so far, without a copy + stream synchronisation: the publish
// kernel stores them and then a sequence number into host-mapped memory; the host spins on
// the sequence number (the level loops read a few words per level, so the wake-up latency of
// a blocking synchronisation dominated short levels).  A stream error ends the spin.
//
// Spin on the publish sequence number (a periodic stream query ends the spin on a failure).  or_later: the
// wait for a publish that later ones may have overwritten (the words then hold that publish or a later one).
inline int wait_publish(tgo_ctx* ctx, unsigned long long seq, bool or_later = false) {
    const volatile unsigned long long* flag = host_words(ctx) + kCounterWords;
    auto there = [&] { return or_later ? *flag >= seq : *flag == seq; };
    for (uint64_t it = 1; !there(); ++it) {
        if ((it & 0x3FFF) == 0) {
            const hipError_t q = hipStreamQuery(ctx->stream);
            if (q != hipSuccess && q != hipErrorNotReady) return fail(ctx, TGO_E_HIP, hipGetErrorString(q));
            if (q == hipSuccess && !there())
                return fail(ctx, TGO_E_HIP, or_later ? "loop state publish not visible after the stream drained"
                                                     : "counter publish not visible after the stream drained");
        }
        __builtin_ia32_pause();
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    return TGO_OK;
}

inline int read_counters(tgo_ctx* ctx) {
    Scratch& s = ctx->sc;
    const unsigned long long seq = ++s.pub_seq;
    HIP_TRY(k_publish_counters(s.cnt, s.hcnt_dev, seq, ctx->stream));
    return wait_publish(ctx, seq);
}

// A level turn: the counters are published (with the 64 words of src64, when given, after them) and
// zero again afterwards, in one launch.  turn_begin queues it and leaves the wait to the caller, who may
// queue the next level's prefix in between; seq is what wait_publish takes.
inline int turn_begin(tgo_ctx* ctx, unsigned long long& seq, unsigned long long* src64 = nullptr) {
    Scratch& s = ctx->sc;
    seq = ++s.pub_seq;
    HIP_TRY(k_publish_turn(s.cnt, s.hcnt_dev, seq, src64, ctx->stream));
    return TGO_OK;
}
inline int turn(tgo_ctx* ctx) {
    unsigned long long seq = 0;
    if (int rc = turn_begin(ctx, seq)) return rc;
    return wait_publish(ctx, seq);
}
// ... of a program whose kernels set Counters::err when a queue overflows: "<what>: a queue overflowed ..."
inline int turn_checked(tgo_ctx* ctx, const char* what) {
    if (int rc = turn(ctx)) return rc;
    if (ctx->sc.hcnt->err) return fail(ctx, TGO_E_HIP, std::string(what) + ": a queue overflowed (inconsistent lists)");
    return TGO_OK;
}

// The peel loops' bookkeeping (api_kcore.cpp, api_truss.cpp).  level_min: the smallest value above
// the level that a scan or peel launch left in Counters::red[0] as max(INT32_MAX - value)
// (wave.hpp publish_min), INT64_MAX when it published none.
inline int64_t level_min(unsigned long long word) {
    return word ? static_cast<int64_t>(INT32_MAX) - static_cast<int64_t>(word) : INT64_MAX;
}
// The alive items a level's scan reads: list[0, len), null = every item of [0, len).  A scan given
// keep_buffer() writes the items still alive there, and adopt(their number) makes that the list.
struct AliveList {
    const int32_t* list;
    int64_t len;
    int spare;                  // the buffer the list is not in
    int32_t* buffers[2];
    AliveList(int64_t n, int32_t* b0, int32_t* b1) : list(nullptr), len(n), spare(0), buffers{b0, b1} {}
    bool wants_rebuild(int64_t alive) const { return 2 * alive <= len; }       // the list has at least halved
    int32_t* keep_buffer() const { return buffers[spare]; }
    void adopt(int64_t new_len) {
        list = buffers[spare];
        spare ^= 1;
        len = new_len;
    }
};

// `count` device words (on the ctx stream, after the work queued so far) to out through the counter
// page, kCounterWords words a publish: a tiny kernel and a spin instead of a copy and a stream wait.
inline int read_words(tgo_ctx* ctx, const int64_t* dev, int64_t count, int64_t* out) {
    Scratch& s = ctx->sc;
    for (int64_t w0 = 0; w0 < count; w0 += kCounterWords) {
        const int m = static_cast<int>(std::min<int64_t>(kCounterWords, count - w0));
        const unsigned long long seq = ++s.pub_seq;
        HIP_TRY(k_publish_words(dev + w0, m, s.hcnt_dev, seq, ctx->stream));
        if (int rc = wait_publish(ctx, seq)) return rc;
        for (int i = 0; i < m; ++i) out[w0 + i] = static_cast<int64_t>(host_words(ctx)[i]);
    }
    return TGO_OK;
}

// Exclusive scan of qdeg[0..qlen) into qpre[0..qlen] (qpre[qlen] = total).
inline int scan_frontier(tgo_ctx* ctx, int64_t qlen) {
    Scratch& s = ctx->sc;
    HIP_TRY(hipMemsetAsync(s.qdeg + qlen, 0, sizeof(int64_t), ctx->stream));
    HIP_TRY(scan_exclusive_i64(s.cub_tmp, s.cub_bytes, s.qdeg, s.qpre, qlen + 1, ctx->stream));
    return TGO_OK;
}

// ------------------------------------------------------------------ api_part.cpp
// The partitioned primitives open and close with these three.
inline int part_check(tgo_ctx* ctx) {
    if (!ctx) return TGO_E_INVALID;
    if (!ctx->loaded || !ctx->g.partitioned) return fail(ctx, TGO_E_STATE, "no partitioned graph loaded");
    (void)hipSetDevice(ctx->opts.device);
    return TGO_OK;
}

// Entry points that leave work queued: on a ctx-owned stream the caller cannot order its
// collectives after that work, so finish it before returning; on the caller's stream the
// work stays stream-ordered (the caller's collectives follow it on the same stream).
inline int part_done(tgo_ctx* ctx) {
    if (ctx->own_stream) HIP_TRY(hipStreamSynchronize(ctx->stream));
    return TGO_OK;
}

// Level counters {next queue length, its push entries}.  Host mode: read (one stream sync)
// into counts.  Device mode (tgo_part_device_counts): published to the caller's device
// buffer without a sync — the caller all-reduces it and reads the global counts once; the
// local queue length is fetched lazily by the next call that needs it (part_qlen_now).
inline int part_counts(tgo_ctx* ctx, int64_t* counts, bool device_ok = true) {
    if (ctx->part_dcounts && device_ok) {
        HIP_TRY(k_publish_counts(ctx->sc.cnt, ctx->part_dcounts, ctx->part_qlen_dev, ctx->stream));
        ctx->part_qlen_stale = true;
        return part_done(ctx);
    }
    int rc = read_counters(ctx);
    if (rc) return rc;
    ctx->part_qlen = static_cast<int64_t>(ctx->sc.hcnt->qlen);
    ctx->part_qlen_stale = false;
    if (counts) {
        counts[0] = ctx->part_qlen;
        counts[1] = static_cast<int64_t>(ctx->sc.hcnt->mf);
    }
    return TGO_OK;
}

// ... and what part_driver.cpp's loops call between them
int part_dims(tgo_ctx* ctx, int64_t* n_local, int64_t* lo, int64_t* n_global, int64_t* entries);
int part_scratch(tgo_ctx* ctx, void** p, int64_t bytes, Scratch::DrvSlot slot);
// The multi-source steps as tgo_part_msbfs_run calls them: what the rank's own slice does is an
// argument of every call.  The C entry points of the same names pass the defaults (self = -1,
// MsOwn{}): every slice packed, nothing written directly, no sums, a queue built.
// What a settle / or reads: `nslices` fixed slots of `cap` pairs (tgo_part_ms_pack_fixed's
// layout), or sized pairs back to back with the host pair counts per slice.
struct MsRecv {
    const int64_t* recv;
    int32_t nslices;
    int64_t cap;                // fixed slots
    const int64_t* counts;      // sized pairs
    bool sized;
    static MsRecv fixed(const int64_t* recv, int32_t nslices, int64_t cap) { return {recv, nslices, cap, nullptr, false}; }
    static MsRecv pairs(const int64_t* recv, const int64_t* counts, int32_t nslices) { return {recv, nslices, 0, counts, true}; }
};
struct MsOwn {
    uint64_t* cand = nullptr;   // candidate masks whose slice `self` the pack skipped: ORed into the
    int self = -1;              // next masks here (and cleared); null / -1: every slice travelled
    bool direct = false;        // the push wrote the owned targets' candidates into the next masks
                                // (part_ms_push own_next): they are neither zeroed nor ORed here
    int64_t* sums = nullptr;    // settle: the new frontier's push entries per source are added to
                                // these 64 words (the caller zeroes them on the ctx stream)
    bool count_only = false;    // settle: no frontier queue (the next level will likely pull;
                                // the next push builds the queue if it runs after all)
};
// own_next with self >= 0: the candidates of the targets this rank owns go straight into these
// next masks (zeroed here) instead of slice `self` of cand_global
int part_ms_push(tgo_ctx* ctx, const uint64_t* fr_local, uint64_t* cand_global, uint64_t* own_next, int self);
// self: the slice of cand_global the pack skips (left for MsOwn::cand), -1: none
int part_ms_pack_dev(tgo_ctx* ctx, uint64_t* cand_global, int32_t nranks, int64_t* send, int64_t* send_elems_dev, int self);
int part_ms_pack_fixed(tgo_ctx* ctx, uint64_t* cand_global, int32_t nranks, int64_t cap, int64_t* send, int self);
int part_ms_or(tgo_ctx* ctx, const MsRecv& in, uint64_t* fr_next, const MsOwn& own);
int part_ms_settle(tgo_ctx* ctx, int32_t level, const MsRecv& in, uint64_t* fr_next, const MsOwn& own, int64_t* counts);
// device words to the host through the mapped counter page (no stream synchronisation)
int part_read_words(tgo_ctx* ctx, const int64_t* dev, int count, int64_t* out);
int part_in_list(tgo_ctx* ctx, const int32_t** adj, int64_t* nnz);
int part_out_list(tgo_ctx* ctx, const int32_t** adj, int64_t* nnz);
int part_pr_layout_of(tgo_ctx* ctx, int32_t* world, int64_t* hot, int64_t* span);
int part_sssp_relax_dev(tgo_ctx* ctx, int64_t thr, int32_t nranks, int64_t* send, int64_t* sizes);
int part_sssp_header_fold(tgo_ctx* ctx, const int64_t* own, const int64_t* recv, int nranks, int64_t* out);
int part_sssp_header_read(tgo_ctx* ctx, const int64_t* own, const int64_t* recv, int nranks, int64_t* out,
                          int64_t* words);
int part_sssp_split(tgo_ctx* ctx, int64_t delta, bool* on);
int part_sssp_dev_relax(tgo_ctx* ctx, int32_t nranks, int64_t* send, int64_t* sizes, int64_t* fold);
int part_sssp_dev_apply(tgo_ctx* ctx, const int64_t* recv, int64_t npairs);
int part_sssp_dev_extract(tgo_ctx* ctx, int64_t thr);

// ------------------------------------------------------------------ api_load.cpp
struct TrimTemps { ~TrimTemps() { tmp_trim(); } };     // tmp_cache.cpp: nothing stays reserved between loads
int64_t pr_hot_default();
int upload_cold_blocks(tgo_ctx* ctx, const std::vector<int64_t>& off, const std::vector<int32_t>& adj,
                       int64_t n_src, int64_t hot, int64_t n_rows, ColdBlocks& cb, bool& ready,
                       const int64_t* d_off = nullptr, const int32_t* d_adj = nullptr, int64_t d_nnz = 0,
                       int64_t win = 0, int64_t job_row = 0);
int part_upload(tgo_ctx* ctx, HostGraph& h, int64_t n_global, int64_t lo);
int part_rows_take(tgo_ctx* ctx, RowStaging& st, std::string& err);
// a failed row load: the staged rows and the decoder's buffers go together
void part_drop_staging(tgo_ctx* ctx);

// ------------------------------------------------------------------ api_pagerank.cpp
int fx_take_bad(tgo_ctx* ctx, ColdBlocks& cb, bool* bad);

// ------------------------------------------------------------------ api_traverse.cpp
int64_t default_delta(const DevGraph& g, bool weighted);
// The direction-optimizing BFS from internal vertex `seed` (< 0: nobody is reached) along `scope`'s
// lists: levels in sc.level (-1 unreached), distances in sc.dist, tgo_stats.levels = levels run
// (the deepest level + 1).  tgo_bfs and tgo_betweenness (api_bc.cpp) run it.
int run_bfs(tgo_ctx* ctx, int64_t seed, int max_depth, int scope);

// ------------------------------------------------------------------ api_cc.cpp
// g.cc_tid = the Titan id of every internal index, built once per graph: tgo_components, tgo_scc and
// tgo_peer_pressure label with it.
int titan_ids_by_index(tgo_ctx* ctx);

// ------------------------------------------------------------------ api_tri.cpp
// The forward lists and degrees of the simple undirected graph (g.tri_*), built once per graph:
// tgo_triangles and tgo_kcore walk them.
int tri_forward_lists(tgo_ctx* ctx);

// ------------------------------------------------------------------ api_bc.cpp
// The sorted simple adjacency of the undirected projection (g.bc_s*), built once per graph (the caller
// checks g.bc_sadj and n > 0): tgo_betweenness and tgo_ktruss walk it.
int bc_simple_adjacency(tgo_ctx* ctx);

// ------------------------------------------------------------------ api_msbfs.cpp
int ms_alloc(tgo_ctx* ctx);
double ms_split_of(const tgo_ctx* ctx);
double ms_stay_of(const tgo_ctx* ctx);
double ms_sparse_of(const tgo_ctx* ctx);
int64_t ms_head_of(const tgo_ctx* ctx);
// One sweep of up to 64 sources given as internal ids (all >= 0; ms_alloc done): the level loop of
// tgo_bfs_multi between its seed resolution and its extraction.  Leaves sc.ms_vis, the level planes
// [0, sc.ms_nplanes) and sc.ms_nsrc; tgo_stats as tgo_bfs_multi reports them.  tgo_bfs_multi and
// tgo_closeness (api_cl.cpp) run it.
int run_ms_sweep(tgo_ctx* ctx, const int64_t* seeds, int32_t nseeds, int32_t max_depth, int32_t scope, int32_t flags);

inline LevelPlanes ms_planes(tgo_ctx* ctx) { return LevelPlanes{ctx->sc.ms_lvl, ctx->g.n}; }

// Zero the level planes a discovery at `level` writes (planes 0..floor(log2(level))) that
// this sweep has not zeroed yet: vertices reached earlier have levels < 2^k, whose bit k
// is 0, so a plane is valid from the moment it is zeroed.
// keep_clean (the one-GPU sweep): only the rows a level can write, [0, n_active) — the rest is zero
// since ms_alloc — and not at all a plane that sc.ms_clean knows to be zero still (filled by an
// earlier sweep for a level that then found nothing).  The caller takes a plane's bit down
// before it launches a level that writes the plane (ms_planes_written).  Without keep_clean (the
// partitioned sweep, which does not track its writes) the whole plane is filled and its bit dropped.
inline int ms_planes_for(tgo_ctx* ctx, int32_t level, bool keep_clean = false) {
    Scratch& s = ctx->sc;
    while (s.ms_nplanes < kLevelPlanes && (level >> s.ms_nplanes) != 0) {
        const uint32_t bit = 1u << s.ms_nplanes;
        uint64_t* plane = s.ms_lvl + static_cast<int64_t>(s.ms_nplanes) * ctx->g.n;
        if (!keep_clean) {
            s.ms_clean &= ~bit;
            HIP_TRY(hipMemsetAsync(plane, 0, ctx->g.n * sizeof(uint64_t), ctx->stream));
        } else if (!(s.ms_clean & bit)) {
            // up to a 4 KB boundary (the rows above n_active are zero already): a length the fill
            // kernel takes in one dispatch — an odd one cost a second, 5 us, for its tail
            const int64_t rows = std::min<int64_t>(ctx->g.n, (ctx->g.n_active + 511) & ~int64_t(511));
            if (rows > 0) HIP_TRY(hipMemsetAsync(plane, 0, rows * sizeof(uint64_t), ctx->stream));
            s.ms_clean |= bit;
        }
        ++s.ms_nplanes;
    }
    return TGO_OK;
}
// the planes a discovery at `level` writes, as bits of sc.ms_clean (record_level: one per set level bit)
inline uint32_t ms_planes_written(int32_t level) { return static_cast<uint32_t>(level) & ((1u << kLevelPlanes) - 1u); }

}  // namespace tgo

#include "program.hpp"
