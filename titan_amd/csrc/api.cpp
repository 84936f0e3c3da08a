// api.cpp — the C-ABI (include/titan_gpu_olap.h): the context's lifecycle and tuning, graph accessors,
// stats.  Loads: api_load.cpp; program drivers: api_traverse, api_msbfs, api_pagerank, api_generic (with
// the result write-back), api_part, and one file per analytic (api_cc, api_tri, api_kcore, api_scc,
// api_bc, api_pp, api_cl); ctx.hpp and program.hpp hold what they share, tuning.hpp the knobs' table.
//
// The program drivers replace FulgoraGraphComputer.submit's superstep loop
// (FulgoraGraphComputer.java:151-189): instead of one full edgestore scan per superstep,
// each iteration is one or two kernel launches over the device-resident adjacency, and
// only the frontier is touched for BFS/SSSP.
#include <cstring>
#include <new>
#include <thread>
#include "codec.hpp"
#include "ctx.hpp"

using namespace tgo;

namespace tgo {

void free_graph(tgo_ctx* ctx) {
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->sc.cub_tmp) (void)hipFree(ctx->sc.cub_tmp);       // grown by the scans, not in allocs
    if (ctx->sc.sort_tmp) (void)hipFree(ctx->sc.sort_tmp);
    for (void* p : ctx->allocs) (void)hipFree(p);
    ctx->allocs.clear();
    ctx->dev_bytes = 0;
    ctx->g = DevGraph();
    Scratch keep;                   // the mapped host counters outlive the graph (tgo_destroy frees them)
    keep.hcnt = ctx->sc.hcnt;
    keep.hcnt_dev = ctx->sc.hcnt_dev;
    keep.pub_seq = ctx->sc.pub_seq;
    ctx->sc = keep;
    ctx->loaded = false;
    ctx->res_kind = -1;         // the last program's results lived in the freed scratch
    ctx->part_state.reset();
}

int threads_of(const tgo_ctx* ctx) {
    int t = ctx->opts.host_threads;
    if (t <= 0) t = static_cast<int>(std::thread::hardware_concurrency());
    return std::max(1, std::min(t, 64));
}

// Row-order dense index of a Titan id, -1 when no executed vertex has it.
int64_t dense_of(tgo_ctx* ctx, int64_t id) {
    const std::vector<int64_t>& t = ctx->titan_id;
    if (ctx->id_sorted) {
        const auto it = std::lower_bound(t.begin(), t.end(), id);
        return it != t.end() && *it == id ? static_cast<int64_t>(it - t.begin()) : -1;
    }
    if (ctx->id_index.size() != t.size()) {
        ctx->id_index.resize(t.size());
        for (size_t v = 0; v < t.size(); ++v) ctx->id_index[v] = {t[v], static_cast<int32_t>(v)};
        std::sort(ctx->id_index.begin(), ctx->id_index.end());
    }
    const auto it = std::lower_bound(ctx->id_index.begin(), ctx->id_index.end(), std::make_pair(id, INT32_MIN));
    return it != ctx->id_index.end() && it->first == id ? it->second : -1;
}

int resolve_seed(tgo_ctx* ctx, int64_t seed, int is_dense, int64_t& out) {
    if (is_dense) {
        if (seed < 0 || seed >= ctx->g.n) return fail(ctx, TGO_E_INVALID, "dense seed out of range");
        out = ctx->perm[seed];
        return TGO_OK;
    }
    const int64_t d = dense_of(ctx, seed);
    out = d < 0 ? -1 : ctx->perm[d];                                 // unknown seed: nobody gets a distance
    return TGO_OK;
}

int check_program(tgo_ctx* ctx, int scope) {
    if (!ctx->loaded) return fail(ctx, TGO_E_STATE, "no graph loaded");
    if (scope < 0 || scope > 2) return fail(ctx, TGO_E_INVALID, "invalid scope");
    if (scope != ctx->g.scope)
        return fail(ctx, TGO_E_INVALID, "program scope differs from the scope the graph was loaded (preloaded) for");
    return TGO_OK;
}

}  // namespace tgo

extern "C" {

void tgo_default_options(tgo_options* o) {
    std::memset(o, 0, sizeof(*o));
    o->abi_version = TGO_ABI_VERSION;
    o->device = 0;
    o->partition_bits = 5;
    o->host_threads = 0;
    o->hard_query_limit = 100000;
    o->stream = nullptr;
}

// the bounds tuning.hpp repeats, since it includes no engine header
static_assert(kTuneCoreQueue == kCoreQueue && kTuneMsHeadMax == kMsHeadMax && kTunePpMinSlots == kPpMinSlots &&
                  kTunePpMaxSlots == kPpMaxSlots, "tuning.hpp: bounds out of step with engine.hpp");

int tgo_set_tuning(tgo_ctx* ctx, int32_t key, double value) {
    if (!ctx) return TGO_E_INVALID;
    return tuning_set(ctx->tune, key, value, ctx->err);
}

int tgo_create(const tgo_options* opts, tgo_ctx** out) {
    if (!opts || !out) return TGO_E_INVALID;
    *out = nullptr;
    if (opts->abi_version != TGO_ABI_VERSION) return TGO_E_INVALID;
    if (opts->partition_bits < 0 || opts->partition_bits > 16) return TGO_E_INVALID;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return TGO_E_HIP;
    if (opts->device < 0 || opts->device >= ndev) return TGO_E_INVALID;
    if (hipSetDevice(opts->device) != hipSuccess) return TGO_E_HIP;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, opts->device) != hipSuccess) return TGO_E_HIP;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return TGO_E_HIP;   // gfx950 code objects only
    tgo_ctx* ctx = new (std::nothrow) tgo_ctx();
    if (!ctx) return TGO_E_OOM;
    ctx->opts = *opts;
    ctx->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (ctx->opts.hard_query_limit <= 0) ctx->opts.hard_query_limit = 100000;
    if (opts->stream) {
        ctx->stream = static_cast<hipStream_t>(opts->stream);
    } else {
        if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) { delete ctx; return TGO_E_HIP; }
        ctx->own_stream = true;
    }
    if (hipEventCreate(&ctx->ev0) != hipSuccess || hipEventCreate(&ctx->ev1) != hipSuccess) {
        delete ctx;
        return TGO_E_HIP;
    }
    *out = ctx;
    return TGO_OK;
}

void tgo_destroy(tgo_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->opts.device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    free_graph(ctx);
    ctx->dec.release();
    if (ctx->sc.hcnt) (void)hipHostFree(ctx->sc.hcnt);
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

const char* tgo_last_error(const tgo_ctx* ctx) { return ctx ? ctx->err.c_str() : "null ctx"; }

int64_t tgo_num_vertices(const tgo_ctx* ctx) { return ctx && ctx->loaded ? ctx->g.n : 0; }

int tgo_vertex_ids(tgo_ctx* ctx, int64_t* out) {
    if (!ctx || !out) return TGO_E_INVALID;
    if (!ctx->loaded) return fail(ctx, TGO_E_STATE, "no graph loaded");
    std::memcpy(out, ctx->titan_id.data(), ctx->titan_id.size() * sizeof(int64_t));
    return TGO_OK;
}

int tgo_graph_csr(tgo_ctx* ctx, int32_t which, int64_t* nnz, int64_t* off, int32_t* adj, int32_t* w, uint32_t* col) {
    if (!ctx || !nnz || which < 0 || which > 2) return TGO_E_INVALID;
    if (!ctx->loaded) return fail(ctx, TGO_E_STATE, "no graph loaded");
    const DevGraph& g = ctx->g;
    if (which == 2 && !g.has_transpose) { *nnz = -1; return TGO_OK; }
    const DevCsr& c = which == 0 ? g.out : which == 1 ? g.in : g.push_t;
    *nnz = c.nnz;
    (void)hipSetDevice(ctx->opts.device);
    if (off) HIP_TRY(copy_chunked(off, c.off, (g.n + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (adj && c.nnz) HIP_TRY(copy_chunked(adj, c.adj, c.nnz * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (w && c.w && c.nnz) HIP_TRY(copy_chunked(w, c.w, c.nnz * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (col && c.col && c.nnz) HIP_TRY(copy_chunked(col, c.col, c.nnz * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return TGO_OK;
}

int tgo_graph_perm(tgo_ctx* ctx, int32_t* perm) {
    if (!ctx || !perm) return TGO_E_INVALID;
    if (!ctx->loaded) return fail(ctx, TGO_E_STATE, "no graph loaded");
    (void)hipSetDevice(ctx->opts.device);
    HIP_TRY(hipMemcpy(perm, ctx->g.perm, ctx->g.n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return TGO_OK;
}

int tgo_dense_ids(tgo_ctx* ctx, const int64_t* titan_ids, int64_t count, int64_t* dense_out) {
    if (!ctx) return TGO_E_INVALID;
    if (count < 0 || (count > 0 && (!titan_ids || !dense_out))) return fail(ctx, TGO_E_INVALID, "null argument");
    if (!ctx->loaded) return fail(ctx, TGO_E_STATE, "no graph loaded");
    const int pb = ctx->opts.partition_bits;
    for (int64_t i = 0; i < count; ++i) {
        int64_t id = titan_ids[i];
        if (is_partitioned_vertex(id, pb)) id = canonical_vertex_id(id, pb);    // getCanonicalId
        dense_out[i] = dense_of(ctx, id);
    }
    return TGO_OK;
}

int tgo_stats_get(tgo_ctx* ctx, tgo_stats* out) {
    if (!ctx || !out) return TGO_E_INVALID;
    *out = ctx->st;
    return TGO_OK;
}

int tgo_sync(tgo_ctx* ctx) {
    if (!ctx) return TGO_E_INVALID;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return TGO_OK;
}

}  // extern "C"
