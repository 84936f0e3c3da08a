// part_load.cpp — the partitioned load from edgestore rows.  Rank r hands in the rows of its vertices (a row
// holds the vertex's OUT and IN entries, so a 1-D vertex partition is a row-range partition of
// the scan); the decode and the cut are the one-GPU rules per row (VertexJobConverter.java:
// 109-129, the 100 000 cap in column order: QueryContainer.java:28,122, ColumnValueStore.java:
// 47-69), so every rank's lists are exactly the lists tgo_load_rows would hold for those rows.
// Collectives (all on the exchange, every rank in the same order):
//   1. MAX of {decode failed, live rows}: a failure on any rank fails every rank here;
//      S = the largest live count rounded up to 64 (slot ids r * S + i, padding entry-less);
//   2. all-gather of the live Titan ids at their slots: the global id map;
//   3. (layout) all-gather of the degree-grouped slot layout;
//   4. SUM of the cut rows; when a single-direction scope cut any row, its push view is no
//      transpose of the stored opposite lists: the pull entries go to their sources' owners
//      (all-to-all of the counts, all-to-allv of the pairs) and become the push rows there.
#include <algorithm>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "part_exchange.hpp"

using namespace tgo;

namespace {
struct DevTmp {                 // a device temporary of the load (the ctx holds no graph yet)
    void* p = nullptr;
    ~DevTmp() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, std::max<size_t>(bytes, 8)); }
};
}  // namespace

// local_rc: a failure this rank met before the collective part (its staging is dropped); the
// ranks still agree on it, so every rank returns an error and none waits in an exchange.
static int finish_partition_rows(tgo_ctx* ctx, tgo_exchange* x, int32_t layout, int64_t* part_out, int local_rc,
                                 const std::string& local_err) {
    const int W = x->world, R = x->rank;
    hipStream_t st = ctx->stream;
    std::string err = local_err;
    // a HIP failure here releases the peers (abort); an exchange failure does not
    Driver d;
    d.ctx = ctx; d.x = x; d.st = st;
    d.prefix = "tgo_finish_partition_rows: ";
    d.hip_aborts = true;
    DevTmp red;
    if (red.alloc(8 * sizeof(int64_t)) != hipSuccess) return d.hip("scratch");
    // element-wise reduction of k host words over the ranks
    auto reduce = [&](int64_t* v, int k, int op) { return d.reduce_copy(static_cast<int64_t*>(red.p), v, k, op, "reduce"); };
    // 1. decode, then agree on failure and on the slot size
    RowStaging stg;
    int drc = local_rc;
    if (drc) part_drop_staging(ctx);
    else drc = part_rows_take(ctx, stg, err);
    const int64_t count = drc ? 0 : static_cast<int64_t>(stg.vid.size());
    // a rank without staged rows (an empty range) takes the scope / weightedness of the others
    const bool staged = !drc && stg.active;
    int64_t v1[4] = {drc ? 1 : 0, count, staged ? stg.opts.scope + 1 : 0, staged && stg.opts.weight_key != 0 ? 1 : 0};
    const int64_t own_scope = v1[2], own_weighted = v1[3];
    if (int rc = reduce(v1, 4, tgo_exchange::kRedMax)) return rc;
    if (drc) return fail(ctx, drc, "tgo_finish_partition_rows: " + err);
    if (v1[0]) return fail(ctx, TGO_E_INVALID, "tgo_finish_partition_rows: another rank failed to decode its rows");
    if (!staged) {
        stg.opts.scope = static_cast<int32_t>(std::max<int64_t>(0, v1[2] - 1));
        stg.opts.weight_key = v1[3];
    }
    // ranks that disagree on the scope or the weight key fail below (agreed with the assembly)
    int mismatch = staged && (own_scope != v1[2] || own_weighted != v1[3]);
    const int64_t S = std::max<int64_t>(64, (v1[1] + 63) / 64 * 64), lo = static_cast<int64_t>(R) * S;
    const int64_t n_global = static_cast<int64_t>(W) * S;
    if (n_global >= INT32_MAX) return fail(ctx, TGO_E_UNSUPPORTED, "tgo_finish_partition_rows: more than 2^31 - 1 slots");
    // 2. the global id map: every rank's live ids at their slots
    std::vector<int64_t> slot_vid(static_cast<size_t>(n_global));
    {
        DevTmp buf;
        if (buf.alloc(n_global * sizeof(int64_t)) != hipSuccess) return d.hip("id buffer");
        std::vector<int64_t> own(static_cast<size_t>(S));
        for (int64_t i = 0; i < S; ++i) own[i] = i < count ? stg.vid[i] : -1 - (lo + i);   // padding: never a Titan id
        int64_t* b = static_cast<int64_t*>(buf.p);
        if (int rc = d.upload(b + lo, own.data(), S * sizeof(int64_t), "id upload")) return rc;
        if (int r = x->all_gather(b, static_cast<size_t>(S) * sizeof(int64_t), st)) return d.xfail(r);
        if (int rc = d.download(slot_vid.data(), b, n_global * sizeof(int64_t), "id read")) return rc;
    }
    HostGraph h;
    const int threads = threads_of(ctx);
    int arc = assemble_partition_rows(stg, slot_vid, S, R, h, threads, err);
    if (!arc && mismatch) {
        err = "the ranks staged rows with different scopes or weight keys";
        arc = TGO_E_INVALID;
    }
    std::vector<int64_t>().swap(slot_vid);
    // 3. the degree-grouped layout of every rank's slots (a rank whose assembly failed still
    //    takes part in the collective; the failure is agreed in step 4)
    if (layout) {
        DevTmp buf;
        if (buf.alloc(n_global * sizeof(int32_t)) != hipSuccess) return d.hip("layout buffer");
        std::vector<int32_t> lay(static_cast<size_t>(n_global));
        if (arc) for (int64_t i = 0; i < S; ++i) lay[lo + i] = static_cast<int32_t>(lo + i);
        else partition_rows_layout(h, lo, lay.data() + lo);
        int32_t* b = static_cast<int32_t*>(buf.p);
        if (int rc = d.upload(b + lo, lay.data() + lo, S * sizeof(int32_t), "layout upload")) return rc;
        if (int r = x->all_gather(b, static_cast<size_t>(S) * sizeof(int32_t), st)) return d.xfail(r);
        if (int rc = d.download(lay.data(), b, n_global * sizeof(int32_t), "layout read")) return rc;
        if (!arc) arc = apply_partition_layout(h, lo, lay.data(), threads, err);
    }
    // 4. cut rows anywhere: the push view from every rank's pull entries (and a last agreement
    //    on failure before the graph replaces the ctx's)
    int64_t v4[3] = {arc ? 1 : 0, h.truncated, count};
    if (int rc = reduce(v4, 3, tgo_exchange::kRedSum)) return rc;
    if (arc) return fail(ctx, arc, "tgo_finish_partition_rows: " + err);
    if (v4[0]) return fail(ctx, TGO_E_INVALID, "tgo_finish_partition_rows: another rank failed to assemble its rows");
    if (v4[1] > 0 && h.scope != TGO_SCOPE_BOTH_E) {
        std::vector<int64_t> cnt, pairs;
        partition_pull_pairs(h, lo, S, W, cnt, pairs);
        DevTmp dc, rc_, sbuf, rbuf;
        if (dc.alloc(W * sizeof(int64_t)) != hipSuccess || rc_.alloc(W * sizeof(int64_t)) != hipSuccess) return d.hip("count buffers");
        std::vector<int64_t> rcnt(W);
        if (int rc = d.upload(dc.p, cnt.data(), W * sizeof(int64_t), "counts")) return rc;
        if (int r = x->all_to_all(dc.p, rc_.p, sizeof(int64_t), st)) return d.xfail(r);
        if (int rc = d.download(rcnt.data(), rc_.p, W * sizeof(int64_t), "count read")) return rc;
        std::vector<size_t> sb, so, rb, ro;
        const size_t a = peer_splits(cnt.data(), W, 16, sb, so), b = peer_splits(rcnt.data(), W, 16, rb, ro);
        if (sbuf.alloc(a) != hipSuccess || rbuf.alloc(b) != hipSuccess) return d.hip("pair buffers");
        if (a) if (int rc = d.upload(sbuf.p, pairs.data(), a, "pairs")) return rc;
        if (int r = x->all_to_allv(sbuf.p, sb.data(), so.data(), rbuf.p, rb.data(), ro.data(), st)) return d.xfail(r);
        std::vector<int64_t> recv(b / 8);
        if (int rc = d.download(recv.data(), rbuf.p, b, "pair read")) return rc;
        partition_push_from_pairs(h, recv.data(), static_cast<int64_t>(b / 16));
    }
    if (int rc = part_upload(ctx, h, n_global, lo)) return rc;
    ctx->st.num_vertices = count;
    part_out[0] = count;
    part_out[1] = S;
    part_out[2] = v4[2];
    return TGO_OK;
}

extern "C" int tgo_finish_partition_rows(tgo_ctx* ctx, tgo_exchange* x, int32_t layout, int64_t* part) {
    if (!ctx) return TGO_E_INVALID;
    if (!x || !part || x->world < 1 || x->rank < 0 || x->rank >= x->world)
        return fail(ctx, TGO_E_INVALID, "tgo_finish_partition_rows: bad arguments");
    return finish_partition_rows(ctx, x, layout, part, TGO_OK, std::string());
}

extern "C" int tgo_load_partition_rows(tgo_ctx* ctx, tgo_exchange* x, const tgo_rows* rows, const tgo_schema* schema,
                                       const tgo_load_opts* opts, int32_t layout, int64_t* part) {
    if (!ctx) return TGO_E_INVALID;
    if (!x || !part || x->world < 1 || x->rank < 0 || x->rank >= x->world)
        return fail(ctx, TGO_E_INVALID, "tgo_load_partition_rows: bad arguments");
    const int rc = tgo_load_rows(ctx, rows, schema, opts);
    return finish_partition_rows(ctx, x, layout, part, rc, rc ? std::string(tgo_last_error(ctx)) : std::string());
}
