// api_generic.cpp — the primitives of a generic vertex program (edge programs, gathers, the global
// combine) and the result write-back of every program (results.hip), which shares their scratch.
#include "ctx.hpp"

using namespace tgo;

extern "C" {

// ------------------------------------------------------------------ generic vertex programs
static int generic_alloc(tgo_ctx* ctx) {
    Scratch& s = ctx->sc;
    if (s.gv[0]) return TGO_OK;
    for (int i = 0; i < 3; ++i) {
        HIP_TRY(dev_alloc(ctx, s.gv[i], ctx->g.n + 1));
        HIP_TRY(dev_alloc(ctx, s.gh[i], ctx->g.n + 1));
    }
    ctx->st.device_bytes = ctx->dev_bytes;
    return TGO_OK;
}

// Whether the gather's edge function reads e.value(weight).
static bool weight_edge_fn(const tgo_ctx* ctx, int fn) {
    return (fn >= TGO_EDGE_ADD_WEIGHT && fn <= TGO_EDGE_DIV_WEIGHT) || (fn == TGO_EDGE_PROGRAM && ctx->edge_prog.uses_w);
}

// Validate a postfix edge-function program (stack effects, constant indices, one result).
int tgo_set_edge_program(tgo_ctx* ctx, const tgo_edge_program* p) {
    if (!ctx) return TGO_E_INVALID;
    if (!p) { ctx->edge_prog = EdgeProg(); return TGO_OK; }
    if (p->n_ops < 1 || p->n_ops > TGO_EDGE_PROGRAM_MAX_OPS || !p->ops)
        return fail(ctx, TGO_E_INVALID, "edge program: 1 to " + std::to_string(TGO_EDGE_PROGRAM_MAX_OPS) + " ops");
    if (p->n_consts < 0 || p->n_consts > TGO_EDGE_PROGRAM_MAX_CONSTS || (p->n_consts > 0 && !p->iconsts && !p->fconsts))
        return fail(ctx, TGO_E_INVALID, "edge program: 0 to " + std::to_string(TGO_EDGE_PROGRAM_MAX_CONSTS) +
                                        " constants, long and / or double values");
    EdgeProg pg;
    int depth = 0;
    for (int i = 0; i < p->n_ops; ++i) {
        const int op = p->ops[i] & 0xFF, arg = p->ops[i] >> 8;
        const std::string at = "edge program op " + std::to_string(i) + ": ";
        if (op < TGO_OP_MSG || op > TGO_OP_ABS) return fail(ctx, TGO_E_INVALID, at + "unknown op");
        if (op != TGO_OP_CONST && arg != 0) return fail(ctx, TGO_E_INVALID, at + "only CONST takes an argument");
        if (op == TGO_OP_CONST && (arg < 0 || arg >= p->n_consts)) return fail(ctx, TGO_E_INVALID, at + "constant index");
        const int pops = op <= TGO_OP_CONST ? 0 : op >= TGO_OP_NEG ? 1 : 2;
        if (depth < pops) return fail(ctx, TGO_E_INVALID, at + "stack underflow");
        depth += (op <= TGO_OP_CONST ? 1 : op >= TGO_OP_NEG ? 0 : -1);
        if (depth > TGO_EDGE_PROGRAM_MAX_STACK) return fail(ctx, TGO_E_INVALID, at + "stack deeper than " +
                                                            std::to_string(TGO_EDGE_PROGRAM_MAX_STACK));
        if (op == TGO_OP_WEIGHT) pg.uses_w = 1;
        pg.ops[i] = p->ops[i];
    }
    if (depth != 1) return fail(ctx, TGO_E_INVALID, "edge program must leave exactly one value");
    pg.n = p->n_ops;
    pg.has_i = p->n_consts == 0 || p->iconsts;
    pg.has_f = p->n_consts == 0 || p->fconsts;
    for (int i = 0; i < p->n_consts; ++i) {
        if (p->iconsts) pg.ic[i] = p->iconsts[i];
        if (p->fconsts) pg.fc[i] = p->fconsts[i];
    }
    ctx->edge_prog = pg;
    return TGO_OK;
}

// Scope, value type, combiner (when used) and edge function of a Local receive.
static int check_gather_args(tgo_ctx* ctx, const tgo_gather_args* a, bool combiner) {
    if (!ctx->loaded) return fail(ctx, TGO_E_STATE, "no graph loaded");
    if (ctx->g.partitioned) return fail(ctx, TGO_E_UNSUPPORTED, "generic gathers run on a one-GPU load");
    if (a->scope < 0 || a->scope > 2) return fail(ctx, TGO_E_INVALID, "invalid scope");
    if (a->scope != ctx->g.scope && ctx->g.scope != TGO_SCOPE_BOTH_E)
        return fail(ctx, TGO_E_INVALID, "message scope differs from the scope the graph was loaded (preloaded) for");
    if (a->value_type < 0 || a->value_type > 1 || (combiner && (a->combiner < 0 || a->combiner > 2)) ||
        a->edge_fn < TGO_EDGE_IDENTITY || a->edge_fn > TGO_EDGE_PROGRAM)
        return fail(ctx, TGO_E_INVALID, "invalid value type, combiner or edge function");
    if (a->edge_fn == TGO_EDGE_PROGRAM) {
        const EdgeProg& pg = ctx->edge_prog;
        if (pg.n == 0) return fail(ctx, TGO_E_STATE, "TGO_EDGE_PROGRAM without a program (tgo_set_edge_program)");
        if (a->value_type == TGO_VAL_INT64 ? !pg.has_i : !pg.has_f)
            return fail(ctx, TGO_E_INVALID, "the edge program has no constants of the message type");
    }
    if (weight_edge_fn(ctx, a->edge_fn) && !ctx->g.has_weight)
        return fail(ctx, TGO_E_INVALID, "weight edge function on a graph loaded without a weight property");
    if (weight_edge_fn(ctx, a->edge_fn) && (ctx->g.weight_dt == TGO_DT_FLOAT || ctx->g.weight_dt == TGO_DT_DOUBLE) &&
        a->value_type == TGO_VAL_INT64)
        return fail(ctx, TGO_E_INVALID, "a Float / Double weight needs fp64 messages (long op double is a double in Java)");
    return TGO_OK;
}

static WeightCol weight_col(const DevGraph& g) {
    WeightCol wc;
    wc.kind = g.weight_dt == TGO_DT_FLOAT ? 1 : g.weight_dt == TGO_DT_LONG ? 2 : g.weight_dt == TGO_DT_DOUBLE ? 3 : 0;
    wc.wide = g.wval;
    return wc;
}

static int gather_error(tgo_ctx* ctx, unsigned long long err) {
    if (err & 2) return fail(ctx, TGO_E_PROGRAM, "vertex program failed: integer division by zero in an edge function");
    if (err) return fail(ctx, TGO_E_PROGRAM, "vertex program failed: a traversed edge has no value for the weight property");
    return TGO_OK;
}

int tgo_gather(tgo_ctx* ctx, const tgo_gather_args* a, const void* msg, const uint8_t* has, void* out,
               uint8_t* out_has) {
    if (!ctx) return TGO_E_INVALID;
    ctx->res_kind = -1;
    if (!a || !msg || !out || !out_has) return fail(ctx, TGO_E_INVALID, "null argument");
    int rc;
    if ((rc = check_gather_args(ctx, a, true))) return rc;
    (void)hipSetDevice(ctx->opts.device);
    if ((rc = generic_alloc(ctx))) return rc;
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    const int64_t n = ctx->g.n;
    HIP_TRY(hipEventRecord(ctx->ev0, st));
    HIP_TRY(hipMemcpyAsync(s.gv[0], msg, n * 8, hipMemcpyHostToDevice, st));
    if (has) HIP_TRY(hipMemcpyAsync(s.gh[0], has, n, hipMemcpyHostToDevice, st));
    else HIP_TRY(hipMemsetAsync(s.gh[0], 1, n, st));
    HIP_TRY(hipMemsetAsync(s.cnt, 0, sizeof(Counters), st));
    HIP_TRY(k_to_internal(s.gv[0], s.gh[0], ctx->g.perm, s.gv[1], s.gh[1], n, st));
    HIP_TRY(k_local_gather(pull_view(ctx->g, a->scope), n, a->value_type, s.gv[1], s.gh[1], a->combiner, a->edge_fn,
                           weight_col(ctx->g), ctx->edge_prog, s.gv[2], s.gh[2], &s.cnt->err, st));
    HIP_TRY(k_to_rows(s.gv[2], s.gh[2], ctx->g.perm, s.gv[0], s.gh[0], n, st));
    HIP_TRY(hipEventRecord(ctx->ev1, st));
    HIP_TRY(hipMemcpyAsync(out, s.gv[0], n * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out_has, s.gh[0], n, hipMemcpyDeviceToHost, st));
    // no event wait and no trace_resolve: the counter read, queued after ev1, is the gather's one wait
    if ((rc = read_counters(ctx))) return rc;
    if ((rc = program_elapsed(ctx))) return rc;
    return gather_error(ctx, s.hcnt->err);
}

int tgo_gather_lists(tgo_ctx* ctx, const tgo_gather_args* a, const void* msg, const uint8_t* has, int64_t* row_offsets,
                     void* values) {
    if (!ctx) return TGO_E_INVALID;
    ctx->res_kind = -1;
    if (!a || !msg || !row_offsets) return fail(ctx, TGO_E_INVALID, "null argument");
    int rc;
    if ((rc = check_gather_args(ctx, a, false))) return rc;
    (void)hipSetDevice(ctx->opts.device);
    if ((rc = generic_alloc(ctx))) return rc;
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    const DevGraph& g = ctx->g;
    const int64_t n = g.n;
    const View pull = pull_view(g, a->scope);
    const WeightCol wc = weight_col(g);
    HIP_TRY(hipMemcpyAsync(s.gv[0], msg, n * 8, hipMemcpyHostToDevice, st));
    if (has) HIP_TRY(hipMemcpyAsync(s.gh[0], has, n, hipMemcpyHostToDevice, st));
    else HIP_TRY(hipMemsetAsync(s.gh[0], 1, n, st));
    HIP_TRY(hipMemsetAsync(s.cnt, 0, sizeof(Counters), st));
    HIP_TRY(k_to_internal(s.gv[0], s.gh[0], g.perm, s.gv[1], s.gh[1], n, st));
    // offsets: counts per row (s.gv[2] as int64 n+1), scanned into s.gv[0]
    int64_t* cnt = reinterpret_cast<int64_t*>(s.gv[2]);
    int64_t* off = reinterpret_cast<int64_t*>(s.gv[0]);
    HIP_TRY(k_list_count(pull, g.perm, n, s.gh[1], weight_edge_fn(ctx, a->edge_fn), cnt, &s.cnt->err, st));
    HIP_TRY(scan_exclusive_i64(s.cub_tmp, s.cub_bytes, cnt, off, n + 1, st));
    HIP_TRY(hipMemcpyAsync(row_offsets, off, (n + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if ((rc = read_counters(ctx))) return rc;
    if ((rc = gather_error(ctx, s.hcnt->err))) return rc;
    // a vertex cut that receives two messages meets FulgoraUtil's ThrowingCombiner (:80-91)
    for (int64_t r : ctx->pv_rows)
        if (row_offsets[r + 1] - row_offsets[r] >= 2)
            return fail(ctx, TGO_E_PROGRAM, "The VertexProgram needs to define a message combiner in order to preserve "
                                            "memory and handle partitioned vertices");
    const int64_t total = row_offsets[n];
    if (!values || total == 0) return TGO_OK;
    if (total >= (int64_t(1) << 31)) return fail(ctx, TGO_E_UNSUPPORTED, "more than 2^31 messages in one receive");
    // keys in/out (4 B each) + values in/out (8 B each) + the internal -> row map
    char* buf = nullptr;
    const size_t bytes = static_cast<size_t>(total) * 24 + static_cast<size_t>(n) * 4 + 64;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&buf), bytes));
    uint64_t* val_in = reinterpret_cast<uint64_t*>(buf);
    uint64_t* val_out = val_in + total;
    uint32_t* key_in = reinterpret_cast<uint32_t*>(val_out + total);
    uint32_t* key_out = key_in + total;
    int32_t* inv = reinterpret_cast<int32_t*>(key_out + total);
    // column positions of the pull lists (pull_view: inE walks OUT entries, outE IN, bothE both)
    const uint32_t* col0 = !g.has_col ? nullptr : a->scope == TGO_SCOPE_OUT_E ? g.in.col : g.out.col;
    const uint32_t* col1 = !g.has_col || a->scope != TGO_SCOPE_BOTH_E ? nullptr : g.in.col;
    hipError_t e = k_list_fill_sort(pull, col0, col1, g.perm, inv, n,
                                    a->value_type, s.gv[1], s.gh[1], a->edge_fn, wc, ctx->edge_prog, off, total,
                                    key_in, key_out,
                                    val_in, val_out, s.sort_tmp, s.sort_bytes, &s.cnt->err, st);
    if (e == hipSuccess) e = hipMemcpyAsync(values, val_out, total * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(buf);
    HIP_TRY(e);
    if ((rc = read_counters(ctx))) return rc;
    return gather_error(ctx, s.hcnt->err);
}

int tgo_combine_global(tgo_ctx* ctx, int32_t value_type, int32_t combiner, int64_t nmsgs, const int64_t* targets,
                       const void* values, void* out, uint8_t* out_has) {
    if (!ctx) return TGO_E_INVALID;
    ctx->res_kind = -1;
    if (nmsgs < 0 || (nmsgs > 0 && (!targets || !values)) || !out || !out_has) return fail(ctx, TGO_E_INVALID, "null argument");
    if (!ctx->loaded) return fail(ctx, TGO_E_STATE, "no graph loaded");
    if (value_type < 0 || value_type > 1 || combiner < 0 || combiner > 2)
        return fail(ctx, TGO_E_INVALID, "invalid value type or combiner");
    if (nmsgs >= (int64_t(1) << 31)) return fail(ctx, TGO_E_UNSUPPORTED, "more than 2^31 global messages in one superstep");
    const int64_t n = ctx->g.n;
    for (int64_t i = 0; i < nmsgs; ++i)
        if (targets[i] < 0 || targets[i] >= n) return fail(ctx, TGO_E_INVALID, "global message target out of range");
    (void)hipSetDevice(ctx->opts.device);
    int rc = generic_alloc(ctx);
    if (rc) return rc;
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    HIP_TRY(hipMemsetAsync(s.gv[0], 0, n * 8, st));
    HIP_TRY(hipMemsetAsync(s.gh[0], 0, n, st));
    if (nmsgs > 0) {
        int64_t* buf = nullptr;          // targets, values, sort scratch (3 m): freed below
        HIP_TRY(hipMalloc(&buf, static_cast<size_t>(nmsgs) * 5 * sizeof(int64_t)));
        hipError_t e = hipMemcpyAsync(buf, targets, nmsgs * 8, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(buf + nmsgs, values, nmsgs * 8, hipMemcpyHostToDevice, st);
        if (e == hipSuccess)
            e = k_global_combine(s.sort_tmp, s.sort_bytes, buf, nmsgs, n, value_type, buf + nmsgs, combiner, buf + 2 * nmsgs,
                                 s.gv[0], s.gh[0], st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        (void)hipFree(buf);
        HIP_TRY(e);
    }
    HIP_TRY(hipMemcpyAsync(out, s.gv[0], n * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out_has, s.gh[0], n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return TGO_OK;
}

static int result_rows_impl(tgo_ctx* ctx, const tgo_result_args* a, const ResultSource& src, bool empty,
                            tgo_result_size* size, const tgo_rows_buf* out) {
    if (out && (!out->row_keys || !out->row_entry_begin || !out->row_byte_begin || !out->entry_bytes ||
                !out->entry_limit_valpos))
        return fail(ctx, TGO_E_INVALID, "incomplete tgo_rows_buf");
    (void)hipSetDevice(ctx->opts.device);
    const int64_t n = ctx->g.n;
    const tgo_result_size want = *size;
    if (empty) {
        *size = tgo_result_size{0, 0, 0};
        if (out) out->row_entry_begin[0] = out->row_byte_begin[0] = 0;
        return TGO_OK;
    }
    int64_t* scratch[4] = {nullptr, nullptr, nullptr, nullptr};
    auto release = [&] { for (auto* p : scratch) if (p) (void)hipFree(p); };
    for (auto*& p : scratch)
        if (hipMalloc(&p, (n + 1) * sizeof(int64_t)) != hipSuccess) { release(); return fail(ctx, TGO_E_OOM, "result scratch"); }
    ResultRows rr;
    std::vector<int64_t> row_src;
    std::string err;
    int rc = encode_results(src, a, ctx->g.perm, n, scratch, ctx->sc.cub_tmp, ctx->sc.cub_bytes, &rr,
                            ctx->stream, err);
    if (!rc && out) {
        if (want.nrows < rr.nrows || want.nentries < rr.nentries || want.nbytes < rr.nbytes) {
            release();
            *size = tgo_result_size{rr.nrows, rr.nentries, rr.nbytes};
            return fail(ctx, TGO_E_INVALID, "result buffers smaller than the sizes of the first call");
        }
        row_src.resize(static_cast<size_t>(std::max<int64_t>(1, rr.nrows)));
        rr.write = true;
        rr.row_src = row_src.data();
        rr.row_entry_begin = out->row_entry_begin;
        rr.row_byte_begin = out->row_byte_begin;
        rr.entry_bytes = out->entry_bytes;
        rr.entry_limit_valpos = out->entry_limit_valpos;
        rc = encode_results(src, a, ctx->g.perm, n, scratch, ctx->sc.cub_tmp, ctx->sc.cub_bytes, &rr,
                            ctx->stream, err);
        // row keys: IDManager.getKey of each vertex id (IDManager.java:461-473)
        const int pb = ctx->opts.partition_bits;
        for (int64_t i = 0; !rc && i < rr.nrows; ++i) {
            const uint64_t vid = static_cast<uint64_t>(ctx->titan_id[static_cast<size_t>(row_src[i])]);
            const uint64_t part = pb ? (vid >> 3) & ((1ULL << pb) - 1) : 0;
            const uint64_t count = vid >> (3 + pb);
            out->row_keys[i] = static_cast<int64_t>((pb ? part << (64 - pb) : 0) | (count << 3) | (vid & 7));
        }
    }
    release();
    if (rc) return fail(ctx, rc, err);
    *size = tgo_result_size{rr.nrows, rr.nentries, rr.nbytes};
    return TGO_OK;
}

int tgo_result_rows(tgo_ctx* ctx, const tgo_result_args* a, tgo_result_size* size, const tgo_rows_buf* out) {
    if (!ctx) return TGO_E_INVALID;
    if (!a || !size) return fail(ctx, TGO_E_INVALID, "null args");
    if (a->kind < TGO_RESULT_DISTANCE || a->kind > TGO_RESULT_TRUSS || a->kind == TGO_RESULT_VALUES)
        return fail(ctx, TGO_E_INVALID, "invalid result kind");
    if (ctx->res_kind != a->kind)
        return fail(ctx, TGO_E_STATE, "no finished program of that kind is the last one run on this ctx");
    // a component label is a Titan id of the graph: an Integer key must be able to hold them all
    if ((a->kind == TGO_RESULT_COMPONENT || a->kind == TGO_RESULT_SCC || a->kind == TGO_RESULT_PEER_PRESSURE) &&
        a->datatypes[0] == TGO_DT_INTEGER)
        for (const int64_t id : ctx->titan_id)
            if (id < INT32_MIN || id > INT32_MAX)
                return fail(ctx, TGO_E_INVALID, "a value of an Integer compute key is out of int range");
    if (a->kind == TGO_RESULT_TRIANGLES && a->datatypes[0] == TGO_DT_INTEGER && ctx->tri_max > INT32_MAX)
        return fail(ctx, TGO_E_INVALID, "a value of an Integer compute key is out of int range");
    // a core number is at most d(v) < 2^31: an Integer key holds every one
    if (a->kind == TGO_RESULT_CORE && a->datatypes[0] != TGO_DT_LONG && a->datatypes[0] != TGO_DT_INTEGER &&
        a->datatypes[0] != TGO_DT_OBJECT)
        return fail(ctx, TGO_E_INVALID, "the core number's compute key must be Long, Integer or generic (Object)");
    // a truss value is at most d(v) + 1 < 2^31: as the core number
    if (a->kind == TGO_RESULT_TRUSS && a->datatypes[0] != TGO_DT_LONG && a->datatypes[0] != TGO_DT_INTEGER &&
        a->datatypes[0] != TGO_DT_OBJECT)
        return fail(ctx, TGO_E_INVALID, "the truss number's compute key must be Long, Integer or generic (Object)");
    if ((a->kind == TGO_RESULT_SCC || a->kind == TGO_RESULT_PEER_PRESSURE) && a->datatypes[0] != TGO_DT_LONG && a->datatypes[0] != TGO_DT_INTEGER &&
        a->datatypes[0] != TGO_DT_OBJECT)
        return fail(ctx, TGO_E_INVALID, "the component label's compute key must be Long, Integer or generic (Object)");
    if (a->kind == TGO_RESULT_BETWEENNESS && a->datatypes[0] != TGO_DT_DOUBLE && a->datatypes[0] != TGO_DT_OBJECT)
        return fail(ctx, TGO_E_INVALID, "the betweenness value's compute key must be Double or generic (Object)");
    if (a->kind == TGO_RESULT_CLOSENESS)
        for (int k = 0; k < 2; ++k)
            if (a->datatypes[k] != TGO_DT_DOUBLE && a->datatypes[k] != TGO_DT_OBJECT)
                return fail(ctx, TGO_E_INVALID, "the closeness and harmonic compute keys must be Double or generic (Object)");
    return result_rows_impl(ctx, a, ctx->res_src, ctx->res_empty, size, out);
}

int tgo_result_rows_values(tgo_ctx* ctx, const tgo_result_args* a, const void* values, const uint8_t* present,
                           tgo_result_size* size, const tgo_rows_buf* out) {
    if (!ctx) return TGO_E_INVALID;
    if (!a || !size || !values || !present) return fail(ctx, TGO_E_INVALID, "null args");
    if (!ctx->loaded) return fail(ctx, TGO_E_STATE, "no graph loaded");
    if (a->kind != TGO_RESULT_VALUES) return fail(ctx, TGO_E_INVALID, "tgo_result_rows_values takes kind TGO_RESULT_VALUES");
    if (ctx->g.partitioned) return fail(ctx, TGO_E_UNSUPPORTED, "generic programs run on a one-GPU load");
    const int64_t n = ctx->g.n;
    if (a->reserved == TGO_VAL_INT64 && a->datatypes[0] == TGO_DT_INTEGER) {
        const int64_t* v = static_cast<const int64_t*>(values);
        for (int64_t i = 0; i < n; ++i)
            if (present[i] && (v[i] < INT32_MIN || v[i] > INT32_MAX))
                return fail(ctx, TGO_E_INVALID, "a value of an Integer compute key is out of int range");
    }
    (void)hipSetDevice(ctx->opts.device);
    int rc = generic_alloc(ctx);
    if (rc) return rc;
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    HIP_TRY(hipMemcpyAsync(s.gv[0], values, n * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(s.gh[0], present, n, hipMemcpyHostToDevice, st));
    HIP_TRY(k_to_internal(s.gv[0], s.gh[0], ctx->g.perm, s.gv[1], s.gh[1], n, st));
    HIP_TRY(hipStreamSynchronize(st));
    return result_rows_impl(ctx, a, ResultSource{s.gv[1], s.gh[1]}, false, size, out);
}

}  // extern "C"
