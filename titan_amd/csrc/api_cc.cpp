// api_cc.cpp — weakly connected components of a bothE load (cc.hip): tgo_components, tgo_copy_components.
// "changed" / "roots" words: Counters::qlen / red[0], read through the published mirror.
#include "ctx.hpp"

using namespace tgo;

namespace {

// The Scratch arrays one run uses, under the types it uses them as (row-order staging: sc.msg).
struct CcArrays {
    int32_t* parent;    // sc.level: n x int32
    int64_t* minid;     // sc.vec[0]: n x 8 bytes; the per-root minimum
    int64_t* label;     // sc.dist: n x int64; the labels in internal order, the published result
};

CcArrays cc_arrays(Scratch& s) { return CcArrays{s.level, reinterpret_cast<int64_t*>(s.vec[0]), s.dist}; }

int cc_word(tgo_ctx* ctx, bool roots, unsigned long long& out) {
    if (int rc = read_counters(ctx)) return rc;
    out = roots ? ctx->sc.hcnt->red[0] : ctx->sc.hcnt->qlen;
    return TGO_OK;
}

// Flatten the parent trees: pointer-jumping launches until one finds every vertex under a root.
int cc_compress(tgo_ctx* ctx, int32_t* parent, int32_t& rounds) {
    Scratch& s = ctx->sc;
    for (;;) {
        HIP_TRY(k_level_prep(s.cnt, nullptr, 0, nullptr, ctx->stream));
        {
            DevSpan span(ctx->stream, "components.jump", {"round", rounds});
            HIP_TRY(k_cc_jump(parent, ctx->g.n, &s.cnt->qlen, ctx->stream));
        }
        ++rounds;
        unsigned long long changed = 0;
        if (int rc = cc_word(ctx, false, changed)) return rc;
        if (!changed) return TGO_OK;
    }
}

}  // namespace

int tgo::titan_ids_by_index(tgo_ctx* ctx) {
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

extern "C" {

int tgo_components(tgo_ctx* ctx, const tgo_cc_args* a, int64_t* label_out, tgo_cc_info* info) {
    int rc = bothE_program_check(ctx, a, "tgo_cc_args", "connected components run", nullptr);
    if (rc) return rc;
    DevGraph& g = ctx->g;
    Scratch& s = ctx->sc;
    hipStream_t st = ctx->stream;
    const int64_t n = g.n;
    const CcArrays A = cc_arrays(s);
    if ((rc = titan_ids_by_index(ctx))) return rc;
    HIP_TRY(hipEventRecord(ctx->ev0, st));
    int32_t rounds = 0;
    const int path = g.has_transpose ? TGO_CC_PROPAGATE : TGO_CC_HOOK;
    unsigned long long components = 0;
    if (path == TGO_CC_HOOK) {
        // every edge sits once in the OUT lists; the first entries are hooked and flattened
        // first so that the bulk of the entries meets short trees
        HIP_TRY(k_cc_init(A.parent, n, st));
        {
            DevSpan span(st, "components.hook_sample");
            HIP_TRY(k_cc_hook(g.out, n, 0, 2, A.parent, st));
            HIP_TRY(k_cc_hook(g.in, n, 0, 1, A.parent, st));
        }
        rounds += 2;
        if ((rc = cc_compress(ctx, A.parent, rounds))) return rc;
        {
            DevSpan span(st, "components.hook_rest");
            HIP_TRY(k_cc_hook(g.out, n, 2, -1, A.parent, st));
        }
        ++rounds;
        if ((rc = cc_compress(ctx, A.parent, rounds))) return rc;
        DevSpan span(st, "components.label");
        HIP_TRY(k_fill_i64(A.minid, INT64_MAX, n, st));
        HIP_TRY(k_level_prep(s.cnt, nullptr, 0, nullptr, st));
        HIP_TRY(k_cc_min_id(A.parent, g.cc_tid, n, A.minid, st));
        HIP_TRY(k_cc_label(A.parent, A.minid, n, A.label, &s.cnt->red[0], st));
        span.end();
        if ((rc = cc_word(ctx, true, components))) return rc;
    } else {
        const View pull = pull_view(g, TGO_SCOPE_BOTH_E);
        HIP_TRY(hipMemcpyAsync(A.label, g.cc_tid, n * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
        for (;;) {
            HIP_TRY(k_level_prep(s.cnt, nullptr, 0, nullptr, st));
            {
                DevSpan span(st, "components.pull_round", {"round", rounds});
                HIP_TRY(k_cc_pull_round(pull, n, A.label, &s.cnt->qlen, st));
            }
            ++rounds;
            unsigned long long changed = 0;
            if ((rc = cc_word(ctx, false, changed))) return rc;
            if (!changed) break;
        }
        HIP_TRY(k_level_prep(s.cnt, nullptr, 0, nullptr, st));
        HIP_TRY(k_cc_count_own(A.label, g.cc_tid, n, &s.cnt->red[0], st));
        if ((rc = cc_word(ctx, true, components))) return rc;
    }
    if ((rc = program_end(ctx, rounds))) return rc;
    if (info) *info = tgo_cc_info{static_cast<int64_t>(components), rounds, path};
    if (label_out && (rc = rows_out(ctx, A.label, label_out))) return rc;
    publish_result(ctx, TGO_RESULT_COMPONENT, ResultSource{A.label, nullptr});
    return TGO_OK;
}

int tgo_copy_components(tgo_ctx* ctx, int64_t* label_out) {
    if (!ctx || !label_out) return TGO_E_INVALID;
    if (int rc = copy_open(ctx, TGO_RESULT_COMPONENT, "tgo_components")) return rc;
    return rows_out(ctx, ctx->sc.dist, label_out);
}

}  // extern "C"
