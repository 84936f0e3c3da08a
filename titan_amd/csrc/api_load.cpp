// api_load.cpp — a host graph onto the device (CSRs, row blocks, the PageRank layout, scratch) and
// the load entry points, one-GPU and partitioned.
#include <chrono>
#include <cstdio>
#include <cstring>
#include "codec.hpp"
#include "ctx.hpp"

using namespace tgo;

namespace tgo {

// Cache-blocked PageRank in-lists (ColdBlocks, engine.hpp) for one-GPU PageRank.
// TGO_PR_BLOCKED=0 turns it off; TGO_PR_HOT / TGO_PR_SEG set the hot threshold and the cold
// segment size in sources (defaults: 384 K sources = 3 MB of fp64 messages each, under one
// XCD's 4 MB L2 so the row streams do not evict the head; swept on RMAT-24 in
// profiles/r02m_pr_probe.log and profiles/r02an_pr_hot_seg_probe*.log).
constexpr int64_t kPrSegDefault = 393216;   // 3 MB (profiles/r02an_pr_hot_seg_probe*.log)
// hot head: 3 MB for the slot tiles; 6 MB for the fixed-point super-tiles, whose source-sorted
// 380 K-entry tiles reuse lines enough that a head past one XCD's L2 still pays (RMAT-24
// ms/update: 384 K 0.852, 512 K 0.827, 768 K 0.814-0.818, 1 M 0.830, 1.5 M 0.913;
// profiles/r05j_pr_fx_hot_ab.log, r05k_pr_fx_hot_ab.log)
// The hot head (sources of the hot pass; the partitioned layout's gathered head, over every
// rank).  Round 5's source-split hot pass (TGO_PR_FX_SPLIT=2, 1 M sources, each half's 4 MB an
// XCD's L2) won with returning 128-bit LDS atomics; with the split non-returning accumulators
// the one-launch 768 K head is faster (same box, RMAT-24: split 1 M 0.897-0.902, unsplit 768 K
// 0.802-0.807, 655 K 0.806, 1 M 0.828 ms/update; profiles/r06r_*, r06s_pr_unsplit_sweep.log),
// so the split is off by default (TGO_PR_FX_SPLIT=1)
static int64_t pr_fx_split_default() { return env_i64("TGO_PR_FX_SPLIT", 1); }
int64_t pr_hot_default() {
    if (env_i64("TGO_PR_FX", 1) == 0) return 393216;
    return pr_fx_split_default() > 1 ? 1048576 : 786432;
}
// LDS window of the hottest sources (lds_window, spmv.hip; TGO_PR_WIN, at most 12288 doubles =
// 96 KB beside the 16 waves' 4 KB item buffers).  Off by default: measured slower at every
// window size (negative result 13: 1.252 -> 1.385-1.476 ms/update at RMAT-24)
constexpr int64_t kPrWinDefault = 0, kPrWinMax = 12288;

struct HostRowBlocks {              // build_row_blocks' vectors, and their upload into rb
    std::vector<int64_t> blk, crow, cbeg, cend, lrow, lch;
};
static hipError_t upload_blocks(tgo_ctx* ctx, const std::vector<int64_t>& off, const HostRowBlocks& h, RowBlocks& rb) {
    rb.nblocks = static_cast<int64_t>(h.blk.size()) - 1;
    rb.nchunks = static_cast<int64_t>(h.crow.size());
    rb.nlong = static_cast<int64_t>(h.lrow.size());
    hipError_t e;
    if ((e = upload(ctx, rb.blk, h.blk)) != hipSuccess) return e;
    if ((e = upload(ctx, rb.chunk_row, h.crow)) != hipSuccess) return e;
    if ((e = upload(ctx, rb.chunk_beg, h.cbeg)) != hipSuccess) return e;
    if ((e = upload(ctx, rb.chunk_end, h.cend)) != hipSuccess) return e;
    if ((e = upload(ctx, rb.long_row, h.lrow)) != hipSuccess) return e;
    if ((e = upload(ctx, rb.long_chunk, h.lch)) != hipSuccess) return e;
    std::vector<int64_t> desc(2 * h.blk.size());
    for (size_t b = 0; b < h.blk.size(); ++b) { desc[2 * b] = h.blk[b]; desc[2 * b + 1] = off[h.blk[b]]; }
    return upload(ctx, rb.bdesc, desc);
}

// CSR-adaptive row blocks of one CSR; `pack` (optional) source-sorts and packs the CSR's
// tiles first (spmv.hip gather_short_packed).
static hipError_t upload_row_blocks(tgo_ctx* ctx, const std::vector<int64_t>& off, RowBlocks& rb,
                                    std::vector<int32_t>* pack = nullptr, bool* packed = nullptr,
                                    int64_t tile = kTile, int shift = kPackShift) {
    HostRowBlocks h;
    build_row_blocks(off, tile, kMaxRows, h.blk, h.crow, h.cbeg, h.cend, h.lrow, h.lch);
    if (pack) *packed = pack_tiles(off, *pack, h.blk, h.cbeg, h.cend, tile, threads_of(ctx), shift);
    return upload_blocks(ctx, off, h, rb);
}

// upload_row_blocks with the tiles packed on the device, in place in d_adj (pr_layout.hip):
// the same blocks (built on the host from the offsets) and the same packed words.  *packed =
// false (d_adj untouched) when a source is too wide for the slot space (pack_tiles' rule).
static int upload_row_blocks_dev(tgo_ctx* ctx, const std::vector<int64_t>& off, RowBlocks& rb, int32_t* d_adj,
                                 int32_t max_src, bool* packed, int64_t tile, int shift, int64_t max_rows = kMaxRows) {
    HostRowBlocks h;
    build_row_blocks(off, tile, max_rows, h.blk, h.crow, h.cbeg, h.cend, h.lrow, h.lch);
    const std::vector<int64_t>&blk = h.blk, &cbeg = h.cbeg, &cend = h.cend;
    *packed = false;
    const int64_t src_limit = shift == kPackShift ? (int64_t(1) << (31 - shift)) : (int64_t(1) << (32 - shift));
    if (d_adj && shift >= 1 && shift <= 20 && tile <= (int64_t(1) << shift) && max_src < src_limit) {
        // tiles in entry order: short blocks, and the chunks of each long row (they cover it)
        std::vector<std::pair<int64_t, int64_t>> t;
        for (size_t b = 0; b + 1 < blk.size(); ++b) {
            const int64_t s0 = off[blk[b]], s1 = off[blk[b + 1]];
            if (s1 - s0 <= tile) t.emplace_back(s0, s1);
        }
        for (size_t c = 0; c < cbeg.size(); ++c) t.emplace_back(cbeg[c], cend[c]);
        std::sort(t.begin(), t.end());
        std::vector<int64_t> ts(t.size());
        for (size_t i = 0; i < t.size(); ++i) ts[i] = t[i].first;
        std::string err;
        if (int rc = pack_tiles_device(d_adj, off.back(), ts, nullptr, shift, ctx->stream, err)) return fail(ctx, rc, err);
        *packed = true;
    }
    HIP_TRY(upload_blocks(ctx, off, h, rb));
    return TGO_OK;
}

// Biased-exponent range [elo, ehi) in which the fixed-point PageRank sums are exact (spmv.hip
// kFxPoint): |v| >= 2^-53 (the 2^-80 resolution then costs < 2^-27 of a value), a row of
// max_len entries below 2^47 (|v| < 2^(47 - c) with 2^c >= max_len), and a tile's split H words
// (X >> 40, summed over at most min(max_len, kFxTileMax) entries of a row) below 2^63:
// |v| < 2^(23 - min(c, 22)); and |v| < 2^11 for the entry conversion (spmv.hip fx_hl).
constexpr int64_t kFxTileMax = int64_t(1) << 22;      // entries of a fixed-point tile / cold block
static void fx_range(int64_t max_len, int& elo, int& ehi) {
    int c = 0;
    while ((int64_t(1) << c) < max_len && c < 47) ++c;
    elo = 1023 - 53;
    ehi = std::min({1023 + 47 - c, 1023 + 23 - std::min(c, 22), 1023 + 11});
}

// Cache-blocked PageRank in-lists of the rows [0, n_rows) (rows past n_rows have no entries)
// over sources [0, n_src): built on the device from the uploaded in-lists (d_off / d_adj,
// pr_layout.hip) unless TGO_HOST_ASSEMBLY=1 (or a row is not sorted by source), then on the
// host; uploaded into cb.  job_row: the longest in-row of the whole job where `off` holds one
// rank's rows of it — the fixed-point range comes from the longer of the two, so every rank of a
// partitioned job checks what it emits against the range of the rank that sums the longest row.
int upload_cold_blocks(tgo_ctx* ctx, const std::vector<int64_t>& off, const std::vector<int32_t>& adj,
                       int64_t n_src, int64_t hot, int64_t n_rows, ColdBlocks& cb, bool& ready,
                       const int64_t* d_off, const int32_t* d_adj, int64_t d_nnz, int64_t win, int64_t job_row) {
    cb = ColdBlocks();
    ready = false;
    HostColdBlocks hc;
    static const bool trace = trace_on();
    auto t_last = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
        if (!trace && !tracing()) return;
        const auto now = std::chrono::steady_clock::now();
        const double ms = std::chrono::duration<double, std::milli>(now - t_last).count();
        if (trace) std::fprintf(stderr, "[tgo]   cold %-18s %8.1f ms\n", what, ms);
        trace_complete(std::string("pagerank_layout.") + what, ms * 1e3);
        t_last = now;
    };
    bool on_dev = false;
    win = std::min<int64_t>(win, kPrWinMax);        // the window and the waves' item buffers share 160 KB of LDS
    // TGO_PR_FX_COLD (default on): fixed-point cold blocks (spmv.hip cold_fx) of up to 4096
    // pieces and TGO_PR_FX_CE entries
    const bool cold_fx = env_i64("TGO_PR_FX", 1) != 0 && env_i64("TGO_PR_FX_COLD", 1) != 0 && win == 0;
    if (d_off && d_adj && !host_assembly()) {
        std::string err;
        if (int rc = build_cold_blocks_device(d_off, d_adj, static_cast<int64_t>(off.size()) - 1, d_nnz, n_src, hot,
                                              env_i64("TGO_PR_SEG", kPrSegDefault),
                                              cold_fx ? std::min(kFxTileMax, env_i64("TGO_PR_FX_CE", 65536)) : kTile,
                                              cold_fx ? std::min<int64_t>(env_i64("TGO_PR_FX_CP", 4096), int64_t(1) << (kPackShift + 1))
                                                      : kMaxRows,
                                              env_i64("TGO_PR_CPACK", 1) != 0, hc, on_dev, ctx->stream, err, win, cold_fx))
            return fail(ctx, rc, err);
        if (on_dev) lap("build (device)");
    }
    std::vector<int32_t> adj_dl;        // host copy of a device-resident list, for the host build
    if (!on_dev && d_adj && static_cast<int64_t>(adj.size()) != d_nnz) {
        adj_dl.resize(static_cast<size_t>(d_nnz));
        HIP_TRY(copy_chunked(adj_dl.data(), d_adj, static_cast<size_t>(d_nnz) * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    if (!on_dev) {
        if (!build_cold_blocks(off, adj_dl.empty() ? adj : adj_dl, n_src, hot, env_i64("TGO_PR_SEG", kPrSegDefault), kTile, kMaxRows,
                               threads_of(ctx), env_i64("TGO_PR_CPACK", 1) != 0, hc, win))
            return TGO_OK;                                // too small to block: plain gather
        lap("build (host)");
    }
    cb.hot = hc.hot;
    cb.seg = hc.seg;
    cb.npieces = static_cast<int64_t>(hc.cpid.size());
    cb.nblocks = static_cast<int64_t>(hc.bbeg.size());
    cb.max_xcd_blocks = hc.max_xcd_blocks;
    cb.xbase = hc.xbase;
    cb.n_rows = n_rows;
    const std::vector<int64_t> hoff_act(hc.hoff.begin(), hc.hoff.begin() + n_rows + 1);
    // hot tiles: 4096 entries (256 threads, 32 KB of LDS), 8192 (512 threads, 64 KB) or 16384
    // (1024 threads, 128 KB): a larger tile shares more 128-byte lines between the lanes of one
    // gather instruction (fewer L2 requests per entry) at fewer workgroups per CU
    const int64_t ht = env_i64("TGO_PR_HOT_TILE", 4096);
    cb.hot_tile = ht == 16384 ? 16384 : ht == 8192 ? 8192 : 4096;
    cb.hot_shift = cb.hot_tile == 16384 ? 14 : cb.hot_tile == 8192 ? 13 : kPackShift;
    cb.hot_pipe = static_cast<int>(env_i64("TGO_PR_HOT_PIPE", 0));
    cb.num_cus = ctx->num_cus;
    const bool pack = env_i64("TGO_PR_PACK", 1) != 0;
    if (!pack) cb.hot_tile = static_cast<int>(kTile), cb.hot_shift = kPackShift;
    // Fixed-point hot pass (TGO_PR_FX, default on; spmv.hip gather_hot_fx): super-tiles of
    // TGO_PR_FX_E entries, built on the device from the hot CSR (its sources must leave at least
    // 6 bits of the packed word for the row)
    if (on_dev && pack && env_i64("TGO_PR_FX", 1) != 0) {
        const int64_t hmax = std::min<int64_t>(hot, n_src);
        int sb = 1;
        while ((int64_t(1) << sb) < hmax) ++sb;         // sources < 2^sb
        // rows per super-tile: 2^12 (64 KB of LDS accumulators), or 2^13 with TGO_PR_FX_HROWS=8192
        // when the hot sources leave 13 bits of the packed word (hot <= 512 K)
        const int want_rbits = env_i64("TGO_PR_FX_HROWS", 4096) == 8192 ? 13 : 12;
        const int rbits = std::min(want_rbits, 32 - sb);
        if (rbits >= 6) {
            cb.hcsr.nnz = hc.d_hadj.n;
            adopt(ctx, cb.hcsr.adj, hc.d_hadj);
            HIP_TRY(upload(ctx, cb.hcsr.off, hc.hoff));
            std::vector<int64_t> tdesc, long_len;
            std::vector<int32_t> long_rows;
            std::string err;
            // entries per super-tile: larger tiles share more lines; about one tile a CU (hot
            // entries / 256, at most 1 M) — with the split accumulators and the one-launch head,
            // RMAT-24 (768 K head): 262 K 0.848, 430 K 0.802, 860 K 0.779, 1 M 0.772-0.786, 1.3 M
            // 0.832, 2 M 0.97 ms/update (profiles/r06t_pr_tile_entries_sweep.log, r06u_*); round 5
            // with returning atomics measured 512 K best (r05e_pr_fx_probe.log)
            const int64_t fx_e = std::min(kFxTileMax, env_i64("TGO_PR_FX_E", std::min<int64_t>(int64_t(1) << 20,
                                                                          std::max<int64_t>(int64_t(1) << 16, hc.hoff[n_rows] / 256))));
            if (int rc = pack_supertiles_device(cb.hcsr.adj, cb.hcsr.off, hc.hoff, n_rows, fx_e,
                                                rbits, tdesc, long_rows, long_len, ctx->stream, err))
                return fail(ctx, rc, err);
            cb.fx = true;
            cb.fx_rbits = rbits;
            cb.fx_ntiles = static_cast<int64_t>(tdesc.size() / 4);
            cb.fx_nlong = static_cast<int64_t>(long_rows.size());
            HIP_TRY(upload(ctx, cb.fx_desc, tdesc));
            HIP_TRY(upload(ctx, cb.fx_long_row, long_rows));
            HIP_TRY(dev_alloc(ctx, cb.fx_long_acc, 2 * std::max<int64_t>(cb.fx_nlong, 1)));
            HIP_TRY(hipMemset(cb.fx_long_acc, 0, 2 * std::max<int64_t>(cb.fx_nlong, 1) * sizeof(unsigned long long)));
            // TGO_PR_FX_SPLIT=S > 1: the hot pass in S launches over S ranges of the hot sources
            // (each range's messages fit an XCD's L2: 3 MB a half at 768 K hot sources)
            const int64_t split = std::min<int64_t>(8, std::max<int64_t>(1, pr_fx_split_default()));
            if (split > 1 && cb.fx_ntiles > 0) {
                HIP_TRY(dev_alloc(ctx, cb.fx_mid, cb.fx_ntiles * (split + 1)));
                HIP_TRY(dev_alloc(ctx, cb.fx_part, 2 * std::max<int64_t>(n_rows, 1)));
                const int64_t first = std::min<int64_t>(hmax, std::max<int64_t>(0, env_i64("TGO_PR_FX_SPLIT_AT", 0)));
                HIP_TRY(k_fx_split_points(reinterpret_cast<const uint32_t*>(cb.hcsr.adj), cb.fx_desc, cb.fx_ntiles, rbits,
                                          hmax, static_cast<int>(split), first, cb.fx_mid, ctx->stream));
                cb.fx_split = static_cast<int>(split);
            }
            lap("hot super-tiles");
        }
    }
    if (cb.fx) {
        // hot CSR adopted and packed above
    } else if (on_dev) {                            // hot tiles packed on the device
        cb.hcsr.nnz = hc.d_hadj.n;
        adopt(ctx, cb.hcsr.adj, hc.d_hadj);
        const int32_t max_src = static_cast<int32_t>(std::min<int64_t>(hot, n_src) - 1);
        if (int rc = upload_row_blocks_dev(ctx, hoff_act, cb.rb_hot, pack ? cb.hcsr.adj : nullptr, max_src, &cb.packed,
                                           cb.hot_tile, cb.hot_shift))
            return rc;
        if (pack && !cb.packed && cb.hot_tile != kTile) {
            cb.hot_tile = static_cast<int>(kTile);
            cb.hot_shift = kPackShift;
            cb.rb_hot = RowBlocks();
            if (int rc = upload_row_blocks_dev(ctx, hoff_act, cb.rb_hot, cb.hcsr.adj, max_src, &cb.packed, kTile,
                                               kPackShift))
                return rc;
        }
    } else {
        HIP_TRY(upload_row_blocks(ctx, hoff_act, cb.rb_hot, pack ? &hc.hadj : nullptr, &cb.packed, cb.hot_tile,
                                  cb.hot_shift));
        if (!cb.packed && cb.hot_tile != kTile) {  // sources too wide for the slot space: the 4096 form
            cb.hot_tile = static_cast<int>(kTile);
            cb.hot_shift = kPackShift;
            cb.rb_hot = RowBlocks();
            HIP_TRY(upload_row_blocks(ctx, hoff_act, cb.rb_hot, pack ? &hc.hadj : nullptr, &cb.packed));
        }
        HIP_TRY(upload(ctx, cb.hcsr.adj, hc.hadj));
        cb.hcsr.nnz = static_cast<int64_t>(hc.hadj.size());
    }
    lap("hot row blocks+pack");
    if (hc.win > 0) {                               // LDS window CSR: blocks over the active rows
        const std::vector<int64_t> woff_act(hc.woff.begin(), hc.woff.begin() + n_rows + 1);
        bool unused = false;
        // wave items of the window pass (lds_window): <= 512 entries, <= 64 rows
        if (int rc = upload_row_blocks_dev(ctx, woff_act, cb.rb_win, nullptr, 0, &unused, 512, kPackShift, 64)) return rc;
        HIP_TRY(upload(ctx, cb.woff, woff_act));
        if (hc.d_widx.present()) adopt(ctx, cb.widx, hc.d_widx);
        else HIP_TRY(upload(ctx, cb.widx, hc.widx));
        cb.win = hc.win;
    }
    if (!cb.fx) HIP_TRY(upload(ctx, cb.hcsr.off, hc.hoff));
    HIP_TRY(upload(ctx, cb.poff, hc.poff));
    if (hc.d_cadj.present()) adopt(ctx, cb.cadj, hc.d_cadj);
    else HIP_TRY(upload(ctx, cb.cadj, hc.cadj));
    HIP_TRY(upload(ctx, cb.cptr, hc.cptr));
    HIP_TRY(upload(ctx, cb.cpid, hc.cpid));
    HIP_TRY(upload(ctx, cb.bbeg, hc.bbeg));
    HIP_TRY(upload(ctx, cb.bend, hc.bend));
    HIP_TRY(upload(ctx, cb.xblk, hc.xblk));
    HIP_TRY(upload(ctx, cb.bsrc, hc.bsrc));
    if (hc.cfx) {                                   // cold_fx descriptors, launch-slot order
        std::vector<int64_t> desc(4 * hc.xblk.size());
        for (size_t j = 0; j < hc.xblk.size(); ++j) {
            const int32_t b = hc.xblk[j];
            const int64_t p0 = hc.bbeg[b], p1 = hc.bend[b];
            const int64_t src = hc.bsrc[b];
            if (p1 - p0 > (int64_t(1) << hc.cfx_shift) || src < 0) return fail(ctx, TGO_E_STATE, "cold block descriptor out of range");
            desc[4 * j] = hc.poff[p0]; desc[4 * j + 1] = hc.poff[p1]; desc[4 * j + 2] = p0;
            desc[4 * j + 3] = (src << 16) | (p1 - p0);
        }
        HIP_TRY(upload(ctx, cb.cfx_desc, desc));
        cb.cfx = true;
        cb.cfx_shift = hc.cfx_shift;
    } else {
        std::vector<int64_t> desc(4 * hc.xblk.size());
        for (size_t j = 0; j < hc.xblk.size(); ++j) {
            const int32_t b = hc.xblk[j];
            const int64_t p0 = hc.bbeg[b], p1 = hc.bend[b], s0 = hc.poff[p0], nnz = hc.poff[p1] - s0;
            const int64_t src = hc.bsrc.empty() ? 0 : hc.bsrc[b];
            if (nnz > kTile || src < 0) return fail(ctx, TGO_E_STATE, "cold block descriptor out of range");
            desc[4 * j] = p0; desc[4 * j + 1] = p1; desc[4 * j + 2] = s0; desc[4 * j + 3] = (src << 16) | nnz;
        }
        HIP_TRY(upload(ctx, cb.cdesc, desc));
    }
    cb.cpacked = hc.cpacked;
    HIP_TRY(dev_alloc(ctx, cb.partial, cb.npieces));
    HIP_TRY(dev_alloc(ctx, cb.csum, std::max<int64_t>(cb.n_rows, 1)));
    HIP_TRY(hipMemset(cb.csum, 0, std::max<int64_t>(cb.n_rows, 1) * sizeof(double)));
    cb.n_crows = static_cast<int64_t>(hc.crow.size());
    HIP_TRY(upload(ctx, cb.crow, hc.crow));
    if (cb.fx || cb.cfx) {                          // the fixed-point passes' range flag (FxGuard)
        int64_t max_len = job_row;
        for (size_t r = 0; r + 1 < off.size(); ++r) max_len = std::max(max_len, off[r + 1] - off[r]);
        fx_range(max_len, cb.fx_elo, cb.fx_ehi);
        HIP_TRY(dev_alloc(ctx, cb.fx_bad, 1));
        HIP_TRY(hipMemset(cb.fx_bad, 0, sizeof(unsigned)));
    }
    lap("uploads");
    ready = true;
    return TGO_OK;
}

static int upload_graph(tgo_ctx* ctx, HostGraph& h, bool allow_segments = true) {
    DevGraph& g = ctx->g;
    // TGO_TRACE=1: per-phase load times on stderr
    static const bool trace = trace_on();
    auto t_last = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
        if (!trace && !tracing()) return;
        const auto now = std::chrono::steady_clock::now();
        const double ms = std::chrono::duration<double, std::milli>(now - t_last).count();
        if (trace) std::fprintf(stderr, "[tgo] upload %-14s %8.1f ms\n", what, ms);
        trace_complete(std::string("upload.") + what, ms * 1e3);
        t_last = now;
    };
    g.n = h.n;
    g.scope = h.scope;
    g.has_weight = h.has_weight;
    g.weight_dt = h.weight_dt;
    g.has_col = h.out.has_col() || h.in.has_col();
    g.has_transpose = h.has_transpose;
    g.n_active = 0;
    for (int64_t v = h.n - 1; v >= 0; --v)
        if (h.out.off[v + 1] > h.out.off[v] || h.in.off[v + 1] > h.in.off[v]) { g.n_active = v + 1; break; }
    g.min_weight = 0;
    g.max_weight = 0;
    double wsum = 0.0;
    int64_t wcnt = 0;
    const bool wide = h.has_weight && wide_weight_dt(h.weight_dt);   // the column holds value-table indices
    for (const HostCsr* c : {&h.out, &h.in})
        for (int32_t x : c->w)
            if (x != kMissingWeight && !wide) {
                g.min_weight = std::min(g.min_weight, x);
                g.max_weight = std::max(g.max_weight, x);
                wsum += x;
                ++wcnt;
            }
    g.mean_weight = wcnt ? wsum / static_cast<double>(wcnt) : 1.0;
    auto up = [&](HostCsr& src, DevCsr& dst) -> hipError_t {
        hipError_t e;
        dst.nnz = src.nnz();
        if ((e = upload(ctx, dst.off, src.off)) != hipSuccess) return e;
        // lists assembled on the device stay there (adopted); host-assembled ones are copied
        if (src.dadj.present()) adopt(ctx, dst.adj, src.dadj);
        else if ((e = upload(ctx, dst.adj, src.adj)) != hipSuccess) return e;
        if (h.has_weight) {
            if (src.dw.present()) adopt(ctx, dst.w, src.dw);
            else if ((e = upload(ctx, dst.w, src.w)) != hipSuccess) return e;
        }
        if (src.dcol.present()) adopt(ctx, dst.col, src.dcol);
        else if (!src.col.empty() && (e = upload(ctx, dst.col, src.col)) != hipSuccess) return e;
        return hipSuccess;
    };
    HIP_TRY(up(h.out, g.out));
    HIP_TRY(up(h.in, g.in));
    if (h.has_transpose) HIP_TRY(up(h.push_t, g.push_t));
    g.wval = nullptr;
    if (wide) {
        const int64_t nv = h.d_wval.present() ? h.d_wval.n : static_cast<int64_t>(h.wval.size());
        if (nv == 0 && (g.out.nnz > 0 || g.in.nnz > 0)) return fail(ctx, TGO_E_STATE, "wide weights: the value table is missing");
        if (h.d_wval.present()) adopt(ctx, g.wval, h.d_wval);
        else HIP_TRY(upload(ctx, g.wval, h.wval));
    }
    lap("csr");
    // CSR-adaptive blocks for the two pull gathers (walk counts: out; PageRank: in).
    HIP_TRY(upload_row_blocks(ctx, h.out.off, g.rb_out));
    HIP_TRY(upload_row_blocks(ctx, h.in.off, g.rb_in));
    g.rb_out_ready = g.rb_in_ready = true;
    lap("row blocks");
    g.push_ws = DevCsr();
    g.push_ws_ready = false;
    if (allow_segments && h.has_weight && !wide && env_i64("TGO_DS_SPLIT", 1) != 0) {
        HostCsr ws;                      // light/heavy delta-stepping: push entries sorted by weight
        weight_sorted_push(h, ws, threads_of(ctx));
        HIP_TRY(up(ws, g.push_ws));
        g.push_ws_ready = true;
        lap("weight-sorted");
    }
    g.cold_in = ColdBlocks();
    g.cold_in_ready = false;
    if (allow_segments && h.scope != TGO_SCOPE_BOTH_E && env_i64("TGO_PR_BLOCKED", 1) != 0) {
        // rows >= n_active have no entries at all: the hot pass skips them (their rank
        // after any update is (1-a)/N, written once at the end of the program)
        if (int rc = upload_cold_blocks(ctx, h.in.off, h.in.adj, h.n, env_i64("TGO_PR_HOT", pr_hot_default()), g.n_active,
                                        g.cold_in, g.cold_in_ready, g.in.off, g.in.adj, g.in.nnz,
                                        env_i64("TGO_PR_WIN", kPrWinDefault)))
            return rc;
        lap("cold blocks");
    }
    // scratch
    Scratch& s = ctx->sc;
    const int64_t n = h.n, words = (n + 63) / 64 + 1;
    s.n = n;
    HIP_TRY(dev_alloc(ctx, s.level, n));
    HIP_TRY(dev_alloc(ctx, s.q[0], n + 1));
    HIP_TRY(dev_alloc(ctx, s.q[1], n + 1));
    HIP_TRY(dev_alloc(ctx, s.qdeg, n + 2));
    HIP_TRY(dev_alloc(ctx, s.qpre, n + 2));
    HIP_TRY(dev_alloc(ctx, s.fb, words));
    HIP_TRY(dev_alloc(ctx, s.nb, words));
    HIP_TRY(dev_alloc(ctx, s.vb, words));
    HIP_TRY(dev_alloc(ctx, s.dist, n));
    HIP_TRY(dev_alloc(ctx, s.msg, n));
    for (int i = 0; i < 3; ++i) HIP_TRY(dev_alloc(ctx, s.vec[i], n));
    s.partial_cap = std::max<int64_t>({g.rb_out.nchunks, g.rb_in.nchunks, g.cold_in.rb_hot.nchunks, 1});
    HIP_TRY(dev_alloc(ctx, s.partial, s.partial_cap));
    HIP_TRY(dev_alloc(ctx, s.cnt, 1));
    if (!s.hcnt) {
        void* hp = nullptr;
        // fine-grained: the publish kernel's system-scope stores reach the spinning host
        HIP_TRY(hipHostMalloc(&hp, kPublishWords * 8, hipHostMallocMapped | hipHostMallocCoherent));
        std::memset(hp, 0, kPublishWords * 8);
        s.hcnt = static_cast<Counters*>(hp);
        void* dp = nullptr;
        HIP_TRY(hipHostGetDevicePointer(&dp, hp, 0));
        s.hcnt_dev = static_cast<unsigned long long*>(dp);
        s.pub_seq = 0;
    }
    HIP_TRY(hipDeviceSynchronize());
    // the host graph is dropped after the upload: its id and perm vectors move (1.5 GB at 2^27)
    ctx->titan_id = std::move(h.titan_id);
    ctx->perm = std::move(h.perm);
    if (ctx->perm.empty()) { ctx->perm.resize(n); for (int64_t v = 0; v < n; ++v) ctx->perm[v] = static_cast<int32_t>(v); }
    HIP_TRY(upload(ctx, g.perm, ctx->perm));
    ctx->id_index.clear();
    ctx->id_sorted = true;
    if (!h.ids_sorted)
        for (int64_t v = 1; v < n && ctx->id_sorted; ++v) ctx->id_sorted = ctx->titan_id[v] > ctx->titan_id[v - 1];
    ctx->st.num_vertices = n;
    ctx->st.out_entries = g.out.nnz;       // (the device lists were adopted: h's are empty)
    ctx->st.in_entries = g.in.nnz;
    ctx->st.ghost_vertices = h.ghost;
    ctx->st.truncated_results = h.truncated;
    ctx->st.skipped_rows = h.skipped;
    ctx->st.partitioned_vertices = h.partitioned;
    ctx->st.partition_rows = h.partition_rows;
    ctx->st.ghost_partition_rows = h.ghost_partition_rows;
    ctx->pv_max_out = h.pv_max_out;
    ctx->pv_max_in = h.pv_max_in;
    ctx->pv_rows.clear();
    for (size_t r = 0; r < h.pv_flags.size(); ++r)
        if (h.pv_flags[r]) ctx->pv_rows.push_back(static_cast<int64_t>(r));
    ctx->st.device_bytes = ctx->dev_bytes;
    ctx->loaded = true;
    lap("scratch, ids");
    return TGO_OK;
}

// A partition's host graph onto the device (tgo_load_partition_layout, tgo_load_partition_rows).
int part_upload(tgo_ctx* ctx, HostGraph& h, int64_t n_global, int64_t lo) {
    free_graph(ctx);
    ctx->staging = RowStaging();
    int64_t max_in = 0;
    for (size_t r = 0; r + 1 < h.in.off.size(); ++r) max_in = std::max(max_in, h.in.off[r + 1] - h.in.off[r]);
    int rc = upload_graph(ctx, h, false);     // partitioned PageRank gathers global ids: plain CSR
    if (rc) return rc;
    ctx->g.partitioned = true;
    ctx->part_pr_world = 0;
    ctx->part_pr_plain = false;
    ctx->part_pr_hot = ctx->part_pr_span = 0;
    ctx->part_max_in_row = max_in;
    ctx->part_pr_job_row = ctx->part_pr_built_row = 0;
    ctx->part_pr_iter = ctx->part_pr_iters = 0;
    ctx->g.lo = lo;
    ctx->g.n_global = n_global;
    return TGO_OK;
}
// tgo_finish_partition_rows: the rows this rank staged with tgo_load_rows, decoded with the
// one-GPU rules (device decoder, or the host one under TGO_HOST_DECODE: key filter, ghosts,
// typed scopes, the cut in column order per row) into host vectors.  Vertex cuts fold on one GPU
// only; the partitioned programs read Integer weights.
int part_rows_take(tgo_ctx* ctx, RowStaging& st, std::string& err) {
    (void)hipSetDevice(ctx->opts.device);
    ctx->res_kind = -1;
    if (!ctx->staging.active) {          // no rows staged here: an empty range (the caller's scope agreed later)
        st = RowStaging();
        st.row_begin.push_back(0);
        return TGO_OK;
    }
    int rc = decode_staged_raw(ctx->staging, ctx->opts.partition_bits, ctx->opts.hard_query_limit, ctx->dec, ctx->stream,
                               err, false);
    ctx->dec.release();
    if (!rc) rc = staging_entries_to_host(ctx->staging, ctx->stream, err);
    st = std::move(ctx->staging);
    ctx->staging = RowStaging();
    if (rc) return rc;
    if (st.n_rep > 0 || std::any_of(st.vid.begin(), st.vid.end(), [](int64_t v) { return (v & 7) == 2; })) {
        err = "vertex cuts fold into their canonical vertex on a one-GPU load (VertexProgramScanJob.java:76-92)";
        return TGO_E_UNSUPPORTED;
    }
    if (st.opts.weight_key != 0 && st.plan.weight_dt != 0 && st.plan.weight_dt != TGO_DT_INTEGER) {
        err = "the partitioned programs read edge.<Integer>value(weight) (ShortestDistanceVertexProgram.java:53)";
        return TGO_E_UNSUPPORTED;
    }
    return TGO_OK;
}
void part_drop_staging(tgo_ctx* ctx) { ctx->staging = RowStaging(); ctx->dec.release(); }

}  // namespace tgo

extern "C" {

int tgo_decode_edge_entry(const tgo_schema* schema, const tgo_load_opts* opts, const uint8_t* entry,
                          int64_t len, int64_t value_pos, tgo_edge_entry* out) {
    if (!schema || !opts || !out) return TGO_E_INVALID;
    std::string err;
    return decode_one_entry(schema, opts, entry, len, value_pos, out, err);
}

int tgo_load_rows(tgo_ctx* ctx, const tgo_rows* rows, const tgo_schema* schema, const tgo_load_opts* opts) {
    if (!ctx) return TGO_E_INVALID;
    ctx->res_kind = -1;
    if (!rows || !schema || !opts) return fail(ctx, TGO_E_INVALID, "null argument");
    if (rows->nrows < 0 || (rows->nrows > 0 && (!rows->row_keys || !rows->row_entry_begin ||
        !rows->row_byte_begin || !rows->entry_bytes || !rows->entry_limit_valpos)))
        return fail(ctx, TGO_E_INVALID, "incomplete tgo_rows");
    if (opts->scope < 0 || opts->scope > 2) return fail(ctx, TGO_E_INVALID, "invalid scope");
    if (ctx->loaded && !ctx->staging.active) free_graph(ctx);
    (void)hipSetDevice(ctx->opts.device);
    const auto t0 = std::chrono::steady_clock::now();
    std::string err;
    // device decode (decode.hip) unless TGO_HOST_DECODE=1 picks the multi-threaded host decoder
    // (latched at the first batch of a load, so one load never mixes the two)
    if (!ctx->staging.active) ctx->host_decode = env_i64("TGO_HOST_DECODE", 0) != 0;
    int rc = ctx->host_decode ? decode_rows(ctx->staging, rows, schema, opts, ctx->opts.partition_bits,
                                       ctx->opts.hard_query_limit, threads_of(ctx), err)
                         : stage_rows_raw(ctx->staging, rows, schema, opts, ctx->dec, ctx->stream, err);
    ctx->st.load_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (rc) { ctx->staging = RowStaging(); return fail(ctx, rc, err); }
    return TGO_OK;
}

int tgo_finish_load(tgo_ctx* ctx) {
    Span load_span("load.finish_rows");
    TrimTemps trim_temps;   // the build temporaries are released when the load returns
    if (!ctx) return TGO_E_INVALID;
    if (!ctx->staging.active) return fail(ctx, TGO_E_STATE, "tgo_finish_load without tgo_load_rows");
    (void)hipSetDevice(ctx->opts.device);
    const auto t0 = std::chrono::steady_clock::now();
    HostGraph h;
    std::string err;
    // the staged work blocks, decoded in one device pass (decode.hip); the kept entries stay
    // on the device for the device assembly
    const bool dev_asm = !host_assembly();
    int rc = decode_staged_raw(ctx->staging, ctx->opts.partition_bits, ctx->opts.hard_query_limit, ctx->dec,
                               ctx->stream, err, dev_asm);
    ctx->dec.release();
    if (rc) { ctx->staging = RowStaging(); return fail(ctx, rc, err); }
    if (trace_on())
        std::fprintf(stderr, "[tgo] finish_load decode %8.1f ms\n",
                     std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    // CSR assembly on the device (assemble.hip) unless TGO_HOST_ASSEMBLY=1 or the scan holds
    // vertex cuts (their representative rows fold on the host, graph_build.cpp)
    const RowStaging& stg = ctx->staging;
    const bool cuts = stg.n_rep > 0 || std::any_of(stg.vid.begin(), stg.vid.end(), [](int64_t v) { return (v & 7) == 2; });
    const bool on_dev = dev_asm && !cuts;
    if (!on_dev) rc = staging_entries_to_host(ctx->staging, ctx->stream, err);
    // a wide (Long / Double) weight key: the staged values become the graph's value table (taken
    // before the assembly, which consumes the staging)
    std::vector<int64_t> wval = std::move(ctx->staging.wv);
    DevArray<int64_t> d_wval = std::move(ctx->staging.d_wv);
    if (!rc)
        rc = on_dev ? assemble_rows_device(ctx->staging, h, ctx->stream, err)
                    : assemble_from_rows(ctx->staging, h, threads_of(ctx), err);
    if (rc) { ctx->staging = RowStaging(); return fail(ctx, rc, err); }
    h.wval = std::move(wval);
    h.d_wval = std::move(d_wval);
    if (trace_on())
        std::fprintf(stderr, "[tgo] finish_load decode + assembly (%s) %8.1f ms\n", on_dev ? "device" : "host",
                     std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    free_graph(ctx);
    rc = upload_graph(ctx, h);
    ctx->st.load_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}

int tgo_load_edges(tgo_ctx* ctx, const tgo_edges* edges, const tgo_load_opts* opts) {
    Span load_span("load.edges");
    TrimTemps trim_temps;   // the build temporaries are released when the load returns
    if (!ctx) return TGO_E_INVALID;
    ctx->res_kind = -1;
    if (!edges || !opts || (edges->m > 0 && (!edges->src || !edges->dst)))
        return fail(ctx, TGO_E_INVALID, "null argument");
    if (opts->scope < 0 || opts->scope > 2) return fail(ctx, TGO_E_INVALID, "invalid scope");
    (void)hipSetDevice(ctx->opts.device);
    const auto t0 = std::chrono::steady_clock::now();
    HostGraph h;
    std::string err;
    // device assembly (assemble.hip) unless TGO_HOST_ASSEMBLY=1
    const bool on_dev = !host_assembly();
    int rc = on_dev ? assemble_edges_device(edges, opts, ctx->opts.hard_query_limit, h, ctx->stream, err)
                    : assemble_from_edges(edges, opts, ctx->opts.hard_query_limit, h, threads_of(ctx), err);
    if (rc) return fail(ctx, rc, err);
    if (trace_on())
        std::fprintf(stderr, "[tgo] load_edges assembly (%s) %8.1f ms\n", on_dev ? "device" : "host",
                     std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    free_graph(ctx);
    ctx->staging = RowStaging();
    rc = upload_graph(ctx, h);
    ctx->st.load_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}

int tgo_load_csr(tgo_ctx* ctx, int64_t n, const int64_t* titan_ids, const int64_t* out_off, const int32_t* out_idx,
                 const int32_t* out_w, const int64_t* in_off, const int32_t* in_idx, const int32_t* in_w,
                 const tgo_load_opts* opts) {
    if (!ctx) return TGO_E_INVALID;
    Span load_span("load.csr");
    TrimTemps trim_temps;   // the build temporaries are released when the load returns
    ctx->res_kind = -1;
    if (!opts || !out_off || !in_off) return fail(ctx, TGO_E_INVALID, "null argument");
    if (opts->scope < 0 || opts->scope > 2) return fail(ctx, TGO_E_INVALID, "invalid scope");
    if (opts->n_labels != 0) return fail(ctx, TGO_E_INVALID, "tgo_load_csr takes no label_ids (the rows are already sliced)");
    if (ctx->staging.active)            // a tgo_load_rows scan is in progress: finish (or destroy) it first
        return fail(ctx, TGO_E_STATE, "tgo_load_csr during a row load (tgo_load_rows without tgo_finish_load)");
    (void)hipSetDevice(ctx->opts.device);
    const auto t0 = std::chrono::steady_clock::now();
    // the rows as a staging of decoded rows (each row's OUT entries, then its IN entries), on
    // the device; then the row assembly of tgo_finish_load
    RowStaging st;
    st.active = true;
    st.opts = *opts;
    st.opts.label_ids = nullptr;
    const bool weighted = opts->weight_key != 0;
    const CsrInput in{n, titan_ids, {out_off, in_off}, {out_idx, in_idx}, {out_w, in_w}};
    std::string err;
    int rc = stage_csr_device(in, weighted, st, ctx->stream, err);
    if (rc) return fail(ctx, rc, err);
    HostGraph h;
    const bool on_dev = !host_assembly();
    if (!on_dev) rc = staging_entries_to_host(st, ctx->stream, err);
    if (!rc) rc = on_dev ? assemble_rows_device(st, h, ctx->stream, err) : assemble_from_rows(st, h, threads_of(ctx), err);
    if (rc) return fail(ctx, rc, err);
    free_graph(ctx);
    ctx->staging = RowStaging();
    rc = upload_graph(ctx, h);
    ctx->st.load_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}

// ------------------------------------------------------------------ 1-D partitioned (multi-GPU)
int tgo_part_layout(const tgo_edges* edges, int64_t n_global, int64_t lo, int64_t hi, int32_t threads,
                    int32_t* layout_local) {
    if (!edges || !layout_local || (edges->m > 0 && (!edges->src || !edges->dst))) return TGO_E_INVALID;
    std::string err;
    return partition_layout(edges, n_global, lo, hi, threads > 0 ? threads : 1, layout_local, err);
}

int tgo_load_partition(tgo_ctx* ctx, int64_t n_global, int64_t lo, int64_t hi, const tgo_edges* edges,
                       const tgo_load_opts* opts) {
    return tgo_load_partition_layout(ctx, n_global, lo, hi, edges, opts, nullptr);
}

int tgo_load_partition_layout(tgo_ctx* ctx, int64_t n_global, int64_t lo, int64_t hi, const tgo_edges* edges,
                              const tgo_load_opts* opts, const int32_t* layout_global) {
    if (!ctx) return TGO_E_INVALID;
    Span load_span("load.partition");
    TrimTemps trim_temps;   // the build temporaries are released when the load returns
    if (!edges || !opts || (edges->m > 0 && (!edges->src || !edges->dst))) return fail(ctx, TGO_E_INVALID, "null argument");
    if ((hi - lo) % 64 != 0) return fail(ctx, TGO_E_INVALID, "partition size must be a multiple of 64");
    (void)hipSetDevice(ctx->opts.device);
    const auto t0 = std::chrono::steady_clock::now();
    HostGraph h;
    std::string err;
    // device assembly (assemble.hip) unless TGO_HOST_ASSEMBLY=1
    const bool on_dev = !host_assembly();
    int rc = on_dev ? assemble_partition_device(edges, n_global, lo, hi, opts, ctx->opts.hard_query_limit, layout_global,
                                                h, ctx->stream, err)
                    : assemble_partition(edges, n_global, lo, hi, opts, ctx->opts.hard_query_limit, layout_global, h,
                                         threads_of(ctx), err);
    if (rc == TGO_OK && trace_on())
        std::fprintf(stderr, "[tgo] load_partition assembly (%s) %8.1f ms\n", on_dev ? "device" : "host",
                     std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    if (rc) return fail(ctx, rc, err);
    rc = tgo::part_upload(ctx, h, n_global, lo);
    ctx->st.load_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}

}  // extern "C"
