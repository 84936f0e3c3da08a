// truss.hip — k-truss decomposition on gfx950 (tgo_ktruss).
//
// Contract: the simple undirected projection of a bothE load (tri.hip: u ~ v iff u != v and an OUT
// or IN entry of u names v).  support[e] = |N(u) ∩ N(v)| of the simple edge e = {u, v};
// truss[e] = the largest k such that e lies in a subgraph in which every edge is in at least
// k - 2 triangles of that subgraph (2 for an edge in no triangle).  The decomposition is unique.
//
// Edges: the id of a simple edge is its position in the forward lists (tri.hip) — entry j of
// fwd(c) is the edge {c, fadj[foff[c] + j]}, erow[e] = c.  seid, aligned with the sorted simple
// adjacency sadj (bc.hip), holds the edge id of every adjacency entry: fwd(v) is the sorted run of
// sadj(v)'s entries below v, so those ids are foff[v] + j; the id of an entry w > v is foff[w] +
// the position of v in fwd(w) (binary search).  Both are built once per load.
//
// Support: tri.hip's enumeration with the credits going to edges.  The triangle a < b < c is found
// once, at the oriented entry (c, b), as a member a of fwd(c) ∩ fwd(b); both positions are known
// there, so the three edge ids are foff[c] + kb, foff[c] + position of a in fwd(c), foff[b] +
// position of a in fwd(b).  The first two are entries of row c: the block path counts them in LDS
// beside the staged row and flushes once per row (an atomic add: row c also receives (b, a)
// credits from higher rows); the third is one global 32-bit atomic per triangle.  Row classes
// (lane, wave, block) and the ticket queues are tri.hip's.
//
// Peel (PKT): level l = 0, 1, ... gives truss l + 2.  sup[] (int32) is the working support,
// tr[] (int32) an edge's state: 0 alive, -1 in the current frontier, > 0 its final truss value.
// tr is only written between launches (truss_scan, truss_settle), so a peel launch reads a stable
// state.  A frontier edge e = {u, v} searches the shorter of sadj(u), sadj(v) into the longer; for
// a common w, with e1 = {u, w} and e2 = {v, w}: a final e1 or e2 means the triangle is gone;
// both in the frontier: nothing; neither: both are decremented; only one of them in the frontier:
// the other is decremented by the smaller of e and that one (once per triangle).  A decrement is
// old = atomicSub(&sup[t], 1):
//   old == l + 1   t drops to the level: it is appended to the next sub-round's queue, once
//   old <= l       t was at the level already: the decrement is undone (core.hip's clamp)
//   old >= l + 2   a real decrement; old - 1 feeds the minimum that names the next level
// The plain filter read before the atomic is safe for core.hip's reason: a value above l only
// falls during a level, a value at or below l stays there.
// No grid barrier, no spin, no loop that waits for another workgroup's write.  Wave = 64 lanes.
// All values are integers: the result does not depend on the thresholds or on the atomics' order.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <mutex>
#include "frontier.hpp"

namespace tgo {
namespace {

using u64 = unsigned long long;

inline int truss_grid(int64_t work, int64_t cap = 2048) {
    const int64_t g = (work + kBlock - 1) / kBlock;
    return static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(g, cap)));
}

__device__ __forceinline__ u64 wave_sum_u64(u64 x) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d, 64);
    return x;
}
__device__ __forceinline__ u64 wave_max_u64(u64 x) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) x = max(x, static_cast<u64>(__shfl_xor(x, d, 64)));
    return x;
}
__device__ __forceinline__ int wave_min_i32(int x) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) x = min(x, __shfl_xor(x, d, 64));
    return x;
}

// The position of x among the sorted p[0, len), -1 when it is not there.
template <class Ptr>
__device__ __forceinline__ int64_t find(Ptr p, int64_t len, int32_t x) {
    int64_t lo = 0, hi = len;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (p[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo < len && p[lo] == x ? lo : -1;
}

// The calling wave's lanes with `take` set append v to list (one atomicAdd on *count per wave).
__device__ __forceinline__ void wave_append(bool take, int32_t v, int32_t* list, u64* count) {
    const u64 qm = __ballot(take);
    if (!qm) return;
    const int lead = __ffsll(static_cast<long long>(qm)) - 1;
    u64 base = 0;
    if (lane() == lead) base = atomicAdd(count, static_cast<u64>(__popcll(qm)));
    base = __shfl(base, lead, 64);
    if (take) list[base + __popcll(qm & ((1ULL << lane()) - 1))] = v;
}

// ---------------------------------------------------------------- lists
// erow[e] = c for every entry e of fwd(c).  Rows go to lanes as in core_bwd_fill.
__global__ void __launch_bounds__(kBlock) truss_edge_rows(const int64_t* __restrict__ foff, int64_t n, int32_t* erow) {
    const int64_t words = (n + 63) >> 6;
    for (int64_t b = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock; b < words;
         b += static_cast<int64_t>(gridDim.x) * kWavesPerBlock) {
        const int64_t wd = b + (threadIdx.x >> 6);
        const int64_t v = (wd << 6) + lane();
        int64_t fb = 0, fl = 0;
        if (wd < words && v < n) {
            fb = foff[v];
            fl = foff[v + 1] - fb;
        }
        const bool wide = fl >= 64;
        if (!wide)
            for (int64_t j = 0; j < fl; ++j) erow[fb + j] = static_cast<int32_t>(v);
        u64 big = __ballot(wide);
        while (big) {
            const int src = __ffsll(static_cast<long long>(big)) - 1;
            big &= big - 1;
            const int64_t sb = __shfl(fb, src, 64), sl = __shfl(fl, src, 64);
            const int32_t sv = static_cast<int32_t>((wd << 6) + src);
            for (int64_t j = lane(); j < sl; j += 64) erow[sb + j] = sv;
        }
    }
}

// seid[p] = the edge id of adjacency entry p (one thread per entry; its row by binary search over
// soff).  An entry that the forward lists do not hold raises *err (the two lists disagree).
__global__ void __launch_bounds__(kBlock) truss_seid(const int64_t* __restrict__ soff, const int32_t* __restrict__ sadj,
                                                     int64_t n, int64_t snnz, const int64_t* __restrict__ foff,
                                                     const int32_t* __restrict__ fadj, int32_t* seid, u64* err) {
    for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < snnz; p += (int64_t)gridDim.x * blockDim.x) {
        int64_t lo = 0, hi = n;                 // the largest v with soff[v] <= p (soff[n] = snnz > p)
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) >> 1;
            if (soff[mid] <= p) lo = mid; else hi = mid - 1;
        }
        const int64_t v = lo;
        const int32_t w = sadj[p];
        int64_t id = -1;
        if (w < v) {
            const int64_t j = p - soff[v];
            if (j < foff[v + 1] - foff[v] && fadj[foff[v] + j] == w) id = foff[v] + j;
        } else if (w > v && w < n) {
            const int64_t fb = foff[w];
            const int64_t j = find(fadj + fb, foff[w + 1] - fb, static_cast<int32_t>(v));
            if (j >= 0) id = fb + j;
        }
        if (id < 0) {
            atomicMax(err, 1ULL);
            id = 0;
        }
        seid[p] = static_cast<int32_t>(id);
    }
}

// ---------------------------------------------------------------- support
// The matches of fwd(b) in row[0, kb) by the calling wave (row = fwd(c) in global memory or in LDS,
// cb = foff[c], b = row[kb]).  Credits: sup[(b, a)] += 1 per match; (c, a) += 1 per match and
// (c, b) += their number, in sup — or, with row_cnt (LDS counters beside a staged row, flushed by
// the caller), in row_cnt.
template <class Ptr>
__device__ __forceinline__ void support_entry(Ptr row, int64_t cb, int64_t kb, int32_t b, const int64_t* __restrict__ foff,
                                              const int32_t* __restrict__ fadj, int32_t* sup, unsigned* row_cnt = nullptr) {
    const int64_t bb = foff[b], lb = foff[b + 1] - bb;
    unsigned cnt = 0;
    for (int64_t k = lane(); k < lb; k += 64) {
        const int64_t pos = find(row, kb, fadj[bb + k]);
        if (pos >= 0) {
            atomicAdd(&sup[bb + k], 1);
            if (row_cnt) atomicAdd(&row_cnt[pos], 1u);
            else atomicAdd(&sup[cb + pos], 1);
            ++cnt;
        }
    }
    if (!__ballot(cnt != 0)) return;
    cnt = static_cast<unsigned>(wave_sum_u64(cnt));
    if (lane() == 0) {
        if (row_cnt) atomicAdd(&row_cnt[kb], cnt);
        else atomicAdd(&sup[cb + kb], static_cast<int32_t>(cnt));
    }
}

// Lane rows; wave rows are appended to wlist, block rows (block_row <= L <= lds_cap) to blist.
__global__ void __launch_bounds__(kBlock) truss_support(const int64_t* __restrict__ foff, const int32_t* __restrict__ fadj,
                                                        int64_t n, int64_t wave_row, int64_t block_row, int64_t lds_cap,
                                                        int32_t* sup, int32_t* blist, u64* bcount, int32_t* wlist, u64* wcount) {
    const int64_t words = (n + 63) >> 6;
    for (int64_t blk = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock; blk < words;
         blk += static_cast<int64_t>(gridDim.x) * kWavesPerBlock) {
        const int64_t wd = blk + (threadIdx.x >> 6);
        const int64_t c = (wd << 6) + lane();
        int64_t cb = 0, L = 0;
        if (wd < words && c < n) {
            cb = foff[c];
            L = foff[c + 1] - cb;
        }
        const bool to_block = L >= block_row && L <= lds_cap && L >= 2;
        const bool to_wave = !to_block && L >= wave_row && L >= 2;
        if (!to_block && !to_wave && L >= 2) {
            for (int64_t kb = 1; kb < L; ++kb) {
                const int32_t b = fadj[cb + kb];
                const int64_t bb = foff[b], lb = foff[b + 1] - bb;
                if (lb == 0) continue;
                int64_t i = 0, j = 0;
                int32_t x = fadj[cb], y = fadj[bb];
                int32_t cnt = 0;
                for (;;) {
                    if (x == y) {
                        atomicAdd(&sup[cb + i], 1);
                        atomicAdd(&sup[bb + j], 1);
                        ++cnt;
                    }
                    const bool ai = x <= y, aj = y <= x;
                    if (ai) { if (++i >= kb) break; x = fadj[cb + i]; }
                    if (aj) { if (++j >= lb) break; y = fadj[bb + j]; }
                }
                if (cnt) atomicAdd(&sup[cb + kb], cnt);
            }
        }
        wave_append(to_wave, static_cast<int32_t>(c), wlist, wcount);
        wave_append(to_block, static_cast<int32_t>(c), blist, bcount);
    }
}

// The queued wave rows, one row per wave and ticket.
__global__ void __launch_bounds__(kBlock) truss_support_wave(const int64_t* __restrict__ foff, const int32_t* __restrict__ fadj,
                                                             const int32_t* __restrict__ wlist, const u64* __restrict__ wcount,
                                                             u64* ticket, int32_t* sup) {
    const u64 rows = *wcount;
    for (;;) {
        u64 r = 0;
        if (lane() == 0) r = atomicAdd(ticket, 1ULL);
        r = __shfl(r, 0, 64);
        if (r >= rows) return;
        const int32_t c = wlist[r];
        const int64_t cb = foff[c];
        const int32_t* const row = fadj + cb;
        const int64_t L = foff[c + 1] - cb;
        for (int64_t kb = 1; kb < L; ++kb) support_entry(row, cb, kb, row[kb], foff, fadj, sup);
    }
}

// The queued block rows: fwd(c) staged in LDS with one 32-bit counter per entry (tri_count_block).
__global__ void __launch_bounds__(kBlock) truss_support_block(const int64_t* __restrict__ foff, const int32_t* __restrict__ fadj,
                                                              const int32_t* __restrict__ blist, const u64* __restrict__ bcount,
                                                              u64* ticket, int64_t lds_cap, int32_t* sup) {
    extern __shared__ int32_t s_row[];
    unsigned* const s_cnt = reinterpret_cast<unsigned*>(s_row + lds_cap);
    __shared__ u64 s_ticket;
    const u64 rows = *bcount;
    for (;;) {
        if (threadIdx.x == 0) s_ticket = atomicAdd(ticket, 1ULL);
        __syncthreads();
        const u64 r = s_ticket;                                 // (rewritten only after the barrier that ends the row)
        if (r >= rows) return;
        const int32_t c = blist[r];
        const int64_t cb = foff[c];
        const int64_t L = min(foff[c + 1] - cb, lds_cap);       // == the row's length: truss_support queued it
        for (int64_t k = threadIdx.x; k < L; k += kBlock) {
            s_row[k] = fadj[cb + k];
            s_cnt[k] = 0;
        }
        __syncthreads();
        for (int64_t kb = 1 + (threadIdx.x >> 6); kb < L; kb += kWavesPerBlock)
            support_entry(s_row, cb, kb, s_row[kb], foff, fadj, sup, s_cnt);
        __syncthreads();
        for (int64_t k = threadIdx.x; k < L; k += kBlock)
            if (const unsigned m = s_cnt[k]) atomicAdd(&sup[cb + k], static_cast<int32_t>(m));
        __syncthreads();
    }
}

// dynamic LDS past 64 KB, raised once (tri.hip tri_big_lds)
hipError_t truss_big_lds(size_t lds) {
    static std::mutex mu;
    static size_t raised = 0;
    std::lock_guard<std::mutex> lk(mu);
    if (lds <= raised) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&truss_support_block),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
    if (e == hipSuccess) raised = lds;
    return e;
}

// ---------------------------------------------------------------- peel
// The smallest support above l as max(INT32_MAX - support): the counters are zeroed between rounds.
__device__ __forceinline__ void publish_min(int mn, u64* word) {
    mn = wave_min_i32(mn);
    if (lane() == 0 && mn != INT_MAX) atomicMax(word, static_cast<u64>(INT_MAX - mn));
}

// Level l's scan of the alive list (list == nullptr: every edge): an alive edge whose support reads
// <= l is queued and marked as frontier; one above l feeds the minimum and, with `keep`, goes to the
// rebuilt alive list.  queue == nullptr: nothing is queued or marked (the first scan's minimum).
__global__ void __launch_bounds__(kBlock) truss_scan(const int32_t* __restrict__ list, int64_t len, const int32_t* sup,
                                                     int32_t* tr, int32_t l, int32_t* queue, int32_t* keep, Counters* cnt) {
    int mn = INT_MAX;
    const int64_t span = ((len + 63) >> 6) << 6;            // whole waves: wave_append's ballots
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < span; i += (int64_t)gridDim.x * blockDim.x) {
        const bool in = i < len;
        const int32_t e = in ? (list ? list[i] : static_cast<int32_t>(i)) : 0;
        const bool alive = in && tr[e] == 0;
        const int32_t s = alive ? __hip_atomic_load(&sup[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : INT_MAX;
        const bool take = alive && queue && s <= l;
        const bool stay = alive && !take;
        if (stay) mn = min(mn, s);
        if (take) tr[e] = -1;
        if (queue) wave_append(take, e, queue, &cnt->qlen);
        if (keep) wave_append(stay, e, keep, &cnt->mf);
    }
    publish_min(mn, &cnt->red[0]);
}

struct TrussLists {
    const int64_t* foff; const int32_t* fadj;
    const int64_t* soff; const int32_t* sadj;
    const int32_t* seid; const int32_t* erow;
};

struct PeelOut {
    int32_t* sup; int32_t* next; int64_t m; Counters* cnt;
};

// One decrement of an alive edge t outside the frontier at level l.
__device__ __forceinline__ void lower(const PeelOut& o, int32_t t, int32_t l, int& mn) {
    if (o.sup[t] <= l) return;              // a plain read: any older value is safe (head of this file)
    const int32_t old = atomicSub(&o.sup[t], 1);
    if (old == l + 1) {
        const u64 g = atomicAdd(&o.cnt->qlen, 1ULL);
        if (g < static_cast<u64>(o.m)) o.next[g] = t;       // an edge drops once per run: m entries hold them
        else atomicMax(&o.cnt->err, 1ULL);
    } else if (old <= l) {
        atomicAdd(&o.sup[t], 1);
    } else {
        mn = min(mn, old - 1);
    }
}

// Entry j of the shorter row (at ab) of frontier edge e against the longer row (at bb, bl entries).
__device__ __forceinline__ void common(const TrussLists& G, const int32_t* __restrict__ tr, const PeelOut& o, int32_t e,
                                       int64_t ab, int64_t j, int64_t bb, int64_t bl, int32_t l, int& mn) {
    const int64_t pos = find(G.sadj + bb, bl, G.sadj[ab + j]);
    if (pos < 0) return;
    const int32_t e1 = G.seid[ab + j], e2 = G.seid[bb + pos];
    const int32_t t1 = tr[e1], t2 = tr[e2];
    if (t1 > 0 || t2 > 0) return;           // the triangle went with an earlier sub-round
    const bool c1 = t1 < 0, c2 = t2 < 0;
    if (c1 && c2) return;
    if (!c1 && !c2) {
        lower(o, e1, l, mn);
        lower(o, e2, l, mn);
    } else if (c1) {
        if (e < e1) lower(o, e2, l, mn);
    } else {
        if (e < e2) lower(o, e1, l, mn);
    }
}

// One sub-round of level l: every edge of cur, a lane each; an edge whose shorter endpoint row has
// at least wave_row entries by the whole wave.  The drops go to next (cnt->qlen).
__global__ void __launch_bounds__(kBlock) truss_peel(const int32_t* __restrict__ cur, int64_t qlen, TrussLists G,
                                                     const int32_t* __restrict__ tr, int32_t l, int64_t wave_row, PeelOut o) {
    int mn = INT_MAX;
    for (int64_t base = static_cast<int64_t>(blockIdx.x) * kBlock; base < qlen; base += static_cast<int64_t>(gridDim.x) * kBlock) {
        const int64_t i = base + threadIdx.x;
        const bool has = i < qlen;
        int32_t e = 0;
        int64_t ab = 0, al = 0, bb = 0, bl = 0;
        if (has) {
            e = cur[i];
            const int32_t u = G.erow[e], v = G.fadj[e];
            ab = G.soff[u]; al = G.soff[u + 1] - ab;
            bb = G.soff[v]; bl = G.soff[v + 1] - bb;
            if (bl < al) {
                int64_t t = ab; ab = bb; bb = t;
                t = al; al = bl; bl = t;
            }
        }
        const bool wide = has && al >= wave_row;
        if (has && !wide)
            for (int64_t j = 0; j < al; ++j) common(G, tr, o, e, ab, j, bb, bl, l, mn);
        u64 big = __ballot(wide);
        while (big) {
            const int src = __ffsll(static_cast<long long>(big)) - 1;
            big &= big - 1;
            const int32_t se = __shfl(e, src, 64);
            const int64_t sab = __shfl(ab, src, 64), sal = __shfl(al, src, 64);
            const int64_t sbb = __shfl(bb, src, 64), sbl = __shfl(bl, src, 64);
            for (int64_t j = lane(); j < sal; j += 64) common(G, tr, o, se, sab, j, sbb, sbl, l, mn);
        }
    }
    publish_min(mn, &o.cnt->red[0]);
}

// After a sub-round: its edges are final at `value`, the next queue's edges are the frontier.
__global__ void __launch_bounds__(kBlock) truss_settle(const int32_t* __restrict__ cur, int64_t qlen, int32_t value,
                                                       const int32_t* __restrict__ next, int64_t nlen, int32_t* tr) {
    const int64_t all = qlen + nlen;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < all; i += (int64_t)gridDim.x * blockDim.x) {
        if (i < qlen) tr[cur[i]] = value;
        else tr[next[i - qlen]] = -1;
    }
}

// Every edge still alive gets `value` (the clamp of a run with k set).
__global__ void __launch_bounds__(kBlock) truss_clamp(int32_t* tr, int64_t m, int32_t value) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < m; e += (int64_t)gridDim.x * blockDim.x)
        if (tr[e] == 0) tr[e] = value;
}

// ---------------------------------------------------------------- finish
// vtruss[v] = the largest truss value over v's adjacency entries (0 without one): a lane per row,
// the wave for a row of 64 entries or more.
__global__ void __launch_bounds__(kBlock) truss_vertex(const int64_t* __restrict__ soff, const int32_t* __restrict__ seid,
                                                       const int32_t* __restrict__ tr, int64_t n, int64_t* vtruss) {
    const int64_t words = (n + 63) >> 6;
    for (int64_t b = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock; b < words;
         b += static_cast<int64_t>(gridDim.x) * kWavesPerBlock) {
        const int64_t wd = b + (threadIdx.x >> 6);
        const int64_t v = (wd << 6) + lane();
        const bool live = wd < words && v < n;
        int64_t sb = 0, sl = 0;
        if (live) {
            sb = soff[v];
            sl = soff[v + 1] - sb;
        }
        const bool wide = sl >= 64;
        int32_t mx = 0;
        if (!wide)
            for (int64_t j = 0; j < sl; ++j) mx = max(mx, tr[seid[sb + j]]);
        u64 big = __ballot(wide);
        while (big) {
            const int src = __ffsll(static_cast<long long>(big)) - 1;
            big &= big - 1;
            const int64_t rb = __shfl(sb, src, 64), rl = __shfl(sl, src, 64);
            u64 m = 0;
            for (int64_t j = lane(); j < rl; j += 64) m = max(m, static_cast<u64>(tr[seid[rb + j]]));
            m = wave_max_u64(m);
            if (lane() == src) mx = static_cast<int32_t>(m);
        }
        if (live) vtruss[v] = mx;
    }
}

// tot[0] += edges with truss == top, tot[1] = max truss, tot[2] += sum of the initial supports.
__global__ void __launch_bounds__(kBlock) truss_totals(const int32_t* __restrict__ tr, const int32_t* __restrict__ sup0,
                                                       int64_t m, int32_t top, u64* tot) {
    u64 at_top = 0, mx = 0, ss = 0;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < m; e += (int64_t)gridDim.x * blockDim.x) {
        const int32_t t = tr[e];
        at_top += t == top;
        mx = max(mx, static_cast<u64>(max(t, 0)));
        ss += static_cast<u64>(sup0[e]);
    }
    at_top = wave_sum_u64(at_top);
    ss = wave_sum_u64(ss);
    mx = wave_max_u64(mx);
    if (lane() == 0) {
        if (at_top) atomicAdd(&tot[0], at_top);
        if (mx) atomicMax(&tot[1], mx);
        if (ss) atomicAdd(&tot[2], ss);
    }
}

// One column of the edge result: 0 / 1 the smaller / larger Titan id of the endpoints, 2 the truss
// value, 3 the initial support.
__global__ void __launch_bounds__(kBlock) truss_edge_column(int which, const int32_t* __restrict__ erow,
                                                            const int32_t* __restrict__ fadj, const int64_t* __restrict__ tid,
                                                            const int32_t* __restrict__ tr, const int32_t* __restrict__ sup0,
                                                            int64_t m, int64_t* out) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < m; e += (int64_t)gridDim.x * blockDim.x) {
        int64_t x;
        if (which <= 1) {
            const int64_t a = tid[erow[e]], b = tid[fadj[e]];
            x = which == 0 ? min(a, b) : max(a, b);
        } else {
            x = which == 2 ? tr[e] : sup0[e];
        }
        out[e] = x;
    }
}

}  // namespace

// ---------------------------------------------------------------- launchers
hipError_t k_truss_edge_rows(const int64_t* foff, int64_t n, int32_t* erow, hipStream_t s) {
    truss_edge_rows<<<truss_grid(((n + 63) / 64) * 64, 1 << 20), kBlock, 0, s>>>(foff, n, erow);
    return hipGetLastError();
}
hipError_t k_truss_seid(const int64_t* soff, const int32_t* sadj, int64_t n, int64_t snnz, const int64_t* foff,
                        const int32_t* fadj, int32_t* seid, unsigned long long* err, hipStream_t s) {
    truss_seid<<<truss_grid(snnz, 1 << 16), kBlock, 0, s>>>(soff, sadj, n, snnz, foff, fadj, seid, err);
    return hipGetLastError();
}
hipError_t k_truss_support(const int64_t* foff, const int32_t* fadj, int64_t n, int64_t wave_row, int64_t block_row,
                           int64_t max_fwd, int32_t* sup, int32_t* blist, int32_t* wlist, unsigned long long* q,
                           hipStream_t s) {
    // LDS entries of the block kernel: the longest row, at most kTriLdsEntries
    const int64_t cap = std::max<int64_t>(64, std::min<int64_t>(max_fwd, kTriLdsEntries));
    truss_support<<<truss_grid(((n + 63) / 64) * 64, 1 << 20), kBlock, 0, s>>>(foff, fadj, n, wave_row, block_row, cap, sup,
                                                                              blist, &q[0], wlist, &q[1]);
    hipError_t e = hipGetLastError();
    const int blocks = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>((n + 63) / 64, 2048)));
    if (e == hipSuccess && block_row <= max_fwd) {              // else no row was queued
        const size_t lds = static_cast<size_t>(cap) * (sizeof(int32_t) + sizeof(unsigned));
        if (lds > 64 * 1024 && (e = truss_big_lds(lds)) != hipSuccess) return e;
        truss_support_block<<<blocks, kBlock, lds, s>>>(foff, fadj, blist, &q[0], &q[2], cap, sup);
        e = hipGetLastError();
    }
    if (e == hipSuccess && wave_row <= max_fwd) {
        truss_support_wave<<<blocks, kBlock, 0, s>>>(foff, fadj, wlist, &q[1], &q[3], sup);
        e = hipGetLastError();
    }
    return e;
}
hipError_t k_truss_scan(const int32_t* list, int64_t len, const int32_t* sup, int32_t* tr, int32_t l, int32_t* queue,
                        int32_t* keep, Counters* cnt, hipStream_t s) {
    truss_scan<<<truss_grid(len), kBlock, 0, s>>>(list, len, sup, tr, l, queue, keep, cnt);
    return hipGetLastError();
}
hipError_t k_truss_peel(const int32_t* cur, int64_t qlen, const TrussView& g, int32_t* sup, const int32_t* tr, int32_t l,
                        int64_t wave_row, int32_t* next, int64_t m, Counters* cnt, hipStream_t s) {
    const TrussLists G{g.foff, g.fadj, g.soff, g.sadj, g.seid, g.erow};
    truss_peel<<<truss_grid(qlen), kBlock, 0, s>>>(cur, qlen, G, tr, l, wave_row, PeelOut{sup, next, m, cnt});
    return hipGetLastError();
}
hipError_t k_truss_settle(const int32_t* cur, int64_t qlen, int32_t value, const int32_t* next, int64_t nlen, int32_t* tr,
                          hipStream_t s) {
    truss_settle<<<truss_grid(qlen + nlen), kBlock, 0, s>>>(cur, qlen, value, next, nlen, tr);
    return hipGetLastError();
}
hipError_t k_truss_clamp(int32_t* tr, int64_t m, int32_t value, hipStream_t s) {
    truss_clamp<<<truss_grid(m), kBlock, 0, s>>>(tr, m, value);
    return hipGetLastError();
}
hipError_t k_truss_vertex(const int64_t* soff, const int32_t* seid, const int32_t* tr, int64_t n, int64_t* vtruss,
                          hipStream_t s) {
    truss_vertex<<<truss_grid(((n + 63) / 64) * 64, 1 << 20), kBlock, 0, s>>>(soff, seid, tr, n, vtruss);
    return hipGetLastError();
}
hipError_t k_truss_totals(const int32_t* tr, const int32_t* sup0, int64_t m, int32_t top, unsigned long long* tot,
                          hipStream_t s) {
    truss_totals<<<truss_grid(m), kBlock, 0, s>>>(tr, sup0, m, top, tot);
    return hipGetLastError();
}
hipError_t k_truss_edge_column(int which, const int32_t* erow, const int32_t* fadj, const int64_t* tid, const int32_t* tr,
                               const int32_t* sup0, int64_t m, int64_t* out, hipStream_t s) {
    truss_edge_column<<<truss_grid(m), kBlock, 0, s>>>(which, erow, fadj, tid, tr, sup0, m, out);
    return hipGetLastError();
}

}  // namespace tgo
