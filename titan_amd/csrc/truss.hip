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
// Support: tri_walk.hpp's enumeration with the credits going to edges.  The triangle a < b < c is
// found once, at the oriented entry (c, b), as a member a of fwd(c) ∩ fwd(b); both positions are
// known there, so the three edge ids are foff[c] + kb, foff[c] + position of a in fwd(c), foff[b] +
// position of a in fwd(b).  The first two are entries of row c: the block path counts them in LDS
// beside the staged row and flushes once per row (an atomic add: row c also receives (b, a)
// credits from higher rows); the third is one global 32-bit atomic per triangle.
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
#include "engine.hpp"
#include "tri_walk.hpp"

namespace tgo {
namespace {

// ---------------------------------------------------------------- lists
// erow[e] = c for every entry e of fwd(c): a lane per row, the wave for a row of 64 entries or more.
__global__ void __launch_bounds__(kBlock) truss_edge_rows(const int64_t* __restrict__ foff, int64_t n, int32_t* erow) {
    for_each_row_64(n, [&](int64_t v, bool live) {
        int64_t fb = 0, fl = 0;
        if (live) {
            fb = foff[v];
            fl = foff[v + 1] - fb;
        }
        lane_or_wave(fl >= 64, [&] {
            for (int64_t j = 0; j < fl; ++j) erow[fb + j] = static_cast<int32_t>(v);
        }, [&](int src) {
            const int64_t sb = __shfl(fb, src, 64), sl = __shfl(fl, src, 64);
            const int32_t sv = static_cast<int32_t>(v - lane() + src);
            for (int64_t j = lane(); j < sl; j += 64) erow[sb + j] = sv;
        });
    });
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
// Triangle credits to edges: sup[(c, b)], sup[(c, a)], sup[(b, a)] += 1 per triangle a < b < c.
struct EdgeCredit {
    int32_t* sup;
    __device__ __forceinline__ void other(int64_t e) const { atomicAdd(&sup[e], 1); }
    __device__ __forceinline__ void entry(int64_t cb, int64_t pos, int32_t, u64 m) const {
        atomicAdd(&sup[cb + pos], static_cast<int32_t>(m));
    }
    __device__ __forceinline__ void apex(int32_t, u64) const {}
};

// ---------------------------------------------------------------- peel
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
        lane_or_wave(has && al >= wave_row, [&] {
            for (int64_t j = 0; j < al; ++j) common(G, tr, o, e, ab, j, bb, bl, l, mn);
        }, [&](int src) {
            const int32_t se = __shfl(e, src, 64);
            const int64_t sab = __shfl(ab, src, 64), sal = __shfl(al, src, 64);
            const int64_t sbb = __shfl(bb, src, 64), sbl = __shfl(bl, src, 64);
            for (int64_t j = lane(); j < sal; j += 64) common(G, tr, o, se, sab, j, sbb, sbl, l, mn);
        });
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
    for_each_row_64(n, [&](int64_t v, bool live) {
        int64_t sb = 0, sl = 0;
        if (live) {
            sb = soff[v];
            sl = soff[v + 1] - sb;
        }
        int32_t mx = 0;
        lane_or_wave(sl >= 64, [&] {
            for (int64_t j = 0; j < sl; ++j) mx = max(mx, tr[seid[sb + j]]);
        }, [&](int src) {
            const int64_t rb = __shfl(sb, src, 64), rl = __shfl(sl, src, 64);
            u64 m = 0;
            for (int64_t j = lane(); j < rl; j += 64) m = max(m, static_cast<u64>(tr[seid[rb + j]]));
            m = wave_max(m);
            if (lane() == src) mx = static_cast<int32_t>(m);
        });
        if (live) vtruss[v] = mx;
    });
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
    at_top = wave_sum(at_top);
    ss = wave_sum(ss);
    mx = wave_max(mx);
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
    truss_edge_rows<<<grid_for(((n + 63) / 64) * 64, 1 << 20), kBlock, 0, s>>>(foff, n, erow);
    return hipGetLastError();
}
hipError_t k_truss_seid(const int64_t* soff, const int32_t* sadj, int64_t n, int64_t snnz, const int64_t* foff,
                        const int32_t* fadj, int32_t* seid, unsigned long long* err, hipStream_t s) {
    truss_seid<<<grid_for(snnz, 1 << 16), kBlock, 0, s>>>(soff, sadj, n, snnz, foff, fadj, seid, err);
    return hipGetLastError();
}
hipError_t k_truss_support(const int64_t* foff, const int32_t* fadj, int64_t n, int64_t wave_row, int64_t block_row,
                           int64_t max_fwd, int32_t* sup, int32_t* blist, int32_t* wlist, unsigned long long* q,
                           hipStream_t s) {
    return tri_walk(foff, fadj, n, wave_row, block_row, max_fwd, EdgeCredit{sup}, blist, wlist, q, s);
}
hipError_t k_truss_scan(const int32_t* list, int64_t len, const int32_t* sup, int32_t* tr, int32_t l, int32_t* queue,
                        int32_t* keep, Counters* cnt, hipStream_t s) {
    truss_scan<<<grid_for(len, 2048), kBlock, 0, s>>>(list, len, sup, tr, l, queue, keep, cnt);
    return hipGetLastError();
}
hipError_t k_truss_peel(const int32_t* cur, int64_t qlen, const TrussView& g, int32_t* sup, const int32_t* tr, int32_t l,
                        int64_t wave_row, int32_t* next, int64_t m, Counters* cnt, hipStream_t s) {
    const TrussLists G{g.foff, g.fadj, g.soff, g.sadj, g.seid, g.erow};
    truss_peel<<<grid_for(qlen, 2048), kBlock, 0, s>>>(cur, qlen, G, tr, l, wave_row, PeelOut{sup, next, m, cnt});
    return hipGetLastError();
}
hipError_t k_truss_settle(const int32_t* cur, int64_t qlen, int32_t value, const int32_t* next, int64_t nlen, int32_t* tr,
                          hipStream_t s) {
    truss_settle<<<grid_for(qlen + nlen, 2048), kBlock, 0, s>>>(cur, qlen, value, next, nlen, tr);
    return hipGetLastError();
}
hipError_t k_truss_clamp(int32_t* tr, int64_t m, int32_t value, hipStream_t s) {
    truss_clamp<<<grid_for(m, 2048), kBlock, 0, s>>>(tr, m, value);
    return hipGetLastError();
}
hipError_t k_truss_vertex(const int64_t* soff, const int32_t* seid, const int32_t* tr, int64_t n, int64_t* vtruss,
                          hipStream_t s) {
    truss_vertex<<<grid_for(((n + 63) / 64) * 64, 1 << 20), kBlock, 0, s>>>(soff, seid, tr, n, vtruss);
    return hipGetLastError();
}
hipError_t k_truss_totals(const int32_t* tr, const int32_t* sup0, int64_t m, int32_t top, unsigned long long* tot,
                          hipStream_t s) {
    truss_totals<<<grid_for(m, 2048), kBlock, 0, s>>>(tr, sup0, m, top, tot);
    return hipGetLastError();
}
hipError_t k_truss_edge_column(int which, const int32_t* erow, const int32_t* fadj, const int64_t* tid, const int32_t* tr,
                               const int32_t* sup0, int64_t m, int64_t* out, hipStream_t s) {
    truss_edge_column<<<grid_for(m, 2048), kBlock, 0, s>>>(which, erow, fadj, tid, tr, sup0, m, out);
    return hipGetLastError();
}

}  // namespace tgo
