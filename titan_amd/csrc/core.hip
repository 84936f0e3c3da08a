// core.hip — k-core decomposition on gfx950 (tgo_kcore).
//
// Contract: the simple undirected projection of a bothE load (tri.hip: u ~ v iff u != v and an OUT
// or IN entry of u names v).  core[v] = the largest k such that v lies in a subgraph in which every
// vertex has at least k neighbours.  The decomposition is unique.
//
// Neighbourhoods: N(v) = fwd(v) + bwd(v).  fwd(v) (tri.hip) = the distinct neighbours u < v in
// internal ids, one entry per simple edge; bwd(v) = the neighbours u > v, the transpose of fwd,
// built once per load by count / scan / fill with an atomic cursor (the order inside a backward
// row is not used).  The two rows are disjoint and free of duplicates and loops, so one walk of
// both rows visits every neighbour exactly once: no dedup per decrement.
//
// Peel: deg[] (int32) starts as d(v) and ENDS as core[v].  Level k peels every vertex whose
// degree reads k; walking a peeled vertex's rows, a neighbour u whose degree reads > k gets
// old = atomicSub(&deg[u], 1):
//   old == k + 1   u drops to k: u joins this level (queued once: see below)
//   old <= k       u was at this level (or an earlier one) already: the decrement is undone
//   old >= k + 2   a real decrement; old - 1 feeds the minimum that names the next level
// Why the stale filter read is harmless: a word's value above k only ever falls (undo pairs
// happen at values <= k, which stay <= k for the rest of the level), so a filter read that is too
// old is too HIGH, or it is a transient of an undo pair and <= k like the settled value.  Too
// high: the atomic decides on the word's true value and the undo repairs it.  <= k: the skip is
// what the true value asks for.  After the first old == k + 1 the word never exceeds k again in
// this level, so exactly one lane sees k + 1 and u is queued once.  A vertex peeled at level j
// ends every later level with deg == j: each undo pair restores it.
//
// A workgroup keeps peeling what it dropped itself: drops go to an LDS queue (two buffers, one
// being drained while the other fills), and only what does not fit spills to the global next
// queue, which the next launch of the level takes.  No grid barrier, no spin, no loop that waits
// for another workgroup's write.  core_tail: one workgroup runs every remaining level in one
// launch once few vertices are left (the innermost cores of a power-law graph are thousands of
// levels of a handful of vertices).  Wave = 64 lanes.  Rows go to lanes as in tri.hip: a row with
// fewer than wave_row entries is walked by its own lane, a longer one by the whole wave.
#include <hip/hip_runtime.h>
#include "engine.hpp"
#include "wave.hpp"

namespace tgo {
namespace {

// deg[] as the memory holds it (agent scope: not a line of this CU's L1): core_scan / core_tail
// read a vertex's word again after other launches or levels changed it, and must not see a peeled
// vertex as alive.  The peel's own filter read is a plain load: it is correct with any older value
// (see the head of this file), and the fresh read measured 2 - 3 % slower.
__device__ __forceinline__ int32_t deg_now(const int32_t* deg, int64_t v) {
    return __hip_atomic_load(&deg[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------- backward lists
// bcnt[u] += 1 per forward entry (v, u): |bwd(u)|.  bcnt is zero before (n + 1 words).
__global__ void __launch_bounds__(kBlock) core_bwd_count(const int32_t* __restrict__ fadj, int64_t fnnz, u64* bcnt) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < fnnz; e += (int64_t)gridDim.x * blockDim.x)
        atomicAdd(&bcnt[fadj[e]], 1ULL);
}

// badj[cursor[u]++] = v for every forward entry (v, u); cursor starts as a copy of boff.  Rows go
// to lanes as above: 64 consecutive rows a wave, a row of 64 entries or more by the whole wave.
__global__ void __launch_bounds__(kBlock) core_bwd_fill(const int64_t* __restrict__ foff, const int32_t* __restrict__ fadj,
                                                        int64_t n, u64* cursor, int32_t* badj) {
    for_each_row_64(n, [&](int64_t v, bool live) {
        int64_t fb = 0, fl = 0;
        if (live) {
            fb = foff[v];
            fl = foff[v + 1] - fb;
        }
        lane_or_wave(fl >= 64, [&] {
            for (int64_t j = 0; j < fl; ++j) badj[atomicAdd(&cursor[fadj[fb + j]], 1ULL)] = static_cast<int32_t>(v);
        }, [&](int src) {
            const int64_t sb = __shfl(fb, src, 64), sl = __shfl(fl, src, 64);
            const int32_t sv = static_cast<int32_t>(v - lane() + src);
            for (int64_t j = lane(); j < sl; j += 64) badj[atomicAdd(&cursor[fadj[sb + j]], 1ULL)] = sv;
        });
    });
}

__global__ void core_deg_init(const int64_t* __restrict__ d, int64_t n, int32_t* deg) {
    for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < n; v += (int64_t)gridDim.x * blockDim.x)
        deg[v] = static_cast<int32_t>(d[v]);
}

// ---------------------------------------------------------------- peel
using CoreLists = CoreView;

// One neighbour of a vertex peeled at level k.  Returns true when u drops to k here (the caller
// queues it); mn: the smallest degree > k a decrement of this lane left behind.
__device__ __forceinline__ bool visit(int32_t* deg, int32_t u, int32_t k, int& mn) {
    if (deg[u] <= k) return false;         // a plain read: any older value is safe (head of this file)
    const int32_t old = atomicSub(&deg[u], 1);
    if (old == k + 1) return true;
    if (old <= k) atomicAdd(&deg[u], 1);
    else mn = min(mn, old - 1);
    return false;
}

// The calling wave walks N(v) of its lanes' vertices (has: the lane holds one).  Every lane of the
// wave calls this together.  drop(u): u joined level k.
template <class Drop>
__device__ __forceinline__ void peel_rows(bool has, int32_t v, const CoreLists& L, int32_t* deg, int32_t k,
                                          int64_t wave_row, int& mn, Drop&& drop) {
    int64_t fb = 0, fl = 0, bb = 0, bl = 0;
    if (has) {
        fb = L.foff[v]; fl = L.foff[v + 1] - fb;
        bb = L.boff[v]; bl = L.boff[v + 1] - bb;
    }
    lane_or_wave(has && fl + bl >= wave_row, [&] {
        for (int64_t j = 0; j < fl; ++j) { const int32_t u = L.fadj[fb + j]; if (visit(deg, u, k, mn)) drop(u); }
        for (int64_t j = 0; j < bl; ++j) { const int32_t u = L.badj[bb + j]; if (visit(deg, u, k, mn)) drop(u); }
    }, [&](int src) {
        const int64_t sfb = __shfl(fb, src, 64), sfl = __shfl(fl, src, 64);
        const int64_t sbb = __shfl(bb, src, 64), sbl = __shfl(bl, src, 64);
        for (int64_t j = lane(); j < sfl; j += 64) { const int32_t u = L.fadj[sfb + j]; if (visit(deg, u, k, mn)) drop(u); }
        for (int64_t j = lane(); j < sbl; j += 64) { const int32_t u = L.badj[sbb + j]; if (visit(deg, u, k, mn)) drop(u); }
    });
}

// The workgroup's LDS queue: two buffers of kCoreQueue entries; count[b] may run past the
// capacity in use (the entries beyond it went elsewhere), readers clamp it.
struct LdsQueue {
    int32_t q[2][kCoreQueue];
    unsigned count[2];
};

// Drain the workgroup's LDS queue, starting at buffer 0: the drops of one buffer's vertices fill
// the other, until a buffer stays empty.  Every thread of the block calls this after a barrier;
// on return both counts are zero and a barrier has passed.  Returns the vertices drained.
template <class Spill>
__device__ __forceinline__ unsigned drain(LdsQueue& s, unsigned cap, const CoreLists& L, int32_t* deg, int32_t k,
                                          int64_t wave_row, int& mn, Spill&& spill) {
    unsigned drained = 0;
    for (int b = 0;; b ^= 1) {
        const unsigned c = min(s.count[b], cap);
        __syncthreads();                        // every thread has read the count before it changes
        if (!c) return drained;
        drained += c;
        for (unsigned base = 0; base < c; base += kBlock) {
            const unsigned i = base + threadIdx.x;
            const bool has = i < c;
            peel_rows(has, has ? s.q[b][i] : 0, L, deg, k, wave_row, mn, [&](int32_t u) {
                const unsigned slot = atomicAdd(&s.count[b ^ 1], 1u);
                if (slot < cap) s.q[b ^ 1][slot] = u;
                else spill(u);
            });
        }
        __syncthreads();
        if (threadIdx.x == 0) s.count[b] = 0;
        __syncthreads();
    }
}

// Level k's scan of the alive list (list == nullptr: every vertex): a vertex whose degree reads k
// is queued; one above k is still alive — its degree feeds the minimum and, with `keep`, it goes
// to the rebuilt alive list; one below k was peeled at an earlier level.  queue == nullptr: nothing
// is queued or counted (the first scan's minimum, the compaction before the tail).
__global__ void __launch_bounds__(kBlock) core_scan(const int32_t* __restrict__ list, int64_t len, const int32_t* deg,
                                                    int32_t k, int32_t* queue, int32_t* keep, Counters* cnt) {
    int mn = INT_MAX;
    const int64_t span = ((len + 63) >> 6) << 6;            // whole waves: wave_append's ballots
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < span; i += (int64_t)gridDim.x * blockDim.x) {
        const bool in = i < len;
        const int32_t v = in ? (list ? list[i] : static_cast<int32_t>(i)) : 0;
        const int32_t d = in ? deg_now(deg, v) : INT_MIN;
        if (in && d > k) mn = min(mn, d);
        if (queue) wave_append(in && d == k, v, queue, &cnt->qlen);
        if (keep) wave_append(in && d > k, v, keep, &cnt->mf);
    }
    publish_min(mn, &cnt->red[0]);
}

// One launch of level k: the vertices of cur are peeled, and whatever their workgroup drops it
// peels itself from its LDS queue; the drops beyond lds_cap go to next (cnt->qlen).  cnt->mf +=
// every drop, queued or peeled here.  A vertex is dropped at most once per run, so next
// (n entries) cannot overflow; the guard is for a broken invariant and raises cnt->err.
__global__ void __launch_bounds__(kBlock) core_peel(const int32_t* __restrict__ cur, int64_t qlen, CoreLists L, int32_t* deg,
                                                    int32_t k, int64_t wave_row, unsigned lds_cap, int32_t* next,
                                                    int64_t n, Counters* cnt) {
    __shared__ LdsQueue s;
    if (threadIdx.x == 0) s.count[0] = s.count[1] = 0;
    __syncthreads();
    int mn = INT_MAX;
    u64 spilled = 0, drained = 0;
    auto spill = [&](int32_t u) {
        const u64 g = atomicAdd(&cnt->qlen, 1ULL);
        if (g < static_cast<u64>(n)) next[g] = u;
        else atomicMax(&cnt->err, 1ULL);
        ++spilled;
    };
    for (int64_t base = static_cast<int64_t>(blockIdx.x) * kBlock; base < qlen; base += static_cast<int64_t>(gridDim.x) * kBlock) {
        const int64_t i = base + threadIdx.x;
        const bool has = i < qlen;
        peel_rows(has, has ? cur[i] : 0, L, deg, k, wave_row, mn, [&](int32_t u) {
            const unsigned slot = atomicAdd(&s.count[0], 1u);
            if (slot < lds_cap) s.q[0][slot] = u;
            else spill(u);
        });
        __syncthreads();
        drained += drain(s, lds_cap, L, deg, k, wave_row, mn, spill);
    }
    publish_min(mn, &cnt->red[0]);
    // drops = the spills (per lane) + what the workgroup drained (the same count on every thread)
    spilled = wave_sum(spilled);
    if (lane() == 0 && spilled) atomicAdd(&cnt->mf, spilled);
    if (threadIdx.x == 0 && drained) atomicAdd(&cnt->mf, drained);
}

// Every remaining level in one launch by one workgroup: the alive vertices are those of list
// (list == nullptr: every vertex) whose degree is above k_prev, at most kCoreQueue of them, so the
// LDS queue holds a whole level and nothing spills.  Out: cnt->qlen = levels run here,
// cnt->mf = vertices of the last one, cnt->red[0] = its k, cnt->red[1] = barrier-separated steps.
__global__ void __launch_bounds__(kBlock) core_tail(const int32_t* __restrict__ list, int64_t len, CoreLists L, int32_t* deg,
                                                    int32_t k_prev, int64_t wave_row, Counters* cnt) {
    __shared__ LdsQueue s;
    __shared__ int s_min;
    int32_t k = k_prev;
    u64 levels = 0, last = 0, steps = 0;
    int unused = INT_MAX;
    if (threadIdx.x == 0) s.count[0] = s.count[1] = 0;
    for (;;) {
        if (threadIdx.x == 0) s_min = INT_MAX;
        __syncthreads();
        int mn = INT_MAX;
        for (int64_t i = threadIdx.x; i < len; i += kBlock) {
            const int32_t d = deg_now(deg, list ? list[i] : static_cast<int32_t>(i));
            if (d > k) mn = min(mn, d);
        }
        mn = wave_min(mn);
        if (lane() == 0 && mn != INT_MAX) atomicMin(&s_min, mn);
        __syncthreads();
        const int m = s_min;
        if (m == INT_MAX) break;
        k = m;
        ++levels;
        for (int64_t i = threadIdx.x; i < len; i += kBlock) {
            const int32_t v = list ? list[i] : static_cast<int32_t>(i);
            if (deg_now(deg, v) == k) {
                const unsigned slot = atomicAdd(&s.count[0], 1u);
                if (slot < kCoreQueue) s.q[0][slot] = v;
                else atomicMax(&cnt->err, 1ULL);    // more alive vertices than the caller promised
            }
        }
        __syncthreads();
        const unsigned c = drain(s, kCoreQueue, L, deg, k, wave_row, unused,
                                 [&](int32_t) { atomicMax(&cnt->err, 1ULL); });
        last = c;
        steps += 1;
    }
    if (threadIdx.x == 0) {
        cnt->qlen = levels;
        cnt->mf = last;
        cnt->red[0] = static_cast<u64>(k);
        cnt->red[1] = steps;
    }
}

// core[v] = deg[v] as int64; tot[0] += vertices with core == top, tot[1] = max core.
__global__ void __launch_bounds__(kBlock) core_finish(const int32_t* __restrict__ deg, int64_t n, int32_t top, int64_t* core,
                                                      u64* tot) {
    u64 at_top = 0, mx = 0;
    for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < n; v += (int64_t)gridDim.x * blockDim.x) {
        const int32_t c = deg[v];
        core[v] = c;
        at_top += c == top;
        mx = max(mx, static_cast<u64>(c));
    }
    at_top = wave_sum(at_top);
    mx = wave_max(mx);
    if (lane() == 0) {
        if (at_top) atomicAdd(&tot[0], at_top);
        if (mx) atomicMax(&tot[1], mx);
    }
}

}  // namespace

// ---------------------------------------------------------------- launchers
hipError_t k_core_bwd_count(const int32_t* fadj, int64_t fnnz, int64_t* bcnt, hipStream_t s) {
    core_bwd_count<<<grid_for(fnnz, 2048), kBlock, 0, s>>>(fadj, fnnz, reinterpret_cast<u64*>(bcnt));
    return hipGetLastError();
}
hipError_t k_core_bwd_fill(const int64_t* foff, const int32_t* fadj, int64_t n, int64_t* cursor, int32_t* badj,
                           hipStream_t s) {
    core_bwd_fill<<<grid_for(((n + 63) / 64) * 64, 1 << 20), kBlock, 0, s>>>(foff, fadj, n, reinterpret_cast<u64*>(cursor), badj);
    return hipGetLastError();
}
hipError_t k_core_deg_init(const int64_t* d, int64_t n, int32_t* deg, hipStream_t s) {
    core_deg_init<<<grid_for(n, 2048), kBlock, 0, s>>>(d, n, deg);
    return hipGetLastError();
}
hipError_t k_core_scan(const int32_t* list, int64_t len, const int32_t* deg, int32_t k, int32_t* queue, int32_t* keep,
                       Counters* cnt, hipStream_t s) {
    core_scan<<<grid_for(len, 2048), kBlock, 0, s>>>(list, len, deg, k, queue, keep, cnt);
    return hipGetLastError();
}
hipError_t k_core_peel(const int32_t* cur, int64_t qlen, const CoreView& g, int32_t* deg, int32_t k, int64_t wave_row,
                       int64_t lds_cap, int32_t* next, int64_t n, Counters* cnt, hipStream_t s) {
    const unsigned cap = static_cast<unsigned>(std::max<int64_t>(1, std::min<int64_t>(lds_cap, kCoreQueue)));
    core_peel<<<grid_for(qlen, 2048), kBlock, 0, s>>>(cur, qlen, g, deg, k, wave_row, cap,
                                                next, n, cnt);
    return hipGetLastError();
}
hipError_t k_core_tail(const int32_t* list, int64_t len, const CoreView& g, int32_t* deg, int32_t k_prev, int64_t wave_row,
                       Counters* cnt, hipStream_t s) {
    core_tail<<<1, kBlock, 0, s>>>(list, len, g, deg, k_prev, wave_row, cnt);
    return hipGetLastError();
}
hipError_t k_core_finish(const int32_t* deg, int64_t n, int32_t top, int64_t* core, unsigned long long* tot,
                         hipStream_t s) {
    core_finish<<<grid_for(n, 2048), kBlock, 0, s>>>(deg, n, top, core, tot);
    return hipGetLastError();
}

}  // namespace tgo
