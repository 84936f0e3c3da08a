// scc.hip — strongly connected components on gfx950 (tgo_scc).
//
// Contract: the directed graph of a bothE load: an arc u -> v iff an OUT entry of u names v (the
// IN lists are its transpose).  label[v] = the smallest Titan id among the vertices that v reaches
// and that reach v.  The partition is unique; parallel arcs and self-loops change nothing.
//
// State over internal ids: comp[v] (int32) = -1 while v is live, else the internal id of its
// component's representative; din / dout (int32) = the entries of v's IN / OUT list that name a
// live vertex other than v.  Four phases, all of them retiring whole components:
//   trim     a live vertex whose din or dout is 0 is a component of its own.  A retired vertex's
//            rows are walked ONCE: every live neighbour's matching degree is lowered by an atomic,
//            and the lane whose atomicSub returns 1 took it to 0.  Both of a vertex's degrees can
//            reach 0 at once, so the CAS comp[w]: -1 -> w decides who retires w and walks it.
//   pivot    forward reach over OUT and backward reach over IN from one pivot, as bits 1 and 2 of
//            mark[]; the vertices with both bits are the pivot's component.
//   colour   colour[v] = v, MAX-propagated along arcs among live vertices to the fixed point; a
//            vertex that kept its own colour is a root, and what reaches it backward inside its
//            colour is its component.
//   tail     one workgroup runs trim and colouring passes on at most kSccTail live vertices with
//            their colours, marks and representatives in LDS.
//
// The queue walks (trim, both reaches, the colouring's backward marks) share one kernel shape,
// core.hip's: a workgroup takes 256 queue entries, and what it discovers goes to its own LDS queue,
// which it keeps draining, so a chain costs a barrier per vertex and not a launch; what does not
// fit spills to the global next queue.  A buffer that overflowed is a wide frontier, not a chain:
// it is spilled whole for the grid's next launch.  No grid barrier, no spin, no loop that waits for
// another workgroup's write.
//
// Stale reads (a line of this CU's L1 or this XCD's L2 that another CU has since rewritten) are
// older values, and every word moves one way inside a launch: comp -1 -> id, mark bits are only
// set, colours only rise, degrees only fall.  A filter read that is too old therefore only sends
// the lane to the atomic, which decides on the word's true value; it never skips work that is due.
// The colour propagation ends with a launch that changes nothing; a launch starts with cold
// caches, so that launch read every word as the memory held it.  Wave = 64 lanes.  Rows go to
// lanes by length: one lane per row, the whole wave from wave_row entries on.
#include <hip/hip_runtime.h>
#include "engine.hpp"
#include "wave.hpp"

namespace tgo {
namespace {

enum : int { kTrim = 0, kForward = 1, kBackward = 2, kColourBack = 3 };

__device__ __forceinline__ int32_t now(const int32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The calling wave walks one list's row of its lanes' vertices (has: the lane holds one); every lane
// of the wave calls this together.  f(v, tag, u) once per entry u of v's row, tag being v's lane's.
template <class F>
__device__ __forceinline__ void rows(bool has, int32_t v, int32_t tag, const int64_t* __restrict__ off,
                                     const int32_t* __restrict__ adj, int64_t wave_row, F&& f) {
    int64_t b = 0, l = 0;
    if (has) {
        b = off[v];
        l = off[v + 1] - b;
    }
    lane_or_wave(has && l >= wave_row, [&] {
        for (int64_t j = 0; j < l; ++j) f(v, tag, adj[b + j]);
    }, [&](int src) {
        const int64_t sb = __shfl(b, src, 64), sl = __shfl(l, src, 64);
        const int32_t sv = __shfl(v, src, 64), st = __shfl(tag, src, 64);
        for (int64_t j = lane(); j < sl; j += 64) f(sv, st, adj[sb + j]);
    });
}

// The entries of the lane's own row that do not name v itself (wide rows counted by the wave).
__device__ __forceinline__ int32_t row_degree(bool has, int32_t v, const int64_t* __restrict__ off,
                                              const int32_t* __restrict__ adj, int64_t wave_row) {
    int64_t b = 0, l = 0;
    if (has) {
        b = off[v];
        l = off[v + 1] - b;
    }
    u64 mine = 0;
    lane_or_wave(has && l >= wave_row, [&] {
        for (int64_t j = 0; j < l; ++j) mine += adj[b + j] != v;
    }, [&](int src) {
        const int64_t sb = __shfl(b, src, 64), sl = __shfl(l, src, 64);
        const int32_t sv = __shfl(v, src, 64);
        u64 part = 0;
        for (int64_t j = lane(); j < sl; j += 64) part += adj[sb + j] != sv;
        part = wave_sum(part);
        if (lane() == src) mine = part;
    });
    return static_cast<int32_t>(mine);
}

// ---------------------------------------------------------------- start
// din / dout of every vertex; with trim, a vertex without an arc in or without an arc out retires
// here (comp = v) and is queued for its walk; otherwise comp = -1.  cnt->qlen = the queued.
__global__ void __launch_bounds__(kBlock) scc_init(SccGraph G, int64_t n, SccState S, int trim, int64_t wave_row,
                                                   int32_t* queue, Counters* cnt) {
    const int64_t span = (n + 63) & ~int64_t(63);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < span; i += (int64_t)gridDim.x * blockDim.x) {
        const bool has = i < n;
        const int32_t v = static_cast<int32_t>(has ? i : 0);
        const int32_t dout = row_degree(has, v, G.ooff, G.oadj, wave_row);
        const int32_t din = row_degree(has, v, G.ioff, G.iadj, wave_row);
        const bool retire = has && trim && (din == 0 || dout == 0);
        if (has) {
            S.din[v] = din;
            S.dout[v] = dout;
            S.comp[v] = retire ? v : -1;
        }
        wave_append(retire, v, queue, &cnt->qlen, static_cast<u64>(n), &cnt->err);
    }
}

// ---------------------------------------------------------------- queue walks
// One entry u of a walked vertex's row.  Returns true when u is discovered here (the caller queues it).
__device__ __forceinline__ bool trim_hit(const SccState& S, int32_t* deg, int32_t u) {
    if (S.comp[u] != -1) return false;          // retired (an older -1 only costs the atomic)
    if (atomicSub(&deg[u], 1) != 1) return false;
    int32_t expect = -1;                        // its other degree may have reached 0 as well: one owner
    return __hip_atomic_compare_exchange_strong(&S.comp[u], &expect, u, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ bool mark_hit(const SccState& S, int32_t u, int32_t bit) {
    if (S.comp[u] != -1 || (S.mark[u] & bit)) return false;
    return !(atomicOr(&S.mark[u], bit) & bit);
}

// Walks the rows of the calling wave's vertices as MODE asks; push(u): u was discovered.
template <int MODE, class Push>
__device__ __forceinline__ void expand(bool has, int32_t v, const SccGraph& G, const SccState& S, int64_t wave_row,
                                       Push&& push) {
    if (MODE == kTrim) {
        rows(has, v, 0, G.ooff, G.oadj, wave_row, [&](int32_t s, int32_t, int32_t u) {
            if (u != s && trim_hit(S, S.din, u)) push(u);
        });
        rows(has, v, 0, G.ioff, G.iadj, wave_row, [&](int32_t s, int32_t, int32_t u) {
            if (u != s && trim_hit(S, S.dout, u)) push(u);
        });
    } else if (MODE == kForward) {
        rows(has, v, 0, G.ooff, G.oadj, wave_row, [&](int32_t, int32_t, int32_t u) {
            if (mark_hit(S, u, 1)) push(u);
        });
    } else if (MODE == kBackward) {
        rows(has, v, 0, G.ioff, G.iadj, wave_row, [&](int32_t, int32_t, int32_t u) {
            if (mark_hit(S, u, 2)) push(u);
        });
    } else {
        // the colours are at their fixed point: read-only here
        rows(has, v, has ? S.colour[v] : 0, G.ioff, G.iadj, wave_row, [&](int32_t, int32_t c, int32_t u) {
            if (S.colour[u] == c && mark_hit(S, u, 1)) push(u);
        });
    }
}

// The workgroup's LDS queue: two buffers; count[b] may run past the capacity (the entries beyond
// it were spilled), readers clamp it.
struct SccLds {
    int32_t q[2][kSccQueue];
    unsigned count[2];
};

// One launch over the queue cur: its vertices are walked, and what their workgroup discovers it
// walks itself from its LDS queue while the buffers stay within cap.  cnt->qlen = the discoveries
// left for the next launch (in next), cnt->mf += every discovery.  A vertex is discovered at most
// once per walk, so next (n entries) cannot overflow; the guard raises cnt->err.
template <int MODE>
__global__ void __launch_bounds__(kBlock) scc_walk(const int32_t* __restrict__ cur, int64_t qlen, SccGraph G, SccState S,
                                                   int64_t wave_row, unsigned cap, int32_t* next, int64_t n,
                                                   Counters* cnt) {
    __shared__ SccLds s;
    if (threadIdx.x == 0) s.count[0] = s.count[1] = 0;
    __syncthreads();
    u64 found = 0;
    auto spill = [&](int32_t u) {
        const u64 g = atomicAdd(&cnt->qlen, 1ULL);
        if (g < static_cast<u64>(n)) next[g] = u;
        else atomicMax(&cnt->err, 1ULL);
    };
    for (int64_t base = static_cast<int64_t>(blockIdx.x) * kBlock; base < qlen;
         base += static_cast<int64_t>(gridDim.x) * kBlock) {
        const int64_t i = base + threadIdx.x;
        const bool has = i < qlen;
        expand<MODE>(has, has ? cur[i] : 0, G, S, wave_row, [&](int32_t u) {
            ++found;
            const unsigned slot = atomicAdd(&s.count[0], 1u);
            if (slot < cap) s.q[0][slot] = u;
            else spill(u);
        });
        __syncthreads();
        for (int b = 0;; b ^= 1) {
            const unsigned raw = s.count[b];
            __syncthreads();                    // every thread has read the count before it changes
            if (!raw) break;
            const unsigned c = min(raw, cap);
            if (raw > cap) {                    // a wide frontier: all of it to the grid's next launch
                for (unsigned j = threadIdx.x; j < c; j += kBlock) spill(s.q[b][j]);
            } else {
                for (unsigned jb = 0; jb < c; jb += kBlock) {
                    const unsigned j = jb + threadIdx.x;
                    const bool h = j < c;
                    expand<MODE>(h, h ? s.q[b][j] : 0, G, S, wave_row, [&](int32_t u) {
                        ++found;
                        const unsigned slot = atomicAdd(&s.count[b ^ 1], 1u);
                        if (slot < cap) s.q[b ^ 1][slot] = u;
                        else spill(u);
                    });
                }
            }
            __syncthreads();
            if (threadIdx.x == 0) s.count[b] = 0;
            __syncthreads();
            if (raw > cap) break;               // (the other buffer is empty: it was drained before)
        }
    }
    found = wave_sum(found);
    if (lane() == 0 && found) atomicAdd(&cnt->mf, found);
}

// ---------------------------------------------------------------- pivot
// step 0: cnt->red[0] = max over the live vertices of din * dout + 1; step 1: among those at
// `product`, cnt->red[0] = UINT32_MAX - the smallest id.
__global__ void __launch_bounds__(kBlock) scc_pivot_pick(SccState S, int64_t n, int step, u64 product, Counters* cnt) {
    u64 best = 0;
    for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < n; v += (int64_t)gridDim.x * blockDim.x) {
        if (S.comp[v] != -1) continue;
        const u64 p = static_cast<u64>(S.din[v]) * static_cast<u64>(S.dout[v]) + 1;
        if (step == 0) best = max(best, p);
        else if (p == product) best = max(best, 0xFFFFFFFFULL - static_cast<u64>(v));
    }
    best = wave_max(best);
    if (lane() == 0 && best) atomicMax(&cnt->red[0], best);
}

// queue[0] = pivot, mark[pivot] |= bits.
__global__ void scc_seed(SccState S, int32_t pivot, int32_t bits, int32_t* queue) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        S.mark[pivot] |= bits;
        queue[0] = pivot;
    }
}

// ---------------------------------------------------------------- retire, live list
// The live vertices of list (null: every vertex) whose mark holds all of `bits` retire with
// representative rep (< 0: their colour).  cnt->mf = how many; with queue, they are queued for
// their trim walk (cnt->qlen).
__global__ void __launch_bounds__(kBlock) scc_retire(const int32_t* __restrict__ list, int64_t len, SccState S, int32_t bits,
                                                     int32_t rep, int32_t* queue, int64_t n, Counters* cnt) {
    const int64_t span = (len + 63) & ~int64_t(63);
    u64 mine = 0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < span; i += (int64_t)gridDim.x * blockDim.x) {
        const bool in = i < len;
        const int32_t v = in ? (list ? list[i] : static_cast<int32_t>(i)) : 0;
        const bool take = in && S.comp[v] == -1 && (S.mark[v] & bits) == bits;
        if (take) {
            S.comp[v] = rep < 0 ? S.colour[v] : rep;
            ++mine;
        }
        if (queue) wave_append(take, v, queue, &cnt->qlen, static_cast<u64>(n), &cnt->err);
    }
    mine = wave_sum(mine);
    if (lane() == 0 && mine) atomicAdd(&cnt->mf, mine);
}

// keep = the live vertices of list (null: every vertex), pos[v] = v's place in keep; cnt->qlen = how many.
__global__ void __launch_bounds__(kBlock) scc_live_list(const int32_t* __restrict__ list, int64_t len, SccState S, int32_t* keep,
                                                        int32_t* pos, int64_t n, Counters* cnt) {
    const int64_t span = (len + 63) & ~int64_t(63);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < span; i += (int64_t)gridDim.x * blockDim.x) {
        const bool in = i < len;
        const int32_t v = in ? (list ? list[i] : static_cast<int32_t>(i)) : 0;
        const bool take = in && S.comp[v] == -1;
        const u64 qm = __ballot(take);
        if (!qm) continue;
        const int lead = __ffsll(static_cast<long long>(qm)) - 1;
        u64 base = 0;
        if (lane() == lead) base = atomicAdd(&cnt->qlen, static_cast<u64>(__popcll(qm)));
        base = __shfl(base, lead, 64);
        if (take) {
            const u64 slot = base + __popcll(qm & ((1ULL << lane()) - 1));
            if (slot < static_cast<u64>(n)) {
                keep[slot] = v;
                pos[v] = static_cast<int32_t>(slot);
            } else {
                atomicMax(&cnt->err, 1ULL);
            }
        }
    }
}

// ---------------------------------------------------------------- colouring
__global__ void scc_colour_init(const int32_t* __restrict__ list, int64_t len, SccState S) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < len; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t v = list[i];
        S.colour[v] = v;
        S.mark[v] = 0;
    }
}

// One launch of the MAX propagation: every live vertex raises its live OUT neighbours to its colour.
// *changed (cnt->qlen) += the waves that raised one.
__global__ void __launch_bounds__(kBlock) scc_colour_round(const int32_t* __restrict__ list, int64_t len, SccGraph G, SccState S,
                                                           int64_t wave_row, Counters* cnt) {
    const int64_t span = (len + 63) & ~int64_t(63);
    bool any = false;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < span; i += (int64_t)gridDim.x * blockDim.x) {
        const bool has = i < len;
        const int32_t v = has ? list[i] : 0;
        // as the memory holds it: a colour raised earlier in this launch travels on in this launch
        const int32_t c = has ? now(&S.colour[v]) : 0;
        rows(has, v, c, G.ooff, G.oadj, wave_row, [&](int32_t, int32_t cs, int32_t u) {
            if (S.comp[u] != -1 || S.colour[u] >= cs) return;      // an older colour is a smaller one
            if (atomicMax(&S.colour[u], cs) < cs) any = true;
        });
    }
    if (__ballot(any) && lane() == 0) atomicAdd(&cnt->qlen, 1ULL);
}

// The roots (colour[v] == v) get mark 1 and are queued (cnt->qlen) for the backward marks.
__global__ void __launch_bounds__(kBlock) scc_roots(const int32_t* __restrict__ list, int64_t len, SccState S, int32_t* queue,
                                                    int64_t n, Counters* cnt) {
    const int64_t span = (len + 63) & ~int64_t(63);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < span; i += (int64_t)gridDim.x * blockDim.x) {
        const bool in = i < len;
        const int32_t v = in ? list[i] : 0;
        const bool root = in && S.colour[v] == v;
        if (root) S.mark[v] = 1;
        wave_append(root, v, queue, &cnt->qlen, static_cast<u64>(n), &cnt->err);
    }
}

// ---------------------------------------------------------------- tail
// Every remaining pass in one launch by one workgroup: the live vertices are those of list (len <=
// kSccTail, pos[v] = v's place in it; comp[v] == -1 exactly for them).  Liveness, colours and marks
// are LDS words; comp is read for the neighbours outside the list only and written once at the end.
// Out: cnt->qlen = colouring passes, cnt->mf = vertices retired, cnt->red[0] = barrier-separated sweeps.
struct TailLds {
    int32_t id[kSccTail];
    int32_t col[kSccTail];
    int32_t rep[kSccTail];      // -1 = live
    uint8_t mk[kSccTail];
    unsigned flag, count;
};

__global__ void __launch_bounds__(kBlock) scc_tail(const int32_t* __restrict__ list, int32_t len, SccGraph G, int32_t* comp,
                                                   const int32_t* __restrict__ pos, int trim, int64_t wave_row,
                                                   Counters* cnt) {
    __shared__ TailLds t;
    if (len > kSccTail) {
        if (threadIdx.x == 0) atomicMax(&cnt->err, 1ULL);
        return;
    }
    for (int32_t i = threadIdx.x; i < len; i += kBlock) {
        t.id[i] = list[i];
        t.rep[i] = -1;
    }
    // the place of a live vertex u in the list, else -1
    auto place = [&](int32_t u) -> int32_t {
        if (comp[u] != -1) return -1;
        const int32_t p = pos[u];
        if (static_cast<unsigned>(p) >= static_cast<unsigned>(len)) return -1;
        return t.rep[p] == -1 ? p : -1;
    };
    auto any_live = [&](const int64_t* off, const int32_t* adj, int32_t v) {
        for (int64_t k = off[v], e = off[v + 1]; k < e; ++k)
            if (adj[k] != v && place(adj[k]) >= 0) return true;
        return false;
    };
    u64 passes = 0, sweeps = 0;
    for (;;) {
        if (trim) {
            for (;;) {
                __syncthreads();
                if (threadIdx.x == 0) t.flag = 0;
                __syncthreads();
                // a neighbour read as live that has just retired only delays v to the next sweep
                for (int32_t i = threadIdx.x; i < len; i += kBlock) {
                    if (t.rep[i] != -1) continue;
                    const int32_t v = t.id[i];
                    if (!any_live(G.ioff, G.iadj, v) || !any_live(G.ooff, G.oadj, v)) {
                        t.rep[i] = v;
                        t.flag = 1;
                    }
                }
                __syncthreads();
                ++sweeps;
                if (!t.flag) break;
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) t.count = 0;
        __syncthreads();
        for (int32_t i = threadIdx.x; i < len; i += kBlock) {
            const bool live = t.rep[i] == -1;
            t.col[i] = live ? t.id[i] : -1;
            t.mk[i] = 0;
            if (live) atomicAdd(&t.count, 1u);
        }
        __syncthreads();
        if (!t.count) break;
        ++passes;
        for (;;) {                              // MAX propagation to the fixed point
            __syncthreads();
            if (threadIdx.x == 0) t.flag = 0;
            __syncthreads();
            for (int32_t base = 0; base < len; base += kBlock) {
                const int32_t i = base + threadIdx.x;
                const bool has = i < len && t.rep[i] == -1;
                rows(has, has ? t.id[i] : 0, has ? t.col[i] : 0, G.ooff, G.oadj, wave_row,
                     [&](int32_t, int32_t c, int32_t u) {
                         const int32_t p = place(u);
                         if (p >= 0 && t.col[p] < c && atomicMax(&t.col[p], c) < c) t.flag = 1;
                     });
            }
            __syncthreads();
            ++sweeps;
            if (!t.flag) break;
        }
        for (int32_t i = threadIdx.x; i < len; i += kBlock)
            if (t.rep[i] == -1 && t.col[i] == t.id[i]) t.mk[i] = 1;
        for (;;) {                              // v is marked when an arc of v ends at a marked vertex of its colour
            __syncthreads();
            if (threadIdx.x == 0) t.flag = 0;
            __syncthreads();
            for (int32_t base = 0; base < len; base += kBlock) {
                const int32_t i = base + threadIdx.x;
                const bool has = i < len && t.rep[i] == -1 && !t.mk[i];
                rows(has, has ? t.id[i] : 0, i, G.ooff, G.oadj, wave_row, [&](int32_t, int32_t me, int32_t u) {
                    const int32_t p = place(u);
                    if (p >= 0 && t.mk[p] && t.col[p] == t.col[me] && !t.mk[me]) {
                        t.mk[me] = 1;
                        t.flag = 1;
                    }
                });
            }
            __syncthreads();
            ++sweeps;
            if (!t.flag) break;
        }
        for (int32_t i = threadIdx.x; i < len; i += kBlock)
            if (t.rep[i] == -1 && t.mk[i]) t.rep[i] = t.col[i];
    }
    __syncthreads();
    u64 done = 0;
    for (int32_t i = threadIdx.x; i < len; i += kBlock) {
        comp[t.id[i]] = t.rep[i];
        done += t.rep[i] != -1;
    }
    done = wave_sum(done);
    if (lane() == 0 && done) atomicAdd(&cnt->mf, done);
    if (threadIdx.x == 0) {
        cnt->qlen = passes;
        cnt->red[0] = sweeps;
    }
}

// ---------------------------------------------------------------- labels
// Per representative: minid = the smallest Titan id under it, size = its vertices.  Lanes of a wave
// that share a representative fold first (cc.hip's cc_min_id: the giant component's words would
// otherwise take an atomic per vertex).  A vertex that is still live is left out.
__global__ void __launch_bounds__(kBlock) scc_fold(const int32_t* __restrict__ comp, const int64_t* __restrict__ tid, int64_t n,
                                                   long long* minid, int32_t* size) {
    const int64_t span = (n + 63) & ~int64_t(63);
    for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < span; v += (int64_t)gridDim.x * blockDim.x) {
        const int32_t r = v < n ? comp[v] : -1;
        const bool in = r >= 0 && r < n;
        const long long id = in ? tid[v] : INT64_MAX;
        bool todo = in;
        for (int round = 0; round < 2; ++round) {
            const u64 m = __ballot(todo);
            if (!m) break;
            const int lead = __ffsll(static_cast<long long>(m)) - 1;
            const int32_t r0 = __shfl(r, lead, 64);
            const bool mine = todo && r == r0;
            const long long lo = wave_min(mine ? id : INT64_MAX);
            const int cnt = __popcll(__ballot(mine));
            if (lane() == lead) {
                atomicMin(&minid[r0], lo);
                atomicAdd(&size[r0], cnt);
            }
            if (mine) todo = false;
        }
        if (todo) {
            atomicMin(&minid[r], id);
            atomicAdd(&size[r], 1);
        }
    }
}

// label[v] = minid[comp[v]]; cnt->qlen += components, cnt->mf += those of one vertex, cnt->red[0] =
// the largest, cnt->red[1] += the vertices that have a representative.
__global__ void __launch_bounds__(kBlock) scc_label(const int32_t* __restrict__ comp, const long long* __restrict__ minid,
                                                    const int32_t* __restrict__ size, int64_t n, int64_t* label,
                                                    Counters* cnt) {
    u64 comps = 0, single = 0, largest = 0, retired = 0;
    for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < n; v += (int64_t)gridDim.x * blockDim.x) {
        const int32_t r = comp[v];
        if (r < 0 || r >= n) continue;
        ++retired;
        label[v] = minid[r];
        if (r == v) {
            const u64 sz = static_cast<u64>(size[v]);
            ++comps;
            single += sz == 1;
            largest = max(largest, sz);
        }
    }
    comps = wave_sum(comps);
    single = wave_sum(single);
    retired = wave_sum(retired);
    largest = wave_max(largest);
    if (lane() == 0) {
        if (comps) atomicAdd(&cnt->qlen, comps);
        if (single) atomicAdd(&cnt->mf, single);
        if (largest) atomicMax(&cnt->red[0], largest);
        if (retired) atomicAdd(&cnt->red[1], retired);
    }
}

}  // namespace

// ---------------------------------------------------------------- launchers
hipError_t k_scc_init(const SccGraph& g, int64_t n, const SccState& st, bool trim, int64_t wave_row, int32_t* queue,
                      Counters* cnt, hipStream_t s) {
    scc_init<<<grid_for(((n + 63) / 64) * 64, 1 << 20), kBlock, 0, s>>>(g, n, st, trim ? 1 : 0, wave_row, queue, cnt);
    return hipGetLastError();
}
hipError_t k_scc_walk(int mode, const int32_t* cur, int64_t qlen, const SccGraph& g, const SccState& st, int64_t wave_row,
                      int32_t* next, int64_t n, Counters* cnt, hipStream_t s) {
    const unsigned cap = kSccQueue;
    const int grid = grid_for(qlen, 2048);
    switch (mode) {
    case kTrim: scc_walk<kTrim><<<grid, kBlock, 0, s>>>(cur, qlen, g, st, wave_row, cap, next, n, cnt); break;
    case kForward: scc_walk<kForward><<<grid, kBlock, 0, s>>>(cur, qlen, g, st, wave_row, cap, next, n, cnt); break;
    case kBackward: scc_walk<kBackward><<<grid, kBlock, 0, s>>>(cur, qlen, g, st, wave_row, cap, next, n, cnt); break;
    case kColourBack: scc_walk<kColourBack><<<grid, kBlock, 0, s>>>(cur, qlen, g, st, wave_row, cap, next, n, cnt); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
hipError_t k_scc_pivot_pick(const SccState& st, int64_t n, int step, unsigned long long product, Counters* cnt,
                            hipStream_t s) {
    scc_pivot_pick<<<grid_for(n, 2048), kBlock, 0, s>>>(st, n, step, product, cnt);
    return hipGetLastError();
}
hipError_t k_scc_seed(const SccState& st, int32_t pivot, int32_t bits, int32_t* queue, hipStream_t s) {
    scc_seed<<<1, 64, 0, s>>>(st, pivot, bits, queue);
    return hipGetLastError();
}
hipError_t k_scc_retire(const int32_t* list, int64_t len, const SccState& st, int32_t bits, int32_t rep, int32_t* queue,
                        int64_t n, Counters* cnt, hipStream_t s) {
    scc_retire<<<grid_for(((len + 63) / 64) * 64, 2048), kBlock, 0, s>>>(list, len, st, bits, rep, queue, n, cnt);
    return hipGetLastError();
}
hipError_t k_scc_live_list(const int32_t* list, int64_t len, const SccState& st, int32_t* keep, int32_t* pos, int64_t n,
                           Counters* cnt, hipStream_t s) {
    scc_live_list<<<grid_for(((len + 63) / 64) * 64, 2048), kBlock, 0, s>>>(list, len, st, keep, pos, n, cnt);
    return hipGetLastError();
}
hipError_t k_scc_colour_init(const int32_t* list, int64_t len, const SccState& st, hipStream_t s) {
    scc_colour_init<<<grid_for(len, 2048), kBlock, 0, s>>>(list, len, st);
    return hipGetLastError();
}
hipError_t k_scc_colour_round(const int32_t* list, int64_t len, const SccGraph& g, const SccState& st, int64_t wave_row,
                              Counters* cnt, hipStream_t s) {
    scc_colour_round<<<grid_for(((len + 63) / 64) * 64, 2048), kBlock, 0, s>>>(list, len, g, st, wave_row, cnt);
    return hipGetLastError();
}
hipError_t k_scc_roots(const int32_t* list, int64_t len, const SccState& st, int32_t* queue, int64_t n, Counters* cnt,
                       hipStream_t s) {
    scc_roots<<<grid_for(((len + 63) / 64) * 64, 2048), kBlock, 0, s>>>(list, len, st, queue, n, cnt);
    return hipGetLastError();
}
hipError_t k_scc_tail(const int32_t* list, int64_t len, const SccGraph& g, int32_t* comp, const int32_t* pos, bool trim,
                      int64_t wave_row, Counters* cnt, hipStream_t s) {
    if (len < 0 || len > kSccTail) return hipErrorInvalidValue;
    scc_tail<<<1, kBlock, 0, s>>>(list, static_cast<int32_t>(len), g, comp, pos, trim ? 1 : 0, wave_row, cnt);
    return hipGetLastError();
}
hipError_t k_scc_fold(const int32_t* comp, const int64_t* tid, int64_t n, int64_t* minid, int32_t* size, hipStream_t s) {
    scc_fold<<<grid_for(((n + 63) / 64) * 64, 2048), kBlock, 0, s>>>(comp, tid, n, reinterpret_cast<long long*>(minid), size);
    return hipGetLastError();
}
hipError_t k_scc_label(const int32_t* comp, const int64_t* minid, const int32_t* size, int64_t n, int64_t* label,
                       Counters* cnt, hipStream_t s) {
    scc_label<<<grid_for(n, 2048), kBlock, 0, s>>>(comp, reinterpret_cast<const long long*>(minid), size, n, label, cnt);
    return hipGetLastError();
}

}  // namespace tgo
