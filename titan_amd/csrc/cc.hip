// cc.hip — weakly connected components on gfx950 (tgo_components).
//
// Contract: label[v] = the fixed point of MIN label propagation over the loaded bothE pull
// lists, labels being Titan ids (tests/generic_programs.py ConnectedComponents is the same
// program run superstep by superstep).  Two device paths (DESIGN.md "Connected components"):
//
//   hook      (the lists are each other's transpose) concurrent union-find over an int32 parent
//             array in internal ids.  Invariant: parent[x] <= x.  A tree changes shape only by
//               - a hook: atomicCAS(parent[hi], hi, lo) on a ROOT hi with lo < hi (agent scope),
//               - pointer jumping in a launch of its own: parent[v] = an ancestor of v.
//             So whatever value a lane reads for parent[x] — current, or a stale line of its L1
//             or of its XCD's L2 — is an ancestor of x (or x) in x's tree and <= x.  Climbing by
//             plain loads therefore ends at a vertex that merely LOOKS like a root; the CAS on
//             that vertex's own word decides, and when it fails it returns the word's true value,
//             from which the lane goes on.  No loop waits for another workgroup: every step of
//             link() lowers max(a, b), so it ends on its own.
//   propagate (explicit transpose: the lists are not symmetric, union-find would merge too much)
//             in-place MIN pull over both lists on int64 Titan-id labels, one launch per round.
//
// Rows go to lanes by degree as in bu_step / ms_pull: one wave per 64 consecutive rows (internal
// ids are degree-grouped, so a wave's rows are alike), a row of up to kSerialRow entries walked
// by its own lane, a longer one by the whole wave, 64 entries a trip.  Wave = 64 lanes.
#include <hip/hip_runtime.h>
#include "engine.hpp"
#include "wave.hpp"

namespace tgo {
namespace {

constexpr int64_t kSerialRow = 32;
constexpr int kJump = 32;           // parents a lane follows per pointer-jumping launch

__device__ __forceinline__ int32_t cas_parent(int32_t* p, int32_t expect, int32_t want) {
    __hip_atomic_compare_exchange_strong(p, &expect, want, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return expect;                  // the word's value before the exchange
}

// The vertex above x whose parent word reads as itself.  parent[] <= index: ends within x steps.
__device__ __forceinline__ int32_t climb(const int32_t* parent, int32_t x) {
    for (int32_t p; (p = parent[x]) != x;) x = p;
    return x;
}

// Union the trees of a (an ancestor-or-self of the row's vertex) and vertex u; returns an
// ancestor-or-self of both, the next entry's starting point.
__device__ __forceinline__ int32_t link(int32_t* parent, int32_t a, int32_t u) {
    int32_t b = climb(parent, u);
    a = climb(parent, a);
    while (a != b) {
        const int32_t hi = max(a, b), lo = min(a, b);
        const int32_t old = cas_parent(&parent[hi], hi, lo);
        if (old == hi || old == lo) return lo;      // hooked here, or by someone else just so
        // hi was no root: old (< hi) is its parent as the memory holds it; go on from there
        a = climb(parent, old);
        b = lo;
    }
    return a;
}

__global__ void cc_init(int32_t* parent, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        parent[i] = static_cast<int32_t>(i);
}

// Hook the entries [from, to) of every row of list `off/adj` (to < 0: to the row's end).
__global__ void __launch_bounds__(kBlock) cc_hook(const int64_t* __restrict__ off, const int32_t* __restrict__ adj,
                                                  int64_t n, int64_t from, int64_t to, int32_t* parent) {
    for_each_row_64(n, [&](int64_t v, bool live) {
        int64_t kb = 0, ke = 0;
        if (live) {
            kb = off[v];
            ke = off[v + 1];
            if (to >= 0) ke = min(ke, kb + to);
            kb = min(ke, kb + from);
        }
        lane_or_wave(ke - kb > kSerialRow, [&] {
            int32_t a = static_cast<int32_t>(v);
            for (int64_t k = kb; k < ke; ++k) a = link(parent, a, adj[k]);
        }, [&](int src) {
            const int64_t bb = __shfl(kb, src, 64), ee = __shfl(ke, src, 64);
            int32_t a = static_cast<int32_t>(v - lane() + src);
            for (int64_t k = bb + lane(); k < ee; k += 64) a = link(parent, a, adj[k]);
        });
    });
}

// Pointer jumping: every vertex moves under the ancestor kJump parents up (a root at the latest).
// *changed counts the vertices that were not yet directly under a root when this launch read them.
__global__ void __launch_bounds__(kBlock) cc_jump(int32_t* parent, int64_t n, unsigned long long* changed) {
    bool any = false;
    for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < n; v += (int64_t)gridDim.x * blockDim.x) {
        const int32_t p = parent[v];
        int32_t r = p;
        for (int j = 0; j < kJump; ++j) {
            const int32_t q = parent[r];
            if (q == r) break;
            r = q;
        }
        if (r != p) {
            parent[v] = r;
            any = true;
        }
    }
    if (__ballot(any) && lane() == 0) atomicAdd(changed, 1ULL);
}

__global__ void cc_scatter_ids(const int64_t* __restrict__ row_ids, const int32_t* __restrict__ perm, int64_t* tid,
                               int64_t n) {
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x)
        tid[perm[r]] = row_ids[r];
}

// minid[root] = min Titan id of the tree (parent[] is flat: every vertex sits under its root).
// Lanes of a wave that share a root fold their ids first — on a power-law graph nearly every lane
// is in the giant component, whose root word would otherwise take one atomic per vertex.
__global__ void __launch_bounds__(kBlock) cc_min_id(const int32_t* __restrict__ parent, const int64_t* __restrict__ tid,
                                                    int64_t n, long long* minid) {
    const int64_t span = (n + 63) & ~int64_t(63);
    for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < span; v += (int64_t)gridDim.x * blockDim.x) {
        const bool live = v < n;
        const int32_t r = live ? parent[v] : -1;
        const long long id = live ? tid[v] : INT64_MAX;
        bool todo = live;
        for (int round = 0; round < 2; ++round) {
            const unsigned long long m = __ballot(todo);
            if (!m) break;
            const int lead = __ffsll(static_cast<long long>(m)) - 1;
            const int32_t r0 = __shfl(r, lead, 64);
            const bool mine = todo && r == r0;
            const long long lo = wave_min(mine ? id : INT64_MAX);
            if (lane() == lead) atomicMin(&minid[r0], lo);
            if (mine) todo = false;
        }
        if (todo) atomicMin(&minid[r], id);
    }
}

__global__ void __launch_bounds__(kBlock) cc_label(const int32_t* __restrict__ parent, const long long* __restrict__ minid,
                                                   int64_t n, int64_t* label, unsigned long long* roots) {
    unsigned long long mine = 0;
    for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < n; v += (int64_t)gridDim.x * blockDim.x) {
        const int32_t r = parent[v];
        label[v] = minid[r];
        mine += r == v;
    }
    mine = wave_sum(mine);
    if (lane() == 0 && mine) atomicAdd(roots, mine);
}

// One round of in-place MIN pull over both lists.  Only v's lane writes label[v]; a neighbour's
// label read here is its current one or an earlier, larger one — both are ids of vertices that
// reach v, so labels only fall towards the fixed point, and a round that lowers nothing read
// nothing stale (a launch starts with cold caches) and proves it.
__global__ void __launch_bounds__(kBlock) cc_pull_round(View pull, int64_t n, int64_t* label, unsigned long long* changed) {
    bool any = false;
    for_each_row_64(n, [&](int64_t v, bool live) {
        int64_t b0 = 0, e0 = 0, b1 = 0, e1 = 0;
        if (live) {
            b0 = pull.off0[v]; e0 = pull.off0[v + 1];
            if (pull.nlists > 1) { b1 = pull.off1[v]; e1 = pull.off1[v + 1]; }
        }
        const int64_t deg = (e0 - b0) + (e1 - b1);
        const int64_t cur = live ? label[v] : 0;
        int64_t m = cur;
        lane_or_wave(deg > kSerialRow, [&] {
            for (int64_t k = b0; k < e0; ++k) m = min(m, label[pull.adj0[k]]);
            for (int64_t k = b1; k < e1; ++k) m = min(m, label[pull.adj1[k]]);
        }, [&](int src) {
            long long w = INT64_MAX;
            for (int l = 0; l < 2; ++l) {
                const int64_t bb = __shfl(l == 0 ? b0 : b1, src, 64), ee = __shfl(l == 0 ? e0 : e1, src, 64);
                const int32_t* adj = l == 0 ? pull.adj0 : pull.adj1;
                for (int64_t k = bb + lane(); k < ee; k += 64) w = min(w, static_cast<long long>(label[adj[k]]));
            }
            w = wave_min(w);
            if (lane() == src) m = min(m, static_cast<int64_t>(w));
        });
        if (live && m < cur) {
            label[v] = m;
            any = true;
        }
    });
    if (__ballot(any) && lane() == 0) atomicAdd(changed, 1ULL);
}

__global__ void __launch_bounds__(kBlock) cc_count_own(const int64_t* __restrict__ label, const int64_t* __restrict__ tid,
                                                       int64_t n, unsigned long long* roots) {
    unsigned long long mine = 0;
    for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < n; v += (int64_t)gridDim.x * blockDim.x)
        mine += label[v] == tid[v];
    mine = wave_sum(mine);
    if (lane() == 0 && mine) atomicAdd(roots, mine);
}

}  // namespace

// ---------------------------------------------------------------- launchers
hipError_t k_cc_init(int32_t* parent, int64_t n, hipStream_t s) {
    cc_init<<<grid_for(n, 2048), kBlock, 0, s>>>(parent, n);
    return hipGetLastError();
}
hipError_t k_cc_hook(const DevCsr& list, int64_t n, int64_t from, int64_t to, int32_t* parent, hipStream_t s) {
    cc_hook<<<grid_for(((n + 63) / 64) * 64, 2048), kBlock, 0, s>>>(list.off, list.adj, n, from, to, parent);
    return hipGetLastError();
}
hipError_t k_cc_jump(int32_t* parent, int64_t n, unsigned long long* changed, hipStream_t s) {
    cc_jump<<<grid_for(n, 2048), kBlock, 0, s>>>(parent, n, changed);
    return hipGetLastError();
}
hipError_t k_cc_scatter_ids(const int64_t* row_ids, const int32_t* perm, int64_t* tid, int64_t n, hipStream_t s) {
    cc_scatter_ids<<<grid_for(n, 2048), kBlock, 0, s>>>(row_ids, perm, tid, n);
    return hipGetLastError();
}
hipError_t k_cc_min_id(const int32_t* parent, const int64_t* tid, int64_t n, int64_t* minid, hipStream_t s) {
    cc_min_id<<<grid_for(n, 2048), kBlock, 0, s>>>(parent, tid, n, reinterpret_cast<long long*>(minid));
    return hipGetLastError();
}
hipError_t k_cc_label(const int32_t* parent, const int64_t* minid, int64_t n, int64_t* label, unsigned long long* roots,
                      hipStream_t s) {
    cc_label<<<grid_for(n, 2048), kBlock, 0, s>>>(parent, reinterpret_cast<const long long*>(minid), n, label, roots);
    return hipGetLastError();
}
hipError_t k_cc_pull_round(const View& pull, int64_t n, int64_t* label, unsigned long long* changed, hipStream_t s) {
    cc_pull_round<<<grid_for(((n + 63) / 64) * 64, 2048), kBlock, 0, s>>>(pull, n, label, changed);
    return hipGetLastError();
}
hipError_t k_cc_count_own(const int64_t* label, const int64_t* tid, int64_t n, unsigned long long* roots, hipStream_t s) {
    cc_count_own<<<grid_for(n, 2048), kBlock, 0, s>>>(label, tid, n, roots);
    return hipGetLastError();
}

}  // namespace tgo
