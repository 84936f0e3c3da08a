// pp.hip — peer-pressure clustering on gfx950 (tgo_peer_pressure).
//
// Contract: over a bothE load read as the directed multigraph of tgo_scc, every entry one edge and one
// vote.  cluster(v) starts as v's Titan id; in a round every vertex v tallies, per cluster c,
//   T_v(c) = [c = cluster(v)] S(v) + the sum of S(u) over the entries of v's receive rows whose sender
//            u has cluster(u) = c
// from the previous round's clusters (Jacobi) and moves to the c of the largest T_v(c), ties to the
// smallest Titan id.  S is an unsigned integer in units of 2^-32 (2^32, or floor(2^32 / d(u)) with
// distribute), so a tally is an exact integer sum, independent of the order it is folded in: LDS
// atomics may add in any order and every tier, table size and run gives the same bits.
//
// Labels are int32 ranks of the Titan ids (a permutation cached with the graph): a tie breaks by an
// integer compare and a label is a 4-byte gather.  The votes of a round are one array indexed by
// sender, double-buffered: the int32 label (distribute = 0: S is constant) or the 8-byte word
// label << 33 | S (distribute = 1: one random read per entry, not two).  A word whose S is 0 belongs
// to a vertex that sends over no entry; it names no row and never leaves its own cluster.
//
// Rows are tiered by their receive-row length, which no round changes: pp_init queues the rows of
// at least wave_row / block_row entries once per call, and every round launches
//   G = 1    the rows below both lengths, one lane each over every vertex
//   G = 64   the wave queue, one wave per row
//   G = 256  the block queue, one workgroup per row
// Round 1 (pp_first): every sender still has its own label and the rows are sorted by internal id, so
// the entries of one sender are adjacent (and found in the other list of a bothE tally by a binary
// search): the head of each run tallies multiplicity x S(u), nothing is grouped and no table is
// needed — a hub's row has as many labels as distinct senders, which would overflow any table.
// Later rounds (pp_vote): G = 1 folds its short row pairwise; G = 64 / 256 tally into an LDS
// open-addressed table (atomicCAS on the key, 64-bit atomicAdd on the tally; `slots` entries per
// wave, four times that per workgroup) and take the argmax of (tally, -rank) over the slots.  A row
// with more labels than slots overflows: the table is dropped and the row is tallied again in K =
// ceil(2 (l + 1) / slots) passes, pass k over the labels of hash class k (a second hash), which leave
// the table half empty on average.  Should a class still outgrow it, the row is tallied once more in
// passes over the classes [lo + k slots, lo + (k + 1) slots) of the rank range [lo, hi] its labels
// span, direct-mapped (slot = rank - base, so no key and no probe): at most ceil(n / slots) classes
// always fit, so the path ends with the exact answer for any row.
// Global atomics: the queue appends of pp_init, the changed count (one per wave), the histogram of
// pp_finish (one per vertex, once per call).  No grid barrier, no spin.  Wave = 64 lanes.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include "engine.hpp"
#include "wave.hpp"

namespace tgo {
namespace {

constexpr u64 kPpOne = 1ULL << 32;              // a whole vote
constexpr u64 kPpSMask = (1ULL << 33) - 1;      // S of a vote word (S <= 2^32)

__device__ __forceinline__ void wave_sync() {          // a wave's LDS writes visible to its own later reads
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The vote of sender u in the round's array: its label and its strength.
template <bool DIST>
__device__ __forceinline__ void vote_of(const void* __restrict__ cur, int32_t u, int32_t& label, u64& s) {
    if (DIST) {
        const u64 w = static_cast<const u64*>(cur)[u];
        label = static_cast<int32_t>(w >> 33);
        s = w & kPpSMask;
    } else {
        label = static_cast<const int32_t*>(cur)[u];
        s = kPpOne;
    }
}
template <bool DIST>
__device__ __forceinline__ void vote_store(void* next, const void* __restrict__ cur, int32_t v, int32_t label) {
    if (DIST) static_cast<u64*>(next)[v] = (static_cast<u64>(label) << 33) | (static_cast<const u64*>(cur)[v] & kPpSMask);
    else static_cast<int32_t*>(next)[v] = label;
}

// The larger tally wins, among equals the smaller rank.
struct Best {
    u64 t;
    int32_t c;
    __device__ __forceinline__ void take(u64 t2, int32_t c2) {
        if (t2 > t || (t2 == t && c2 < c)) { t = t2; c = c2; }
    }
};

// v's receive rows as one list of l0 + l1 entries.
struct Row {
    const int32_t* a0;
    const int32_t* a1;
    int64_t l0, l1;
    __device__ __forceinline__ int64_t len() const { return l0 + l1; }
    __device__ __forceinline__ int32_t at(int64_t j) const { return j < l0 ? a0[j] : a1[j - l0]; }
};
__device__ __forceinline__ Row row_of(const View& r, int64_t v) {
    Row w;
    const int64_t b0 = r.off0[v];
    w.a0 = r.adj0 + b0;
    w.l0 = r.off0[v + 1] - b0;
    w.a1 = w.a0;
    w.l1 = 0;
    if (r.nlists == 2) {
        const int64_t b1 = r.off1[v];
        w.a1 = r.adj1 + b1;
        w.l1 = r.off1[v + 1] - b1;
    }
    return w;
}
__device__ __forceinline__ int64_t row_len(const View& r, int64_t v) {
    int64_t l = r.off0[v + 1] - r.off0[v];
    if (r.nlists == 2) l += r.off1[v + 1] - r.off1[v];
    return l;
}

// ---------------------------------------------------------------- group folds (G = 1, 64, 256)
struct PpShared {
    u64 t[kWavesPerBlock];
    int32_t c[kWavesPerBlock], lo[kWavesPerBlock], hi[kWavesPerBlock];
    int any[kWavesPerBlock];
};

__device__ __forceinline__ Best wave_best(Best b) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) b.take(__shfl_xor(b.t, d, 64), __shfl_xor(b.c, d, 64));
    return b;
}

// The best of the group's lanes on every lane of it.  G = 256: every thread of the block calls.
template <int G>
__device__ __forceinline__ Best group_best(Best b, PpShared& sh) {
    if (G == 1) return b;
    b = wave_best(b);
    if (G == 64) return b;
    const int w = threadIdx.x >> 6;
    __syncthreads();                    // sh's last use is over
    if (lane() == 0) { sh.t[w] = b.t; sh.c[w] = b.c; }
    __syncthreads();
    Best r{sh.t[0], sh.c[0]};
#pragma unroll
    for (int k = 1; k < kWavesPerBlock; ++k) r.take(sh.t[k], sh.c[k]);
    return r;
}

template <int G>
__device__ __forceinline__ void group_sync() {
    if (G == 64) wave_sync();
    if (G == 256) __syncthreads();
}

// {any lane's flag, the smallest lo, the largest hi} of the group, on every lane.
template <int G>
__device__ __forceinline__ void group_span(bool& any, int32_t& lo, int32_t& hi, PpShared& sh) {
    any = __ballot(any) != 0;
    lo = wave_min(lo);
    hi = wave_max(hi);
    if (G != 256) return;
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if (lane() == 0) { sh.any[w] = any; sh.lo[w] = lo; sh.hi[w] = hi; }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kWavesPerBlock; ++k) {
        any = any || sh.any[k];
        lo = min(lo, sh.lo[k]);
        hi = max(hi, sh.hi[k]);
    }
}

// ---------------------------------------------------------------- init
// The first votes (label = rank, S by d(v) = the entries of v's send rows) and the two row queues
// (wave_append: a vertex is appended to one queue once, so a queue of n + 1 entries cannot overflow).
template <bool DIST>
__global__ void __launch_bounds__(kBlock) pp_init(View recv, View send, int64_t n, const int32_t* __restrict__ rank,
                                                  void* cur, int64_t wave_row, int64_t block_row, int32_t* wq, u64* wcount,
                                                  int32_t* bq, u64* bcount) {
    const int64_t span = (n + 63) & ~int64_t(63);
    for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < span; v += (int64_t)gridDim.x * blockDim.x) {
        const bool has = v < n;
        int64_t l = 0;
        if (has) {
            const int32_t r = rank[v];
            if (DIST) {
                const int64_t d = row_len(send, v);
                const u64 s = d > 0 ? kPpOne / static_cast<u64>(d) : 0;
                static_cast<u64*>(cur)[v] = (static_cast<u64>(r) << 33) | s;
            } else {
                static_cast<int32_t*>(cur)[v] = r;
            }
            l = row_len(recv, v);
        }
        const bool block = has && l >= block_row;
        wave_append(block, static_cast<int32_t>(v), bq, bcount);
        wave_append(has && !block && l >= wave_row, static_cast<int32_t>(v), wq, wcount);
    }
}

// ---------------------------------------------------------------- the rows of a launch
// Which row the calling group takes on trip `it` of its loop (-1: none left; G = 1: none on this lane).
// The loop's trip count is the same for every lane of a group (of a wave for G = 1).
template <int G>
__device__ __forceinline__ int64_t group_trips(int64_t n, int64_t count) {
    if (G == 1) {
        const int64_t span = (n + 63) & ~int64_t(63), step = (int64_t)gridDim.x * blockDim.x;
        const int64_t first = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
        return first < span ? (span - first + step - 1) / step : 0;
    }
    const int64_t step = G == 64 ? (int64_t)gridDim.x * kWavesPerBlock : (int64_t)gridDim.x;
    const int64_t first = G == 64 ? (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6) : (int64_t)blockIdx.x;
    return first < count ? (count - first + step - 1) / step : 0;
}
template <int G>
__device__ __forceinline__ int32_t group_row(int64_t it, const View& recv, int64_t n, int64_t wave_row,
                                             const int32_t* __restrict__ queue) {
    if (G == 1) {
        const int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x + it * (int64_t)gridDim.x * blockDim.x;
        return v < n && row_len(recv, v) < wave_row ? static_cast<int32_t>(v) : -1;
    }
    if (G == 64) return queue[(int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6) + it * (int64_t)gridDim.x * kWavesPerBlock];
    return queue[(int64_t)blockIdx.x + it * (int64_t)gridDim.x];
}

// `moved` (on the lane that stored a row's label) into *changed: one atomic per wave.
template <int G>
__device__ __forceinline__ void count_changed(u64 moved, u64* changed) {
    if (G == 1) {
        moved = wave_sum(moved);
        if (lane() == 0 && moved) atomicAdd(changed, moved);
    } else if (moved) {
        atomicAdd(changed, moved);
    }
}

// ---------------------------------------------------------------- round 1
// Every sender u still votes for rank(u), and the rows are sorted by internal id: the first entry of u
// in v's rows (list 0 before list 1) is the head of u's run and tallies all its entries at once.
template <bool DIST, int G>
__global__ void __launch_bounds__(kBlock) pp_first(View recv, int64_t n, const void* __restrict__ cur, void* next,
                                                   int64_t wave_row, const int32_t* __restrict__ queue, int64_t count,
                                                   u64* changed) {
    __shared__ PpShared sh;
    const int gl = G == 1 ? 0 : static_cast<int>(threadIdx.x & (G - 1));
    const int64_t trips = group_trips<G>(n, count);
    u64 moved = 0;
    for (int64_t it = 0; it < trips; ++it) {
        const int32_t v = group_row<G>(it, recv, n, wave_row, queue);
        if (v < 0) continue;                    // (G = 1 only: no group fold follows)
        int32_t ol;
        u64 os;
        vote_of<DIST>(cur, v, ol, os);
        const Row w = row_of(recv, v);
        Best b{os, ol};                         // v's own vote (a self-entry's run adds it again below and wins)
        for (int64_t j = gl; j < w.len(); j += G) {
            const int32_t u = w.at(j);
            int64_t mult = 0;
            if (j < w.l0) {
                if (j > 0 && w.a0[j - 1] == u) continue;
                for (int64_t k = j; k < w.l0 && w.a0[k] == u; ++k) ++mult;
                if (w.l1 > 0)
                    for (int64_t k = lower_bound(w.a1, w.l1, u); k < w.l1 && w.a1[k] == u; ++k) ++mult;
            } else {
                const int64_t j1 = j - w.l0;
                if (j1 > 0 && w.a1[j1 - 1] == u) continue;
                const int64_t p = lower_bound(w.a0, w.l0, u);
                if (p < w.l0 && w.a0[p] == u) continue;
                for (int64_t k = j1; k < w.l1 && w.a1[k] == u; ++k) ++mult;
            }
            int32_t c;
            u64 s;
            vote_of<DIST>(cur, u, c, s);
            b.take(static_cast<u64>(mult) * s + (u == v ? os : 0), c);
        }
        b = group_best<G>(b, sh);
        if (gl == 0) {
            const int32_t to = DIST && os == 0 ? ol : b.c;
            vote_store<DIST>(next, cur, v, to);
            moved += to != ol;
        }
    }
    count_changed<G>(moved, changed);
}

// ---------------------------------------------------------------- later rounds
// One lane per short row: each label's tally is folded at its first entry (the own label's first).
template <bool DIST>
__global__ void __launch_bounds__(kBlock) pp_vote_lane(View recv, int64_t n, const void* __restrict__ cur, void* next,
                                                       int64_t wave_row, u64* changed) {
    const int64_t trips = group_trips<1>(n, 0);
    u64 moved = 0;
    for (int64_t it = 0; it < trips; ++it) {
        const int32_t v = group_row<1>(it, recv, n, wave_row, nullptr);
        if (v < 0) continue;
        int32_t ol;
        u64 os;
        vote_of<DIST>(cur, v, ol, os);
        int32_t to = ol;
        if (!DIST || os != 0) {
            const Row w = row_of(recv, v);
            const int64_t l = w.len();
            Best b{os, ol};
            for (int64_t i = 0; i < l; ++i) {
                int32_t c;
                u64 s;
                vote_of<DIST>(cur, w.at(i), c, s);
                if (c == ol) b.t += s;
            }
            for (int64_t j = 0; j < l; ++j) {
                int32_t cj;
                u64 t;
                vote_of<DIST>(cur, w.at(j), cj, t);
                if (cj == ol) continue;
                bool head = true;
                for (int64_t i = 0; i < j && head; ++i) {
                    int32_t c;
                    u64 s;
                    vote_of<DIST>(cur, w.at(i), c, s);
                    head = c != cj;
                }
                if (!head) continue;
                for (int64_t i = j + 1; i < l; ++i) {
                    int32_t c;
                    u64 s;
                    vote_of<DIST>(cur, w.at(i), c, s);
                    if (c == cj) t += s;
                }
                b.take(t, cj);
            }
            to = b.c;
        }
        vote_store<DIST>(next, cur, v, to);
        moved += to != ol;
    }
    count_changed<1>(moved, changed);
}

__device__ __forceinline__ uint32_t pp_hash(int32_t c) { return (static_cast<uint32_t>(c) * 2654435761u) >> 8; }
__device__ __forceinline__ uint32_t pp_class(int32_t c) { return (static_cast<uint32_t>(c) * 0x85EBCA6Bu) >> 10; }

// One wave (G = 64) or workgroup (G = 256) per queued row.  pool: the block's 4 slots tallies, then
// its 4 slots keys; a wave uses its quarter of both, a workgroup all of them.
template <bool DIST, int G>
__global__ void __launch_bounds__(kBlock) pp_vote_table(View recv, const void* __restrict__ cur, void* next, int32_t slots,
                                                        const int32_t* __restrict__ queue, int64_t count, u64* changed) {
    extern __shared__ u64 pp_pool[];
    __shared__ PpShared sh;
    const int gl = static_cast<int>(threadIdx.x & (G - 1));
    const int32_t m = G == 64 ? slots : slots * kWavesPerBlock;           // the group's table
    u64* const tal = pp_pool + (G == 64 ? (threadIdx.x >> 6) * slots : 0);
    int32_t* const key = reinterpret_cast<int32_t*>(pp_pool + slots * kWavesPerBlock) + (G == 64 ? (threadIdx.x >> 6) * slots : 0);
    const int64_t trips = group_trips<G>(0, count);
    u64 moved = 0;
    for (int64_t it = 0; it < trips; ++it) {
        const int32_t v = group_row<G>(it, recv, 0, 0, queue);
        int32_t ol;
        u64 os;
        vote_of<DIST>(cur, v, ol, os);
        if (DIST && os == 0) {                  // sends over no entry: stays (group-uniform)
            if (gl == 0) vote_store<DIST>(next, cur, v, ol);
            continue;
        }
        const Row w = row_of(recv, v);
        const int64_t l = w.len();
        group_sync<G>();                        // the table's last use is over
        for (int32_t i = gl; i < m; i += G) { tal[i] = 0; key[i] = -1; }
        group_sync<G>();
        // entry l is v's own vote
        bool over = false;
        int32_t lo = INT32_MAX, hi = -1;
        for (int64_t j = gl; j <= l; j += G) {
            int32_t c = ol;
            u64 s = os;
            if (j < l) vote_of<DIST>(cur, w.at(j), c, s);
            lo = min(lo, c);
            hi = max(hi, c);
            int32_t h = static_cast<int32_t>(pp_hash(c) % static_cast<uint32_t>(m));
            bool put = false;
            for (int32_t probe = 0; probe < m && !put; ++probe) {
                const int32_t old = atomicCAS(&key[h], -1, c);
                if (old == -1 || old == c) {
                    atomicAdd(&tal[h], s);
                    put = true;
                }
                h = h + 1 == m ? 0 : h + 1;
            }
            over = over || !put;
        }
        group_span<G>(over, lo, hi, sh);
        group_sync<G>();
        Best b{0, INT32_MAX};
        if (!over) {
            for (int32_t i = gl; i < m; i += G)
                if (key[i] >= 0) b.take(tal[i], key[i]);
        } else {
            // hashed classes: the row has at most l + 1 labels, so K classes leave a table half empty on average
            const uint32_t K = static_cast<uint32_t>((2 * (l + 1) + m - 1) / m);
            bool over2 = false;
            for (uint32_t k = 0; k < K; ++k) {
                group_sync<G>();
                for (int32_t i = gl; i < m; i += G) { tal[i] = 0; key[i] = -1; }
                group_sync<G>();
                for (int64_t j = gl; j <= l; j += G) {
                    int32_t c = ol;
                    u64 s = os;
                    if (j < l) vote_of<DIST>(cur, w.at(j), c, s);
                    if (pp_class(c) % K != k) continue;
                    int32_t h = static_cast<int32_t>(pp_hash(c) % static_cast<uint32_t>(m));
                    bool put = false;
                    for (int32_t probe = 0; probe < m && !put; ++probe) {
                        const int32_t old = atomicCAS(&key[h], -1, c);
                        if (old == -1 || old == c) {
                            atomicAdd(&tal[h], s);
                            put = true;
                        }
                        h = h + 1 == m ? 0 : h + 1;
                    }
                    over2 = over2 || !put;
                }
                group_sync<G>();
                for (int32_t i = gl; i < m; i += G)
                    if (key[i] >= 0) b.take(tal[i], key[i]);
            }
            int32_t lo2 = lo, hi2 = hi;
            group_span<G>(over2, lo2, hi2, sh);
            if (over2) {
                // a class outgrew the table: the labels span [lo, hi], class by class, direct-mapped
                b = Best{0, INT32_MAX};
                for (int64_t base = lo; base <= hi; base += m) {
                    group_sync<G>();
                    for (int32_t i = gl; i < m; i += G) tal[i] = 0;
                    group_sync<G>();
                    for (int64_t j = gl; j <= l; j += G) {
                        int32_t c = ol;
                        u64 s = os;
                        if (j < l) vote_of<DIST>(cur, w.at(j), c, s);
                        if (c >= base && c - base < m) atomicAdd(&tal[c - base], s);
                    }
                    group_sync<G>();
                    for (int32_t i = gl; i < m; i += G)
                        if (tal[i] != 0) b.take(tal[i], static_cast<int32_t>(base + i));      // (every vote is > 0)
                }
            }
        }
        b = group_best<G>(b, sh);
        if (gl == 0) {
            vote_store<DIST>(next, cur, v, b.c);
            moved += b.c != ol;
        }
    }
    count_changed<G>(moved, changed);
}

// ---------------------------------------------------------------- labels and their census
// label[v] = the Titan id of v's cluster; hist[rank] += 1 (hist zero before).
template <bool DIST>
__global__ void __launch_bounds__(kBlock) pp_finish(const void* __restrict__ cur, int64_t n, const int32_t* __restrict__ inv,
                                                    const int64_t* __restrict__ tid, int64_t* label, int32_t* hist) {
    for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < n; v += (int64_t)gridDim.x * blockDim.x) {
        int32_t c;
        u64 s;
        vote_of<DIST>(cur, static_cast<int32_t>(v), c, s);
        label[v] = tid[inv[c]];
        atomicAdd(&hist[c], 1);
    }
}

// *clusters += the non-empty clusters, *largest = the largest population: one atomic each per wave.
__global__ void __launch_bounds__(kBlock) pp_census(const int32_t* __restrict__ hist, int64_t n, u64* clusters, u64* largest) {
    u64 mine = 0, most = 0;
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
        const u64 h = static_cast<u64>(hist[r]);
        mine += h != 0;
        most = max(most, h);
    }
    mine = wave_sum(mine);
    most = wave_max(most);
    if (lane() == 0 && mine) {
        atomicAdd(clusters, mine);
        atomicMax(largest, most);
    }
}

inline int pp_wave_grid(int64_t rows) {
    return static_cast<int>(std::max<int64_t>(1, std::min<int64_t>((rows + kWavesPerBlock - 1) / kWavesPerBlock, 8192)));
}
inline int pp_block_grid(int64_t rows) { return static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(rows, 4096))); }

// tier 0: the rows in neither queue by their lanes; 1: the wave queue; 2: the block queue.
template <bool DIST>
hipError_t pp_round(const PpRun& r, bool first, int tier, const void* cur, void* next, Counters* cnt, hipStream_t s) {
    u64* const changed = &cnt->red[0];
    const size_t lds = static_cast<size_t>(r.slots) * kWavesPerBlock * (sizeof(u64) + sizeof(int32_t));
    if (tier == 0) {
        const int64_t lane_row = std::min(r.wave_row, r.block_row);     // shorter rows are in neither queue
        if (first) pp_first<DIST, 1><<<grid_for(r.n, 1 << 16), kBlock, 0, s>>>(r.recv, r.n, cur, next, lane_row, nullptr, 0, changed);
        else pp_vote_lane<DIST><<<grid_for(r.n, 1 << 16), kBlock, 0, s>>>(r.recv, r.n, cur, next, lane_row, changed);
    } else if (tier == 1 && r.nwave > 0) {
        if (first) pp_first<DIST, 64><<<pp_wave_grid(r.nwave), kBlock, 0, s>>>(r.recv, r.n, cur, next, 0, r.wq, r.nwave, changed);
        else pp_vote_table<DIST, 64><<<pp_wave_grid(r.nwave), kBlock, lds, s>>>(r.recv, cur, next, r.slots, r.wq, r.nwave, changed);
    } else if (tier == 2 && r.nblock > 0) {
        if (first) pp_first<DIST, 256><<<pp_block_grid(r.nblock), kBlock, 0, s>>>(r.recv, r.n, cur, next, 0, r.bq, r.nblock, changed);
        else pp_vote_table<DIST, 256><<<pp_block_grid(r.nblock), kBlock, lds, s>>>(r.recv, cur, next, r.slots, r.bq, r.nblock, changed);
    }
    return hipGetLastError();
}

}  // namespace

hipError_t k_pp_init(const PpRun& r, const View& send, const int32_t* rank, void* cur, Counters* cnt, hipStream_t s) {
    if (r.distribute)
        pp_init<true><<<grid_for(r.n, 2048), kBlock, 0, s>>>(r.recv, send, r.n, rank, cur, r.wave_row, r.block_row, r.wq,
                                                             &cnt->qlen, r.bq, &cnt->mf);
    else
        pp_init<false><<<grid_for(r.n, 2048), kBlock, 0, s>>>(r.recv, send, r.n, rank, cur, r.wave_row, r.block_row, r.wq,
                                                              &cnt->qlen, r.bq, &cnt->mf);
    return hipGetLastError();
}

hipError_t k_pp_round(const PpRun& r, bool first, int tier, const void* cur, void* next, Counters* cnt, hipStream_t s) {
    if (r.slots < kPpMinSlots || r.slots > kPpMaxSlots || tier < 0 || tier > 2) return hipErrorInvalidValue;
    return r.distribute ? pp_round<true>(r, first, tier, cur, next, cnt, s) : pp_round<false>(r, first, tier, cur, next, cnt, s);
}

hipError_t k_pp_finish(const PpRun& r, const void* cur, const int32_t* inv, const int64_t* tid, int64_t* label, int32_t* hist,
                       Counters* cnt, hipStream_t s) {
    if (r.distribute) pp_finish<true><<<grid_for(r.n, 2048), kBlock, 0, s>>>(cur, r.n, inv, tid, label, hist);
    else pp_finish<false><<<grid_for(r.n, 2048), kBlock, 0, s>>>(cur, r.n, inv, tid, label, hist);
    pp_census<<<grid_for(r.n, 2048), kBlock, 0, s>>>(hist, r.n, &cnt->qlen, &cnt->red[0]);
    return hipGetLastError();
}

}  // namespace tgo
