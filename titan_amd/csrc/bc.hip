// bc.hip — betweenness centrality on gfx950 (tgo_betweenness): Brandes' two sweeps per seed.
//
// Contract: over a bothE load, read as the simple undirected projection (u ~ v iff u != v and an OUT
// or IN entry of u names v) or as the directed graph (an arc u -> v iff an OUT entry of u names v).
// bc[v] = sum over the seeds s of delta_s(v), delta_s(v) = sum over t not in {s, v} reachable from s
// of sigma_st(v) / sigma_st; a shortest path is a sequence of vertices, so a parallel edge counts once.
//
// Per seed the driver has the BFS level of every vertex (int32, -1 unreached).  bc_level_count /
// bc_level_scatter bucket the reached vertices by level into one list with level offsets; a wave
// folds its lanes of one level into one integer atomic, so 64 consecutive internal ids of a level —
// degree-grouped, hence alike — stay side by side in the list, and the order of the waves' chunks
// inside a level is the only thing scheduling decides.  Nothing below depends on it:
//   bc_sigma (level L = 1..D)     sigma[v] = sum of sigma[u] over the distinct predecessors u of v
//                                 with level[u] == L - 1, in list order
//   bc_delta (level L = D-1..1)   delta[v] = sum over the distinct successors w with level[w] == L + 1
//                                 of (sigma[v] / sigma[w]) * (1 + delta[w]), in list order; bc[v] += delta[v]
// Both are pulls: a vertex reads its neighbours' finished values (written by earlier launches) and
// writes only its own, so there is no floating-point atomic (they execute memory-side, the bound
// that tri.hip's first form and the delta-stepping relaxations met) and every sum is folded in an
// order that the row alone fixes: results are bit-identical run to run.  delta is zero before the
// sweep, which is level D's value; level 0 holds the seed alone, which takes no credit, so its
// launch is not made.
//
// Rows: the undirected reading walks the simple adjacency (bc_adj_count / bc_adj_fill: the sorted
// distinct neighbours other than the vertex, merged once per graph from its two sorted rows); the
// directed reading walks the IN row (predecessors) and the OUT row (successors) as loaded — both are
// sorted by internal id, so a duplicate equals the entry before it and a self-loop equals v, and the
// kernel skips both (DEDUP).  A row shorter than wave_row is summed by its own lane; a longer one by
// its whole wave: lane j folds entries j, j + 64, ... in order, then a fixed xor tree over the 64
// partial sums.  The two paths order a sum differently: across wave_row values results agree within
// rounding, not bit for bit.  A sigma beyond the finite range raises Counters::err.
// No grid barrier, no spin.  Wave = 64 lanes.
#include <hip/hip_runtime.h>
#include "engine.hpp"
#include "wave.hpp"

namespace tgo {
namespace {

// The same value on every lane: fp64 addition commutes, so both sides of an exchange add alike.
__device__ __forceinline__ double wave_fold(double x) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d, 64);
    return x;
}

// ---------------------------------------------------------------- simple adjacency
// The distinct entries other than v of the sorted rows a[0, na) and b[0, nb), merged in order;
// FILL: written to dst.  Returns their number.
template <bool FILL>
__device__ __forceinline__ int64_t merge_simple(const int32_t* __restrict__ a, int64_t na, const int32_t* __restrict__ b,
                                                int64_t nb, int32_t v, int32_t* dst) {
    int64_t i = 0, j = 0, total = 0;
    int32_t last = -1;                  // ids are >= 0
    int32_t x = i < na ? a[i] : INT32_MAX, y = j < nb ? b[j] : INT32_MAX;
    for (;;) {
        const int32_t m = min(x, y);
        if (m == INT32_MAX) break;
        if (x == m) { ++i; x = i < na ? a[i] : INT32_MAX; }
        if (y == m) { ++j; y = j < nb ? b[j] : INT32_MAX; }
        if (m != last && m != v) {
            if (FILL) dst[total] = m;
            ++total;
        }
        last = m;
    }
    return total;
}

__global__ void __launch_bounds__(kBlock) bc_adj_count(const int64_t* __restrict__ ooff, const int32_t* __restrict__ oadj,
                                                       const int64_t* __restrict__ ioff, const int32_t* __restrict__ iadj,
                                                       int64_t n, int64_t* cnt, u64* longest) {
    u64 most = 0;
    for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v <= n; v += (int64_t)gridDim.x * blockDim.x) {
        if (v == n) { cnt[n] = 0; continue; }
        const int64_t ob = ooff[v], ib = ioff[v];
        const int64_t c = merge_simple<false>(oadj + ob, ooff[v + 1] - ob, iadj + ib, ioff[v + 1] - ib, static_cast<int32_t>(v), nullptr);
        cnt[v] = c;
        most = max(most, static_cast<u64>(c));
    }
    if (most) atomicMax(longest, most);
}

// soff is the scan of bc_adj_count's counts over the same rows: a row's merge writes exactly its share.
__global__ void __launch_bounds__(kBlock) bc_adj_fill(const int64_t* __restrict__ ooff, const int32_t* __restrict__ oadj,
                                                      const int64_t* __restrict__ ioff, const int32_t* __restrict__ iadj,
                                                      int64_t n, const int64_t* __restrict__ soff, int32_t* sadj) {
    for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < n; v += (int64_t)gridDim.x * blockDim.x) {
        const int64_t sb = soff[v];
        if (soff[v + 1] == sb) continue;
        const int64_t ob = ooff[v], ib = ioff[v];
        merge_simple<true>(oadj + ob, ooff[v + 1] - ob, iadj + ib, ioff[v + 1] - ib, static_cast<int32_t>(v), sadj + sb);
    }
}

// ---------------------------------------------------------------- level buckets
// hist[l] += the vertices of level l (hist zero before): one atomic per level a wave holds.  A level
// past depth raises *err (the driver's depth comes from the same BFS).
__global__ void __launch_bounds__(kBlock) bc_level_count(const int32_t* __restrict__ level, int64_t n, int32_t depth,
                                                         u64* hist, u64* err) {
    const int64_t span = (n + 63) & ~int64_t(63);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < span; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t l = i < n ? level[i] : -1;
        if (l > depth) atomicMax(err, 1ULL);
        const bool has = l >= 0 && l <= depth;
        u64 todo = __ballot(has);
        while (todo) {                  // wave-uniform
            const int lead = __ffsll(static_cast<long long>(todo)) - 1;
            const int32_t ll = __shfl(l, lead, 64);
            const u64 same = __ballot(has && l == ll);
            if (lane() == lead) atomicAdd(&hist[ll], static_cast<u64>(__popcll(same)));
            todo &= ~same;
        }
    }
}

// order[cursor[l]++] = v for every vertex of level l (cursor = the levels' offsets before), a wave's
// lanes of one level side by side in lane order.  A slot at or past n raises *err and is not written.
__global__ void __launch_bounds__(kBlock) bc_level_scatter(const int32_t* __restrict__ level, int64_t n, int32_t depth,
                                                           u64* cursor, int32_t* order, u64* err) {
    const int64_t span = (n + 63) & ~int64_t(63);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < span; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t l = i < n ? level[i] : -1;
        const bool has = l >= 0 && l <= depth;
        u64 todo = __ballot(has);
        while (todo) {                  // wave-uniform
            const int lead = __ffsll(static_cast<long long>(todo)) - 1;
            const int32_t ll = __shfl(l, lead, 64);
            const u64 same = __ballot(has && l == ll);
            u64 base = 0;
            if (lane() == lead) base = atomicAdd(&cursor[ll], static_cast<u64>(__popcll(same)));
            base = __shfl(base, lead, 64);
            if (has && l == ll) {
                const u64 slot = base + __popcll(same & ((1ULL << lane()) - 1));
                if (slot < static_cast<u64>(n)) order[slot] = static_cast<int32_t>(i);
                else atomicMax(err, 1ULL);
            }
            todo &= ~same;
        }
    }
}

__global__ void bc_seed(double* sigma, int32_t seed) {
    if (blockIdx.x == 0 && threadIdx.x == 0) sigma[seed] = 1.0;
}

// ---------------------------------------------------------------- the sweeps
// The wide rows are queued with wave_append: a level's slice names a vertex once, so the queue
// (n + 1 entries) cannot overflow.

// The fold of f(tag, u) over the entries u of v's row adj[b, b + l) by one lane, in list order.
// DEDUP: an entry equal to the one before it or to v is skipped.
template <bool DEDUP, class F>
__device__ __forceinline__ double lane_fold(int32_t v, double tag, int64_t b, int64_t l, const int32_t* __restrict__ adj,
                                            F&& f) {
    double acc = 0.0;
    int32_t prev = -1;                  // ids are >= 0
    for (int64_t j = 0; j < l; ++j) {
        const int32_t u = adj[b + j];
        if (!DEDUP || (u != prev && u != v)) acc += f(tag, u);
        prev = u;
    }
    return acc;
}

// The same fold by the calling wave (every lane calls with the same row): lane j folds entries j,
// j + 64, ... in order, then the xor tree; the result on every lane.  kBcUnroll entries of a lane
// are loaded before the first is added — the adds keep their order — so a hub's row is not one
// memory latency per 64 entries; g is f without a branch around its loads (a skipped entry adds 0.0).
constexpr int kBcUnroll = 8;
template <bool DEDUP, class G>
__device__ __forceinline__ double wave_row_fold(int32_t v, double tag, int64_t b, int64_t l, const int32_t* __restrict__ adj,
                                                G&& g) {
    double part = 0.0;
    int64_t j = lane();
    for (; j + 64 * (kBcUnroll - 1) < l; j += 64 * kBcUnroll) {
        int32_t u[kBcUnroll];
        double t[kBcUnroll];
#pragma unroll
        for (int k = 0; k < kBcUnroll; ++k) u[k] = adj[b + j + 64 * k];
#pragma unroll
        for (int k = 0; k < kBcUnroll; ++k) {
            const int64_t at = j + 64 * k;
            const bool skip = DEDUP && (u[k] == v || (at > 0 && adj[b + at - 1] == u[k]));
            const double x = g(tag, u[k]);
            t[k] = skip ? 0.0 : x;
        }
#pragma unroll
        for (int k = 0; k < kBcUnroll; ++k) part += t[k];
    }
    for (; j < l; j += 64) {
        const int32_t u = adj[b + j];
        const bool skip = DEDUP && (u == v || (j > 0 && adj[b + j - 1] == u));
        const double x = g(tag, u);
        part += skip ? 0.0 : x;
    }
    return wave_fold(part);
}

__device__ __forceinline__ void sigma_store(double* sigma, int32_t v, double s, u64* err) {
    sigma[v] = s;
    if (!(s <= 1.7976931348623157e308)) atomicMax(err, 1ULL);   // inf (or the NaN an inf would breed)
}

// sigma of the vertices list[0, len), all of level L, from their predecessors' rows (off, adj): a
// row shorter than wave_row by its lane; the others are queued (*qcount zero before) for bc_sigma_wave.
template <bool DEDUP>
__global__ void __launch_bounds__(kBlock) bc_sigma(const int32_t* __restrict__ list, int64_t len,
                                                   const int64_t* __restrict__ off, const int32_t* __restrict__ adj,
                                                   const int32_t* __restrict__ level, int32_t L, double* sigma,
                                                   int64_t wave_row, int32_t* queue, u64* qcount, u64* err) {
    const int64_t span = (len + 63) & ~int64_t(63);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < span; i += (int64_t)gridDim.x * blockDim.x) {
        const bool has = i < len;
        const int32_t v = has ? list[i] : 0;
        int64_t b = 0, l = 0;
        if (has) {
            b = off[v];
            l = off[v + 1] - b;
        }
        const bool wide = has && l >= wave_row;
        if (has && !wide)
            sigma_store(sigma, v, lane_fold<DEDUP>(v, 0.0, b, l, adj, [&](double, int32_t u) {
                return level[u] == L - 1 ? sigma[u] : 0.0;
            }), err);
        wave_append(wide, v, queue, qcount);
    }
}

// One wave per queued row.
template <bool DEDUP>
__global__ void __launch_bounds__(kBlock) bc_sigma_wave(const int32_t* __restrict__ queue, const u64* __restrict__ qcount,
                                                        const int64_t* __restrict__ off, const int32_t* __restrict__ adj,
                                                        const int32_t* __restrict__ level, int32_t L, double* sigma,
                                                        u64* err) {
    const int64_t count = static_cast<int64_t>(*qcount);
    for (int64_t r = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6); r < count;
         r += static_cast<int64_t>(gridDim.x) * kWavesPerBlock) {
        const int32_t v = queue[r];
        const int64_t b = off[v], l = off[v + 1] - b;
        const double s = wave_row_fold<DEDUP>(v, 0.0, b, l, adj, [&](double, int32_t u) {
            const int32_t lu = level[u];
            const double x = sigma[u];          // (an unreached vertex's word is read and dropped)
            return lu == L - 1 ? x : 0.0;
        });
        if (lane() == 0) sigma_store(sigma, v, s, err);
    }
}

// delta of the vertices list[0, len), all of level L >= 1, from their successors' rows; bc += delta.
template <bool DEDUP>
__global__ void __launch_bounds__(kBlock) bc_delta(const int32_t* __restrict__ list, int64_t len,
                                                   const int64_t* __restrict__ off, const int32_t* __restrict__ adj,
                                                   const int32_t* __restrict__ level, int32_t L,
                                                   const double* __restrict__ sigma, double* delta, double* bc,
                                                   int64_t wave_row, int32_t* queue, u64* qcount) {
    const int64_t span = (len + 63) & ~int64_t(63);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < span; i += (int64_t)gridDim.x * blockDim.x) {
        const bool has = i < len;
        const int32_t v = has ? list[i] : 0;
        int64_t b = 0, l = 0;
        if (has) {
            b = off[v];
            l = off[v + 1] - b;
        }
        const bool wide = has && l >= wave_row;
        if (has && !wide) {
            const double d = lane_fold<DEDUP>(v, sigma[v], b, l, adj, [&](double s, int32_t w) {
                return level[w] == L + 1 ? (s / sigma[w]) * (1.0 + delta[w]) : 0.0;
            });
            delta[v] = d;
            bc[v] += d;
        }
        wave_append(wide, v, queue, qcount);
    }
}

template <bool DEDUP>
__global__ void __launch_bounds__(kBlock) bc_delta_wave(const int32_t* __restrict__ queue, const u64* __restrict__ qcount,
                                                        const int64_t* __restrict__ off, const int32_t* __restrict__ adj,
                                                        const int32_t* __restrict__ level, int32_t L,
                                                        const double* __restrict__ sigma, double* delta, double* bc) {
    const int64_t count = static_cast<int64_t>(*qcount);
    for (int64_t r = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6); r < count;
         r += static_cast<int64_t>(gridDim.x) * kWavesPerBlock) {
        const int32_t v = queue[r];
        const int64_t b = off[v], l = off[v + 1] - b;
        const double d = wave_row_fold<DEDUP>(v, sigma[v], b, l, adj, [&](double s, int32_t w) {
            const int32_t lw = level[w];
            const double sw = sigma[w], dw = delta[w];  // (read and dropped for a vertex of another level)
            return lw == L + 1 ? (s / sw) * (1.0 + dw) : 0.0;
        });
        if (lane() == 0) {
            delta[v] = d;
            bc[v] += d;
        }
    }
}

}  // namespace

hipError_t k_bc_adj_count(const DevCsr& out, const DevCsr& in, int64_t n, int64_t* cnt, unsigned long long* longest,
                          hipStream_t s) {
    bc_adj_count<<<grid_for(n + 1, 1 << 16), kBlock, 0, s>>>(out.off, out.adj, in.off, in.adj, n, cnt, longest);
    return hipGetLastError();
}
hipError_t k_bc_adj_fill(const DevCsr& out, const DevCsr& in, int64_t n, const int64_t* soff, int32_t* sadj,
                         hipStream_t s) {
    bc_adj_fill<<<grid_for(n, 1 << 16), kBlock, 0, s>>>(out.off, out.adj, in.off, in.adj, n, soff, sadj);
    return hipGetLastError();
}
hipError_t k_bc_level_count(const int32_t* level, int64_t n, int32_t depth, int64_t* hist, Counters* cnt, hipStream_t s) {
    bc_level_count<<<grid_for(n, 2048), kBlock, 0, s>>>(level, n, depth, reinterpret_cast<u64*>(hist), &cnt->err);
    return hipGetLastError();
}
hipError_t k_bc_level_scatter(const int32_t* level, int64_t n, int32_t depth, int64_t* cursor, int32_t* order,
                              Counters* cnt, hipStream_t s) {
    bc_level_scatter<<<grid_for(n, 2048), kBlock, 0, s>>>(level, n, depth, reinterpret_cast<u64*>(cursor), order, &cnt->err);
    return hipGetLastError();
}
hipError_t k_bc_seed(double* sigma, int32_t seed, hipStream_t s) {
    bc_seed<<<1, 64, 0, s>>>(sigma, seed);
    return hipGetLastError();
}
// waves of the queued rows' launch: one per row of the slice at most
inline int bc_wave_grid(int64_t len) {
    return static_cast<int>(std::max<int64_t>(1, std::min<int64_t>((len + kWavesPerBlock - 1) / kWavesPerBlock, 8192)));
}
hipError_t k_bc_sigma(const int32_t* list, int64_t len, const int64_t* off, const int32_t* adj, bool dedup,
                      const int32_t* level, int32_t L, double* sigma, int64_t wave_row, int32_t* queue, int64_t* qcount,
                      bool long_rows, Counters* cnt, hipStream_t s) {
    if (len <= 0) return hipSuccess;
    u64* const qc = reinterpret_cast<u64*>(qcount);
    if (dedup) bc_sigma<true><<<grid_for(len, 1 << 16), kBlock, 0, s>>>(list, len, off, adj, level, L, sigma, wave_row, queue, qc, &cnt->err);
    else bc_sigma<false><<<grid_for(len, 1 << 16), kBlock, 0, s>>>(list, len, off, adj, level, L, sigma, wave_row, queue, qc, &cnt->err);
    if (!long_rows) return hipGetLastError();
    if (dedup) bc_sigma_wave<true><<<bc_wave_grid(len), kBlock, 0, s>>>(queue, qc, off, adj, level, L, sigma, &cnt->err);
    else bc_sigma_wave<false><<<bc_wave_grid(len), kBlock, 0, s>>>(queue, qc, off, adj, level, L, sigma, &cnt->err);
    return hipGetLastError();
}
hipError_t k_bc_delta(const int32_t* list, int64_t len, const int64_t* off, const int32_t* adj, bool dedup,
                      const int32_t* level, int32_t L, const double* sigma, double* delta, double* bc, int64_t wave_row,
                      int32_t* queue, int64_t* qcount, bool long_rows, hipStream_t s) {
    if (len <= 0) return hipSuccess;
    u64* const qc = reinterpret_cast<u64*>(qcount);
    if (dedup) bc_delta<true><<<grid_for(len, 1 << 16), kBlock, 0, s>>>(list, len, off, adj, level, L, sigma, delta, bc, wave_row, queue, qc);
    else bc_delta<false><<<grid_for(len, 1 << 16), kBlock, 0, s>>>(list, len, off, adj, level, L, sigma, delta, bc, wave_row, queue, qc);
    if (!long_rows) return hipGetLastError();
    if (dedup) bc_delta_wave<true><<<bc_wave_grid(len), kBlock, 0, s>>>(queue, qc, off, adj, level, L, sigma, delta, bc);
    else bc_delta_wave<false><<<bc_wave_grid(len), kBlock, 0, s>>>(queue, qc, off, adj, level, L, sigma, delta, bc);
    return hipGetLastError();
}

}  // namespace tgo
