// tri.hip — triangle counting and clustering coefficients on gfx950 (tgo_triangles).
//
// Contract: the simple undirected projection of a bothE load — u ~ v iff u != v and an OUT or IN
// entry of u names v (the lists are each other's transpose, so the relation is symmetric).
// tri[v] = pairs {a, b} of neighbours of v with a ~ b, deg[v] = |N(v)|, lcc[v] = 2 tri / (d (d-1)).
//
// Forward lists (built once per graph): fwd(v) = the sorted, duplicate-free neighbours u < v in
// INTERNAL ids.  Internal ids are degree-grouped, hottest first, so "smaller id" is nearly the
// low-degree -> high-degree orientation: a hub keeps few forward entries, and the longest
// forward row stays near sqrt(2 m) however long the hub's lists are.  Both rows of a vertex are
// sorted by internal id, so fwd(v) is a merge of the two rows' heads (entries < v) and costs
// |fwd(v)|, not the degree; only d(v) needs the whole rows (a lane's merge for a short pair of
// rows, the wave for a long one: unique OUT entries + unique IN entries that OUT does not hold).
//
// Count (tri_walk.hpp: the enumeration, its row classes and ticket queues): every triangle
// a < b < c is found once and credits its three vertices.  In the lane and wave paths tri[a] gets
// one 64-bit atomicAdd per triangle, tri[b] one per (c, b) with a match (a wave folds its lanes'
// matches first), tri[c] one per row (a register until the row ends).  Device atomics run
// memory-side and their rate, not the list traffic, bounded the first form of this kernel (every
// path took the same 4 G atomics/s at RMAT-24); the block path therefore credits a and b in LDS
// counters beside the staged row — a and b are both entries of fwd(c), the binary search returns
// a's position — and flushes them once per row: at most L + 1 global atomics for a row of L
// entries instead of one per triangle.
// All counts are integers: the result does not depend on the thresholds or on the order of the
// atomics.  No grid barrier, no spin.  Wave = 64 lanes.
#include <hip/hip_runtime.h>
#include "engine.hpp"
#include "tri_walk.hpp"

namespace tgo {
namespace {

constexpr int64_t kDegSerial = 64;      // OUT + IN entries up to which a lane counts d(v) itself

template <class Ptr>
__device__ __forceinline__ bool holds(Ptr p, int64_t len, int32_t x) { return find(p, len, x) >= 0; }

// Merge the sorted rows a[0, na) and b[0, nb) up to `limit` (exclusive): the number of distinct
// entries other than v; FILL: also written to dst in order.  all (optional): goes on to the rows'
// ends and counts every distinct entry other than v.
template <bool FILL>
__device__ __forceinline__ int64_t merge_rows(const int32_t* __restrict__ a, int64_t na, const int32_t* __restrict__ b,
                                              int64_t nb, int32_t v, int32_t* dst, int64_t* all) {
    int64_t i = 0, j = 0, below = 0, total = 0;
    int32_t last = -1;                  // ids are >= 0
    int32_t x = i < na ? a[i] : INT32_MAX, y = j < nb ? b[j] : INT32_MAX;
    for (;;) {
        const int32_t m = min(x, y);
        if (m == INT32_MAX || (!all && m >= v)) break;
        if (x == m) { ++i; x = i < na ? a[i] : INT32_MAX; }
        if (y == m) { ++j; y = j < nb ? b[j] : INT32_MAX; }
        if (m != last && m != v) {
            if (m < v) {
                if (FILL) dst[below] = m;
                ++below;
            }
            ++total;
        }
        last = m;
    }
    if (all) *all = total;
    return below;
}

// fcnt[v] = |fwd(v)| (fcnt[n] = 0 for the scan), deg[v] = d(v), *max_fwd = the longest forward row.
__global__ void __launch_bounds__(kBlock) tri_fwd_count(const int64_t* __restrict__ ooff, const int32_t* __restrict__ oadj,
                                                        const int64_t* __restrict__ ioff, const int32_t* __restrict__ iadj,
                                                        int64_t n, int64_t* fcnt, int64_t* deg, u64* max_fwd) {
    const int64_t words = (n + 63) >> 6;
    u64 longest = 0;
    for (int64_t b = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock; b < words;
         b += static_cast<int64_t>(gridDim.x) * kWavesPerBlock) {
        const int64_t wd = b + (threadIdx.x >> 6);
        const int64_t v = (wd << 6) + lane();
        const bool live = wd < words && v < n;
        int64_t ob = 0, na = 0, ib = 0, nb = 0;
        if (live) {
            ob = ooff[v]; na = ooff[v + 1] - ob;
            ib = ioff[v]; nb = ioff[v + 1] - ib;
        }
        const bool serial = na + nb <= kDegSerial;
        int64_t d = 0, f = 0;
        if (live) {
            if (serial) f = merge_rows<false>(oadj + ob, na, iadj + ib, nb, static_cast<int32_t>(v), nullptr, &d);
            else f = merge_rows<false>(oadj + ob, na, iadj + ib, nb, static_cast<int32_t>(v), nullptr, nullptr);
        }
        unsigned long long big = __ballot(live && !serial);
        while (big) {
            const int src = __ffsll(static_cast<long long>(big)) - 1;
            big &= big - 1;
            const int32_t vs = static_cast<int32_t>((wd << 6) + src);
            const int32_t* const A = oadj + __shfl(ob, src, 64);
            const int32_t* const B = iadj + __shfl(ib, src, 64);
            const int64_t la = __shfl(na, src, 64), lb = __shfl(nb, src, 64);
            u64 c = 0;
            for (int64_t k = lane(); k < la; k += 64) {
                const int32_t x = A[k];
                c += x != vs && (k == 0 || A[k - 1] != x);
            }
            for (int64_t k = lane(); k < lb; k += 64) {
                const int32_t x = B[k];
                c += x != vs && (k == 0 || B[k - 1] != x) && !holds(A, la, x);
            }
            c = wave_sum(c);
            if (lane() == src) d = static_cast<int64_t>(c);
        }
        if (live) {
            fcnt[v] = f;
            deg[v] = d;
            longest = max(longest, static_cast<u64>(f));
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) fcnt[n] = 0;
    longest = wave_max(longest);
    if (lane() == 0 && longest) atomicMax(max_fwd, longest);
}

__global__ void __launch_bounds__(kBlock) tri_fwd_fill(const int64_t* __restrict__ ooff, const int32_t* __restrict__ oadj,
                                                       const int64_t* __restrict__ ioff, const int32_t* __restrict__ iadj,
                                                       int64_t n, const int64_t* __restrict__ foff, int32_t* fadj) {
    for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < n; v += (int64_t)gridDim.x * blockDim.x) {
        const int64_t fb = foff[v];
        if (foff[v + 1] == fb) continue;
        const int64_t ob = ooff[v], ib = ioff[v];
        merge_rows<true>(oadj + ob, ooff[v + 1] - ob, iadj + ib, ioff[v + 1] - ib, static_cast<int32_t>(v), fadj + fb,
                         nullptr);
    }
}

// Triangle credits to vertices: tri[a], tri[b], tri[c] += 1 per triangle a < b < c.
struct VertexCredit {
    u64* tri;
    __device__ __forceinline__ void other(int64_t) const {}
    __device__ __forceinline__ void entry(int64_t, int64_t, int32_t id, u64 m) const { atomicAdd(&tri[id], m); }
    __device__ __forceinline__ void apex(int32_t c, u64 total) const { atomicAdd(&tri[c], total); }
};

// lcc, and the totals: tot[0] += sum tri, tot[1] += sum d (d - 1) / 2, tot[2] += sum d,
// tot[3] = max tri.
__global__ void __launch_bounds__(kBlock) tri_finish(const u64* __restrict__ tri, const int64_t* __restrict__ deg, int64_t n,
                                                     double* lcc, u64* tot) {
    u64 st = 0, sw = 0, sd = 0, mx = 0;
    for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < n; v += (int64_t)gridDim.x * blockDim.x) {
        const u64 t = tri[v];
        const u64 d = static_cast<u64>(deg[v]);
        lcc[v] = d < 2 ? 0.0 : static_cast<double>(2 * t) / static_cast<double>(d * (d - 1));
        st += t;
        sw += d < 2 ? 0 : d * (d - 1) / 2;
        sd += d;
        mx = max(mx, t);
    }
    st = wave_sum(st);
    sw = wave_sum(sw);
    sd = wave_sum(sd);
    mx = wave_max(mx);
    if (lane() == 0) {
        if (st) atomicAdd(&tot[0], st);
        if (sw) atomicAdd(&tot[1], sw);
        if (sd) atomicAdd(&tot[2], sd);
        if (mx) atomicMax(&tot[3], mx);
    }
}

}  // namespace

// ---------------------------------------------------------------- launchers
hipError_t k_tri_fwd_count(const DevCsr& out, const DevCsr& in, int64_t n, int64_t* fcnt, int64_t* deg,
                           unsigned long long* max_fwd, hipStream_t s) {
    tri_fwd_count<<<grid_for(((n + 63) / 64) * 64, 1 << 20), kBlock, 0, s>>>(out.off, out.adj, in.off, in.adj, n, fcnt, deg, max_fwd);
    return hipGetLastError();
}
hipError_t k_tri_fwd_fill(const DevCsr& out, const DevCsr& in, int64_t n, const int64_t* foff, int32_t* fadj,
                          hipStream_t s) {
    tri_fwd_fill<<<grid_for(n, 1 << 20), kBlock, 0, s>>>(out.off, out.adj, in.off, in.adj, n, foff, fadj);
    return hipGetLastError();
}
hipError_t k_tri_count(const int64_t* foff, const int32_t* fadj, int64_t n, int64_t wave_row, int64_t block_row,
                       int64_t max_fwd, int64_t* tri, int32_t* blist, int32_t* wlist, unsigned long long* q,
                       hipStream_t s) {
    return tri_walk(foff, fadj, n, wave_row, block_row, max_fwd, VertexCredit{reinterpret_cast<u64*>(tri)}, blist, wlist, q, s);
}
hipError_t k_tri_finish(const int64_t* tri, const int64_t* deg, int64_t n, double* lcc, unsigned long long* tot,
                        hipStream_t s) {
    tri_finish<<<grid_for(n, 2048), kBlock, 0, s>>>(reinterpret_cast<const u64*>(tri), deg, n, lcc, tot);
    return hipGetLastError();
}

}  // namespace tgo
