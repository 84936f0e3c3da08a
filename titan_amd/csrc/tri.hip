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
// Count: the triangle a < b < c is found exactly once, at the oriented entry (c, b), as a member a
// of fwd(c) ∩ fwd(b) — and since a < b, only the entries of fwd(c) before b can match.  In the
// lane and wave paths tri[a] gets one 64-bit atomicAdd per triangle, tri[b] one per (c, b) with a
// match (a wave folds its lanes' matches first), tri[c] one per row (a register until the row
// ends).  Device atomics run memory-side and their rate, not the list traffic, bounded the first
// form of this kernel (every path took the same 4 G atomics/s at RMAT-24); the block path
// therefore credits a and b in LDS counters beside the staged row — a and b are both entries of
// fwd(c), the binary search returns a's position — and flushes them once per row: at most L + 1
// global atomics for a row of L entries instead of one per triangle.  Rows go to lanes by
// their forward length L, one wave per 64 consecutive rows as cc_hook / bu_step / ms_pull:
//   lane   L < wave_row            the row's own lane: two-pointer merge per entry b
//   wave   wave_row <= L           a whole wave: 64 entries of fwd(b) a trip, every lane a binary
//                                  search into fwd(c)[0, position of b)
//   block  block_row <= L <= LDS   a workgroup stages fwd(c) in LDS, its waves take the b's of that
//                                  row in turn
// Internal ids are degree-grouped, so 64 consecutive rows are alike: a wave that walked its own 64
// long rows one after the other was the whole kernel's critical path.  tri_count therefore only
// queues the wave and block rows; tri_count_wave / tri_count_block draw them from the queues by
// ticket (one atomicAdd per row), so a long row never waits behind its neighbours.
// All counts are integers: the result does not depend on the thresholds or on the order of the
// atomics.  No grid barrier, no spin.  Wave = 64 lanes.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <mutex>
#include <vector>
#include "frontier.hpp"

namespace tgo {
namespace {

constexpr int64_t kDegSerial = 64;      // OUT + IN entries up to which a lane counts d(v) itself
using u64 = unsigned long long;

inline int tri_grid(int64_t work, int64_t cap = 1 << 20) {
    const int64_t g = (work + kBlock - 1) / kBlock;
    return static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(g, cap)));
}

__device__ __forceinline__ u64 wave_sum_u64(u64 x) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d, 64);
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
            c = wave_sum_u64(c);
            if (lane() == src) d = static_cast<int64_t>(c);
        }
        if (live) {
            fcnt[v] = f;
            deg[v] = d;
            longest = max(longest, static_cast<u64>(f));
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) fcnt[n] = 0;
#pragma unroll
    for (int dd = 32; dd > 0; dd >>= 1) longest = max(longest, static_cast<u64>(__shfl_xor(longest, dd, 64)));
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

// The matches of fwd(b) in row[0, kb) by the calling wave (row = fwd(c) in global memory or in
// LDS), b = row[kb]; returns their number on every lane.  Credits: tri[a] += 1 per match and
// tri[b] += their number — or, with row_cnt (LDS counters beside a staged row, flushed by the
// caller), row_cnt[position of a] += 1 and row_cnt[kb] += their number.
template <class Ptr>
__device__ __forceinline__ u64 wave_entry(Ptr row, int64_t kb, int32_t b, const int64_t* __restrict__ foff,
                                          const int32_t* __restrict__ fadj, u64* tri, unsigned* row_cnt = nullptr) {
    const int64_t bb = foff[b], lb = foff[b + 1] - bb;
    u64 cnt = 0;
    for (int64_t k = lane(); k < lb; k += 64) {
        const int32_t x = fadj[bb + k];
        const int64_t pos = find(row, kb, x);
        if (pos >= 0) {
            if (row_cnt) atomicAdd(&row_cnt[pos], 1u);
            else atomicAdd(&tri[x], 1ULL);
            ++cnt;
        }
    }
    if (!__ballot(cnt != 0)) return 0;
    cnt = wave_sum_u64(cnt);
    if (lane() == 0) {
        if (row_cnt) atomicAdd(&row_cnt[kb], static_cast<unsigned>(cnt));
        else atomicAdd(&tri[b], cnt);
    }
    return cnt;
}

// The calling wave's lanes with `take` set append v to list (one atomicAdd on *count per wave).
__device__ __forceinline__ void wave_append(bool take, int32_t v, int32_t* list, u64* count) {
    const unsigned long long qm = __ballot(take);
    if (!qm) return;
    const int lead = __ffsll(static_cast<long long>(qm)) - 1;
    u64 base = 0;
    if (lane() == lead) base = atomicAdd(count, static_cast<u64>(__popcll(qm)));
    base = __shfl(base, lead, 64);
    if (take) list[base + __popcll(qm & ((1ULL << lane()) - 1))] = v;
}

// Lane rows; wave rows are appended to wlist, block rows (block_row <= L <= lds_cap) to blist.
__global__ void __launch_bounds__(kBlock) tri_count(const int64_t* __restrict__ foff, const int32_t* __restrict__ fadj,
                                                    int64_t n, int64_t wave_row, int64_t block_row, int64_t lds_cap,
                                                    u64* tri, int32_t* blist, u64* bcount, int32_t* wlist, u64* wcount) {
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
        u64 mine = 0;
        if (!to_block && !to_wave && L >= 2) {
            for (int64_t kb = 1; kb < L; ++kb) {
                const int32_t b = fadj[cb + kb];
                const int64_t bb = foff[b], lb = foff[b + 1] - bb;
                if (lb == 0) continue;
                int64_t i = 0, j = 0;
                int32_t x = fadj[cb], y = fadj[bb];
                u64 cnt = 0;
                for (;;) {
                    if (x == y) {
                        atomicAdd(&tri[x], 1ULL);
                        ++cnt;
                    }
                    const bool ai = x <= y, aj = y <= x;
                    if (ai) { if (++i >= kb) break; x = fadj[cb + i]; }
                    if (aj) { if (++j >= lb) break; y = fadj[bb + j]; }
                }
                if (cnt) {
                    atomicAdd(&tri[b], cnt);
                    mine += cnt;
                }
            }
        }
        if (mine) atomicAdd(&tri[c], mine);
        wave_append(to_wave, static_cast<int32_t>(c), wlist, wcount);
        wave_append(to_block, static_cast<int32_t>(c), blist, bcount);
    }
}

// The queued wave rows, one row per wave and ticket.
__global__ void __launch_bounds__(kBlock) tri_count_wave(const int64_t* __restrict__ foff, const int32_t* __restrict__ fadj,
                                                         const int32_t* __restrict__ wlist, const u64* __restrict__ wcount,
                                                         u64* ticket, u64* tri) {
    const u64 rows = *wcount;
    for (;;) {
        u64 r = 0;
        if (lane() == 0) r = atomicAdd(ticket, 1ULL);
        r = __shfl(r, 0, 64);
        if (r >= rows) return;
        const int32_t c = wlist[r];
        const int32_t* const row = fadj + foff[c];
        const int64_t L = foff[c + 1] - foff[c];
        u64 total = 0;
        for (int64_t kb = 1; kb < L; ++kb) total += wave_entry(row, kb, row[kb], foff, fadj, tri);
        if (lane() == 0 && total) atomicAdd(&tri[c], total);
    }
}

// The queued rows: fwd(c) staged in LDS (L <= lds_cap; the launch's dynamic LDS holds lds_cap
// entries and as many 32-bit counters), the block's waves take its entries b in turn.  A counter
// stays below 2 L <= 2^15: entry k is matched at most once per later entry and credited as a
// middle vertex with at most k matches.
__global__ void __launch_bounds__(kBlock) tri_count_block(const int64_t* __restrict__ foff, const int32_t* __restrict__ fadj,
                                                          const int32_t* __restrict__ blist, const u64* __restrict__ bcount,
                                                          u64* ticket, int64_t lds_cap, u64* tri) {
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
        const int64_t L = min(foff[c + 1] - cb, lds_cap);       // == the row's length: tri_count queued it
        for (int64_t k = threadIdx.x; k < L; k += kBlock) {
            s_row[k] = fadj[cb + k];
            s_cnt[k] = 0;
        }
        __syncthreads();
        u64 total = 0;
        for (int64_t kb = 1 + (threadIdx.x >> 6); kb < L; kb += kWavesPerBlock)
            total += wave_entry(s_row, kb, s_row[kb], foff, fadj, tri, s_cnt);
        if (lane() == 0 && total) atomicAdd(&tri[c], total);
        __syncthreads();
        for (int64_t k = threadIdx.x; k < L; k += kBlock)
            if (const unsigned m = s_cnt[k]) atomicAdd(&tri[s_row[k]], static_cast<u64>(m));
        __syncthreads();
    }
}

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
    st = wave_sum_u64(st);
    sw = wave_sum_u64(sw);
    sd = wave_sum_u64(sd);
#pragma unroll
    for (int dd = 32; dd > 0; dd >>= 1) mx = max(mx, static_cast<u64>(__shfl_xor(mx, dd, 64)));
    if (lane() == 0) {
        if (st) atomicAdd(&tot[0], st);
        if (sw) atomicAdd(&tot[1], sw);
        if (sd) atomicAdd(&tot[2], sd);
        if (mx) atomicMax(&tot[3], mx);
    }
}

// dynamic LDS past 64 KB, raised once (spmv.hip big_lds)
hipError_t tri_big_lds(size_t lds) {
    static std::mutex mu;
    static size_t raised = 0;
    std::lock_guard<std::mutex> lk(mu);
    if (lds <= raised) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&tri_count_block),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
    if (e == hipSuccess) raised = lds;
    return e;
}

}  // namespace

// ---------------------------------------------------------------- launchers
hipError_t k_tri_fwd_count(const DevCsr& out, const DevCsr& in, int64_t n, int64_t* fcnt, int64_t* deg,
                           unsigned long long* max_fwd, hipStream_t s) {
    tri_fwd_count<<<tri_grid(((n + 63) / 64) * 64), kBlock, 0, s>>>(out.off, out.adj, in.off, in.adj, n, fcnt, deg, max_fwd);
    return hipGetLastError();
}
hipError_t k_tri_fwd_fill(const DevCsr& out, const DevCsr& in, int64_t n, const int64_t* foff, int32_t* fadj,
                          hipStream_t s) {
    tri_fwd_fill<<<tri_grid(n), kBlock, 0, s>>>(out.off, out.adj, in.off, in.adj, n, foff, fadj);
    return hipGetLastError();
}
hipError_t k_tri_count(const int64_t* foff, const int32_t* fadj, int64_t n, int64_t wave_row, int64_t block_row,
                       int64_t max_fwd, int64_t* tri, int32_t* blist, int32_t* wlist, unsigned long long* q,
                       hipStream_t s) {
    // LDS entries of the block kernel: the longest row, at most kTriLdsEntries
    const int64_t cap = std::max<int64_t>(64, std::min<int64_t>(max_fwd, kTriLdsEntries));
    u64* const t = reinterpret_cast<u64*>(tri);
    tri_count<<<tri_grid(((n + 63) / 64) * 64), kBlock, 0, s>>>(foff, fadj, n, wave_row, block_row, cap, t, blist,
                                                               &q[0], wlist, &q[1]);
    hipError_t e = hipGetLastError();
    // the longest rows first: the block kernel's tail is then the wave kernel's cover
    const int blocks = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>((n + 63) / 64, 2048)));
    if (e == hipSuccess && block_row <= max_fwd) {              // else no row was queued
        const size_t lds = static_cast<size_t>(cap) * (sizeof(int32_t) + sizeof(unsigned));
        if (lds > 64 * 1024 && (e = tri_big_lds(lds)) != hipSuccess) return e;
        tri_count_block<<<blocks, kBlock, lds, s>>>(foff, fadj, blist, &q[0], &q[2], cap, t);
        e = hipGetLastError();
    }
    if (e == hipSuccess && wave_row <= max_fwd) {
        tri_count_wave<<<blocks, kBlock, 0, s>>>(foff, fadj, wlist, &q[1], &q[3], t);
        e = hipGetLastError();
    }
    return e;
}
hipError_t k_tri_finish(const int64_t* tri, const int64_t* deg, int64_t n, double* lcc, unsigned long long* tot,
                        hipStream_t s) {
    tri_finish<<<tri_grid(n, 2048), kBlock, 0, s>>>(reinterpret_cast<const u64*>(tri), deg, n, lcc, tot);
    return hipGetLastError();
}

}  // namespace tgo
