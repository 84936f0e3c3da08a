// cl.hip — closeness and harmonic centrality on gfx950 (tgo_closeness): the fold of one multi-source
// sweep's state into per-vertex accumulators, and the finish.
//
// Contract: for a vertex v, over the seeds s != v that reach it, far = the sum of d(s, v), reach their
// number, ecc the largest d(s, v), harmonic = the sum of 1 / d(s, v) folded in a fixed order: the
// batches in order, within a batch the distinct levels L >= 1 present at v ascending,
// h = h + (double)c / (double)L with c the batch's sources at level L (IEEE fp64 division and addition).
//
// A sweep of up to 64 sources (msbfs.hip) leaves vis[v] = the mask of the sources that reached v and
// the level planes: bit r of plane k at v = bit k of source r's level at v (planes [0, nplanes) are
// valid; a source that did not reach v has zero bits).  cl_fold runs once per batch with one lane per
// internal vertex: it loads vis[v] and the nplanes plane words (coalesced, 8 bytes a lane each, kept in
// registers: NP is a template argument, so the array is never indexed at run time) and enumerates the
// distinct levels present at v in ascending order by bit-sliced minimum extraction: with rem the
// sources not yet taken, cand = rem, and from the top plane down, if some candidates have bit k clear
// (cand & ~plane_k != 0) the minimum has bit k clear and they are the candidates left; else bit k of
// the minimum is 1.  After plane 0, L is the smallest level in rem and cand the sources at it.  The
// cost per vertex is (distinct levels <= 64) x nplanes word operations, whatever the batch's depth: no
// loop over 1..depth, which a path-like graph would make quadratic.  Level 0 is a seed on itself and
// is skipped.  One lane owns one vertex: no atomics, and a vertex no source reached touches nothing.
// The accumulators stay on the device in internal order across the batches: far and reach u64, ecc
// i32 (a max across batches), harmonic f64 (its fold continues from the previous batch's value).
//
// cl_finish: closeness = (double)reach / (double)far (0.0 when far = 0) in internal order, and the
// block-reduced sum of reach and max of ecc into two counters (one atomic each per block).  cl_ecc_rows:
// ecc to row order as int64.  Wave = 64 lanes.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "engine.hpp"
#include "wave.hpp"

namespace tgo {
namespace {

template <int NP>
__global__ void __launch_bounds__(kBlock)
cl_fold(const uint64_t* __restrict__ vis, const uint64_t* __restrict__ planes, int64_t stride, int64_t n,
        u64* __restrict__ far, u64* __restrict__ reach, int32_t* __restrict__ ecc, double* __restrict__ harm) {
    for (int64_t v = blockIdx.x * static_cast<int64_t>(kBlock) + threadIdx.x; v < n;
         v += static_cast<int64_t>(gridDim.x) * kBlock) {
        uint64_t rem = vis[v];
        if (rem == 0) continue;
        uint64_t p[NP > 0 ? NP : 1];
#pragma unroll
        for (int k = 0; k < NP; ++k) p[k] = planes[k * stride + v];
        u64 f = 0, r = 0;
        int32_t e = 0;
        double h = harm[v];
        while (rem != 0) {
            uint64_t cand = rem;
            int32_t L = 0;
#pragma unroll
            for (int k = NP - 1; k >= 0; --k) {
                const uint64_t t = cand & ~p[k];
                if (t != 0) cand = t;
                else L |= 1 << k;
            }
            rem &= ~cand;
            if (L == 0) continue;           // a seed sitting on itself
            const int c = __popcll(cand);
            f += static_cast<u64>(c) * static_cast<u64>(L);
            r += static_cast<u64>(c);
            e = L;                          // the levels ascend: the last is the batch's deepest
            h = __dadd_rn(h, __ddiv_rn(static_cast<double>(c), static_cast<double>(L)));
        }
        if (r == 0) continue;               // seeds on themselves only
        far[v] += f;
        reach[v] += r;
        ecc[v] = max(ecc[v], e);
        harm[v] = h;
    }
}

__global__ void __launch_bounds__(kBlock)
cl_finish(const u64* __restrict__ far, const u64* __restrict__ reach, const int32_t* __restrict__ ecc, int64_t n,
          double* __restrict__ close, u64* __restrict__ pairs, u64* __restrict__ deepest) {
    u64 sum = 0, top = 0;
    for (int64_t v = blockIdx.x * static_cast<int64_t>(kBlock) + threadIdx.x; v < n;
         v += static_cast<int64_t>(gridDim.x) * kBlock) {
        const u64 f = far[v], r = reach[v];
        close[v] = f ? __ddiv_rn(static_cast<double>(r), static_cast<double>(f)) : 0.0;
        sum += r;
        top = max(top, static_cast<u64>(ecc[v]));
    }
    sum = wave_sum(sum);
    top = wave_max(top);
    __shared__ u64 ssum[kWavesPerBlock], stop[kWavesPerBlock];
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { ssum[w] = sum; stop[w] = top; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < kWavesPerBlock; ++i) { sum += ssum[i]; top = max(top, stop[i]); }
        if (sum) atomicAdd(pairs, sum);
        if (top) atomicMax(deepest, top);
    }
}

__global__ void cl_ecc_rows(const int32_t* __restrict__ ecc, const int32_t* __restrict__ perm, int64_t* __restrict__ out,
                            int64_t n) {
    for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < n;
         i += static_cast<int64_t>(gridDim.x) * blockDim.x)
        out[i] = ecc[perm[i]];
}

template <int NP>
hipError_t fold_planes(int nplanes, const uint64_t* vis, const uint64_t* planes, int64_t stride, int64_t n, u64* far,
                       u64* reach, int32_t* ecc, double* harm, hipStream_t s) {
    if (nplanes == NP) {
        cl_fold<NP><<<grid_for(n, 1 << 16), kBlock, 0, s>>>(vis, planes, stride, n, far, reach, ecc, harm);
        return hipGetLastError();
    }
    if constexpr (NP > 0) return fold_planes<NP - 1>(nplanes, vis, planes, stride, n, far, reach, ecc, harm, s);
    return hipErrorInvalidValue;
}

}  // namespace

hipError_t k_cl_fold(const uint64_t* vis, LevelPlanes lvl, int nplanes, int64_t n, unsigned long long* far,
                     unsigned long long* reach, int32_t* ecc, double* harm, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    return fold_planes<kLevelPlanes>(nplanes, vis, lvl.p, lvl.stride, n, far, reach, ecc, harm, s);
}

hipError_t k_cl_finish(const unsigned long long* far, const unsigned long long* reach, const int32_t* ecc, int64_t n,
                       double* close, unsigned long long* pairs, unsigned long long* deepest, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    cl_finish<<<grid_for(n, 1 << 16), kBlock, 0, s>>>(far, reach, ecc, n, close, pairs, deepest);
    return hipGetLastError();
}

hipError_t k_cl_ecc_rows(const int32_t* ecc, const int32_t* perm, int64_t* out, int64_t n, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    cl_ecc_rows<<<grid_for(n, 1 << 16), kBlock, 0, s>>>(ecc, perm, out, n);
    return hipGetLastError();
}

}  // namespace tgo
