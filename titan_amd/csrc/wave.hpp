// wave.hpp — the wave-level toolkit of the device code: launch geometry, xor-tree folds, the
// wave-aggregated queue append, sorted-row searches, the peel loops' minimum word, the
// lane-or-wave row split and the dynamic-LDS raise.  frontier.hpp includes it; the analytics
// programs (cc, tri, core, truss, scc, bc, pp, cl) include it alone.  Everything here is in an
// anonymous namespace, one copy per translation unit.  Wave = 64 lanes.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <cstdint>
#include <mutex>

namespace tgo {
namespace {

using u64 = unsigned long long;

constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / 64;

__device__ __forceinline__ int lane() { return static_cast<int>(threadIdx.x & 63); }

// Workgroups of kBlock threads for `work` items, at least one and at most cap.
inline int grid_for(int64_t work, int64_t cap) {
    const int64_t g = (work + kBlock - 1) / kBlock;
    return static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(g, cap)));
}

// Folds over the calling wave; the result on every lane.
template <class T>
__device__ __forceinline__ T wave_sum(T x) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d, 64);
    return x;
}
template <class T>
__device__ __forceinline__ T wave_max(T x) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const T y = __shfl_xor(x, d, 64);
        x = x < y ? y : x;
    }
    return x;
}
template <class T>
__device__ __forceinline__ T wave_min(T x) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const T y = __shfl_xor(x, d, 64);
        x = y < x ? y : x;
    }
    return x;
}

// The calling wave's lanes with `take` set append v to list (one atomicAdd on *count per wave).
// Every lane of the wave calls this together.
__device__ __forceinline__ void wave_append(bool take, int32_t v, int32_t* list, u64* count) {
    const u64 qm = __ballot(take);
    if (!qm) return;
    const int lead = __ffsll(static_cast<long long>(qm)) - 1;
    u64 base = 0;
    if (lane() == lead) base = atomicAdd(count, static_cast<u64>(__popcll(qm)));
    base = __shfl(base, lead, 64);
    if (take) list[base + __popcll(qm & ((1ULL << lane()) - 1))] = v;
}
// The same for a list of cap entries: an entry past cap is dropped and raises *err.
__device__ __forceinline__ void wave_append(bool take, int32_t v, int32_t* list, u64* count, u64 cap, u64* err) {
    const u64 qm = __ballot(take);
    if (!qm) return;
    const int lead = __ffsll(static_cast<long long>(qm)) - 1;
    u64 base = 0;
    if (lane() == lead) base = atomicAdd(count, static_cast<u64>(__popcll(qm)));
    base = __shfl(base, lead, 64);
    if (take) {
        const u64 slot = base + __popcll(qm & ((1ULL << lane()) - 1));
        if (slot < cap) list[slot] = v;
        else atomicMax(err, 1ULL);
    }
}

// First index of the sorted p[0, len) whose entry is >= x.
template <class Ptr>
__device__ __forceinline__ int64_t lower_bound(Ptr p, int64_t len, int32_t x) {
    int64_t lo = 0, hi = len;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (p[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// The position of x among the sorted p[0, len), -1 when it is not there.
template <class Ptr>
__device__ __forceinline__ int64_t find(Ptr p, int64_t len, int32_t x) {
    const int64_t lo = lower_bound(p, len, x);
    return lo < len && p[lo] == x ? lo : -1;
}

// A peel launch's smallest value above its level, as max(INT32_MAX - value) in *word (zeroed
// between rounds; the host's level_min decodes it).  Every lane of the wave calls this together.
__device__ __forceinline__ void publish_min(int mn, u64* word) {
    mn = wave_min(mn);
    if (lane() == 0 && mn != INT_MAX) atomicMax(word, static_cast<u64>(INT_MAX - mn));
}

// A row per lane, a long row by the whole wave.  Every lane of the wave calls this together:
// a lane without `wide` runs lane_body() (a lane that holds no row passes wide = false and a
// body that does nothing), then the wave runs wave_body(src) once per lane src that set `wide`,
// in lane order; wave_body fetches that lane's row with __shfl(x, src, 64).
template <class LaneBody, class WaveBody>
__device__ __forceinline__ void lane_or_wave(bool wide, LaneBody&& lane_body, WaveBody&& wave_body) {
    if (!wide) lane_body();
    u64 big = __ballot(wide);
    while (big) {                       // wave-uniform
        const int src = __ffsll(static_cast<long long>(big)) - 1;
        big &= big - 1;
        wave_body(src);
    }
}

// 64 consecutive rows of [0, n) to a wave, grid-strided: every lane of the grid's waves calls
// body(v, live) in the same trips, live = v names a row (so body may ballot and shuffle).
template <class Body>
__device__ __forceinline__ void for_each_row_64(int64_t n, Body&& body) {
    const int64_t words = (n + 63) >> 6;
    for (int64_t b = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock; b < words;
         b += static_cast<int64_t>(gridDim.x) * kWavesPerBlock) {
        const int64_t wd = b + (threadIdx.x >> 6);
        const int64_t v = (wd << 6) + lane();
        body(v, wd < words && v < n);
    }
}

// A kernel's dynamic LDS past 64 KB: its limit is raised to `bytes` unless an earlier call raised
// it that far (one `raised` per kernel; the ranks of an in-process partition launch from threads).
template <auto Kernel>
hipError_t raise_dynamic_lds(size_t bytes) {
    static std::mutex mu;
    static size_t raised = 0;
    std::lock_guard<std::mutex> lk(mu);
    if (bytes <= raised) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(bytes));
    if (e == hipSuccess) raised = bytes;
    return e;
}

}  // namespace
}  // namespace tgo
