// tri_walk.hpp — the triangle enumeration over the forward lists, once, for every program that
// credits triangles (tri.hip: to their vertices; truss.hip: to their edges).
//
// The triangle a < b < c is found exactly once, at the oriented entry (c, b), as a member a of
// fwd(c) ∩ fwd(b) — and since a < b, only the entries of fwd(c) before b can match.  Both
// positions of a are known there.  Rows go to lanes by their forward length L, one wave per 64
// consecutive rows:
//   lane   L < wave_row            the row's own lane: two-pointer merge per entry b
//   wave   wave_row <= L           a whole wave: 64 entries of fwd(b) a trip, every lane a binary
//                                  search into fwd(c)[0, position of b)
//   block  block_row <= L <= LDS   a workgroup stages fwd(c) in LDS with one 32-bit counter per
//                                  entry, its waves take the b's of that row in turn, and the
//                                  counters are flushed once per row
// Internal ids are degree-grouped, so 64 consecutive rows are alike: a wave that walked its own 64
// long rows one after the other was the whole kernel's critical path.  tri_walk_lane therefore
// only queues the wave and block rows; tri_walk_wave / tri_walk_block draw them from the queues by
// ticket (one atomicAdd per row), so a long row never waits behind its neighbours.
//
// Where the credits land is the Credit policy's business (passed by value, three members):
//   other(e)                the (b, a) entry, at fadj index e: once per triangle
//   entry(cb, pos, id, m)   entry pos of row c (cb = foff[c], id = fadj[cb + pos]) earns m: one per
//                           triangle for a, their number per (c, b) for b — or, from the block
//                           path, the LDS counter of that entry once per row
//   apex(c, total)          row c's triangles: once per row (lane, wave) or per wave (block)
// All credits are integer atomics: the result does not depend on the row classes or on the order.
// No grid barrier, no spin.  Wave = 64 lanes.
#pragma once
#include "engine.hpp"
#include "wave.hpp"

namespace tgo {
namespace {

// The matches of fwd(b) in row[0, kb) by the calling wave (row = fwd(c) in global memory or in
// LDS, cb = foff[c], b = row[kb]); returns their number on every lane.  a and b are credited
// through the policy — or, with row_cnt (the LDS counters beside a staged row, flushed by the
// caller), there.
template <class Credit, class Ptr>
__device__ __forceinline__ u64 tri_walk_entry(Ptr row, int64_t cb, int64_t kb, int32_t b, const int64_t* __restrict__ foff,
                                              const int32_t* __restrict__ fadj, Credit credit, unsigned* row_cnt = nullptr) {
    const int64_t bb = foff[b], lb = foff[b + 1] - bb;
    u64 cnt = 0;
    for (int64_t k = lane(); k < lb; k += 64) {
        const int32_t x = fadj[bb + k];
        const int64_t pos = find(row, kb, x);
        if (pos >= 0) {
            credit.other(bb + k);
            if (row_cnt) atomicAdd(&row_cnt[pos], 1u);
            else credit.entry(cb, pos, x, 1);
            ++cnt;
        }
    }
    if (!__ballot(cnt != 0)) return 0;
    cnt = wave_sum(cnt);
    if (lane() == 0) {
        if (row_cnt) atomicAdd(&row_cnt[kb], static_cast<unsigned>(cnt));
        else credit.entry(cb, kb, b, cnt);
    }
    return cnt;
}

// Lane rows; wave rows are appended to wlist, block rows (block_row <= L <= lds_cap) to blist.
template <class Credit>
__global__ void __launch_bounds__(kBlock) tri_walk_lane(const int64_t* __restrict__ foff, const int32_t* __restrict__ fadj,
                                                        int64_t n, int64_t wave_row, int64_t block_row, int64_t lds_cap,
                                                        Credit credit, int32_t* blist, u64* bcount, int32_t* wlist,
                                                        u64* wcount) {
    for_each_row_64(n, [&](int64_t c, bool live) {
        int64_t cb = 0, L = 0;
        if (live) {
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
                        credit.entry(cb, i, x, 1);
                        credit.other(bb + j);
                        ++cnt;
                    }
                    const bool ai = x <= y, aj = y <= x;
                    if (ai) { if (++i >= kb) break; x = fadj[cb + i]; }
                    if (aj) { if (++j >= lb) break; y = fadj[bb + j]; }
                }
                if (cnt) {
                    credit.entry(cb, kb, b, cnt);
                    mine += cnt;
                }
            }
        }
        if (mine) credit.apex(static_cast<int32_t>(c), mine);
        wave_append(to_wave, static_cast<int32_t>(c), wlist, wcount);
        wave_append(to_block, static_cast<int32_t>(c), blist, bcount);
    });
}

// The queued wave rows, one row per wave and ticket.
template <class Credit>
__global__ void __launch_bounds__(kBlock) tri_walk_wave(const int64_t* __restrict__ foff, const int32_t* __restrict__ fadj,
                                                        const int32_t* __restrict__ wlist, const u64* __restrict__ wcount,
                                                        u64* ticket, Credit credit) {
    const u64 rows = *wcount;
    for (;;) {
        u64 r = 0;
        if (lane() == 0) r = atomicAdd(ticket, 1ULL);
        r = __shfl(r, 0, 64);
        if (r >= rows) return;
        const int32_t c = wlist[r];
        const int64_t cb = foff[c];
        const int32_t* const row = fadj + cb;
        const int64_t L = foff[c + 1] - cb;
        u64 total = 0;
        for (int64_t kb = 1; kb < L; ++kb) total += tri_walk_entry(row, cb, kb, row[kb], foff, fadj, credit);
        if (lane() == 0 && total) credit.apex(c, total);
    }
}

// The queued block rows: fwd(c) staged in LDS (L <= lds_cap; the launch's dynamic LDS holds lds_cap
// entries and as many 32-bit counters), the block's waves take its entries b in turn.  A counter
// stays below 2 L <= 2^15: entry k is matched at most once per later entry and credited as a
// middle vertex with at most k matches.
template <class Credit>
__global__ void __launch_bounds__(kBlock) tri_walk_block(const int64_t* __restrict__ foff, const int32_t* __restrict__ fadj,
                                                         const int32_t* __restrict__ blist, const u64* __restrict__ bcount,
                                                         u64* ticket, int64_t lds_cap, Credit credit) {
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
        const int64_t L = min(foff[c + 1] - cb, lds_cap);       // == the row's length: tri_walk_lane queued it
        for (int64_t k = threadIdx.x; k < L; k += kBlock) {
            s_row[k] = fadj[cb + k];
            s_cnt[k] = 0;
        }
        __syncthreads();
        u64 total = 0;
        for (int64_t kb = 1 + (threadIdx.x >> 6); kb < L; kb += kWavesPerBlock)
            total += tri_walk_entry(s_row, cb, kb, s_row[kb], foff, fadj, credit, s_cnt);
        if (lane() == 0 && total) credit.apex(c, total);
        __syncthreads();
        for (int64_t k = threadIdx.x; k < L; k += kBlock)
            if (const unsigned m = s_cnt[k]) credit.entry(cb, k, s_row[k], m);
        __syncthreads();
    }
}

// Every triangle of the forward lists credited once: the lane kernel, then the block rows (the
// longest first: the block kernel's tail is then the wave kernel's cover), then the wave rows.
// max_fwd = the longest forward row; blist / wlist = n entries each; q = 4 zeroed words (the two
// queues' lengths, then their tickets).
template <class Credit>
hipError_t tri_walk(const int64_t* foff, const int32_t* fadj, int64_t n, int64_t wave_row, int64_t block_row,
                    int64_t max_fwd, Credit credit, int32_t* blist, int32_t* wlist, u64* q, hipStream_t s) {
    // LDS entries of the block kernel: the longest row, at most kTriLdsEntries
    const int64_t cap = std::max<int64_t>(64, std::min<int64_t>(max_fwd, kTriLdsEntries));
    tri_walk_lane<<<grid_for(((n + 63) / 64) * 64, 1 << 20), kBlock, 0, s>>>(foff, fadj, n, wave_row, block_row, cap, credit,
                                                                             blist, &q[0], wlist, &q[1]);
    hipError_t e = hipGetLastError();
    const int blocks = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>((n + 63) / 64, 2048)));
    if (e == hipSuccess && block_row <= max_fwd) {              // else no row was queued
        const size_t lds = static_cast<size_t>(cap) * (sizeof(int32_t) + sizeof(unsigned));
        if (lds > 64 * 1024 && (e = raise_dynamic_lds<&tri_walk_block<Credit>>(lds)) != hipSuccess) return e;
        tri_walk_block<<<blocks, kBlock, lds, s>>>(foff, fadj, blist, &q[0], &q[2], cap, credit);
        e = hipGetLastError();
    }
    if (e == hipSuccess && wave_row <= max_fwd) {
        tri_walk_wave<<<blocks, kBlock, 0, s>>>(foff, fadj, wlist, &q[1], &q[3], credit);
        e = hipGetLastError();
    }
    return e;
}

}  // namespace
}  // namespace tgo
