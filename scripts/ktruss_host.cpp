// Host side of scripts/ktruss_bench.py: a multi-threaded k-truss decomposition over the same simple
// undirected projection as tgo_ktruss, from its sorted adjacency (off, adj: scripts/kcore_host.cpp
// builds it from a loaded bothE graph's lists).  The peel is the PKT scheme (Kabir and Madduri,
// "Shared-memory graph truss decomposition"): level by level, every thread scans its share of the
// alive edges for those at the level; a sub-round intersects the endpoints' rows of every frontier
// edge and lowers the two other edges of each triangle that is still there (the smaller frontier
// edge of a triangle with two of them lowers the third), the edges that reach the level form the
// next sub-round, and the threads meet at a barrier between sub-rounds.  Built by the script:
//   g++ -O3 -std=c++17 -shared -fPIC -pthread scripts/ktruss_host.cpp -o scripts/libktruss_host.so
#include <pthread.h>
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <thread>
#include <vector>

namespace {

template <class F>
void run_threads(int threads, F&& body) {
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; ++t) pool.emplace_back([&, t] { body(t); });
    for (auto& th : pool) th.join();
}

// rows [0, n) in chunks of 256, drawn by the threads
template <class F>
void for_rows(int64_t n, int threads, F&& row) {
    std::atomic<int64_t> next{0};
    run_threads(threads, [&](int) {
        for (;;) {
            const int64_t lo = next.fetch_add(256), hi = std::min(n, lo + 256);
            if (lo >= n) return;
            for (int64_t v = lo; v < hi; ++v) row(v);
        }
    });
}

int64_t position(const int32_t* p, int64_t len, int32_t x) {
    return std::lower_bound(p, p + len, x) - p;         // (x is there)
}

}  // namespace

extern "C" {

// eid[p] = the id of adjacency entry p's edge: the edges {v, w}, v < w, numbered in (v, w) order;
// eu / ev (m each, may be null) = the endpoints by id.  Returns m.
int64_t ktruss_host_edge_ids(int64_t n, const int64_t* off, const int32_t* adj, int32_t* eid, int32_t* eu, int32_t* ev,
                             int threads) {
    threads = std::max(1, threads);
    std::vector<int64_t> base(static_cast<size_t>(n) + 1, 0);
    for (int64_t v = 0; v < n; ++v) {
        const int32_t* row = adj + off[v];
        const int64_t len = off[v + 1] - off[v];
        base[v + 1] = base[v] + (len - (std::upper_bound(row, row + len, static_cast<int32_t>(v)) - row));
    }
    for_rows(n, threads, [&](int64_t v) {
        const int32_t* row = adj + off[v];
        const int64_t len = off[v + 1] - off[v];
        const int64_t up = std::upper_bound(row, row + len, static_cast<int32_t>(v)) - row;
        for (int64_t j = up; j < len; ++j) {
            const int64_t id = base[v] + (j - up);
            eid[off[v] + j] = static_cast<int32_t>(id);
            if (eu) { eu[id] = static_cast<int32_t>(v); ev[id] = row[j]; }
        }
    });
    for_rows(n, threads, [&](int64_t v) {
        const int32_t* row = adj + off[v];
        const int64_t len = off[v + 1] - off[v];
        for (int64_t j = 0; j < len && row[j] < v; ++j) {
            const int32_t w = row[j];
            eid[off[v] + j] = eid[off[w] + position(adj + off[w], off[w + 1] - off[w], static_cast<int32_t>(v))];
        }
    });
    return base[n];
}

// sup[e] = |N(u) ∩ N(v)| of every edge
void ktruss_host_support(int64_t n, const int64_t* off, const int32_t* adj, const int32_t* eid, int32_t* sup, int threads) {
    for_rows(n, std::max(1, threads), [&](int64_t v) {
        const int32_t* a = adj + off[v];
        const int64_t na = off[v + 1] - off[v];
        for (int64_t j = 0; j < na; ++j) {
            const int32_t w = a[j];
            if (w < v) continue;
            const int32_t* b = adj + off[w];
            const int64_t nb = off[w + 1] - off[w];
            int64_t x = 0, y = 0;
            int32_t c = 0;
            while (x < na && y < nb) {
                if (a[x] == b[y]) { ++c; ++x; ++y; }
                else if (a[x] < b[y]) ++x;
                else ++y;
            }
            sup[eid[off[v] + j]] = c;
        }
    });
}

// truss[e] from sup0 (m each; eu / ev = the endpoints by id); returns the largest value.  rounds_out
// (may be null): the sub-rounds run.
int64_t ktruss_host_peel(int64_t n, int64_t m, const int64_t* off, const int32_t* adj, const int32_t* eid, const int32_t* eu,
                         const int32_t* ev, const int32_t* sup0, int32_t* truss, int64_t* rounds_out, int threads) {
    (void)n;
    threads = std::max(1, threads);
    std::vector<std::atomic<int32_t>> sup(static_cast<size_t>(m));
    std::vector<int32_t> state(static_cast<size_t>(m), 0);          // 0 alive, -1 frontier, > 0 final
    std::vector<int32_t> alive(static_cast<size_t>(m)), spare(static_cast<size_t>(m));
    for (int64_t e = 0; e < m; ++e) {
        sup[e].store(sup0[e], std::memory_order_relaxed);
        alive[e] = static_cast<int32_t>(e);
    }
    pthread_barrier_t bar;
    pthread_barrier_init(&bar, nullptr, threads);
    int64_t len = m, rounds = 0;
    std::atomic<int64_t> left{m}, kept{0}, pending{0};
    std::atomic<int32_t> next_level{INT32_MAX};
    int32_t level = 0;
    run_threads(threads, [&](int t) {
        std::vector<int32_t> cur, nxt;
        auto lower = [&](int32_t x, int32_t l) {
            if (sup[x].load(std::memory_order_relaxed) <= l) return;
            const int32_t old = sup[x].fetch_sub(1, std::memory_order_relaxed);
            if (old == l + 1) nxt.push_back(x);
            else if (old <= l) sup[x].fetch_add(1, std::memory_order_relaxed);
        };
        int64_t l_left = m;
        while (l_left > 0) {
            const int32_t l = level;
            const int64_t lo = len * t / threads, hi = len * (t + 1) / threads;
            cur.clear();
            for (int64_t i = lo; i < hi; ++i) {
                const int32_t e = alive[i];
                if (state[e] == 0 && sup[e].load(std::memory_order_relaxed) <= l) { cur.push_back(e); state[e] = -1; }
            }
            if (t == 0) { pending.store(0); next_level.store(INT32_MAX); }
            pthread_barrier_wait(&bar);
            for (;;) {                  // sub-rounds
                if (!cur.empty()) pending.fetch_add(static_cast<int64_t>(cur.size()));
                pthread_barrier_wait(&bar);
                const int64_t total = pending.load();
                pthread_barrier_wait(&bar);
                if (total == 0) break;
                if (t == 0) { pending.store(0); ++rounds; }
                nxt.clear();
                for (const int32_t e : cur) {
                    const int32_t u = eu[e], v = ev[e];
                    int64_t ab = off[u], al = off[u + 1] - ab, bb = off[v], bl = off[v + 1] - bb;
                    if (bl < al) { std::swap(ab, bb); std::swap(al, bl); }
                    for (int64_t j = 0; j < al; ++j) {
                        const int32_t w = adj[ab + j];
                        const int32_t* q = std::lower_bound(adj + bb, adj + bb + bl, w);
                        if (q == adj + bb + bl || *q != w) continue;
                        const int32_t e1 = eid[ab + j], e2 = eid[q - adj];
                        const int32_t s1 = state[e1], s2 = state[e2];
                        if (s1 > 0 || s2 > 0) continue;
                        const bool c1 = s1 < 0, c2 = s2 < 0;
                        if (c1 && c2) continue;
                        if (!c1 && !c2) { lower(e1, l); lower(e2, l); }
                        else if (c1) { if (e < e1) lower(e2, l); }
                        else if (e < e2) lower(e1, l);
                    }
                }
                if (!cur.empty()) left.fetch_sub(static_cast<int64_t>(cur.size()));
                pthread_barrier_wait(&bar);     // every read of state is done
                for (const int32_t e : cur) { state[e] = l + 2; truss[e] = l + 2; }
                for (const int32_t e : nxt) state[e] = -1;
                cur.swap(nxt);
                pthread_barrier_wait(&bar);
            }
            // the next level: the smallest support still alive (every thread offers its share's)
            l_left = left.load();
            if (l_left > 0) {
                if (2 * l_left <= len) {        // rebuild the alive list once it has halved
                    if (t == 0) kept.store(0);
                    pthread_barrier_wait(&bar);
                    std::vector<int32_t> mine;
                    for (int64_t i = lo; i < hi; ++i)
                        if (state[alive[i]] == 0) mine.push_back(alive[i]);
                    const int64_t at = kept.fetch_add(static_cast<int64_t>(mine.size()));
                    std::copy(mine.begin(), mine.end(), spare.begin() + at);
                    pthread_barrier_wait(&bar);
                    if (t == 0) { alive.swap(spare); len = kept.load(); }
                    pthread_barrier_wait(&bar);
                }
                int32_t mn = INT32_MAX;
                const int64_t lo2 = len * t / threads, hi2 = len * (t + 1) / threads;
                for (int64_t i = lo2; i < hi2; ++i)
                    if (state[alive[i]] == 0) mn = std::min(mn, sup[alive[i]].load(std::memory_order_relaxed));
                int32_t seen = next_level.load();
                while (mn < seen && !next_level.compare_exchange_weak(seen, mn)) {}
                pthread_barrier_wait(&bar);
                if (t == 0) level = next_level.load();
            }
            pthread_barrier_wait(&bar);
        }
    });
    pthread_barrier_destroy(&bar);
    if (rounds_out) *rounds_out = rounds;
    int64_t top = 0;
    for (int64_t e = 0; e < m; ++e) top = std::max<int64_t>(top, truss[e]);
    return top;
}

}  // extern "C"
