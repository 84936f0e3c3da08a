// Host side of scripts/kcore_bench.py: a multi-threaded k-core peel over the same simple undirected
// projection as tgo_kcore, from a loaded bothE graph's assembled OUT / IN lists (Engine.graph_csr).
// The peel is the PKC scheme (Kabir and Madduri, "Parallel k-core decomposition on multicore
// platforms"): level by level, every thread scans its share of the alive list for vertices at the
// level, peels them and whatever it drops itself from a buffer of its own, and the threads meet at
// a barrier; the alive list is rebuilt once it has halved.  Built by the script:
//   g++ -O3 -std=c++17 -shared -fPIC -pthread scripts/kcore_host.cpp -o scripts/libkcore_host.so
#include <pthread.h>
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <thread>
#include <vector>

namespace {

// distinct entries other than v of the two sorted rows; dst may be null (count only)
int64_t merged_row(const int32_t* a, int64_t na, const int32_t* b, int64_t nb, int32_t v, int32_t* dst) {
    int64_t i = 0, j = 0, c = 0;
    int32_t last = -1;
    while (true) {
        const int32_t x = i < na ? a[i] : INT32_MAX, y = j < nb ? b[j] : INT32_MAX;
        const int32_t m = std::min(x, y);
        if (m == INT32_MAX) break;
        i += x == m;
        j += y == m;
        if (m != last && m != v) {
            if (dst) dst[c] = m;
            ++c;
        }
        last = m;
    }
    return c;
}

template <class F>
void run_threads(int threads, F&& body) {
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; ++t) pool.emplace_back([&, t] { body(t); });
    for (auto& th : pool) th.join();
}

}  // namespace

extern "C" {

// len[v] = d(v) (adj null), or the neighbourhoods written at off (adj non-null)
void kcore_host_projection(int64_t n, const int64_t* ooff, const int32_t* oadj, const int64_t* ioff, const int32_t* iadj,
                           int64_t* len, const int64_t* off, int32_t* adj, int threads) {
    threads = std::max(1, threads);
    std::atomic<int64_t> next{0};
    run_threads(threads, [&](int) {
        for (;;) {
            const int64_t lo = next.fetch_add(1024), hi = std::min(n, lo + 1024);
            if (lo >= n) return;
            for (int64_t v = lo; v < hi; ++v) {
                const int64_t c = merged_row(oadj + ooff[v], ooff[v + 1] - ooff[v], iadj + ioff[v], ioff[v + 1] - ioff[v],
                                             static_cast<int32_t>(v), adj ? adj + off[v] : nullptr);
                if (!adj) len[v] = c;
            }
        }
    });
}

// core[v] of the projection (off, adj); returns the degeneracy
int64_t kcore_host_peel(int64_t n, const int64_t* off, const int32_t* adj, int32_t* core, int threads) {
    threads = std::max(1, threads);
    std::vector<std::atomic<int32_t>> deg(static_cast<size_t>(n));
    std::vector<int32_t> alive(static_cast<size_t>(n)), spare(static_cast<size_t>(n));
    for (int64_t v = 0; v < n; ++v) {
        deg[v].store(static_cast<int32_t>(off[v + 1] - off[v]), std::memory_order_relaxed);
        alive[v] = static_cast<int32_t>(v);
    }
    pthread_barrier_t bar;
    pthread_barrier_init(&bar, nullptr, threads);
    int64_t len = n;                    // alive list length (stale entries included)
    std::atomic<int64_t> left{n}, kept{0};
    run_threads(threads, [&](int t) {
        std::vector<int32_t> buf;
        // (the loop's condition is the count every thread read behind the same barrier: a thread
        // must not see another one's next level already subtracted)
        int64_t l = n;
        for (int32_t k = 0; l > 0; ++k) {
            const int64_t lo = len * t / threads, hi = len * (t + 1) / threads;
            buf.clear();
            for (int64_t i = lo; i < hi; ++i)
                if (deg[alive[i]].load(std::memory_order_relaxed) == k) buf.push_back(alive[i]);
            pthread_barrier_wait(&bar);     // no drop before every scan ended: a vertex is taken once
            for (size_t h = 0; h < buf.size(); ++h) {
                const int32_t v = buf[h];
                for (int64_t e = off[v]; e < off[v + 1]; ++e) {
                    const int32_t u = adj[e];
                    if (deg[u].load(std::memory_order_relaxed) <= k) continue;
                    const int32_t old = deg[u].fetch_sub(1, std::memory_order_relaxed);
                    if (old == k + 1) buf.push_back(u);
                    else if (old <= k) deg[u].fetch_add(1, std::memory_order_relaxed);
                }
            }
            if (!buf.empty()) left.fetch_sub(static_cast<int64_t>(buf.size()));
            pthread_barrier_wait(&bar);
            l = left.load();
            // rebuild the alive list once it has halved
            if (l > 0 && 2 * l <= len) {
                if (t == 0) kept.store(0);
                pthread_barrier_wait(&bar);
                std::vector<int32_t> mine;
                for (int64_t i = lo; i < hi; ++i)
                    if (deg[alive[i]].load(std::memory_order_relaxed) > k) mine.push_back(alive[i]);
                const int64_t at = kept.fetch_add(static_cast<int64_t>(mine.size()));
                std::copy(mine.begin(), mine.end(), spare.begin() + at);
                pthread_barrier_wait(&bar);
                if (t == 0) {
                    alive.swap(spare);
                    len = kept.load();
                }
            }
            pthread_barrier_wait(&bar);
        }
    });
    pthread_barrier_destroy(&bar);
    int64_t top = 0;
    for (int64_t v = 0; v < n; ++v) {
        core[v] = deg[v].load(std::memory_order_relaxed);
        top = std::max<int64_t>(top, core[v]);
    }
    return top;
}

}  // extern "C"
