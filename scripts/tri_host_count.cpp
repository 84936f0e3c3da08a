// Host side of scripts/triangles_bench.py: the forward lists of a loaded bothE graph rebuilt from
// its assembled OUT / IN lists (Engine.graph_csr), the work measure of the device count, and a
// multi-threaded host count of the same lists as a sanity ratio.  Built by the script:
//   g++ -O3 -std=c++17 -shared -fPIC -pthread scripts/tri_host_count.cpp -o scripts/libtri_host_count.so
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <thread>
#include <vector>

namespace {

template <class F>
void parallel_rows(int64_t n, int threads, F&& body) {
    std::atomic<int64_t> next{0};
    const int64_t chunk = 256;
    std::vector<std::thread> pool;
    for (int t = 0; t < std::max(1, threads); ++t)
        pool.emplace_back([&, t] {
            for (;;) {
                const int64_t lo = next.fetch_add(chunk);
                if (lo >= n) return;
                body(lo, std::min(n, lo + chunk), t);
            }
        });
    for (auto& th : pool) th.join();
}

// distinct entries < v of the two sorted rows, in order; dst may be null (count only)
int64_t forward_row(const int32_t* a, int64_t na, const int32_t* b, int64_t nb, int32_t v, int32_t* dst) {
    int64_t i = 0, j = 0, c = 0;
    int32_t last = -1;
    while (true) {
        const int32_t x = i < na ? a[i] : INT32_MAX, y = j < nb ? b[j] : INT32_MAX;
        const int32_t m = std::min(x, y);
        if (m >= v) break;
        i += x == m;
        j += y == m;
        if (m != last) {
            if (dst) dst[c] = m;
            ++c;
            last = m;
        }
    }
    return c;
}

}  // namespace

extern "C" {

// flen[v] = |fwd(v)| (fadj null), or the rows written at foff (fadj non-null)
void tri_host_forward(int64_t n, const int64_t* ooff, const int32_t* oadj, const int64_t* ioff, const int32_t* iadj,
                      int64_t* flen, const int64_t* foff, int32_t* fadj, int threads) {
    parallel_rows(n, threads, [&](int64_t lo, int64_t hi, int) {
        for (int64_t v = lo; v < hi; ++v) {
            const int64_t c = forward_row(oadj + ooff[v], ooff[v + 1] - ooff[v], iadj + ioff[v], ioff[v + 1] - ioff[v],
                                          static_cast<int32_t>(v), fadj ? fadj + foff[v] : nullptr);
            if (!fadj) flen[v] = c;
        }
    });
}

// sum over oriented entries (c, b) of min(|fwd(c)|, |fwd(b)|)
int64_t tri_host_work(int64_t n, const int64_t* foff, const int32_t* fadj, int threads) {
    std::vector<int64_t> part(std::max(1, threads), 0);
    parallel_rows(n, threads, [&](int64_t lo, int64_t hi, int t) {
        int64_t s = 0;
        for (int64_t c = lo; c < hi; ++c)
            for (int64_t k = foff[c]; k < foff[c + 1]; ++k) {
                const int32_t b = fadj[k];
                s += std::min(foff[c + 1] - foff[c], foff[b + 1] - foff[b]);
            }
        part[t] += s;
    });
    int64_t s = 0;
    for (int64_t x : part) s += x;
    return s;
}

// triangles: for every oriented entry (c, b) the members of fwd(c)[0, position of b) in fwd(b)
int64_t tri_host_count(int64_t n, const int64_t* foff, const int32_t* fadj, int threads) {
    std::vector<int64_t> part(std::max(1, threads), 0);
    parallel_rows(n, threads, [&](int64_t lo, int64_t hi, int t) {
        int64_t s = 0;
        for (int64_t c = lo; c < hi; ++c) {
            const int32_t* const row = fadj + foff[c];
            const int64_t L = foff[c + 1] - foff[c];
            for (int64_t kb = 1; kb < L; ++kb) {
                const int32_t b = row[kb];
                const int32_t* const other = fadj + foff[b];
                const int64_t lb = foff[b + 1] - foff[b];
                int64_t i = 0, j = 0;
                while (i < kb && j < lb) {
                    const int32_t x = row[i], y = other[j];
                    s += x == y;
                    i += x <= y;
                    j += y <= x;
                }
            }
        }
        part[t] += s;
    });
    int64_t s = 0;
    for (int64_t x : part) s += x;
    return s;
}

}  // extern "C"
