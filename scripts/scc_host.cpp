// scc_host.cpp — the host baseline of scripts/scc_bench.py: Tarjan's strongly connected components
// over a CSR of OUT lists, one thread (the algorithm is a depth-first search and does not
// parallelise), without recursion.  comp[v] = an index per component; returns their number.
#include <algorithm>
#include <cstdint>
#include <vector>

extern "C" int64_t scc_host_tarjan(int64_t n, const int64_t* off, const int32_t* adj, int32_t* comp) {
    std::vector<int32_t> index(n, -1), low(n, 0), stack, work;
    std::vector<int64_t> next(n, 0);
    std::vector<uint8_t> on(n, 0);
    int32_t counter = 0;
    int64_t ncomp = 0;
    for (int64_t root = 0; root < n; ++root) {
        if (index[root] != -1) continue;
        index[root] = low[root] = counter++;
        next[root] = off[root];
        stack.push_back(static_cast<int32_t>(root));
        on[root] = 1;
        work.push_back(static_cast<int32_t>(root));
        while (!work.empty()) {
            const int32_t v = work.back();
            if (next[v] < off[v + 1]) {
                const int32_t w = adj[next[v]++];
                if (index[w] == -1) {
                    index[w] = low[w] = counter++;
                    next[w] = off[w];
                    stack.push_back(w);
                    on[w] = 1;
                    work.push_back(w);
                } else if (on[w]) {
                    low[v] = std::min(low[v], index[w]);
                }
            } else {
                work.pop_back();
                if (!work.empty()) low[work.back()] = std::min(low[work.back()], low[v]);
                if (low[v] == index[v]) {
                    for (;;) {
                        const int32_t w = stack.back();
                        stack.pop_back();
                        on[w] = 0;
                        comp[w] = static_cast<int32_t>(ncomp);
                        if (w == v) break;
                    }
                    ++ncomp;
                }
            }
        }
    }
    return ncomp;
}
