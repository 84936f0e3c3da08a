"""Plain-Python reference of tgo_peer_pressure (include/titan_gpu_olap.h has the contract).

The graph is a directed multigraph: edge k is src[k] -> dst[k], every edge carries one vote, parallel
edges vote as many times and a self-loop votes for its own vertex.  Tallies are dicts of Python ints
in units of 2^-32; a tie goes to the smallest Titan id.  Vertex i has Titan id ids[i] (default: i).
test_pp_cpu.py checks this file against closed forms; the device is compared with it bit for bit.
"""
import numpy as np

OUT, IN, BOTH = 0, 1, 2             # TGO_SCOPE_OUT_E / _IN_E / _BOTH_E (asserted in test_pp_cpu.py)
ONE = 1 << 32


def receive_lists(n, src, dst, vote_scope):
    """(senders of every vertex, one per entry; d(v) = the entries v sends over)."""
    recv = [[] for _ in range(n)]
    d = [0] * n
    for u, v in zip(np.asarray(src).tolist(), np.asarray(dst).tolist()):
        if vote_scope in (OUT, BOTH):       # the vote travels u -> v
            recv[v].append(u)
            d[u] += 1
        if vote_scope in (IN, BOTH):        # the vote travels v -> u
            recv[u].append(v)
            d[v] += 1
    return recv, d


def reference(n, src, dst, ids=None, vote_scope=OUT, distribute=0, max_rounds=30):
    """(cluster, info): cluster[i] = the Titan id of vertex i's cluster (int64), info = dict(clusters,
    largest, changed_last, rounds, converged)."""
    if vote_scope not in (OUT, IN, BOTH) or distribute not in (0, 1) or max_rounds < 0:
        raise ValueError("bad arguments")
    ids = list(range(n)) if ids is None else [int(x) for x in ids]
    assert len(ids) == n and len(set(ids)) == n
    recv, d = receive_lists(n, src, dst, vote_scope)
    strength = [(ONE // d[v] if d[v] else 0) if distribute else ONE for v in range(n)]
    cluster = list(ids)
    rounds = changed = 0
    while rounds < max_rounds:
        nxt = list(cluster)
        for v in range(n):
            if distribute and d[v] == 0:    # its own vote is 1 / 0 = Infinity: it never leaves
                continue
            tally = {cluster[v]: strength[v]}
            for u in recv[v]:
                tally[cluster[u]] = tally.get(cluster[u], 0) + strength[u]
            best = max(tally.values())
            nxt[v] = min(c for c, t in tally.items() if t == best)
        changed = sum(a != b for a, b in zip(cluster, nxt))
        cluster = nxt
        rounds += 1
        if changed == 0:
            break
    sizes = {}
    for c in cluster:
        sizes[c] = sizes.get(c, 0) + 1
    info = {"clusters": len(sizes), "largest": max(sizes.values()) if sizes else 0, "changed_last": changed,
            "rounds": rounds, "converged": int((changed == 0 and rounds > 0) or n == 0)}
    return np.array(cluster, np.int64), info


def edges_from_lists(out_csr, perm):
    """(src, dst) in row numbers from the device's OUT lists (Engine.graph_csr(0): "off" and "adj" in
    internal ids; Engine.graph_perm(): row -> internal id)."""
    off, adj = (np.asarray(out_csr[k], np.int64) for k in ("off", "adj"))
    n = len(off) - 1
    row = np.empty(n, np.int64)
    row[np.asarray(perm, np.int64)] = np.arange(n)
    return row[np.repeat(np.arange(n, dtype=np.int64), np.diff(off))], row[adj]


# ------------------------------------------------------------------ generators: (n, src, dst)
def _arr(e):
    e = np.array(e, np.int32).reshape(-1, 2)
    return e[:, 0].copy(), e[:, 1].copy()


def cycle(n, times=1):
    return (n, *_arr([(i, (i + 1) % n) for i in range(n) for _ in range(times)]))


def path(n):
    return (n, *_arr([(i, i + 1) for i in range(n - 1)]))


def two_cliques_bridge(k):
    e = [(a + o, b + o) for o in (0, k) for a in range(k) for b in range(a + 1, k)]
    return (2 * k, *_arr(e + [(k - 1, k)]))


def clique(k):
    return (k, *_arr([(a, b) for a in range(k) for b in range(k) if a != b]))


def star(leaves):
    """Vertex 0 is the hub; an edge from it to every leaf."""
    return (leaves + 1, *_arr([(0, i) for i in range(1, leaves + 1)]))


def fan(leaves):
    """Leaves 1..leaves in pairs, every leaf with an edge to the hub (vertex 0): the odd leaf of a pair
    has two parallel edges to the even one, which they pull into its cluster in round 1 (distribute =
    0).  From round 2 the hub's row holds leaves / 2 distinct clusters of two votes each."""
    e = []
    for i in range(1, leaves + 1):
        e.append((i, 0))
        if i % 2 == 1 and i < leaves:
            e += [(i, i + 1), (i, i + 1)]
    return (leaves + 1, *_arr(e))


def fixed_point_pin():
    """a = 0 sends three parallel edges to r = 2 (d = 3), b = 1 one edge (d = 1); r has four edges to
    sinks (d = 4).  With distribute r tallies 3 floor(2^32 / 3) = 2^32 - 1 for a and 2^32 for b."""
    return (7, *_arr([(0, 2)] * 3 + [(1, 2)] + [(2, k) for k in (3, 4, 5, 6)]))


def gnp_digraph(n, p, seed):
    rng = np.random.default_rng(seed)
    s, t = np.nonzero(np.triu(rng.random((n, n)) < p, 1))       # one edge per pair, its direction random
    flip = rng.random(len(s)) < 0.5
    return n, np.where(flip, t, s).astype(np.int32), np.where(flip, s, t).astype(np.int32)
