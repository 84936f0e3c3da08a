"""Host reference for closeness and harmonic centrality (tgo_closeness): one BFS per seed over the
scope's message paths, integer far / reach / ecc, and the harmonic sum folded in the contractual
order — the batches of 64 seeds in order, within a batch the distinct levels L >= 1 present at the
vertex ascending, h = h + (double)c / (double)L.  numpy's float64 division and addition are the IEEE
operations the contract names, so the device result equals this one bit for bit.  A vertex accumulates
its distances FROM the seeds; nothing is normalised.  The graph generators are bc_ref's."""
from fractions import Fraction

import numpy as np

from ragged import scope_messages

BATCH = 64


def lists(n, src, dst, scope):
    """CSR (off, adj) of the scope's message paths: adj[off[u]:off[u + 1]] = the receivers of u."""
    send, recv, _ = scope_messages(scope, src, dst)
    order = np.argsort(send, kind="stable")
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(send, minlength=n))
    return off, np.asarray(recv, np.int64)[order]


def bfs(off, adj, n, seed, max_depth=None):
    """Hop distances from `seed` along the lists, -1 where it does not reach (or not within max_depth)."""
    d = np.full(n, -1, np.int64)
    d[seed] = 0
    fr = np.array([seed], np.int64)
    level = 0
    while len(fr) and (max_depth is None or level < max_depth):
        level += 1
        starts, cnt = off[fr], off[fr + 1] - off[fr]
        total = int(cnt.sum())
        if total == 0:
            break
        idx = np.repeat(starts - (np.cumsum(cnt) - cnt), cnt) + np.arange(total)
        nb = adj[idx]
        fr = np.unique(nb[d[nb] < 0])
        d[fr] = level
    return d


def distances(n, src, dst, scope, seeds, max_depth=None):
    """(len(seeds), n) int64: row i = bfs from seeds[i]."""
    off, adj = lists(n, src, dst, scope)
    out = np.full((len(seeds), n), -1, np.int64)
    for i, s in enumerate(seeds):
        out[i] = bfs(off, adj, n, int(s), max_depth)
    return out


def fold(dist):
    """The five arrays and info of a (seeds, n) distance matrix (-1 = not reached), seeds in the order
    given: dict(far, reach, ecc (int64), closeness, harmonic (float64)), dict(sources, reached_pairs,
    batches, max_depth)."""
    dist = np.asarray(dist, np.int64)
    S, n = dist.shape
    far, reach, ecc = (np.zeros(n, np.int64) for _ in range(3))
    harm = np.zeros(n, np.float64)
    for b0 in range(0, S, BATCH):
        d = dist[b0:b0 + BATCH]
        pos = d > 0                                         # level 0 is the seed on itself
        far += np.where(pos, d, 0).sum(0)
        reach += pos.sum(0)
        if pos.any():
            ecc = np.maximum(ecc, np.where(pos, d, 0).max(0))
        for level in np.unique(d[pos]).tolist():            # ascending; a level absent at v adds nothing there
            c = (d == level).sum(0)
            at = c > 0
            harm[at] = harm[at] + c[at].astype(np.float64) / np.float64(level)
    close = np.zeros(n, np.float64)
    some = far > 0
    close[some] = reach[some].astype(np.float64) / far[some].astype(np.float64)
    info = {"sources": S, "reached_pairs": int(reach.sum()), "batches": (S + BATCH - 1) // BATCH,
            "max_depth": int(ecc.max()) if n else 0}
    return {"far": far, "reach": reach, "ecc": ecc, "closeness": close, "harmonic": harm}, info


def reference(n, src, dst, scope=2, seeds=None, max_depth=None):
    """fold() of the BFS distances from `seeds` (vertex numbers, in order, repeats count; None = every
    vertex) over the scope's message paths (0 outE, 1 inE, 2 bothE)."""
    seeds = list(range(n)) if seeds is None else [int(s) for s in seeds]
    return fold(distances(n, src, dst, scope, seeds, max_depth).reshape(len(seeds), n))


def exact_harmonic(dist):
    """Per vertex the exact sum of 1 / d over the seeds with d > 0, as Fractions."""
    dist = np.asarray(dist, np.int64)
    return [sum((Fraction(1, int(x)) for x in col[col > 0].tolist()), Fraction(0)) for col in dist.T]
