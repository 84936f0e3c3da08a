"""Host reference for betweenness centrality (tgo_betweenness): Brandes' algorithm in exact arithmetic
(sigma as Python ints, delta as fractions.Fraction) on the two readings of a bothE load, and the
generators of the graphs the tests use.  Values are the raw sums over ordered pairs."""
from fractions import Fraction

import numpy as np


def adjacency(n, src, dst, directed=False):
    """(pred, succ): per vertex the sorted distinct predecessors / successors other than itself.
    Undirected: the simple projection (both lists are the neighbours)."""
    src = np.asarray(src, np.int64)
    dst = np.asarray(dst, np.int64)
    succ = [set() for _ in range(n)]
    pred = [set() for _ in range(n)]
    for u, v in zip(src.tolist(), dst.tolist()):
        if u == v:
            continue
        succ[u].add(v)
        pred[v].add(u)
        if not directed:
            succ[v].add(u)
            pred[u].add(v)
    return [sorted(p) for p in pred], [sorted(s) for s in succ]


def reference(n, src, dst, seeds=None, directed=False):
    """(bc, info): bc = list of n Fractions, the sum over `seeds` (vertex numbers, in order, repeats
    count; None = every vertex) of Brandes' dependencies; info = dict(sources, reached_pairs,
    max_depth, D, dmax): D = max_depth, dmax = the longest distinct-neighbour row."""
    pred, succ = adjacency(n, src, dst, directed)
    dmax = max([len(r) for r in pred] + [len(r) for r in succ] + [0])
    bc = [Fraction(0)] * n
    seeds = range(n) if seeds is None else [int(s) for s in seeds]
    sources = reached_pairs = max_depth = 0
    for s in seeds:
        level = [-1] * n
        sigma = [0] * n
        level[s], sigma[s] = 0, 1
        order, frontier = [s], [s]
        while frontier:
            nxt = []
            for u in frontier:
                for w in succ[u]:
                    if level[w] < 0:
                        level[w] = level[u] + 1
                        nxt.append(w)
                    if level[w] == level[u] + 1:
                        sigma[w] += sigma[u]
            order += nxt
            frontier = nxt
        delta = [Fraction(0)] * n
        for v in reversed(order):
            for w in succ[v]:
                if level[w] == level[v] + 1:
                    delta[v] += Fraction(sigma[v], sigma[w]) * (1 + delta[w])
            if v != s:
                bc[v] += delta[v]
        sources += 1
        reached_pairs += len(order) - 1
        max_depth = max(max_depth, level[order[-1]])
    return bc, {"sources": sources, "reached_pairs": reached_pairs, "max_depth": max_depth, "D": max_depth, "dmax": dmax}


def tolerance(info, nseeds):
    """The relative rounding bound of any fp64 summation order: every term is non-negative, so a
    k-term sum errs by at most (k - 1) u relative; a sigma inherits D dmax u; each term of a delta
    adds a division, an addition and a multiplication; delta nests D levels; the outer sum adds S."""
    return Fraction(3 * info["D"] * (info["dmax"] + 3) + nseeds, 1 << 52)


def within(got, exact, tol):
    """Every got[v] within tol * exact[v] of exact[v]; an exact zero must be 0.0.  The worst relative error."""
    worst = Fraction(0)
    for v, (g, e) in enumerate(zip(np.asarray(got, np.float64).tolist(), exact)):
        if e == 0:
            assert g == 0.0, (v, g)
            continue
        err = abs(Fraction(g) - e) / e
        worst = max(worst, err)
        assert err <= tol, (v, g, float(e), float(err), float(tol))
    return float(worst)


def as_floats(exact):
    """The exact values as doubles, asserting that each is one (an integer or a dyadic fraction in range)."""
    out = np.array([float(e) for e in exact], np.float64)
    assert all(Fraction(x) == e for x, e in zip(out.tolist(), exact))
    return out


# ----------------------------------------------------------------------------- generators: (n, src, dst)
def _arr(edges):
    e = np.asarray(edges, np.int32).reshape(-1, 2)
    return e[:, 0].copy(), e[:, 1].copy()


def path(n):
    return (n,) + _arr([(i, i + 1) for i in range(n - 1)])


def star(leaves):
    """Centre 0; every other edge points at the centre."""
    return (leaves + 1,) + _arr([(0, i) if i % 2 else (i, 0) for i in range(1, leaves + 1)])


def cycle(n):
    return (n,) + _arr([(i, (i + 1) % n) for i in range(n)])


def clique(k):
    return (k,) + _arr([(i, j) for i in range(k) for j in range(i + 1, k)])


def complete_bipartite(a, b):
    """Vertices 0..a-1 against a..a+b-1."""
    return (a + b,) + _arr([(i, a + j) for i in range(a) for j in range(b)])


def grid(w, h):
    e = [(y * w + x, y * w + x + 1) for y in range(h) for x in range(w - 1)]
    e += [(y * w + x, (y + 1) * w + x) for y in range(h - 1) for x in range(w)]
    return (w * h,) + _arr(e)


def diamond_chain(k):
    """a_0 <b_0, c_0> a_1 ... a_k: vertex 3 i = a_i, 3 i + 1 / + 2 = b_i / c_i; sigma(a_0 -> a_i) = 2^i."""
    e = []
    for i in range(k):
        a, b, c, a2 = 3 * i, 3 * i + 1, 3 * i + 2, 3 * i + 3
        e += [(a, b), (a, c), (b, a2), (c, a2)]
    return (3 * k + 1,) + _arr(e)


def projection_fixture():
    """Parallel edges, both directions of a pair, a self-loop and an isolated vertex."""
    return (5,) + _arr([(0, 1), (0, 1), (1, 0), (0, 2), (1, 3), (2, 3), (3, 3)])


def gnp(n=301, p=0.03, seed=9):
    """G(n, p), every edge in a random direction."""
    rng = np.random.default_rng(seed)
    iu, ju = np.triu_indices(n, 1)
    keep = rng.random(len(iu)) < p
    s, d = iu[keep], ju[keep]
    flip = rng.random(len(s)) < 0.5
    return n, np.where(flip, d, s).astype(np.int32), np.where(flip, s, d).astype(np.int32)


def two_components_and_isolated():
    """A path of 9 (0..8), a 5-cycle with a chord (9..13), vertices 14..16 without an edge."""
    n, s1, d1 = path(9)
    _, s2, d2 = cycle(5)
    src = np.concatenate([s1, s2 + 9, np.array([9], np.int32)]).astype(np.int32)
    dst = np.concatenate([d1, d2 + 9, np.array([11], np.int32)]).astype(np.int32)
    return 17, src, dst


def relabel(n, src, dst, seed=3, gap=8, base=24):
    """The same graph with its vertices renumbered at random and gapped, increasing Titan ids for the
    new rows: (ids, src', dst', new_of_old)."""
    rng = np.random.default_rng(seed)
    new_of_old = rng.permutation(n).astype(np.int32)
    ids = (np.sort(rng.choice(4 * n, n, replace=False)).astype(np.int64)) * gap + base
    return ids, new_of_old[np.asarray(src)], new_of_old[np.asarray(dst)], new_of_old
