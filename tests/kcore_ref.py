"""Host restatements of tgo_kcore for the tests, over the simple undirected projection of an edge
list (parallel edges, both directions of a pair and self-loops collapse).

Two independent ones: `reference` peels by Batagelj-Zaversnik bucket order; `hindex_fixed_point`
iterates c[v] = min(c[v], H-index of c over N(v)) from the degrees until nothing changes (Lu et
al., "The H-index of a network node and its relation to degree and coreness").  Both are exact
integer computations; the tests compare with array_equal.

info follows the C-ABI: degeneracy = max core, innermost = vertices at it, simple_edges = sum(d) / 2,
levels = distinct core values (0 included when some vertex has none).  A projection without any edge
is not peeled: its info is all zero."""
import numpy as np


def projection(n, src, dst):
    """(off, adj): CSR of the projection, rows sorted, no duplicates, no loops."""
    src = np.asarray(src, np.int64)
    dst = np.asarray(dst, np.int64)
    keep = src != dst
    a = np.concatenate([src[keep], dst[keep]])
    b = np.concatenate([dst[keep], src[keep]])
    key = np.unique(a * n + b)
    rows, adj = key // n, key % n
    off = np.zeros(n + 1, np.int64)
    np.add.at(off, rows + 1, 1)
    return np.cumsum(off), adj


def info_of(core, off):
    core = np.asarray(core, np.int64)
    edges = int(off[-1]) // 2
    if edges == 0:
        return {"degeneracy": 0, "innermost": 0, "simple_edges": 0, "levels": 0}
    top = int(core.max())
    return {"degeneracy": top, "innermost": int((core == top).sum()), "simple_edges": edges,
            "levels": int(len(np.unique(core)))}


def peel(off, adj):
    """Batagelj-Zaversnik: vertices in bucket order of their current degree; removing one lowers
    each higher neighbour by one and moves it a bucket down."""
    n = len(off) - 1
    deg = np.diff(off).astype(np.int64)
    if n == 0:
        return deg
    md = int(deg.max(initial=0))
    start = np.zeros(md + 2, np.int64)                  # bucket starts
    np.add.at(start, deg + 1, 1)
    start = np.cumsum(start)[:-1].tolist()
    order = np.argsort(deg, kind="stable").tolist()     # vert[pos]
    pos = [0] * n
    for p, v in enumerate(order):
        pos[v] = p
    d = deg.tolist()
    offl, adjl = off.tolist(), adj.tolist()
    for i in range(n):
        v = order[i]
        for u in adjl[offl[v]:offl[v + 1]]:
            if d[u] > d[v]:
                du = d[u]
                pw = start[du]                           # first vertex of u's bucket
                w = order[pw]
                if w != u:
                    pu = pos[u]
                    order[pu], order[pw] = w, u
                    pos[u], pos[w] = pw, pu
                start[du] += 1
                d[u] = du - 1
    return np.asarray(d, np.int64)


def hindex_fixed_point(off, adj):
    """(core, sweeps): synchronous sweeps of c <- min(c, H(c over N(v))) from the degrees; the
    sweep that changes nothing is counted."""
    n = len(off) - 1
    c = np.diff(off).astype(np.int64)
    rows = np.repeat(np.arange(n), np.diff(off))
    sweeps = 0
    while True:
        sweeps += 1
        vals = c[adj]
        order = np.lexsort((-vals, rows))               # each row's values, largest first
        rank = np.arange(len(adj)) - off[:-1][rows] + 1
        h = np.bincount(rows, weights=(vals[order] >= rank), minlength=n).astype(np.int64)
        new = np.minimum(c, h)
        if np.array_equal(new, c):
            return c, sweeps
        c = new


def reference(n, src, dst):
    """(core, info) of the projection of the edges src[i] -> dst[i] over vertices 0..n-1."""
    off, adj = projection(n, src, dst)
    core = peel(off, adj)
    return core, info_of(core, off)


def reference_from_lists(out, inn, perm):
    """The same from assembled device lists (Engine.graph_csr(0), graph_csr(1), graph_perm()):
    rows and entries in internal ids, results in row order."""
    n = len(perm)
    rows = np.concatenate([np.repeat(np.arange(n), np.diff(out["off"])), np.repeat(np.arange(n), np.diff(inn["off"]))])
    nbrs = np.concatenate([out["adj"], inn["adj"]]).astype(np.int64)
    core, info = reference(n, rows, nbrs)
    return core[np.asarray(perm, np.int64)], info


# ------------------------------------------------------------------ the tests' graphs: (n, src, dst)
def clique(k, base=0):
    s, d = np.triu_indices(k, 1)
    return k, (s + base).astype(np.int32), (d + base).astype(np.int32)


def wheel(leaves):
    """Hub 0 joined to a ring 1..leaves."""
    ring = np.arange(1, leaves + 1, dtype=np.int32)
    src = np.concatenate([np.zeros(leaves, np.int32), ring])
    dst = np.concatenate([ring, np.roll(ring, -1)])
    return leaves + 1, src, dst


def star(leaves, base=0):
    """Centre `base`, leaves after it; every other edge points at the centre."""
    leaf = np.arange(1, leaves + 1, dtype=np.int32)
    src = np.where(leaf % 2 == 0, 0, leaf).astype(np.int32) + base
    dst = np.where(leaf % 2 == 0, leaf, 0).astype(np.int32) + base
    return leaves + 1, src, dst


def random_path(n, seed=5):
    order = np.random.default_rng(seed).permutation(n)
    return n, order[:-1].astype(np.int32), order[1:].astype(np.int32)


def clique_chain(lo=2, hi=40):
    """K_lo ... K_hi, consecutive cliques joined by one bridge edge (last vertex of one to the first
    of the next).  Returns (n, src, dst, core): members of K_j have core j - 1."""
    src, dst, core, base, prev_last = [], [], [], 0, None
    for j in range(lo, hi + 1):
        _, s, d = clique(j, base)
        src.append(s)
        dst.append(d)
        if prev_last is not None:
            src.append(np.array([prev_last], np.int32))
            dst.append(np.array([base], np.int32))
        core += [j - 1] * j
        prev_last = base + j - 1
        base += j
    return base, np.concatenate(src), np.concatenate(dst), np.asarray(core, np.int64)


def gnp(n=1001, p=0.05, seed=12):
    """G(n, p) with every edge's direction flipped at random; (n, src, dst, rng) — the rng goes on
    to the caller's id shuffle."""
    rng = np.random.default_rng(seed)
    s, d = np.triu_indices(n, 1)
    keep = rng.random(len(s)) < p
    s, d = s[keep], d[keep]
    flip = rng.random(len(s)) < 0.5
    return n, np.where(flip, d, s).astype(np.int32), np.where(flip, s, d).astype(np.int32), rng
