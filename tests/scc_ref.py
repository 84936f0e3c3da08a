"""Host reference of strongly connected components (tgo_scc): an iterative Tarjan over the directed
arcs, a second method (reachability closure by repeated squaring) for small graphs, and the
generators the tests share.  Labels are the smallest Titan id of a component (ids default to the
vertex numbers); info = dict(components, largest, singletons)."""
import numpy as np


def csr(n, src, dst):
    """(off, adj) of the OUT lists of the arcs src -> dst (duplicates and loops kept)."""
    src = np.asarray(src, np.int64)
    dst = np.asarray(dst, np.int64)
    order = np.argsort(src, kind="stable")
    off = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(src, minlength=n), out=off[1:])
    return off, dst[order]


def tarjan(n, off, adj):
    """comp[v] = an index per strongly connected component; no recursion."""
    index = np.full(n, -1, np.int64)
    low = np.zeros(n, np.int64)
    on = np.zeros(n, bool)
    comp = np.full(n, -1, np.int64)
    off = off.tolist()
    adj = adj.tolist()
    stack, counter, ncomp = [], 0, 0
    for root in range(n):
        if index[root] != -1:
            continue
        work = [(root, off[root])]
        index[root] = low[root] = counter
        counter += 1
        stack.append(root)
        on[root] = True
        while work:
            v, k = work[-1]
            if k < off[v + 1]:
                work[-1] = (v, k + 1)
                w = adj[k]
                if index[w] == -1:
                    index[w] = low[w] = counter
                    counter += 1
                    stack.append(w)
                    on[w] = True
                    work.append((w, off[w]))
                elif on[w]:
                    low[v] = min(low[v], index[w])
            else:
                work.pop()
                if work:
                    p = work[-1][0]
                    low[p] = min(low[p], low[v])
                if low[v] == index[v]:
                    while True:
                        w = stack.pop()
                        on[w] = False
                        comp[w] = ncomp
                        if w == v:
                            break
                    ncomp += 1
    return comp


def labels_of(comp, ids=None):
    """(labels, info) from any per-vertex component index: the smallest id per component."""
    comp = np.asarray(comp, np.int64)
    n = len(comp)
    ids = np.arange(n, dtype=np.int64) if ids is None else np.asarray(ids, np.int64)
    if n == 0:
        return np.zeros(0, np.int64), {"components": 0, "largest": 0, "singletons": 0}
    _, inv, cnt = np.unique(comp, return_inverse=True, return_counts=True)
    lo = np.full(len(cnt), np.iinfo(np.int64).max, np.int64)
    np.minimum.at(lo, inv, ids)
    return lo[inv], {"components": int(len(cnt)), "largest": int(cnt.max()), "singletons": int((cnt == 1).sum())}


def reference(n, src, dst, ids=None):
    off, adj = csr(n, src, dst)
    return labels_of(tarjan(n, off, adj), ids)


def reference_from_lists(out_csr, in_csr, perm, ids):
    """The reference over the device's own lists (Engine.graph_csr(0) / (1): dicts with "off" and
    "adj" in internal ids; Engine.graph_perm(): row -> internal id), labels in row order; the IN
    lists must be the transpose of the OUT lists."""
    off, adj = (np.asarray(out_csr[k], np.int64) for k in ("off", "adj"))
    ioff, iadj = (np.asarray(in_csr[k], np.int64) for k in ("off", "adj"))
    n = len(off) - 1
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(off))
    isrc = np.repeat(np.arange(n, dtype=np.int64), np.diff(ioff))
    assert np.array_equal(np.sort(src * n + adj), np.sort(iadj * n + isrc))
    perm = np.asarray(perm, np.int64)
    tid = np.empty(n, np.int64)
    tid[perm] = np.asarray(ids, np.int64)
    lab, info = labels_of(tarjan(n, off, adj), tid)
    return lab[perm], info


def closure_components(n, src, dst):
    """comp by the boolean reachability closure R (repeated squaring) and R & R.T: n <= 200."""
    r = np.eye(n, dtype=bool)
    r[np.asarray(src, np.int64), np.asarray(dst, np.int64)] = True
    while True:
        nxt = (r.astype(np.int32) @ r.astype(np.int32)) > 0
        if np.array_equal(nxt, r):
            break
        r = nxt
    both = r & r.T
    return np.array([int(np.flatnonzero(both[v])[0]) for v in range(n)], np.int64)


# ------------------------------------------------------------------ generators: (n, src, dst)
def _i32(a):
    return np.asarray(a, np.int32)


def cycle(k):
    v = np.arange(k)
    return k, _i32(v), _i32((v + 1) % k)


def random_cycle(k, seed=5):
    p = np.random.default_rng(seed).permutation(k)
    return k, _i32(p), _i32(np.roll(p, -1))


def random_dipath(k, seed=6):
    p = np.random.default_rng(seed).permutation(k)
    return k, _i32(p[:-1]), _i32(p[1:])


def two_cycles_bridge(a, b, forward=True):
    """Cycles 0..a-1 and a..a+b-1 joined by one arc from the first to the second (or back)."""
    _, s1, d1 = cycle(a)
    _, s2, d2 = cycle(b)
    br = (0, a) if forward else (a, 0)
    return a + b, _i32(np.concatenate([s1, s2 + a, [br[0]]])), _i32(np.concatenate([d1, d2 + a, [br[1]]]))


def bidirected_clique(k):
    u, v = np.meshgrid(np.arange(k), np.arange(k))
    keep = u != v
    return k, _i32(u[keep]), _i32(v[keep])


def in_out_star(k):
    """Hub 0 -> leaves 1..k, leaves k+1..2k -> hub."""
    hub = np.zeros(k, np.int64)
    return 2 * k + 1, _i32(np.concatenate([hub, np.arange(k + 1, 2 * k + 1)])), _i32(
        np.concatenate([np.arange(1, k + 1), hub]))


def cycle_chain(k, length, ascending=True):
    """k disjoint cycles of `length`, cycle i -> cycle i + 1 by one arc; vertex numbers rise along
    the chain, or fall."""
    src, dst = [], []
    for i in range(k):
        base = i * length
        for j in range(length):
            src.append(base + j)
            dst.append(base + (j + 1) % length)
        if i + 1 < k:
            src.append(base)
            dst.append(base + length)
    src, dst = np.array(src), np.array(dst)
    n = k * length
    if not ascending:
        src, dst = n - 1 - src, n - 1 - dst
    return n, _i32(src), _i32(dst)


def planted(lengths, extra, seed):
    """Disjoint cycles of the given lengths (1 = a single vertex, every third of which gets a
    self-loop), `extra` random arcs each from a lower-numbered cycle to a strictly higher one, some
    arcs duplicated, all vertex numbers permuted.  Returns (n, src, dst, comp): comp[v] = the
    cycle v was planted in."""
    rng = np.random.default_rng(seed)
    lengths = list(lengths)
    start = np.concatenate([[0], np.cumsum(lengths)])
    n = int(start[-1])
    comp = np.repeat(np.arange(len(lengths)), lengths)
    src, dst, singles = [], [], 0
    for c, ln in enumerate(lengths):
        base = int(start[c])
        if ln == 1:
            if singles % 3 == 0:
                src.append(base)
                dst.append(base)
            singles += 1
            continue
        for j in range(ln):
            src.append(base + j)
            dst.append(base + (j + 1) % ln)
    if len(lengths) > 1:
        a = rng.integers(0, n, extra)
        b = rng.integers(0, n, extra)
        keep = comp[a] != comp[b]
        a, b = a[keep], b[keep]
        swap = comp[a] > comp[b]
        a, b = np.where(swap, b, a), np.where(swap, a, b)
        src.extend(a.tolist())
        dst.extend(b.tolist())
    src, dst = np.array(src, np.int64), np.array(dst, np.int64)
    dup = rng.integers(0, len(src), max(1, len(src) // 10))
    src, dst = np.concatenate([src, src[dup]]), np.concatenate([dst, dst[dup]])
    p = rng.permutation(n)
    out = np.empty(n, np.int64)
    out[p] = comp
    return n, _i32(p[src]), _i32(p[dst]), out


def gnp_digraph(n, p, seed):
    rng = np.random.default_rng(seed)
    m = rng.random((n, n)) < p
    np.fill_diagonal(m, False)
    s, d = np.nonzero(m)
    return n, _i32(s), _i32(d)
