"""CPU: the ragged graphs (tests/ragged.py) are what they claim to be, and the oracle agrees at
these sizes with a plain numpy restatement of each program written from the scope definitions:
level-synchronous BFS, Bellman-Ford (hop-bounded and converged), walk counts as repeated
int64 mat-vecs wrapped to a Java int, PageRank in np.longdouble.  The device parity tests
(test_gpu_ragged.py) compare the engine with this oracle on the same inputs, and their direction
assertions rest on the bottom-up condition proven here without a device.

ShortestDistance takes a scope; PageRank and DegreeCounter fix theirs (inE messages first, then
outE for the ranks), so those two have one form each.
"""
import functools

import numpy as np
import pytest

import fulgora as fr
from ragged import BIG, LADDER, SIZES, isolated_count, ladder_used, ragged_graph, scope_messages

OUT, IN, BOTH = 0, 1, 2
ABSENT = fr.FR_ABSENT
PR_L1_TOL = 1e-6      # north_star: PageRank within 1e-6 L1
SEED = 7
INF = np.int64(1) << 60


@functools.lru_cache(maxsize=None)
def graph(n):
    src, dst, w, ids, info = ragged_graph(n, SEED)
    return src, dst, w, ids, info, fr.OracleGraph.from_edges(n, src, dst, w, titan_ids=ids)


def seeds_of(n, info):
    s = [info["hub"], n - 1, 0]
    s += [int(v) for v in info["isolated"][:1]]
    if info["rungs"]:
        s += list(info["rungs"][max(info["rungs"])])
    return sorted(set(s))


# ----------------------------------------------------------------------------- the generator
@pytest.mark.parametrize("n", SIZES)
def test_generator_claims(n):
    src, dst, w, ids, info = ragged_graph(n, SEED)
    outdeg = np.bincount(src, minlength=n)
    indeg = np.bincount(dst, minlength=n)
    used = ladder_used(n)
    assert sorted(info["rungs"]) == used
    assert used == ([] if n < 127 else [d for d in LADDER if d <= 65] if n < 1000 else LADDER)
    for d, (vin, vout) in info["rungs"].items():
        assert (indeg[vin], outdeg[vin]) == (d, 1)
        assert (outdeg[vout], indeg[vout]) == (d, 1)
    base = set(info["base"].tolist())
    rung_v = {v for pair in info["rungs"].values() for v in pair}
    for v in rung_v:                                       # a rung's other ends are base vertices
        assert set(dst[src == v].tolist()) | set(src[dst == v].tolist()) <= base
    iso = info["isolated"]
    assert len(iso) == isolated_count(n) == (3 if n >= 4 else n // 2)
    assert (outdeg[iso] == 0).all() and (indeg[iso] == 0).all()
    assert int(((outdeg + indeg) == 0).sum()) >= len(iso)
    assert len(base) == info["nb"] == n - len(iso) - 2 * len(used)
    assert len(base | rung_v | set(iso.tolist())) == n
    assert info["hub"] in base
    assert len(src) == 8 * info["nb"] + sum(2 * (d + 1) for d in used)
    assert ids.dtype == np.int64 and len(ids) == n
    assert (ids % 8 == 0).all() and (ids > 0).all() and (np.diff(ids) >= 8).all()
    if n > 8:
        assert (np.diff(ids) > 8).any()                   # non-contiguous: a seed id is a real lookup
    assert w.dtype == np.int32 and w.min() >= 0 and w.max() <= 40
    if n >= 63:
        assert (w == 0).any() and (w == 40).any()
    if n >= 127:
        pairs = src.astype(np.int64) * n + dst
        assert len(np.unique(pairs)) < len(pairs)         # a duplicate edge
        assert (src == dst).any()                         # a self-loop
    again = ragged_graph(n, SEED)
    assert all(np.array_equal(a, b) for a, b in zip(again[:4], (src, dst, w, ids)))


def test_long_rungs_hold_duplicates():
    """A rung longer than the base holds every base vertex several times over."""
    src, dst, w, ids, info = ragged_graph(1001, SEED)
    vin, vout = info["rungs"][4097]
    assert info["nb"] < 4097
    assert len(np.unique(src[dst == vin])) <= info["nb"] < (dst == vin).sum()
    assert len(np.unique(dst[src == vout])) <= info["nb"] < (src == vout).sum()


# ----------------------------------------------------------------------------- restatements
def np_bfs(n, snd, rcv, seed, depth):
    dist = np.full(n, -1, np.int64)
    dist[seed] = 0
    front = np.zeros(n, bool)
    front[seed] = True
    for level in range(1, depth + 1):
        cand = rcv[front[snd]]
        new = np.unique(cand[dist[cand] < 0])
        if not len(new):
            break
        dist[new] = level
        front[:] = False
        front[new] = True
    return np.where(dist < 0, ABSENT, dist)


def np_bellman_ford(n, snd, rcv, wt, seed, depth):
    """`depth` Jacobi rounds: every round relaxes all message paths from the previous round's
    distances (depth = n is the converged answer: a shortest path has fewer than n hops)."""
    d = np.full(n, INF, np.int64)
    d[seed] = 0
    for _ in range(depth):
        ok = d[snd] < INF
        new = d.copy()
        np.minimum.at(new, rcv[ok], d[snd[ok]] + wt[ok])
        if np.array_equal(new, d):
            break
        d = new
    return np.where(d >= INF, ABSENT, d)


def np_walkcount(n, src, dst, k):
    """Walks of length k along the edges out of every vertex, as a Java int."""
    c = np.ones(n, np.int64)
    for _ in range(k):
        new = np.zeros(n, np.int64)
        np.add.at(new, src.astype(np.int64), c[dst])
        c = ((new + (1 << 31)) % (1 << 32)) - (1 << 31)
    return c.astype(np.int32)


def np_pagerank(n, src, dst, alpha, vertex_count, iters):
    ld = np.longdouble
    if iters == 0:
        return np.full(n, np.nan)
    edge_count = np.bincount(src, minlength=n).astype(ld)
    pr = np.full(n, ld(1) / ld(vertex_count), ld)
    for _ in range(2, iters + 1):
        with np.errstate(divide="ignore"):
            msg = pr / edge_count                          # +inf from a vertex nobody hears
        s = np.zeros(n, ld)
        np.add.at(s, dst.astype(np.int64), msg[src])
        pr = ld(alpha) * s + (ld(1) - ld(alpha)) / ld(vertex_count)
    return pr


# ----------------------------------------------------------------------------- oracle vs numpy
@pytest.mark.parametrize("scope", [OUT, IN, BOTH])
@pytest.mark.parametrize("n", SIZES)
def test_oracle_shortest_distance_equals_numpy(n, scope):
    src, dst, w, ids, info, o = graph(n)
    assert np.array_equal(o.vertex_ids(), ids)
    snd, rcv, wt = scope_messages(scope, src, dst, w)
    for s in seeds_of(n, info):
        for depth in (2, n):
            assert np.array_equal(o.shortest_distance(int(ids[s]), depth, scope)[0], np_bfs(n, snd, rcv, s, depth)), (s, depth)
        for depth in (0, 1, 3, n):
            od = o.shortest_distance(int(ids[s]), depth, scope, weighted=True)[0]
            assert np.array_equal(od, np_bellman_ford(n, snd, rcv, wt, s, depth)), (s, depth)
    s = int(info["isolated"][0]) if len(info["isolated"]) else None
    if s is not None:                                      # reaches only itself
        od = o.shortest_distance(int(ids[s]), n, scope)[0]
        assert od[s] == 0 and (np.delete(od, s) == ABSENT).all()


@pytest.mark.parametrize("n", SIZES)
def test_oracle_in_scope_is_out_scope_on_the_reversed_graph(n):
    src, dst, w, ids, info, o = graph(n)
    rev = fr.OracleGraph.from_edges(n, dst, src, w, titan_ids=ids)
    for s in seeds_of(n, info):
        for weighted in (False, True):
            a = o.shortest_distance(int(ids[s]), n, IN, weighted=weighted)[0]
            b = rev.shortest_distance(int(ids[s]), n, OUT, weighted=weighted)[0]
            assert np.array_equal(a, b), (s, weighted)
            a = o.shortest_distance(int(ids[s]), n, BOTH, weighted=weighted)[0]
            b = rev.shortest_distance(int(ids[s]), n, BOTH, weighted=weighted)[0]
            assert np.array_equal(a, b), (s, weighted)


@pytest.mark.parametrize("n", SIZES)
def test_oracle_walkcount_equals_numpy(n):
    src, dst, w, ids, info, o = graph(n)
    for k in (1, 3, 6):
        assert np.array_equal(o.degree_counter(k)[0], np_walkcount(n, src, dst, k)), k
    if n >= 1001:                                          # k = 6 leaves the int range: the wrap is exercised
        c = np.ones(n, np.float64)
        for _ in range(6):
            new = np.zeros(n)
            np.add.at(new, src.astype(np.int64), c[dst])
            c = new
        assert c.max() > 2.0 ** 31


@pytest.mark.parametrize("n", SIZES)
def test_oracle_pagerank_equals_longdouble(n):
    src, dst, w, ids, info, o = graph(n)
    for iters in (1, 2, 20):
        opr, it = o.pagerank(0.85, n, iters)
        ref = np_pagerank(n, src, dst, 0.85, n, iters)
        assert it == iters
        fin = np.isfinite(ref.astype(np.float64))
        assert np.array_equal(np.isfinite(opr), fin) and fin.all()
        assert float(np.abs(opr[fin] - ref[fin]).sum()) <= PR_L1_TOL, iters


# ----------------------------------------------------------------------------- bottom-up condition
def bottom_up_levels(n, src, dst, root, alpha=30.0):
    """Which BFS levels from `root` in bothE meet the switch condition of the level loop:
    the frontier's entries m_f exceed 1/alpha of the entries m_u of the vertices not yet
    reached (the frontier's own already taken out).  Returns one bool per expanded level."""
    deg = (np.bincount(src, minlength=n) + np.bincount(dst, minlength=n)).astype(np.int64)
    snd, rcv, _ = scope_messages(BOTH, src, dst)
    dist = np_bfs(n, snd, rcv, root, n)
    mu = int(deg.sum())
    out = []
    for level in range(int(dist.max()) + 1):
        mf = int(deg[dist == level].sum())
        mu -= mf
        out.append(mf > mu / alpha)
    return out


@pytest.mark.parametrize("n", [n for n in SIZES if n >= 63])
def test_hub_root_meets_the_bottom_up_condition(n):
    src, dst, w, ids, info, o = graph(n)
    q = bottom_up_levels(n, src, dst, info["hub"])
    assert any(q)
    if n in BIG:
        assert not q[0] and len(q) >= 2
        # below n / 5000 frontier vertices the loop would turn back; at these sizes that is
        # below one vertex, so every level after the first qualifying one runs bottom-up
        assert n / 5000.0 < 1.0
