"""Ragged test graphs: vertex counts off the 64 grid and rows whose length sits exactly on a
dispatch threshold of the kernels.  Pure numpy: no product and no oracle import, so the same
inputs feed the CPU checks of the oracle (test_ragged_cpu.py) and the device parity tests
(test_gpu_ragged.py).

ragged_graph(n, seed) is made of
  * base vertices: 8 * nb edges with skewed endpoints floor(nb * u**2) (hubs, duplicates and
    self-loops), shuffled;
  * isolated vertices (3 when n >= 4): no entry in either direction, so the engine's n_active is
    below n, a seed among them reaches only itself and PageRank sees rows with no entries;
  * a degree ladder: per used d of LADDER two dedicated vertices no base edge touches, an IN
    rung with exactly d in-edges (from base vertices) and one out-edge, and an OUT rung with
    exactly d out-edges and one in-edge.  Endpoints are drawn with replacement, so a rung may be
    longer than nb and holds duplicates.
The roles are spread over the dense indices by a random permutation; weights are int32 in
[0, 40]; the Titan ids are strictly increasing, non-contiguous multiples of 8.
"""
import numpy as np

# one below / on / one above: kSerialRow 32 (cc.hip), the wave width and kCoop 64 (msbfs.hip),
# kSerialScan 256 (bfs.hip), kMaxRows 1024 (engine.hpp), kTileEdges 2048 (frontier.hpp), kTile 4096
# (engine.hpp)
LADDER = [1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097]
SIZES = [1, 2, 3, 63, 64, 65, 127, 129, 1001, 4099]
BIG = [1001, 4099]


def ladder_used(n, ladder=True):
    if not ladder or n < 127:
        return []
    return [d for d in LADDER if d <= 65] if n < 1000 else list(LADDER)


def isolated_count(n):
    return 3 if n >= 4 else n // 2


def ragged_graph(n, seed, ladder=True):
    """(src, dst, w, ids, info): an int32 edge list over dense indices 0..n-1, int32 weights,
    int64 Titan ids per dense index, and info = dict(nb, base, isolated, rungs {d: (in_rung,
    out_rung)}, hub) — hub is the base vertex with the most entries (out + in)."""
    rng = np.random.default_rng([n, seed])
    used = ladder_used(n, ladder)
    iso = isolated_count(n)
    nb = n - iso - 2 * len(used)
    assert nb >= 1, (n, iso, used)
    place = rng.permutation(n).astype(np.int64)           # role -> dense index
    base, isolated, rung_v = place[:nb], place[nb:nb + iso], place[nb + iso:]
    m = 8 * nb
    src = [base[np.floor(nb * rng.random(m) ** 2).astype(np.int64)]]
    dst = [base[np.floor(nb * rng.random(m) ** 2).astype(np.int64)]]
    rungs = {}
    for k, d in enumerate(used):
        vin, vout = int(rung_v[2 * k]), int(rung_v[2 * k + 1])
        rungs[d] = (vin, vout)
        src += [base[rng.integers(0, nb, d)], np.array([vin]), np.full(d, vout), base[rng.integers(0, nb, 1)]]
        dst += [np.full(d, vin), base[rng.integers(0, nb, 1)], base[rng.integers(0, nb, d)], np.array([vout])]
    src = np.concatenate(src)
    dst = np.concatenate(dst)
    order = rng.permutation(len(src))
    src, dst = src[order].astype(np.int32), dst[order].astype(np.int32)
    w = rng.integers(0, 41, len(src)).astype(np.int32)
    ids = 8 * np.cumsum(rng.integers(1, 5, n)).astype(np.int64)
    deg = np.bincount(src, minlength=n) + np.bincount(dst, minlength=n)
    hub = int(base[np.argmax(deg[base])])
    info = {"nb": nb, "base": base, "isolated": isolated, "rungs": rungs, "hub": hub}
    return src, dst, w, ids, info


def low_degree_vertex(n, src, dst, info):
    """The base vertex with the fewest entries among those that have any."""
    deg = np.bincount(src, minlength=n) + np.bincount(dst, minlength=n)
    base = info["base"]
    return int(base[np.argmin(np.where(deg[base] > 0, deg[base], np.iinfo(np.int64).max))])


def draw_seeds(n, info, nseeds, seed):
    """nseeds dense indices drawn with replacement; the first ones are replaced by the largest
    OUT rung, an isolated vertex and the largest IN rung where the graph has them (as many as
    fit), so every draw that can holds an isolated and a rung vertex."""
    rng = np.random.default_rng([n, nseeds, seed])
    seeds = rng.integers(0, n, nseeds).astype(np.int64)
    forced = []
    if info["rungs"]:
        forced.append(info["rungs"][max(info["rungs"])][1])
    if len(info["isolated"]):
        forced.append(int(info["isolated"][0]))
    if info["rungs"]:
        forced.append(info["rungs"][max(info["rungs"])][0])
    forced = forced[:nseeds]
    seeds[:len(forced)] = forced
    return seeds


def scope_messages(scope, src, dst, w=None):
    """(sender, receiver, weight) of every message path of a ShortestDistance scope: a vertex
    sends over the scope's edges, so outE carries a message along an edge (tail to head), inE
    against it and bothE both ways.  scope: 0 outE, 1 inE, 2 bothE."""
    src = np.asarray(src, np.int64)
    dst = np.asarray(dst, np.int64)
    ww = np.ones(len(src), np.int64) if w is None else np.asarray(w, np.int64)
    if scope == 0:
        return src, dst, ww
    if scope == 1:
        return dst, src, ww
    return np.concatenate([src, dst]), np.concatenate([dst, src]), np.concatenate([ww, ww])


def numpy_fixed_point(ids, recv, send):
    """label[recv] = min(label[recv], label[send]) over every pull entry until nothing changes."""
    lab = np.asarray(ids, np.int64).copy()
    while True:
        new = lab.copy()
        np.minimum.at(new, recv, lab[send])
        if np.array_equal(new, lab):
            return lab
        lab = new


def edge_fixed_point(ids, src, dst):
    """bothE pull lists of an edge list: a row pulls over its OUT and its IN entries."""
    src = np.asarray(src, np.int64)
    dst = np.asarray(dst, np.int64)
    return numpy_fixed_point(ids, np.concatenate([src, dst]), np.concatenate([dst, src]))
