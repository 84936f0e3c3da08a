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

For the partitioned path (test_ragged_part_cpu.py, test_gpu_ragged_part.py): padded_ragged pads
a ragged graph to whole bitmap words, part_cases names the partitions that put a rank on one
word, on the final word and on nothing but entry-less slots (the only helper here that imports
the product, for SlotPartition, and only when called), and range_fixture / range_reference are
the two-rank PageRank job whose ranks' fixed-point ranges differ, with its exact ranks.
"""
from fractions import Fraction

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


# ----------------------------------------------------------------------------- partitions
def padded_ragged(n, seed):
    """ragged_graph(n, seed) padded with entry-less vertices to whole 64-vertex words:
    (P, src, dst, w, info), P = 64 * ceil(n / 64); the dense indices n..P-1 are pads."""
    src, dst, w, _, info = ragged_graph(n, seed)
    return 64 * ((n + 63) // 64), src, dst, w, info


def part_cases(P, src, dst):
    """[(name, SlotPartition)] over the padded graph.  P = 4160 (n = 4099): a single rank; a
    rank that owns one bitmap word; a last rank that owns the final word (3 real vertices and 61
    pads); entry-balanced ranges; and `empty`, which appends 64 more pads and gives them to a
    rank of their own (part.n = P + 64), a rank without any entry.  P = 1024: equal ranges."""
    from titan_amd.distributed import SlotPartition, word_weights
    if P == 1024:
        return [("equal2", SlotPartition.equal(P, 2)), ("equal4", SlotPartition.equal(P, 4))]
    assert P == 4160, P
    return [("single", SlotPartition([0, P], P)),
            ("one_word", SlotPartition([0, 64, P], P)),
            ("last_word", SlotPartition([0, 2112, 4096, P], P)),
            ("balanced4", SlotPartition.balanced(word_weights(src, dst, 0, P), 4)),
            ("empty", SlotPartition([0, 2112, P, P + 64], P + 64))]


def part_case(P, src, dst, name):
    return dict(part_cases(P, src, dst))[name]


def owner(part, v):
    """The rank that owns caller id v."""
    return int(np.searchsorted(part.bounds, v, side="right") - 1)


# ----------------------------------------------------------------------------- cross-rank range
RANGE_S = 32832                 # vertices per rank: 513 bitmap words
RANGE_D = 32769                 # sources of the long row: 2^15 + 1, so 2^16 is the first power that holds it
RANGE_ALPHA = Fraction(5, 2)


def range_fixture():
    """(n, src, dst, t): two equal ranges of S vertices.  Rank 0 owns t = 0 and nothing else with
    an entry; rank 1 owns D sources s_i = S + i, each with a self-loop and an edge s_i -> t.  Over
    inE the longest in-row of rank 0 (t's) has D entries and that of rank 1 has one."""
    s = RANGE_S + np.arange(RANGE_D, dtype=np.int64)
    src = np.concatenate([s, s]).astype(np.int32)
    dst = np.concatenate([s, np.zeros(RANGE_D, np.int64)]).astype(np.int32)
    return 2 * RANGE_S, src, dst, 0


def range_contributions(iters):
    """[c_1 .. c_iters] of a source as Fractions: x_1 = 1/n, c_k = x_k / 2 (edgeCount 2),
    x_{k+1} = alpha c_k + (1 - alpha) / n (the self-loop is the source's only in-entry)."""
    n = 2 * RANGE_S
    base = (1 - RANGE_ALPHA) / n
    x, c = Fraction(1, n), []
    for _ in range(iters):
        c.append(x / 2)
        x = RANGE_ALPHA * c[-1] + base
    return c


def range_reference(iters):
    """The exact ranks after `iters` iterations, rounded once to float64: every source holds
    x_iters, t holds alpha D c_{iters-1} + (1 - alpha) / n, every other vertex (1 - alpha) / n."""
    n = 2 * RANGE_S
    base = (1 - RANGE_ALPHA) / n
    c = range_contributions(iters)
    pr = np.full(n, float(base))
    pr[RANGE_S:RANGE_S + RANGE_D] = float(2 * c[iters - 1])
    pr[0] = float(RANGE_ALPHA * RANGE_D * c[iters - 2] + base)
    return pr
