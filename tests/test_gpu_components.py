"""GPU: the native weakly-connected-components program (tgo_components, titan_amd/csrc/cc.hip).

The reference is always the fixed point of MIN label propagation over the loaded bothE pull
lists, in one of two forms: the generic ConnectedComponents program driven through the oracle
double (run_generic over OracleEngine), or a numpy restatement that repeats np.minimum.at over
the pull lists until nothing changes.  The fixed point is unique, so every comparison is
bit-exact after reordering by vertex id, and info.components == len(np.unique(reference)).
"""
import numpy as np
import pytest

import fulgora as fr
from conftest import load_fixture
from generic_programs import ConnectedComponents, OracleEngine
from ragged import edge_fixed_point, numpy_fixed_point
from titan_amd import (ClusterCountMapReduce, ClusterPopulationMapReduce, ConnectedComponentVertexProgram, Engine,
                       FulgoraMemory, GpuGraph, Schema, TitanException, TitanGraphComputer, rmat_edges)
from titan_amd import _lib as L
from titan_amd.generic import run_generic

pytestmark = pytest.mark.gpu

BOTH = L.SCOPE_BOTH_E
COMPONENT = ConnectedComponentVertexProgram.COMPONENT


def reorder(ids_from, values, ids_to):
    pos = {int(v): i for i, v in enumerate(ids_from)}
    return np.array([values[pos[int(v)]] for v in ids_to], dtype=np.int64)


def rows_by_id(ids, src, dst):
    """The same graph with its vertices renumbered in increasing id order: load_edges takes the
    rows in the order a scan delivers them, strictly increasing Titan ids."""
    ids = np.asarray(ids, np.int64)
    rank = np.empty(len(ids), np.int32)
    rank[np.argsort(ids)] = np.arange(len(ids), dtype=np.int32)
    return np.sort(ids), rank[src], rank[dst]


def oracle_double(o):
    p = ConnectedComponents()
    verts = run_generic(OracleEngine(o), p, FulgoraMemory(p.memory_compute_keys))
    return verts.ids, np.asarray(verts.property("cc")[0], np.int64)


def check(eng, ref_ids, ref, path=L.CC_HOOK):
    lab, info = eng.components()
    got = reorder(eng.vertex_ids(), lab, ref_ids)
    assert np.array_equal(got, ref)
    assert info["components"] == len(np.unique(ref))
    assert info["path"] == path
    assert info["rounds"] >= 1 and eng.stats()["iterations"] == info["rounds"]
    return lab, info


@pytest.fixture(scope="module")
def rmat11():
    scale = 11
    n = 1 << scale
    src, dst, _ = rmat_edges(scale, 8, seed=31)
    ids = (np.arange(n, dtype=np.int64) + 1) << 3
    return n, src, dst, ids, edge_fixed_point(ids, src, dst)


def test_rmat_equals_oracle_double_and_numpy(rmat11):
    n, src, dst, ids, ref = rmat11
    eng = Engine().load_edges(n, src, dst, BOTH)
    assert np.array_equal(eng.vertex_ids(), ids)
    oids, occ = oracle_double(fr.OracleGraph.from_edges(n, src, dst))
    assert np.array_equal(reorder(oids, occ, ids), ref)          # the two references agree
    lab, info = check(eng, ids, ref)
    again, info2 = eng.components()
    assert np.array_equal(lab, again) and info2 == info           # bitwise equal run to run
    sizes = np.unique(lab, return_counts=True)[1]
    assert (sizes == 1).any() and sizes.max() > n // 2            # singletons and a giant component
    # left on the device and fetched later
    none, _ = eng.components(fetch=False)
    assert none is None and np.array_equal(eng.copy_components(), lab)


def test_rmat_equals_the_generic_program_through_the_computer(rmat11):
    n, src, dst, ids, ref = rmat11
    graph = GpuGraph(edges=(n, src, dst, None))
    native = graph.compute().program(ConnectedComponentVertexProgram.build().create()).submit().get()
    nids, nlab = native.vertex_properties[COMPONENT]
    generic = graph.compute().program(ConnectedComponents()).submit().get()
    gids, (gcc, present) = generic.vertex_properties["cc"]
    assert present.all()
    assert np.array_equal(reorder(nids, nlab, ids), reorder(gids, gcc, ids))
    assert np.array_equal(reorder(nids, nlab, ids), ref)
    # the generic program pays a superstep per hop of the longest label path; the device rounds do not
    assert native.memory().getIteration() >= 1


def test_chain_in_random_order():
    n = 4097                                            # not a multiple of 64; deep trees
    rng = np.random.default_rng(5)
    order = rng.permutation(n)
    src, dst = order[:-1].astype(np.int32), order[1:].astype(np.int32)
    flip = rng.random(n - 1) < 0.5                      # edge directions do not matter
    src, dst = np.where(flip, dst, src), np.where(flip, src, dst)
    ids = rng.permutation(4 * n)[:n].astype(np.int64) * 8 + 24      # a random permutation of distinct multiples of 8
    ids, src, dst = rows_by_id(ids, src, dst)
    ref = edge_fixed_point(ids, src, dst)
    assert (ref == ids.min()).all()
    eng = Engine().load_edges(n, src, dst, BOTH, titan_ids=ids)
    lab, info = check(eng, eng.vertex_ids(), reorder(ids, ref, eng.vertex_ids()))
    assert info["components"] == 1 and (lab == ids.min()).all()
    # not one round per hop (4096 hops): 3 hook launches and two pointer-jumping phases, each
    # at most log2(4096) = 12 halvings of the deepest tree and one launch that finds none left
    assert info["rounds"] <= 3 + 2 * 13


def test_star_hub_has_the_largest_id():
    n = 65
    ids = (np.arange(n, dtype=np.int64) + 10) * 8
    hub, leaf = n - 1, 0                                # rows come in id order
    ids[hub], ids[leaf] = 1 << 20, 8                    # hub: largest id, highest degree; one leaf: smallest id
    others = np.array([v for v in range(n) if v != hub], np.int32)
    src = np.where(others % 2 == 0, hub, others).astype(np.int32)
    dst = np.where(others % 2 == 0, others, hub).astype(np.int32)
    eng = Engine().load_edges(n, src, dst, BOTH, titan_ids=ids)
    assert eng.graph_perm()[hub] == 0                   # the hub got the lowest internal id
    ref = edge_fixed_point(ids, src, dst)
    assert (ref == 8).all()
    lab, info = check(eng, eng.vertex_ids(), reorder(ids, ref, eng.vertex_ids()))
    assert (lab == 8).all() and info["components"] == 1


def test_bridged_cliques_isolated_self_loops_duplicates():
    k, iso = 40, 7
    n = 2 * k + iso
    rng = np.random.default_rng(9)
    ids = (rng.permutation(n).astype(np.int64) + 1) * 8
    a = np.arange(k)
    b = np.arange(k, 2 * k)
    edges = [(int(u), int(v)) for part in (a, b) for i, u in enumerate(part) for v in part[i + 1:]]
    ua = int(a[np.argmax(ids[a])])
    ub = int(b[np.argmax(ids[b])])
    edges.append((ua, ub))                              # the single bridge, between the two largest ids
    edges += [(3, 3), (int(b[5]), int(b[5])), (2 * k + 1, 2 * k + 1)]     # self-loops (one on an isolated vertex)
    edges.append(edges[17])                             # a duplicated edge
    src = np.array([e[0] for e in edges], np.int32)
    dst = np.array([e[1] for e in edges], np.int32)
    ids, src, dst = rows_by_id(ids, src, dst)
    ref = edge_fixed_point(ids, src, dst)
    assert len(np.unique(ref)) == 1 + iso
    eng = Engine().load_edges(n, src, dst, BOTH, titan_ids=ids)
    lab, info = check(eng, eng.vertex_ids(), reorder(ids, ref, eng.vertex_ids()))
    assert info["components"] == 8


@pytest.mark.parametrize("n", [1, 130])
def test_no_edges(n):
    eng = Engine().load_edges(n, np.zeros(0, np.int32), np.zeros(0, np.int32), BOTH)
    lab, info = eng.components()
    assert np.array_equal(lab, eng.vertex_ids())
    assert info["components"] == n and info["path"] == L.CC_HOOK


@pytest.mark.parametrize("fixture", ["gotg", "partition_groups"])
def test_rows_equal_the_oracle_double(fixture):
    rows, vids, sd, npz = load_fixture(fixture)
    o = fr.OracleGraph.from_rows(rows, fr.OracleSchema(sd["edge_types"], [tuple(x) for x in sd["property_keys"]]), BOTH)
    oids, occ = oracle_double(o)
    eng = Engine().load_rows(rows, Schema.from_dict(sd), BOTH)
    assert sorted(eng.vertex_ids()) == sorted(oids)
    lab, info = check(eng, oids, occ)
    assert set(lab.tolist()) <= set(eng.vertex_ids().tolist())     # labels are canonical (executed) ids


def test_non_transpose_lists_take_the_propagate_path():
    """Two halves joined by the single edge u -> v (u in the half holding the smallest id).
    With v's IN entry of that edge removed, v's half no longer hears from u's half while u's
    still hears from v's: the second half keeps its own smallest id, where the symmetric
    lists label everything with the first half's."""
    n, h = 200, 100
    rng = np.random.default_rng(21)
    ids = (np.arange(n, dtype=np.int64) + 1) * 8
    edges = [(i, i + 1) for i in range(h - 1)] + [(i, i + 1) for i in range(h, n - 1)]        # each half connected
    edges += [(int(x), int(y)) for x, y in rng.integers(0, h, (150, 2))]
    edges += [(int(x), int(y)) for x, y in rng.integers(h, n, (150, 2))]
    u, v = 17, 163
    edges.append((u, v))
    src = np.array([e[0] for e in edges], np.int64)
    dst = np.array([e[1] for e in edges], np.int64)
    oo = np.argsort(src, kind="stable")
    io = np.argsort(dst, kind="stable")
    out_idx, in_idx = dst[oo].astype(np.int32), src[io].astype(np.int32)
    in_row = dst[io]
    out_off = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=n))]).astype(np.int64)
    drop = np.nonzero((in_row == v) & (in_idx == u))[0]
    assert len(drop) == 1
    keep = np.ones(len(in_idx), bool)
    keep[drop[0]] = False
    in_idx, in_row = in_idx[keep], in_row[keep]
    in_off = np.concatenate([[0], np.cumsum(np.bincount(in_row, minlength=n))]).astype(np.int64)
    # numpy fixed point over exactly these lists
    recv = np.concatenate([np.repeat(np.arange(n), np.diff(out_off)), in_row])
    send = np.concatenate([out_idx, in_idx]).astype(np.int64)
    ref = numpy_fixed_point(ids, recv, send)
    sym = edge_fixed_point(ids, src, dst)
    assert (sym == ids[0]).all()
    assert (ref[:h] == ids[0]).all() and (ref[h:] == ids[h]).all()       # provably different
    # oracle double over the same lists: each row's OUT entries, then its IN entries
    off = out_off + in_off
    mid = off[:-1] + np.diff(out_off)
    adj = np.empty(off[-1], np.int32)
    for r in range(n):
        adj[off[r]:mid[r]] = out_idx[out_off[r]:out_off[r + 1]]
        adj[mid[r]:off[r + 1]] = in_idx[in_off[r]:in_off[r + 1]]
    oids, occ = oracle_double(fr.OracleGraph.from_adjacency(ids, off, np.ascontiguousarray(mid), adj))
    assert np.array_equal(reorder(oids, occ, ids), ref)
    eng = Engine().load_csr(n, out_off, out_idx, in_off, in_idx, BOTH, titan_ids=ids)
    lab, info = check(eng, ids, ref, path=L.CC_PROPAGATE)
    assert info["components"] == 2
    again, _ = eng.components()
    assert np.array_equal(lab, again)


def test_through_the_computer_with_map_reduces_and_persist():
    rows, vids, sd, npz = load_fixture("gotg")
    key = (7100 << 6) | 5
    graph = GpuGraph(rows, sd, property_keys={COMPONENT: (key, L.DT_LONG)})
    computer = graph.compute()
    computer.resultMode(TitanGraphComputer.ResultMode.PERSIST)
    computer.program(ConnectedComponentVertexProgram.build().create())
    computer.mapReduce(ClusterPopulationMapReduce.build().create())
    computer.mapReduce(ClusterCountMapReduce.build().create())
    res = computer.submit().get()
    ids, lab = res.vertex_properties[COMPONENT]
    assert res.graph() is graph
    o = fr.OracleGraph.from_rows(rows, fr.OracleSchema(sd["edge_types"], [tuple(x) for x in sd["property_keys"]]), BOTH)
    oids, occ = oracle_double(o)
    assert np.array_equal(reorder(ids, lab, oids), occ)
    u, c = np.unique(occ, return_counts=True)
    assert res.memory().get("clusterPopulation") == {int(a): int(b) for a, b in zip(u, c)}
    assert res.memory().get("clusterCount") == len(u)
    for vid, x in zip(ids, lab):
        assert graph.read_property(int(vid), key, L.DT_LONG) == int(x)
    # the device rows equal the oracle's encoder byte for byte, relation ids base + running index
    eng = Engine().load_rows(rows, Schema.from_dict(sd), BOTH)
    with pytest.raises(TitanException) as e:
        eng.result_rows(L.RESULT_COMPONENT, [key], [L.DT_LONG], 1 << 30)      # no finished program yet
    assert e.value.code == L.TGO_E_STATE
    none, _ = eng.components(fetch=False)
    assert none is None
    base = 1 << 30
    got = eng.result_rows(L.RESULT_COMPONENT, [key], [L.DT_LONG], base)
    mine = reorder(ids, lab, eng.vertex_ids())
    assert got.nrows == eng.n
    lib = fr.load()
    for r in range(got.nrows):
        b = bytes(got.data[got.byte_begin[r]:got.byte_begin[r + 1]])
        lv = int(got.limit_valpos[r])
        assert (b, lv & 0x7FFFFFFF) == fr.encode_property(key, L.DT_LONG, int(mine[r]), base + r)
        assert got.keys[r] == lib.fr_key_of(int(eng.vertex_ids()[r]), 5)
    # a generic key carries the Long class; an Integer key holds the labels when they fit
    gen = eng.result_rows(L.RESULT_COMPONENT, [key], [L.DT_OBJECT], base)
    assert bytes(gen.data[:gen.byte_begin[1]]) == fr.encode_property_generic(key, L.DT_LONG, int(mine[0]), base)[0]
    if int(eng.vertex_ids().max()) <= 0x7FFFFFFF:
        small = eng.result_rows(L.RESULT_COMPONENT, [key], [L.DT_INTEGER], base)
        assert bytes(small.data[:small.byte_begin[1]]) == fr.encode_property(key, L.DT_INTEGER, int(mine[0]), base)[0]
    with pytest.raises(TitanException):
        eng.result_rows(L.RESULT_COMPONENT, [key], [L.DT_DOUBLE], base)


def test_errors():
    n = 64
    src = np.arange(n - 1, dtype=np.int32)
    dst = src + 1
    with pytest.raises(TitanException) as e:
        Engine().load_edges(n, src, dst, L.SCOPE_IN_E).components()
    assert e.value.code == L.TGO_E_INVALID
    with pytest.raises(TitanException) as e:
        Engine().components()
    assert e.value.code == L.TGO_E_STATE
