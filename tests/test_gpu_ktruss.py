"""GPU: native k-truss decomposition (tgo_ktruss, titan_amd/csrc/truss.hip).

The reference is always truss_ref.py (a host peel over Python sets on the simple undirected
projection; test_truss_cpu.py checks it against the definitional fixed point and closed forms).
Truss values and supports are integers and the decomposition is unique: every comparison is
array_equal, edge rows are compared after a lexsort by (u, v), and info is compared for max_truss,
innermost_edges, triangles, simple_edges and levels.  rounds is a diagnostic.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

import fulgora as fr
import kcore_ref as kr
import truss_ref as tr
from conftest import load_fixture
from titan_amd import (Engine, GpuGraph, KTrussVertexProgram, MaxTrussMapReduce, Schema, TitanException,
                       TitanGraphComputer, TrussSizeMapReduce, rmat_edges, synth_rows)
from titan_amd import _lib as L
from triangles_ref import reference as tri_reference

pytestmark = pytest.mark.gpu

BOTH = L.SCOPE_BOTH_E
TRUSS = KTrussVertexProgram.TRUSS
INFO = tr.INFO
NONE = (np.zeros(0, np.int32), np.zeros(0, np.int32))


def rows_by_id(ids, src, dst):
    """The same graph with its vertices renumbered in increasing id order: load_edges takes the
    rows in the order a scan delivers them, strictly increasing Titan ids."""
    ids = np.asarray(ids, np.int64)
    rank = np.empty(len(ids), np.int32)
    rank[np.argsort(ids)] = np.arange(len(ids), dtype=np.int32)
    return np.sort(ids), rank[src], rank[dst]


def edges_of(eng):
    """The engine's edge result as sorted rows; every pair comes ordered, every edge once."""
    u, v, t, s = eng.copy_truss_edges()
    assert all(x.dtype == np.int64 for x in (u, v, t, s)) and (u < v).all()
    rows = tr.edge_rows(u, v, t, s)
    assert len(np.unique(rows[:, :2], axis=0)) == len(rows)
    return rows


def check(eng, ref, want_edges=None, **kw):
    """One run against (vtruss, info, edges) of the reference, the result taken both ways.
    want_edges: the reference's rows under the engine's Titan ids (default: vertex i = vertex_ids()[i])."""
    rv, rinfo, redges = ref
    vtruss, info = eng.ktruss(**kw)
    assert vtruss.dtype == np.int64 and np.array_equal(vtruss, rv)
    assert np.array_equal(eng.copy_truss(), vtruss)
    for k in INFO:
        assert info[k] == rinfo[k], k
    assert info["rounds"] >= 0
    assert eng.stats()["iterations"] == info["levels"]
    rows = edges_of(eng)
    if want_edges is None:
        want_edges = tr.with_ids(redges, eng.vertex_ids())
    assert np.array_equal(rows, want_edges)
    if kw.get("k", 0) == 0:
        assert int(rows[:, 3].sum()) == 3 * info["triangles"]
    return vtruss, info, rows


# ------------------------------------------------------------------ closed forms
@pytest.mark.parametrize("k", [4, 5, 70])
def test_cliques(k):
    n, src, dst = kr.clique(k)
    vtruss, info, rows = check(Engine().load_edges(n, src, dst, BOTH), tr.reference(n, src, dst))
    assert (vtruss == k).all() and (rows[:, 2] == k).all() and (rows[:, 3] == k - 2).all()   # K70: rows longer than a wave
    assert info["levels"] == 1 and info["innermost_edges"] == k * (k - 1) // 2


def test_book_1500_the_spine_is_not_driven_below_its_level():
    n, src, dst = tr.book(1500)
    eng = Engine().load_edges(n, src, dst, BOTH)
    vtruss, info, rows = check(eng, tr.reference(n, src, dst))
    assert (rows[:, 2] == 3).all() and (vtruss == 3).all() and info["levels"] == 1
    assert int(rows[:, 3].max()) == 1500 and int((rows[:, 3] == 1).sum()) == 3000
    # the 3 000 page edges are the level's first sub-round: their 1 500 triangles each lower the spine
    # once, all but 1 499 of those decrements are undone, and the spine joins the second sub-round
    print("rounds", info["rounds"])
    assert info["rounds"] >= 2


def test_star_and_graphs_without_an_edge():
    n, src, dst = kr.star(64)                           # n = 65, mixed directions
    vtruss, info, rows = check(Engine().load_edges(n, src, dst, BOTH), tr.reference(n, src, dst))
    assert n == 65 and (vtruss == 2).all() and (rows[:, 2] == 2).all() and info["levels"] == 1
    for n in (1, 130):
        eng = Engine().load_edges(n, *NONE, BOTH)
        vtruss, info, rows = check(eng, tr.reference(n, *NONE))
        assert len(vtruss) == n and not vtruss.any() and rows.shape == (0, 4)
        assert info == {"max_truss": 0, "innermost_edges": 0, "triangles": 0, "simple_edges": 0, "levels": 0, "rounds": 0}


def test_clique_chain():
    n, src, dst, core = kr.clique_chain(2, 40)
    vtruss, info, rows = check(Engine().load_edges(n, src, dst, BOTH), tr.reference(n, src, dst))
    assert n == 819 and np.array_equal(vtruss, core + 1)            # bridges 2, every clique its size
    assert int((rows[:, 2] == 2).sum()) == 1 + 38                   # K_2 and the 38 bridges
    assert info["levels"] == len(np.unique(rows[:, 2])) == 39 and info["max_truss"] == 40
    assert info["innermost_edges"] == 40 * 39 // 2


def test_empty_levels_are_skipped_not_launched():
    _, s1, d1 = kr.clique(70)
    _, s2, d2 = kr.star(64, base=70)
    n, src, dst = 135, np.concatenate([s1, s2]), np.concatenate([d1, d2])
    vtruss, info, rows = check(Engine().load_edges(n, src, dst, BOTH), tr.reference(n, src, dst))
    assert sorted(set(rows[:, 2].tolist())) == [2, 70] and info["levels"] == 2
    # The bound, from the design: a level costs one launch per sub-round.  The star's edges are in no
    # triangle (settled without a launch), the clique's edges all start at the level and drop
    # nothing: one sub-round.  One more per level is allowed, as the k-core test allows.  Launching
    # the 67 empty levels 3 .. 69 would give 69.
    print("rounds", info["rounds"])
    assert info["rounds"] <= 2 * info["levels"]


def test_projection_collapses_duplicates_directions_and_self_loops():
    e = np.array([(0, 1), (0, 1), (1, 0), (1, 2), (2, 0), (2, 2)], np.int32)
    eng = Engine().load_edges(4, e[:, 0], e[:, 1], BOTH)             # vertex 3 is isolated
    vtruss, info, rows = check(eng, tr.reference(4, e[:, 0], e[:, 1]))
    assert vtruss.tolist() == [3, 3, 3, 0] and len(rows) == 3
    assert (rows[:, 2] == 3).all() and (rows[:, 3] == 1).all() and info["triangles"] == 1


# ------------------------------------------------------------------ random graphs
@pytest.fixture(scope="module")
def rmat10():
    scale = 10
    n = 1 << scale
    src, dst, _ = rmat_edges(scale, 8, seed=31)         # hubs, duplicates, self-loops
    assert (src == dst).any() and len(np.unique(src.astype(np.int64) * n + dst)) < len(src)
    ref = tr.reference(n, src, dst)
    # the facts this file relies on: several levels, a row longer than a wave, vertices without a neighbour
    off, _ = kr.projection(n, src, dst)
    assert ref[1]["simple_edges"] == 6015 and ref[1]["triangles"] == 23749
    assert sorted(set(ref[2][:, 2].tolist())) == list(range(2, 17)) and ref[1]["levels"] == 15
    assert int(np.diff(off).max()) == 338 and int((np.diff(off) == 0).sum()) == 221
    return n, src, dst, ref


def test_rmat_equals_the_reference(rmat10):
    n, src, dst, ref = rmat10
    vtruss, info, rows = check(Engine().load_edges(n, src, dst, BOTH), ref)
    assert int((vtruss == 0).sum()) == 221 and info["max_truss"] == 16
    assert int(rows[:, 3].sum()) == 3 * 23749


def test_gnp_random_directions_and_ids():
    n, src, dst, rng = kr.gnp(1001, 0.05, 12)
    ids = rng.permutation(4 * n)[:n].astype(np.int64) * 8 + 24
    ref = tr.reference(n, src, dst)
    want = tr.with_ids(ref[2], ids)                     # the reference's rows under the Titan ids
    sids, s, d = rows_by_id(ids, src, dst)
    eng = Engine().load_edges(n, s, d, BOTH, titan_ids=sids)
    assert np.array_equal(eng.vertex_ids(), sids)
    vt = ref[0][np.argsort(ids)]                        # row r of the load is the vertex with the r-th smallest id
    vtruss, info, rows = check(eng, (vt, ref[1], ref[2]), want_edges=want)
    assert set(rows[:, 0].tolist()) | set(rows[:, 1].tolist()) <= set(ids.tolist())
    assert info["max_truss"] >= 3


@pytest.mark.parametrize("graph", ["rmat10", "book", "chain"])
def test_every_path_gives_the_same_bytes(graph, rmat10):
    if graph == "rmat10":
        n, src, dst, ref = rmat10
    else:
        n, src, dst = tr.book(1500) if graph == "book" else kr.clique_chain(2, 40)[:3]
        ref = tr.reference(n, src, dst)
    eng = Engine().load_edges(n, src, dst, BOTH)
    first, _, first_rows = check(eng, ref)
    # wave_row / block_row: which of the support pass's lane, wave and block kernels takes a forward row
    # (1: every row of two entries or more, 10**6: none); peel_wave_row: a lane or the wave per frontier edge
    for wave_row, block_row, peel in itertools.product((0, 1, 4, 10**6), (0, 1, 10**6), (0, 1, 10**6)):
        vtruss, _ = eng.ktruss(wave_row=wave_row, block_row=block_row, peel_wave_row=peel)
        assert vtruss.tobytes() == first.tobytes(), (wave_row, block_row, peel)
        assert edges_of(eng).tobytes() == first_rows.tobytes(), (wave_row, block_row, peel)
    for bad in ({"wave_row": -1}, {"block_row": -1}, {"peel_wave_row": -7}):
        with pytest.raises(TitanException) as e:
            eng.ktruss(**bad)
        assert e.value.code == L.TGO_E_INVALID
    check(eng, ref)


# ------------------------------------------------------------------ one walk, two credit policies
def gnp64_and_an_isolated_vertex():
    """65 vertices: a ragged last word of rows, and rows of fewer than two forward entries."""
    s, d = np.triu_indices(64, 1)
    rng = np.random.default_rng(65)
    keep = rng.random(len(s)) < 0.3
    flip = rng.random(len(s)) < 0.5
    s, d = s[keep], d[keep]
    flip = flip[keep]
    return 65, np.where(flip, d, s).astype(np.int32), np.where(flip, s, d).astype(np.int32)


@pytest.fixture(scope="module")
def walk_graphs(rmat10):
    graphs = {"clique70": kr.clique(70),                # forward rows of up to 69 entries: one past a wave
              "rmat10": rmat10[:3],
              "gnp64+1": gnp64_and_an_isolated_vertex()}
    return {name: (g, tri_reference(*g)[0]) for name, g in graphs.items()}


FAR = 10**6                                             # a row length above every forward row
ROW_CLASSES = {"lane": (FAR, FAR), "wave": (1, FAR), "block": (FAR, 2)}     # (wave_row, block_row)


@pytest.mark.parametrize("rows", list(ROW_CLASSES))
@pytest.mark.parametrize("graph", ["clique70", "rmat10", "gnp64+1"])
def test_edge_credits_sum_to_vertex_credits(graph, rows, walk_graphs):
    """tgo_ktruss's supports and tgo_triangles' counts come from one enumeration: per vertex, the
    supports of its edges add up to twice its triangles, whichever kernel walks the rows."""
    (n, src, dst), tri_ref = walk_graphs[graph]
    wave_row, block_row = ROW_CLASSES[rows]
    eng = Engine().load_edges(n, src, dst, BOTH)
    eng.set_tuning(L.TUNE_TRI_WAVE_ROW, wave_row).set_tuning(L.TUNE_TRI_BLOCK_ROW, block_row)
    _, tinfo = eng.triangles(fetch=False)
    tri = eng.copy_triangles()[0]
    assert tri_ref.any() and np.array_equal(tri, tri_ref)           # (not zero on both sides)
    _, info = eng.ktruss(wave_row=wave_row, block_row=block_row)
    u, v, _, sup = eng.copy_truss_edges()
    ids = eng.vertex_ids()
    order = np.argsort(ids)
    at = lambda x: order[np.searchsorted(ids[order], x)]             # the row of a Titan id
    per_vertex = np.zeros(n, np.int64)
    np.add.at(per_vertex, at(u), sup)
    np.add.at(per_vertex, at(v), sup)
    assert np.array_equal(per_vertex, 2 * tri)
    assert info["triangles"] == tinfo["triangles"]


# ------------------------------------------------------------------ k
def test_k_clamps_and_stops_the_peel(rmat10):
    n, src, dst, ref = rmat10
    eng = Engine().load_edges(n, src, dst, BOTH)
    vtruss, info, rows = check(eng, tr.clamp(ref, 2), k=2)          # nothing is peeled
    assert (rows[:, 2] == 2).all() and info["levels"] == 1 and info["rounds"] == 0
    assert info["innermost_edges"] == 6015 and info["max_truss"] == 2
    full_rounds = eng.ktruss()[1]["rounds"]
    for k in (3, 5, 16, 40):
        want = tr.clamp(ref, k)
        assert np.array_equal(want[2][:, 2], np.minimum(ref[2][:, 2], k))
        vtruss, info, rows = check(eng, want, k=k)
        assert info["max_truss"] == min(k, 16) and info["levels"] == len(np.unique(rows[:, 2]))
        assert info["innermost_edges"] == int((ref[2][:, 2] >= min(k, 16)).sum())
        assert np.array_equal(rows[:, 3], ref[2][:, 3])             # the support is the initial one
        print("k", k, "rounds", info["rounds"], "of", full_rounds)
    for k in (1, -1):
        with pytest.raises(TitanException) as e:
            eng.ktruss(k=k)
        assert e.value.code == L.TGO_E_INVALID
    check(eng, ref)


# ------------------------------------------------------------------ run to run, load to load
def test_run_to_run_fetch_later_and_rows_load(rmat10):
    import edgestore as es
    n, src, dst, ref = rmat10
    eng = Engine().load_edges(n, src, dst, BOTH)
    vtruss, info = eng.ktruss()
    cols = eng.copy_truss_edges()
    again, info2 = eng.ktruss()
    cols2 = eng.copy_truss_edges()
    assert vtruss.tobytes() == again.tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(cols, cols2))         # unsorted: the order is the load's
    assert {k: info2[k] for k in INFO} == {k: info[k] for k in INFO}            # rounds may differ
    none, info3 = eng.ktruss(fetch=False)
    assert none is None and {k: info3[k] for k in INFO} == {k: info[k] for k in INFO}
    assert np.array_equal(eng.copy_truss(), vtruss) and np.array_equal(vtruss, ref[0])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(cols, eng.copy_truss_edges()))
    # the same graph as byte-exact edgestore rows, through the row decoder
    knows = es.user_edge_label(1)
    rows = synth_rows(n, src, dst, None, label_id=knows)
    sd = {"edge_types": [{"type_id": knows, "multiplicity": 0}], "property_keys": []}
    eng2 = Engine().load_rows(rows, Schema.from_dict(sd), BOTH)
    pos = {es.vertex_id(i): i for i in range(n)}
    at = np.array([pos[int(v)] for v in eng2.vertex_ids()], np.int64)
    assert len(np.unique(at)) == eng2.n
    v2, info_rows = eng2.ktruss()
    assert np.array_equal(v2, vtruss[at])
    assert not vtruss[np.setdiff1d(np.arange(n), at)].any()     # only vertices without an edge have no row
    assert {k: info_rows[k] for k in INFO} == {k: info[k] for k in INFO}
    assert np.array_equal(edges_of(eng2), tr.with_ids(ref[2], [es.vertex_id(i) for i in range(n)]))


def test_beside_triangles_kcore_and_betweenness_on_one_ctx(rmat10):
    n, src, dst, ref = rmat10
    tref = tri_reference(n, src, dst)
    cref = kr.reference(n, src, dst)
    seeds = [0, 5, 17]
    out = np.zeros(n, np.int64)
    p64 = L.ptr(out, C.c_int64)
    eng = Engine().load_edges(n, src, dst, BOTH)
    tri, tinfo = eng.triangles()
    core, _ = eng.kcore()
    bc, _ = eng.betweenness(seeds, dense=True)
    assert np.array_equal(tri, tref[0]) and np.array_equal(core, cref[0])
    assert eng.lib.tgo_copy_truss(eng.ctx, p64) == L.TGO_E_STATE
    assert eng.lib.tgo_copy_truss_edges(eng.ctx, None, None, None, None) == L.TGO_E_STATE
    before = eng.stats()["device_bytes"]
    vtruss, info, _ = check(eng, ref)
    grown = eng.stats()["device_bytes"]
    assert grown > before                               # the edge ids of the adjacency, the per-edge arrays
    assert info["triangles"] == tinfo["triangles"] == tref[0].sum() // 3
    has = cref[0] > 0
    assert (vtruss[has] <= cref[0][has] + 1).all() and not vtruss[~has].any()
    # the other programs' copies answer TGO_E_STATE now
    assert eng.lib.tgo_copy_cores(eng.ctx, p64) == L.TGO_E_STATE
    assert eng.lib.tgo_copy_triangles(eng.ctx, None, None, None) == L.TGO_E_STATE
    assert eng.lib.tgo_copy_betweenness(eng.ctx, L.ptr(np.zeros(n), C.c_double)) == L.TGO_E_STATE
    check(eng, ref)
    assert eng.stats()["device_bytes"] == grown         # nothing more on the second run
    # their results are unchanged afterwards, and each of them takes the truss result away again
    tri2, _ = eng.triangles()
    t2, deg, lcc = eng.copy_triangles()
    assert np.array_equal(tri2, tref[0]) and np.array_equal(deg, tref[1]) and np.array_equal(lcc, tref[2])
    with pytest.raises(TitanException) as e:
        eng.copy_truss()
    assert e.value.code == L.TGO_E_STATE
    assert np.array_equal(eng.kcore()[0], core)
    with pytest.raises(TitanException) as e:
        eng.copy_truss_edges()
    assert e.value.code == L.TGO_E_STATE
    assert eng.betweenness(seeds, dense=True)[0].tobytes() == bc.tobytes()
    check(eng, ref)
    assert eng.stats()["device_bytes"] == grown
    # the other order on a fresh ctx: the k-truss run builds the forward lists and the simple adjacency,
    # triangles and betweenness share them; with the k-core's backward lists both ctxs hold the same bytes
    eng2 = Engine().load_edges(n, src, dst, BOTH)
    check(eng2, ref)
    alone = eng2.stats()["device_bytes"]
    assert np.array_equal(eng2.triangles()[0], tref[0]) and eng2.stats()["device_bytes"] == alone
    assert eng2.betweenness(seeds, dense=True)[0].tobytes() == bc.tobytes()
    assert np.array_equal(eng2.kcore()[0], core)
    check(eng2, ref)
    assert eng2.stats()["device_bytes"] == grown


# ------------------------------------------------------------------ fixtures: vertex cuts
@pytest.mark.parametrize("fixture", ["gotg", "partition_groups"])
def test_fixture_rows_equal_the_reference_over_the_device_lists(fixture):
    rows, vids, sd, npz = load_fixture(fixture)
    eng = Engine().load_rows(rows, Schema.from_dict(sd), BOTH)
    ref = tr.reference_from_lists(eng.graph_csr(0), eng.graph_csr(1), eng.graph_perm())
    check(eng, ref)                                     # (the rows' endpoints are row indices: named by vertex_ids())


# ------------------------------------------------------------------ errors
def test_errors_leave_the_ctx_usable():
    n = 64
    src = np.arange(n - 1, dtype=np.int32)
    dst = src + 1
    eng = Engine().load_edges(n, src, dst, L.SCOPE_IN_E)            # not bothE
    with pytest.raises(TitanException) as e:
        eng.ktruss()
    assert e.value.code == L.TGO_E_INVALID
    assert eng.bfs(n - 1, n, L.SCOPE_IN_E, seed_is_dense=True)[0] == n - 1
    a = L.TrussArgs(BOTH, 0, 0, 0, 0, 0)                             # bothE, but not the loaded scope
    assert eng.lib.tgo_ktruss(eng.ctx, C.byref(a), None, None) == L.TGO_E_INVALID
    assert eng.bfs(n - 1, n, L.SCOPE_IN_E, seed_is_dense=True)[0] == n - 1
    eng = Engine()                                                   # before a load
    with pytest.raises(TitanException) as e:
        eng.ktruss()
    assert e.value.code == L.TGO_E_STATE
    eng.load_edges(n, src, dst, BOTH)
    a = L.TrussArgs(BOTH, 1, 0, 0, 0, 0)                             # flags
    assert eng.lib.tgo_ktruss(eng.ctx, C.byref(a), None, None) == L.TGO_E_INVALID
    out = np.zeros(n, np.int64)
    p64 = L.ptr(out, C.c_int64)
    assert eng.lib.tgo_copy_truss(eng.ctx, p64) == L.TGO_E_STATE                        # no finished run
    assert eng.lib.tgo_copy_truss_edges(eng.ctx, p64, None, None, None) == L.TGO_E_STATE
    assert eng.bfs(0, n, BOTH, seed_is_dense=True)[n - 1] == n - 1
    assert eng.lib.tgo_copy_truss(eng.ctx, p64) == L.TGO_E_STATE                        # ktruss is not the last program
    assert eng.lib.tgo_copy_truss_edges(eng.ctx, p64, None, None, None) == L.TGO_E_STATE
    assert (eng.ktruss()[0] == 2).all()
    assert eng.lib.tgo_copy_truss_edges(eng.ctx, None, None, None, None) == L.TGO_OK    # each array may be NULL
    # lists that are not each other's transpose: a triangle 0 -> 1 -> 2 -> 0 whose IN entry of 0 -> 1 is missing
    out_off, out_idx = np.array([0, 1, 2, 3], np.int64), np.array([1, 2, 0], np.int32)
    in_off, in_idx = np.array([0, 1, 1, 2], np.int64), np.array([2, 1], np.int32)
    eng = Engine().load_csr(3, out_off, out_idx, in_off, in_idx, BOTH, titan_ids=np.array([8, 16, 24], np.int64))
    with pytest.raises(TitanException) as e:
        eng.ktruss()
    assert e.value.code == L.TGO_E_UNSUPPORTED and "transpose" in str(e.value)
    assert (eng.bfs(0, 3, BOTH, seed_is_dense=True) != L.DIST_ABSENT).all()
    # a partitioned ctx; the same ctx then takes a one-GPU load and runs
    eng = Engine().load_partition(n, 0, n, src, dst, BOTH)
    with pytest.raises(TitanException) as e:
        eng.ktruss()
    assert e.value.code == L.TGO_E_UNSUPPORTED
    eng.load_edges(n, src, dst, BOTH)
    assert eng.bfs(0, n, BOTH, seed_is_dense=True)[n - 1] == n - 1
    assert (eng.ktruss()[0] == 2).all()


# ------------------------------------------------------------------ through the computer
def test_through_the_computer_with_map_reduces(rmat10):
    n, src, dst, ref = rmat10
    graph = GpuGraph(edges=(n, src, dst, None))
    c = graph.compute().program(KTrussVertexProgram.build().create())
    c.mapReduce(MaxTrussMapReduce.build().create()).mapReduce(TrussSizeMapReduce.build().create())
    res = c.submit().get()
    ids, got = res.vertex_properties[TRUSS]
    assert np.array_equal(got, ref[0])
    assert res.memory().get("maxTruss") == ref[1]["max_truss"]
    u, cnt = np.unique(ref[0], return_counts=True)
    assert res.memory().get("trussSizes") == {int(k): int(v) for k, v in zip(u, cnt)}
    assert res.memory().getIteration() == ref[1]["levels"]
    want = tr.clamp(ref, 5)
    res = graph.compute().program(KTrussVertexProgram.build().k(5).create()).submit().get()
    assert np.array_equal(res.vertex_properties[TRUSS][1], want[0])
    assert res.memory().getIteration() == want[1]["levels"]


def test_persist_writes_the_truss_number():
    rows, vids, sd, npz = load_fixture("gotg")
    kt = (7400 << 6) | 5
    graph = GpuGraph(rows, sd, property_keys={TRUSS: (kt, L.DT_LONG)})
    c = graph.compute()
    c.resultMode(TitanGraphComputer.ResultMode.PERSIST)
    res = c.program(KTrussVertexProgram.build().create()).submit().get()
    assert res.graph() is graph
    ids, vtruss = res.vertex_properties[TRUSS]
    assert vtruss.max() > 2
    for vid, x in zip(ids, vtruss):
        got = graph.read_property(int(vid), kt, L.DT_LONG)
        assert type(got) is int and got == int(x)
    # the device rows: one entry per vertex, byte for byte the oracle encoder's, relation ids running
    # from the reserved base
    eng = Engine().load_rows(rows, Schema.from_dict(sd), BOTH)
    base = 1 << 30
    with pytest.raises(TitanException) as e:
        eng.result_rows(L.RESULT_TRUSS, [kt], [L.DT_LONG], base)     # no finished program yet
    assert e.value.code == L.TGO_E_STATE
    none, info = eng.ktruss(fetch=False)
    assert none is None and np.array_equal(eng.vertex_ids(), ids)
    assert eng.stats()["iterations"] == info["levels"]
    lib = fr.load()
    for dt, enc in ((L.DT_LONG, lambda x, rel: fr.encode_property(kt, L.DT_LONG, x, rel)),
                    (L.DT_INTEGER, lambda x, rel: fr.encode_property(kt, L.DT_INTEGER, x, rel)),
                    (L.DT_OBJECT, lambda x, rel: fr.encode_property_generic(kt, L.DT_LONG, x, rel))):
        got = eng.result_rows(L.RESULT_TRUSS, [kt], [dt], base)
        assert got.nrows == eng.n and list(got.entry_begin) == list(range(eng.n + 1))
        for r in range(got.nrows):
            b = bytes(got.data[got.byte_begin[r]:got.byte_begin[r + 1]])
            assert b == enc(int(vtruss[r]), base + r)[0], (dt, r)
            assert got.keys[r] == lib.fr_key_of(int(ids[r]), 5)
    with pytest.raises(TitanException) as e:
        eng.result_rows(L.RESULT_TRUSS, [kt], [L.DT_DOUBLE], base)
    assert e.value.code == L.TGO_E_INVALID
    assert np.array_equal(eng.copy_truss(), vtruss)                 # the refused call left the result in place
    with pytest.raises(TitanException) as e:
        eng.result_rows(L.RESULT_CORE, [kt], [L.DT_LONG], base)      # another kind is not this result
    assert e.value.code == L.TGO_E_STATE
