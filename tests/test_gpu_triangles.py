"""GPU: native triangle counting and clustering coefficients (tgo_triangles, titan_amd/csrc/tri.hip).

The reference is always the numpy restatement in triangles_ref.py: the simple undirected
projection as a dense 0/1 matrix, tri = ((A @ A) * A).sum(1) / 2, exact in fp64.  Counts, degrees
and coefficients are compared with array_equal: integers, and one IEEE division of integers.
"""
import ctypes as C

import numpy as np
import pytest

import fulgora as fr
from conftest import load_fixture
from titan_amd import (Engine, GpuGraph, Schema, TitanException, TitanGraphComputer, TransitivityMapReduce,
                       TriangleCountMapReduce, TriangleCountVertexProgram, rmat_edges, synth_rows)
from titan_amd import _lib as L
from triangles_ref import lcc_of, reference, reference_from_lists

pytestmark = pytest.mark.gpu

BOTH = L.SCOPE_BOTH_E
TRI, LCC, DEG = (TriangleCountVertexProgram.TRIANGLES, TriangleCountVertexProgram.CLUSTERING,
                 TriangleCountVertexProgram.DEGREE)


def rows_by_id(ids, src, dst):
    """The same graph with its vertices renumbered in increasing id order: load_edges takes the
    rows in the order a scan delivers them, strictly increasing Titan ids."""
    ids = np.asarray(ids, np.int64)
    rank = np.empty(len(ids), np.int32)
    rank[np.argsort(ids)] = np.arange(len(ids), dtype=np.int32)
    return np.sort(ids), rank[src], rank[dst]


def run(eng):
    """(tri, deg, lcc, info) of one run, every output taken both ways."""
    tri, info = eng.triangles()
    t2, deg, lcc = eng.copy_triangles()
    assert np.array_equal(tri, t2)
    st = eng.stats()
    assert st["iterations"] == 1 and st["last_kernel_ms"] > 0
    return tri, deg, lcc, info


def check(eng, ref):
    rtri, rdeg, rlcc, rinfo = ref
    tri, deg, lcc, info = run(eng)
    assert np.array_equal(tri, rtri)
    assert np.array_equal(deg, rdeg)
    assert lcc.dtype == np.float64 and np.array_equal(lcc, rlcc)       # bit-exact, not merely close
    for k in ("triangles", "wedges", "simple_edges"):
        assert info[k] == rinfo[k], k
    assert info["transitivity"] == (3 * rinfo["triangles"] / rinfo["wedges"] if rinfo["wedges"] else 0.0)
    assert 0 <= info["max_forward"] <= max(int(rdeg.max(initial=0)), 0)
    return tri, deg, lcc, info


def clique(k):
    s, d = np.triu_indices(k, 1)
    return k, s.astype(np.int32), d.astype(np.int32)


def wheel(leaves):
    """Hub 0 joined to a ring 1..leaves."""
    ring = np.arange(1, leaves + 1, dtype=np.int32)
    nxt = np.roll(ring, -1)
    src = np.concatenate([np.zeros(leaves, np.int32), ring])
    dst = np.concatenate([ring, nxt])
    return leaves + 1, src, dst


# ------------------------------------------------------------------ closed forms
@pytest.mark.parametrize("k", [4, 5, 70])
def test_cliques(k):
    n, src, dst = clique(k)
    eng = Engine().load_edges(n, src, dst, BOTH)
    tri, deg, lcc, info = check(eng, reference(n, src, dst))
    each = (k - 1) * (k - 2) // 2
    assert (tri == each).all() and (deg == k - 1).all() and (lcc == 1.0).all()
    assert info["triangles"] == k * (k - 1) * (k - 2) // 6 and info["simple_edges"] == k * (k - 1) // 2
    assert info["max_forward"] == k - 1                 # the last internal vertex sees every other one
    if k == 70:                                         # rows longer than one wave
        assert each == 2346 and info["triangles"] == 54740


def test_wheel_1500():
    n, src, dst = wheel(1500)
    eng = Engine().load_edges(n, src, dst, BOTH)
    tri, deg, lcc, info = check(eng, reference(n, src, dst))
    assert tri[0] == 1500 and (tri[1:] == 2).all()
    assert deg[0] == 1500 and (deg[1:] == 3).all()
    assert info["triangles"] == 1500 and info["simple_edges"] == 3000
    assert lcc[0] == 3000.0 / (1500.0 * 1499.0)


def test_star_chain_and_isolated_vertices_hold_no_triangle():
    n = 65                                              # not a multiple of 64
    leaves = np.arange(1, n, dtype=np.int32)
    src = np.where(leaves % 2 == 0, 0, leaves).astype(np.int32)
    dst = np.where(leaves % 2 == 0, leaves, 0).astype(np.int32)
    tri, deg, lcc, info = check(Engine().load_edges(n, src, dst, BOTH), reference(n, src, dst))
    assert not tri.any() and not lcc.any() and deg[0] == 64 and info["triangles"] == 0 and info["wedges"] == 64 * 63 // 2
    n = 4097
    rng = np.random.default_rng(5)
    order = rng.permutation(n)
    src, dst = order[:-1].astype(np.int32), order[1:].astype(np.int32)
    a = np.zeros(n, np.int64)
    np.add.at(a, src, 1)
    np.add.at(a, dst, 1)
    eng = Engine().load_edges(n, src, dst, BOTH)
    tri, deg, lcc, info = run(eng)                      # (n too large for the dense reference)
    assert not tri.any() and not lcc.any() and np.array_equal(deg, a)
    assert info == {"triangles": 0, "wedges": n - 2, "simple_edges": n - 1, "max_forward": info["max_forward"],
                    "transitivity": 0.0}
    for n in (1, 130):
        eng = Engine().load_edges(n, np.zeros(0, np.int32), np.zeros(0, np.int32), BOTH)
        tri, deg, lcc, info = run(eng)
        assert not tri.any() and not deg.any() and not lcc.any() and len(tri) == n
        assert info == {"triangles": 0, "wedges": 0, "simple_edges": 0, "max_forward": 0, "transitivity": 0.0}


def test_projection_collapses_duplicates_directions_and_self_loops():
    e = np.array([(0, 1), (0, 1), (1, 0), (1, 2), (2, 0), (2, 2)], np.int32)
    eng = Engine().load_edges(4, e[:, 0], e[:, 1], BOTH)             # vertex 3 is isolated
    tri, deg, lcc, info = check(eng, reference(4, e[:, 0], e[:, 1]))
    assert info["triangles"] == 1
    assert deg.tolist() == [2, 2, 2, 0] and lcc.tolist() == [1.0, 1.0, 1.0, 0.0] and tri.tolist() == [1, 1, 1, 0]


# ------------------------------------------------------------------ random graphs
@pytest.fixture(scope="module")
def rmat10():
    scale = 10
    n = 1 << scale
    src, dst, _ = rmat_edges(scale, 8, seed=31)         # hubs, duplicates, self-loops
    assert (src == dst).any() and len(np.unique(src.astype(np.int64) * n + dst)) < len(src)
    return n, src, dst, reference(n, src, dst)


def test_rmat_equals_numpy(rmat10):
    n, src, dst, ref = rmat10
    eng = Engine().load_edges(n, src, dst, BOTH)
    before = eng.stats()["device_bytes"]
    tri, deg, lcc, info = check(eng, ref)
    assert info["triangles"] > 0 and 0 < info["max_forward"] < deg.max()      # the orientation shortens the hubs' rows
    assert eng.stats()["device_bytes"] > before                              # the cached forward lists


def test_gnp_random_directions_and_ids():
    n = 1001
    rng = np.random.default_rng(12)
    s, d = np.triu_indices(n, 1)
    keep = rng.random(len(s)) < 0.05
    s, d = s[keep], d[keep]
    flip = rng.random(len(s)) < 0.5
    src, dst = np.where(flip, d, s).astype(np.int32), np.where(flip, s, d).astype(np.int32)
    ids = rng.permutation(4 * n)[:n].astype(np.int64) * 8 + 24
    ids, src, dst = rows_by_id(ids, src, dst)
    eng = Engine().load_edges(n, src, dst, BOTH, titan_ids=ids)
    assert np.array_equal(eng.vertex_ids(), ids)
    check(eng, reference(n, src, dst))


@pytest.mark.parametrize("graph", ["rmat10", "wheel"])
def test_every_path_gives_the_same_result(graph, rmat10):
    if graph == "rmat10":
        n, src, dst, ref = rmat10
    else:
        n, src, dst = wheel(1500)
        ref = reference(n, src, dst)
    eng = Engine().load_edges(n, src, dst, BOTH)
    longest = check(eng, ref)[3]["max_forward"]
    for wave_row in (1, 4, -1):
        for block_row in (2, 16, -1, longest + 1):
            eng.set_tuning(L.TUNE_TRI_WAVE_ROW, wave_row).set_tuning(L.TUNE_TRI_BLOCK_ROW, block_row)
            check(eng, ref)
    with pytest.raises(TitanException) as e:
        eng.set_tuning(L.TUNE_TRI_WAVE_ROW, 0)
    assert e.value.code == L.TGO_E_INVALID


# ------------------------------------------------------------------ run to run, load to load
def test_run_to_run_fetch_later_and_rows_load(rmat10):
    import edgestore as es
    n, src, dst, ref = rmat10
    eng = Engine().load_edges(n, src, dst, BOTH)
    tri, info = eng.triangles()
    again, info2 = eng.triangles()
    assert np.array_equal(tri, again) and info2 == info
    none, info3 = eng.triangles(fetch=False)
    assert none is None and info3 == info
    t, deg, lcc = eng.copy_triangles()
    assert np.array_equal(t, tri) and np.array_equal(deg, ref[1]) and np.array_equal(lcc, ref[2])
    # the same graph as byte-exact edgestore rows, through the row decoder
    knows = es.user_edge_label(1)
    rows = synth_rows(n, src, dst, None, label_id=knows)
    sd = {"edge_types": [{"type_id": knows, "multiplicity": 0}], "property_keys": []}
    eng2 = Engine().load_rows(rows, Schema.from_dict(sd), BOTH)
    pos = {es.vertex_id(i): i for i in range(n)}
    at = np.array([pos[int(v)] for v in eng2.vertex_ids()], np.int64)
    assert len(np.unique(at)) == eng2.n
    t2, info_rows = eng2.triangles()
    _, d2, l2 = eng2.copy_triangles()
    assert np.array_equal(t2, tri[at]) and np.array_equal(d2, deg[at]) and np.array_equal(l2, lcc[at])
    absent = np.setdiff1d(np.arange(n), at)
    assert not deg[absent].any()                        # only vertices without an edge have no row
    assert {k: info_rows[k] for k in ("triangles", "wedges", "simple_edges")} == \
           {k: info[k] for k in ("triangles", "wedges", "simple_edges")}


# ------------------------------------------------------------------ fixtures: the kernel, not the loader
@pytest.mark.parametrize("fixture", ["gotg", "partition_groups"])
def test_fixture_rows_equal_numpy_over_the_device_lists(fixture):
    rows, vids, sd, npz = load_fixture(fixture)
    eng = Engine().load_rows(rows, Schema.from_dict(sd), BOTH)
    ref = reference_from_lists(eng.graph_csr(0), eng.graph_csr(1), eng.graph_perm())
    check(eng, ref)


# ------------------------------------------------------------------ errors
def test_errors_leave_the_ctx_usable():
    n = 64
    src = np.arange(n - 1, dtype=np.int32)
    dst = src + 1
    eng = Engine().load_edges(n, src, dst, L.SCOPE_IN_E)
    with pytest.raises(TitanException) as e:
        eng.triangles()
    assert e.value.code == L.TGO_E_INVALID
    assert eng.bfs(n - 1, n, L.SCOPE_IN_E, seed_is_dense=True)[0] == n - 1     # messages travel against the edges
    eng = Engine()
    with pytest.raises(TitanException) as e:
        eng.triangles()
    assert e.value.code == L.TGO_E_STATE
    eng.load_edges(n, src, dst, BOTH)
    a = L.TriArgs(BOTH, 1)
    assert eng.lib.tgo_triangles(eng.ctx, C.byref(a), None, None) == L.TGO_E_INVALID
    assert eng.lib.tgo_copy_triangles(eng.ctx, None, None, None) == L.TGO_E_STATE     # no finished run
    assert eng.bfs(0, n, BOTH, seed_is_dense=True)[n - 1] == n - 1
    assert eng.triangles()[1]["triangles"] == 0
    assert eng.lib.tgo_copy_triangles(eng.ctx, None, None, None) == 0                 # every out-pointer may be NULL
    # lists that are not each other's transpose: a triangle 0 -> 1 -> 2 -> 0 whose IN entry of 0 -> 1 is missing
    out_off, out_idx = np.array([0, 1, 2, 3], np.int64), np.array([1, 2, 0], np.int32)
    in_off, in_idx = np.array([0, 1, 1, 2], np.int64), np.array([2, 1], np.int32)
    eng = Engine().load_csr(3, out_off, out_idx, in_off, in_idx, BOTH, titan_ids=np.array([8, 16, 24], np.int64))
    with pytest.raises(TitanException) as e:
        eng.triangles()
    assert e.value.code == L.TGO_E_UNSUPPORTED and "transpose" in str(e.value)
    assert (eng.bfs(0, 3, BOTH, seed_is_dense=True) != L.DIST_ABSENT).all()


# ------------------------------------------------------------------ through the computer
def test_through_the_computer_with_map_reduces(rmat10):
    n, src, dst, ref = rmat10
    graph = GpuGraph(edges=(n, src, dst, None))
    c = graph.compute().program(TriangleCountVertexProgram.build().create())
    c.mapReduce(TriangleCountMapReduce.build().create()).mapReduce(TransitivityMapReduce.build().create())
    res = c.submit().get()
    tri, info = Engine().load_edges(n, src, dst, BOTH).triangles()
    ids, got = res.vertex_properties[TRI]
    assert np.array_equal(got, tri) and np.array_equal(got, ref[0])
    assert np.array_equal(res.vertex_properties[LCC][1], ref[2])
    assert np.array_equal(res.vertex_properties[DEG][1], ref[1])
    assert res.memory().get("triangleCount") == info["triangles"]
    assert res.memory().get("transitivity") == 3 * info["triangles"] / info["wedges"]
    assert res.memory().getIteration() == 1


def test_persist_writes_both_keys():
    rows, vids, sd, npz = load_fixture("gotg")
    kt, kc = (7200 << 6) | 5, (7201 << 6) | 5
    graph = GpuGraph(rows, sd, property_keys={TRI: (kt, L.DT_LONG), LCC: (kc, L.DT_DOUBLE)})
    c = graph.compute()
    c.resultMode(TitanGraphComputer.ResultMode.PERSIST)
    res = c.program(TriangleCountVertexProgram.build().create()).submit().get()
    assert res.graph() is graph
    ids, tri = res.vertex_properties[TRI]
    _, lcc = res.vertex_properties[LCC]
    _, deg = res.vertex_properties[DEG]
    assert tri.sum() > 0 and np.array_equal(lcc, lcc_of(tri, deg))
    for vid, t, x in zip(ids, tri, lcc):
        got_t = graph.read_property(int(vid), kt, L.DT_LONG)
        got_x = graph.read_property(int(vid), kc, L.DT_DOUBLE)
        assert type(got_t) is int and got_t == int(t)
        assert type(got_x) is float and got_x == float(x)
    # the device rows: exactly two entries per vertex, byte for byte the oracle encoder's, relation
    # ids running from the reserved base
    eng = Engine().load_rows(rows, Schema.from_dict(sd), BOTH)
    with pytest.raises(TitanException) as e:
        eng.result_rows(L.RESULT_TRIANGLES, [kt, kc], [L.DT_LONG, L.DT_DOUBLE], 1 << 30)   # no finished program yet
    assert e.value.code == L.TGO_E_STATE
    none, _ = eng.triangles(fetch=False)
    assert none is None
    assert np.array_equal(eng.vertex_ids(), ids)
    base = 1 << 30
    got = eng.result_rows(L.RESULT_TRIANGLES, [kt, kc], [L.DT_LONG, L.DT_DOUBLE], base)
    assert got.nrows == eng.n and list(got.entry_begin) == [2 * r for r in range(eng.n + 1)]
    lib = fr.load()

    def col(k):
        return fr.buf_bytes("fr_write_relation_type", k, 0, 0, 0)

    def want_row(r, enc_t, enc_c):
        ents = sorted([(kt, enc_t), (kc, enc_c)], key=lambda kv: col(kv[0]))
        return b"".join(enc(base + 2 * r + j)[0] for j, (_, enc) in enumerate(ents))

    for r in range(got.nrows):
        b = bytes(got.data[got.byte_begin[r]:got.byte_begin[r + 1]])
        assert b == want_row(r, lambda rel: fr.encode_property(kt, L.DT_LONG, int(tri[r]), rel),
                             lambda rel: fr.encode_property_f64(kc, float(lcc[r]), rel))
        assert got.keys[r] == lib.fr_key_of(int(ids[r]), 5)
    # an Integer count key works on the small graph; generic keys carry the value classes
    small = eng.result_rows(L.RESULT_TRIANGLES, [kt, kc], [L.DT_INTEGER, L.DT_DOUBLE], base)
    assert bytes(small.data[:small.byte_begin[1]]) == want_row(
        0, lambda rel: fr.encode_property(kt, L.DT_INTEGER, int(tri[0]), rel),
        lambda rel: fr.encode_property_f64(kc, float(lcc[0]), rel))
    gen = eng.result_rows(L.RESULT_TRIANGLES, [kt, kc], [L.DT_OBJECT, L.DT_OBJECT], base)
    assert bytes(gen.data[:gen.byte_begin[1]]) == want_row(
        0, lambda rel: fr.encode_property_generic(kt, L.DT_LONG, int(tri[0]), rel),
        lambda rel: fr.encode_property_generic(kc, L.DT_DOUBLE, float(lcc[0]), rel))
    with pytest.raises(TitanException):
        eng.result_rows(L.RESULT_TRIANGLES, [kt, kc], [L.DT_DOUBLE, L.DT_DOUBLE], base)
    with pytest.raises(TitanException):
        eng.result_rows(L.RESULT_TRIANGLES, [kt, kc], [L.DT_LONG, L.DT_LONG], base)
