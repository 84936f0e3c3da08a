"""GPU: native k-core decomposition (tgo_kcore, titan_amd/csrc/core.hip).

The reference is always kcore_ref.py (Batagelj-Zaversnik peeling on the simple undirected
projection; test_kcore_cpu.py checks it against closed forms and the H-index fixed point).  Core
numbers are integers and the decomposition is unique: every comparison is array_equal, and info is
compared for degeneracy, innermost, simple_edges and levels.  rounds is a diagnostic.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

import fulgora as fr
import kcore_ref as kr
from conftest import load_fixture
from kcore_generic import GenericKCore, simple_edges
from titan_amd import (CoreSizeMapReduce, DegeneracyMapReduce, Engine, GpuGraph, KCoreVertexProgram, Schema,
                       TitanException, TitanGraphComputer, rmat_edges, synth_rows)
from titan_amd import _lib as L
from triangles_ref import reference as tri_reference

pytestmark = pytest.mark.gpu

BOTH = L.SCOPE_BOTH_E
CORE = KCoreVertexProgram.CORE
INFO = ("degeneracy", "innermost", "simple_edges", "levels")
NONE = (np.zeros(0, np.int32), np.zeros(0, np.int32))


def rows_by_id(ids, src, dst):
    """The same graph with its vertices renumbered in increasing id order: load_edges takes the
    rows in the order a scan delivers them, strictly increasing Titan ids."""
    ids = np.asarray(ids, np.int64)
    rank = np.empty(len(ids), np.int32)
    rank[np.argsort(ids)] = np.arange(len(ids), dtype=np.int32)
    return np.sort(ids), rank[src], rank[dst]


def check(eng, ref):
    """One run against (core, info) of the reference, the result taken both ways."""
    rcore, rinfo = ref
    core, info = eng.kcore()
    assert core.dtype == np.int64 and np.array_equal(core, rcore)
    assert np.array_equal(eng.copy_cores(), core)
    for k in INFO:
        assert info[k] == rinfo[k], k
    assert info["rounds"] >= (1 if rinfo["simple_edges"] else 0)
    assert eng.stats()["iterations"] == info["levels"]
    return core, info


# ------------------------------------------------------------------ closed forms
@pytest.mark.parametrize("k", [4, 5, 70])
def test_cliques(k):
    n, src, dst = kr.clique(k)
    core, info = check(Engine().load_edges(n, src, dst, BOTH), kr.reference(n, src, dst))
    assert (core == k - 1).all() and info["levels"] == 1 and info["innermost"] == k     # K70: rows longer than a wave


def test_wheel_1500_the_hub_is_not_driven_below_its_level():
    n, src, dst = kr.wheel(1500)
    core, info = check(Engine().load_edges(n, src, dst, BOTH), kr.reference(n, src, dst))
    # 1500 ring vertices peeled in one level all decrement the hub: all but one of them undo
    assert (core == 3).all() and core[0] == 3 and info["levels"] == 1 and info["degeneracy"] == 3


def test_star_and_graphs_without_an_edge():
    n, src, dst = kr.star(64)                           # n = 65, mixed directions
    core, info = check(Engine().load_edges(n, src, dst, BOTH), kr.reference(n, src, dst))
    assert n == 65 and (core == 1).all()
    for n in (1, 130):
        eng = Engine().load_edges(n, *NONE, BOTH)
        core, info = check(eng, kr.reference(n, *NONE))
        assert len(core) == n and not core.any()
        assert info == {"degeneracy": 0, "innermost": 0, "simple_edges": 0, "levels": 0, "rounds": 0}


def test_path_in_random_order():
    n, src, dst = kr.random_path(4097)                  # one level of 2048 dependent steps
    core, info = check(Engine().load_edges(n, src, dst, BOTH), kr.reference(n, src, dst))
    assert (core == 1).all() and info["levels"] == 1 and info["simple_edges"] == n - 1 and info["innermost"] == n
    # The bound, from the design: the level starts with the two end vertices, which one workgroup
    # takes; each of its 2 048 steps drops at most two vertices, which the default LDS queue (far
    # more than two entries) holds, so the workgroup walks both halves of the path itself and
    # nothing reaches a second launch.  One more launch is allowed, as in the skip test.
    print("rounds", info["rounds"])
    assert info["rounds"] <= 2


def test_clique_chain():
    n, src, dst, want = kr.clique_chain(2, 40)
    core, info = check(Engine().load_edges(n, src, dst, BOTH), kr.reference(n, src, dst))
    assert n == 819 and np.array_equal(core, want)
    assert info["levels"] == 39 and info["degeneracy"] == 39 and info["innermost"] == 40


def test_empty_levels_are_skipped_not_launched():
    _, s1, d1 = kr.clique(70)
    _, s2, d2 = kr.star(64, base=70)
    n, src, dst = 135, np.concatenate([s1, s2]), np.concatenate([d1, d2])
    eng = Engine().load_edges(n, src, dst, BOTH)
    eng.set_tuning(L.TUNE_CORE_TAIL, 0)                 # the skip, not the one-launch tail
    core, info = check(eng, kr.reference(n, src, dst))
    assert sorted(set(core.tolist())) == [1, 69] and info["levels"] == 2
    # The bound, from the design: a level costs one launch per chain of drops that leaves its
    # workgroup.  Both levels here fit one workgroup (64 leaves, 70 clique vertices <= 256) and drop
    # at most one vertex (the star's centre), which the default LDS queue holds: one launch each.
    # One more per level is allowed for a drop that went to the next launch instead.  Launching the
    # 67 empty levels 2 .. 68 would give 69.
    print("rounds", info["rounds"])
    assert info["rounds"] <= 2 * info["levels"]


def test_projection_collapses_duplicates_directions_and_self_loops():
    e = np.array([(0, 1), (0, 1), (1, 0), (1, 2), (2, 0), (2, 2)], np.int32)
    eng = Engine().load_edges(4, e[:, 0], e[:, 1], BOTH)             # vertex 3 is isolated
    core, info = check(eng, kr.reference(4, e[:, 0], e[:, 1]))
    assert core.tolist() == [2, 2, 2, 0] and info["levels"] == 2     # a peel over the raw entries starts 0 at 4


# ------------------------------------------------------------------ random graphs
@pytest.fixture(scope="module")
def rmat10():
    scale = 10
    n = 1 << scale
    src, dst, _ = rmat_edges(scale, 8, seed=31)         # hubs, duplicates, self-loops
    assert (src == dst).any() and len(np.unique(src.astype(np.int64) * n + dst)) < len(src)
    return n, src, dst, kr.reference(n, src, dst)


def test_rmat_equals_the_reference(rmat10):
    n, src, dst, ref = rmat10
    core, info = check(Engine().load_edges(n, src, dst, BOTH), ref)
    assert info["degeneracy"] > 3 and info["levels"] > 3 and (core == 0).any()


def test_gnp_random_directions_and_ids():
    n, src, dst, rng = kr.gnp(1001, 0.05, 12)
    ids = rng.permutation(4 * n)[:n].astype(np.int64) * 8 + 24
    ids, src, dst = rows_by_id(ids, src, dst)
    eng = Engine().load_edges(n, src, dst, BOTH, titan_ids=ids)
    assert np.array_equal(eng.vertex_ids(), ids)
    check(eng, kr.reference(n, src, dst))


@pytest.mark.parametrize("graph", ["rmat10", "wheel", "path"])
def test_every_path_gives_the_same_result(graph, rmat10):
    if graph == "rmat10":
        n, src, dst, ref = rmat10
    else:
        n, src, dst = kr.wheel(1500) if graph == "wheel" else kr.random_path(4097)
        ref = kr.reference(n, src, dst)
    eng = Engine().load_edges(n, src, dst, BOTH)
    first = check(eng, ref)[0]
    # wave_row: lane or wave walks; tail: never, late, from the start (n), default; LDS queue of one
    # entry: all but one drop of a step spill to the next launch
    for wave_row, tail, queue in itertools.product((1, 4, -1), (0, 64, n, -1), (1, -1)):
        eng.set_tuning(L.TUNE_CORE_WAVE_ROW, wave_row).set_tuning(L.TUNE_CORE_TAIL, tail)
        eng.set_tuning(L.TUNE_CORE_LDS_QUEUE, queue)
        core, _ = check(eng, ref)
        assert core.tobytes() == first.tobytes(), (wave_row, tail, queue)
    for key, bad in ((L.TUNE_CORE_WAVE_ROW, 0), (L.TUNE_CORE_LDS_QUEUE, 0), (L.TUNE_CORE_LDS_QUEUE, 4097),
                     (L.TUNE_CORE_TAIL, 0.5)):
        with pytest.raises(TitanException) as e:
            eng.set_tuning(key, bad)
        assert e.value.code == L.TGO_E_INVALID
    check(eng, ref)


# ------------------------------------------------------------------ run to run, load to load
def test_run_to_run_fetch_later_and_rows_load(rmat10):
    import edgestore as es
    n, src, dst, ref = rmat10
    eng = Engine().load_edges(n, src, dst, BOTH)
    core, info = eng.kcore()
    again, info2 = eng.kcore()
    assert np.array_equal(core, again)
    assert {k: info2[k] for k in INFO} == {k: info[k] for k in INFO}        # rounds may differ
    none, info3 = eng.kcore(fetch=False)
    assert none is None and {k: info3[k] for k in INFO} == {k: info[k] for k in INFO}
    assert np.array_equal(eng.copy_cores(), core) and np.array_equal(core, ref[0])
    # the same graph as byte-exact edgestore rows, through the row decoder
    knows = es.user_edge_label(1)
    rows = synth_rows(n, src, dst, None, label_id=knows)
    sd = {"edge_types": [{"type_id": knows, "multiplicity": 0}], "property_keys": []}
    eng2 = Engine().load_rows(rows, Schema.from_dict(sd), BOTH)
    pos = {es.vertex_id(i): i for i in range(n)}
    at = np.array([pos[int(v)] for v in eng2.vertex_ids()], np.int64)
    assert len(np.unique(at)) == eng2.n
    c2, info_rows = eng2.kcore()
    assert np.array_equal(c2, core[at])
    assert not core[np.setdiff1d(np.arange(n), at)].any()       # only vertices without an edge have no row
    assert {k: info_rows[k] for k in INFO if k != "levels"} == {k: info[k] for k in INFO if k != "levels"}
    assert info_rows["levels"] == len(np.unique(c2))


def test_beside_triangles_on_one_ctx(rmat10):
    n, src, dst, ref = rmat10
    tref = tri_reference(n, src, dst)
    eng = Engine().load_edges(n, src, dst, BOTH)
    tri, _ = eng.triangles()
    assert np.array_equal(tri, tref[0])
    assert eng.lib.tgo_copy_cores(eng.ctx, L.ptr(np.zeros(n, np.int64), C.c_int64)) == L.TGO_E_STATE
    before = eng.stats()["device_bytes"]
    check(eng, ref)
    grown = eng.stats()["device_bytes"]
    assert grown > before                               # the backward lists
    assert eng.lib.tgo_copy_triangles(eng.ctx, None, None, None) == L.TGO_E_STATE
    tri, _ = eng.triangles()                            # the degrees were not consumed by the peel
    t2, deg, lcc = eng.copy_triangles()
    assert np.array_equal(tri, tref[0]) and np.array_equal(deg, tref[1]) and np.array_equal(lcc, tref[2])
    with pytest.raises(TitanException) as e:
        eng.copy_cores()
    assert e.value.code == L.TGO_E_STATE
    check(eng, ref)
    assert eng.stats()["device_bytes"] == grown
    # the other order on a fresh ctx: the k-core run builds the forward lists, triangles shares them
    eng = Engine().load_edges(n, src, dst, BOTH)
    check(eng, ref)
    grown = eng.stats()["device_bytes"]
    assert np.array_equal(eng.triangles()[0], tref[0]) and eng.stats()["device_bytes"] == grown


# ------------------------------------------------------------------ fixtures: vertex cuts
@pytest.mark.parametrize("fixture", ["gotg", "partition_groups"])
def test_fixture_rows_equal_the_reference_over_the_device_lists(fixture):
    rows, vids, sd, npz = load_fixture(fixture)
    eng = Engine().load_rows(rows, Schema.from_dict(sd), BOTH)
    check(eng, kr.reference_from_lists(eng.graph_csr(0), eng.graph_csr(1), eng.graph_perm()))


# ------------------------------------------------------------------ errors
def test_errors_leave_the_ctx_usable():
    n = 64
    src = np.arange(n - 1, dtype=np.int32)
    dst = src + 1
    eng = Engine().load_edges(n, src, dst, L.SCOPE_IN_E)            # not bothE
    with pytest.raises(TitanException) as e:
        eng.kcore()
    assert e.value.code == L.TGO_E_INVALID
    assert eng.bfs(n - 1, n, L.SCOPE_IN_E, seed_is_dense=True)[0] == n - 1
    a = L.CoreArgs(BOTH, 0)                                          # bothE, but not the loaded scope
    assert eng.lib.tgo_kcore(eng.ctx, C.byref(a), None, None) == L.TGO_E_INVALID
    assert eng.bfs(n - 1, n, L.SCOPE_IN_E, seed_is_dense=True)[0] == n - 1
    eng = Engine()                                                   # before a load
    with pytest.raises(TitanException) as e:
        eng.kcore()
    assert e.value.code == L.TGO_E_STATE
    eng.load_edges(n, src, dst, BOTH)
    a = L.CoreArgs(BOTH, 1)                                          # flags
    assert eng.lib.tgo_kcore(eng.ctx, C.byref(a), None, None) == L.TGO_E_INVALID
    out = np.zeros(n, np.int64)
    assert eng.lib.tgo_copy_cores(eng.ctx, L.ptr(out, C.c_int64)) == L.TGO_E_STATE      # no finished run
    assert eng.bfs(0, n, BOTH, seed_is_dense=True)[n - 1] == n - 1
    assert eng.lib.tgo_copy_cores(eng.ctx, L.ptr(out, C.c_int64)) == L.TGO_E_STATE      # kcore is not the last program
    assert (eng.kcore()[0] == 1).all()
    # lists that are not each other's transpose: a triangle 0 -> 1 -> 2 -> 0 whose IN entry of 0 -> 1 is missing
    out_off, out_idx = np.array([0, 1, 2, 3], np.int64), np.array([1, 2, 0], np.int32)
    in_off, in_idx = np.array([0, 1, 1, 2], np.int64), np.array([2, 1], np.int32)
    eng = Engine().load_csr(3, out_off, out_idx, in_off, in_idx, BOTH, titan_ids=np.array([8, 16, 24], np.int64))
    with pytest.raises(TitanException) as e:
        eng.kcore()
    assert e.value.code == L.TGO_E_UNSUPPORTED and "transpose" in str(e.value)
    assert (eng.bfs(0, 3, BOTH, seed_is_dense=True) != L.DIST_ABSENT).all()
    # a partitioned ctx; the same ctx then takes a one-GPU load and runs
    eng = Engine().load_partition(n, 0, n, src, dst, BOTH)
    with pytest.raises(TitanException) as e:
        eng.kcore()
    assert e.value.code == L.TGO_E_UNSUPPORTED
    eng.load_edges(n, src, dst, BOTH)
    assert eng.bfs(0, n, BOTH, seed_is_dense=True)[n - 1] == n - 1
    assert (eng.kcore()[0] == 1).all()


# ------------------------------------------------------------------ through the computer
def test_through_the_computer_with_map_reduces(rmat10):
    n, src, dst, ref = rmat10
    graph = GpuGraph(edges=(n, src, dst, None))
    c = graph.compute().program(KCoreVertexProgram.build().create())
    c.mapReduce(DegeneracyMapReduce.build().create()).mapReduce(CoreSizeMapReduce.build().create())
    res = c.submit().get()
    ids, got = res.vertex_properties[CORE]
    assert np.array_equal(got, ref[0])
    assert res.memory().get("degeneracy") == ref[1]["degeneracy"]
    u, cnt = np.unique(ref[0], return_counts=True)
    assert res.memory().get("coreSizes") == {int(k): int(v) for k, v in zip(u, cnt)}
    assert res.memory().getIteration() == ref[1]["levels"]


def test_persist_writes_the_core_number():
    rows, vids, sd, npz = load_fixture("gotg")
    kc = (7300 << 6) | 5
    graph = GpuGraph(rows, sd, property_keys={CORE: (kc, L.DT_LONG)})
    c = graph.compute()
    c.resultMode(TitanGraphComputer.ResultMode.PERSIST)
    res = c.program(KCoreVertexProgram.build().create()).submit().get()
    assert res.graph() is graph
    ids, core = res.vertex_properties[CORE]
    assert core.max() > 0
    for vid, x in zip(ids, core):
        got = graph.read_property(int(vid), kc, L.DT_LONG)
        assert type(got) is int and got == int(x)
    # the device rows: one entry per vertex, byte for byte the oracle encoder's, relation ids running
    # from the reserved base
    eng = Engine().load_rows(rows, Schema.from_dict(sd), BOTH)
    base = 1 << 30
    with pytest.raises(TitanException) as e:
        eng.result_rows(L.RESULT_CORE, [kc], [L.DT_LONG], base)      # no finished program yet
    assert e.value.code == L.TGO_E_STATE
    none, _ = eng.kcore(fetch=False)
    assert none is None and np.array_equal(eng.vertex_ids(), ids)
    lib = fr.load()
    for dt, enc in ((L.DT_LONG, lambda x, rel: fr.encode_property(kc, L.DT_LONG, x, rel)),
                    (L.DT_INTEGER, lambda x, rel: fr.encode_property(kc, L.DT_INTEGER, x, rel)),
                    (L.DT_OBJECT, lambda x, rel: fr.encode_property_generic(kc, L.DT_LONG, x, rel))):
        got = eng.result_rows(L.RESULT_CORE, [kc], [dt], base)
        assert got.nrows == eng.n and list(got.entry_begin) == list(range(eng.n + 1))
        for r in range(got.nrows):
            b = bytes(got.data[got.byte_begin[r]:got.byte_begin[r + 1]])
            assert b == enc(int(core[r]), base + r)[0], (dt, r)
            assert got.keys[r] == lib.fr_key_of(int(ids[r]), 5)
    with pytest.raises(TitanException) as e:
        eng.result_rows(L.RESULT_CORE, [kc], [L.DT_DOUBLE], base)
    assert e.value.code == L.TGO_E_INVALID
    assert np.array_equal(eng.copy_cores(), core)                   # the refused call left the result in place


# ------------------------------------------------------------------ native equals generic
def test_native_equals_the_generic_program():
    scale = 11
    n = 1 << scale
    src, dst, _ = rmat_edges(scale, 8, seed=31)
    src, dst = simple_edges(n, src, dst)                            # deduplicated, loop-free
    graph = GpuGraph(edges=(n, src, dst, None))
    native = graph.compute().program(KCoreVertexProgram.build().create()).submit().get()
    nids, ncore = native.vertex_properties[CORE]
    generic = graph.compute().program(GenericKCore()).submit().get()
    gids, (gcore, present) = generic.vertex_properties["core"]
    assert present.all() and np.array_equal(nids, gids)
    assert np.asarray(gcore, np.int64).tobytes() == np.asarray(ncore, np.int64).tobytes()
    assert np.array_equal(ncore, kr.reference(n, src, dst)[0])
    # the generic program pays a superstep per sweep of the fixed point; the native levels are the core values
    assert generic.memory().getIteration() >= 2 and native.memory().getIteration() == len(np.unique(ncore))
