"""GPU: native strongly connected components (tgo_scc, titan_amd/csrc/scc.hip).

The reference is always scc_ref.py (an iterative Tarjan; test_scc_cpu.py checks it against closed
forms, a reachability closure and scipy).  Labels are Titan ids and the partition is unique: every
comparison is array_equal on int64 labels, and info is compared for components, largest and
singletons.  rounds and passes are diagnostics: printed, and bounded where the design gives a bound.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

import fulgora as fr
import scc_ref as sr
from conftest import load_fixture
from scc_generic import GenericScc
from titan_amd import (Engine, GpuGraph, Schema, SccSizeMapReduce, StronglyConnectedComponentsVertexProgram,
                       TitanException, TitanGraphComputer, rmat_edges)
from titan_amd import _lib as L

pytestmark = pytest.mark.gpu

BOTH = L.SCOPE_BOTH_E
COMPONENT = StronglyConnectedComponentsVertexProgram.COMPONENT
INFO = ("components", "largest", "singletons")
NONE = (np.zeros(0, np.int32), np.zeros(0, np.int32))


def rows_by_id(ids, src, dst):
    """The same graph with its vertices renumbered in increasing id order: load_edges takes the
    rows in the order a scan delivers them, strictly increasing Titan ids."""
    ids = np.asarray(ids, np.int64)
    rank = np.empty(len(ids), np.int32)
    rank[np.argsort(ids)] = np.arange(len(ids), dtype=np.int32)
    return np.sort(ids), rank[src], rank[dst]


def tune(eng, wave_row=-1, tail=-1, trim=-1, pivot=-1):
    eng.set_tuning(L.TUNE_SCC_WAVE_ROW, wave_row).set_tuning(L.TUNE_SCC_TAIL, tail)
    eng.set_tuning(L.TUNE_SCC_TRIM, trim).set_tuning(L.TUNE_SCC_PIVOT, pivot)
    return eng


def check(eng, ref, rows=True):
    """One run against (labels, info) of the reference, the result taken both ways.  rows: the
    reference's labels are row numbers (the smallest row of a component, which carries its smallest
    Titan id when the ids rise with the rows); otherwise they are Titan ids already."""
    rlab, rinfo = ref
    if rows:
        ids = eng.vertex_ids()
        assert (np.diff(ids) > 0).all()
        rlab = ids[rlab]
    lab, info = eng.scc()
    assert lab.dtype == np.int64 and np.array_equal(lab, rlab)
    assert np.array_equal(eng.copy_scc(), lab)
    for k in INFO:
        assert info[k] == rinfo[k], k
    assert eng.stats()["iterations"] == info["rounds"]
    return lab, info


@pytest.fixture(scope="module")
def planted():
    n, src, dst, comp = sr.planted(range(1, 61), 3000, 3)
    ids = np.random.default_rng(17).permutation(4 * n)[:n].astype(np.int64) * 8 + 24
    by_construction = sr.labels_of(comp, ids)
    ids_sorted, s2, d2 = rows_by_id(ids, src, dst)
    rank = np.argsort(np.argsort(ids))                   # vertex -> its row
    want = np.empty(n, np.int64)
    want[rank] = by_construction[0]
    ref = sr.reference(n, s2, d2, ids_sorted)
    assert n == 1830 and np.array_equal(ref[0], want) and ref[1] == by_construction[1]
    assert ref[1] == {"components": 60, "largest": 60, "singletons": 1}
    return n, s2, d2, ids_sorted, ref


@pytest.fixture(scope="module")
def rmat10():
    n = 1 << 10
    src, dst, _ = rmat_edges(10, 8, seed=31)            # hubs, duplicates, self-loops
    ref = sr.reference(n, src, dst)
    assert ref[1]["largest"] > 1 and ref[1]["singletons"] > 0 and (src == dst).any()
    return n, src, dst, ref


@pytest.fixture(scope="module")
def cycle1500():
    n, src, dst = sr.random_cycle(1500)
    return n, src, dst, sr.reference(n, src, dst)


# ------------------------------------------------------------------ closed forms
def test_projection_rules():
    e = np.array([(0, 1), (0, 1), (1, 0), (1, 2), (2, 2), (3, 3)], np.int32)
    ref = sr.reference(5, e[:, 0], e[:, 1])
    assert ref[0].tolist() == [0, 0, 2, 3, 4]
    for trim in (1, 0):                                  # the self-loops neither keep 2 and 3 from trimming nor glue them
        lab, info = check(tune(Engine().load_edges(5, e[:, 0], e[:, 1], BOTH), trim=trim), ref)
        assert info["components"] == 4 and info["largest"] == 2 and info["singletons"] == 3


@pytest.mark.parametrize("n", [1, 130])
def test_no_entries(n):
    eng = Engine().load_edges(n, *NONE, BOTH)
    lab, info = check(eng, sr.reference(n, *NONE))
    assert np.array_equal(lab, eng.vertex_ids())
    assert info == {"components": n, "largest": 1, "singletons": n, "rounds": 0, "passes": 0}


def test_two_cycle_clique_and_star():
    check(Engine().load_edges(2, np.array([0, 1], np.int32), np.array([1, 0], np.int32), BOTH),
          (np.zeros(2, np.int64), {"components": 1, "largest": 2, "singletons": 0}))
    n, src, dst = sr.bidirected_clique(70)               # rows longer than a wave
    lab, info = check(Engine().load_edges(n, src, dst, BOTH), sr.reference(n, src, dst))
    assert info["components"] == 1 and info["largest"] == 70
    n, src, dst = sr.in_out_star(1500)                   # 3 000 leaves decrement the hub's two words
    lab, info = check(Engine().load_edges(n, src, dst, BOTH), sr.reference(n, src, dst))
    assert n == 3001 and info["singletons"] == n and info["passes"] == 0


def test_dipath_in_random_order():
    n, src, dst = sr.random_dipath(4097)
    lab, info = check(Engine().load_edges(n, src, dst, BOTH), sr.reference(n, src, dst))
    assert info["singletons"] == n and info["passes"] == 0
    # The bound, from the design: the first launch computes the degrees and retires the path's two
    # ends; one workgroup takes both, each of its steps retires at most two more vertices, which its
    # LDS queue (256 entries) holds, so it follows the path from both ends itself and nothing
    # reaches another launch: 2 launches.  One more is allowed for a vertex that spilled.
    print("rounds", info["rounds"])
    assert info["rounds"] <= 3


def test_cycle_4097_on_the_grid():
    n, src, dst = sr.random_cycle(4097)                  # one more than the largest tail: the pivot's reach runs
    lab, info = check(Engine().load_edges(n, src, dst, BOTH), sr.reference(n, src, dst))
    assert info["components"] == 1 and info["largest"] == n and info["passes"] == 0
    # The bound, from the design: the degrees' launch, each reach following the cycle from its
    # workgroup's LDS queue in one launch, and the trim walk of the retired cycle: 4.  One more is
    # allowed per reach for a vertex that spilled.  A launch per hop would be more than 8 000.
    print("rounds", info["rounds"])
    assert info["rounds"] <= 6


def test_cycle_1500(cycle1500):
    n, src, dst, ref = cycle1500
    eng = Engine().load_edges(n, src, dst, BOTH)
    lab, info = check(eng, ref)
    # The bound, from the design: the degrees' launch (nothing trims), then 1500 <= the default
    # tail, so one workgroup finishes in one launch: 2.
    print("tail rounds", info["rounds"], "passes", info["passes"])
    assert info["rounds"] == 2 and info["passes"] == 1 and info["largest"] == n
    # colouring on the grid, the MAX travels round the cycle: at most live + 1 propagation launches,
    # beside the degrees' launch, the backward marks and the trim walk of the retired cycle
    lab, info = check(tune(eng, tail=0, pivot=0), ref)
    print("grid rounds", info["rounds"], "passes", info["passes"])
    assert info["passes"] == 1 and info["largest"] == n and 3 <= info["rounds"] <= n + 8


@pytest.mark.parametrize("forward", [True, False])
@pytest.mark.parametrize("pivot", [1, 0])
def test_two_cycles_and_a_bridge(forward, pivot):
    n, src, dst = sr.two_cycles_bridge(40, 70, forward)
    ref = sr.reference(n, src, dst)
    assert ref[1] == {"components": 2, "largest": 70, "singletons": 0}
    # tail 0: the pivot's forward reach covers both cycles, its backward reach one
    check(tune(Engine().load_edges(n, src, dst, BOTH), tail=0, pivot=pivot), ref)


def test_cycle_chain_in_both_orders():
    labs = []
    for asc in (True, False):
        n, src, dst = sr.cycle_chain(40, 3, asc)
        ref = sr.reference(n, src, dst)
        eng = tune(Engine().load_edges(n, src, dst, BOTH), tail=0, trim=0, pivot=0)
        lab, info = check(eng, ref)
        print("ascending" if asc else "descending", "passes", info["passes"], "rounds", info["rounds"])
        assert info["components"] == 40 and info["largest"] == 3 and info["singletons"] == 0
        if not asc:
            assert info["passes"] >= 2       # the chain's head carries the largest colour into every cycle
        labs.append(lab)
        check(tune(eng), ref)
    assert np.array_equal(np.sort(labs[0]), np.sort(labs[1]))
    assert np.array_equal(labs[0], eng.vertex_ids()[np.repeat(np.arange(0, 120, 3), 3)])


# ------------------------------------------------------------------ planted and random graphs
def test_planted_components_with_shuffled_ids(planted):
    n, src, dst, ids, ref = planted
    eng = Engine().load_edges(n, src, dst, BOTH, titan_ids=ids)
    assert np.array_equal(eng.vertex_ids(), ids)
    lab, info = check(eng, ref, rows=False)
    assert sorted(np.unique(lab, return_counts=True)[1].tolist()) == list(range(1, 61))


def test_rmat_and_gnp_equal_the_reference(rmat10):
    n, src, dst, ref = rmat10
    check(Engine().load_edges(n, src, dst, BOTH), ref)
    n, src, dst = sr.gnp_digraph(1001, 0.0012, 7)
    ref = sr.reference(n, src, dst)
    assert ref[1]["largest"] > 9 and ref[1]["components"] - ref[1]["singletons"] >= 3
    check(Engine().load_edges(n, src, dst, BOTH), ref)


@pytest.mark.parametrize("graph", ["planted", "rmat10", "cycle1500"])
def test_every_path_gives_the_same_result(graph, planted, rmat10, cycle1500):
    if graph == "planted":
        n, src, dst, ids, ref = planted
    else:
        n, src, dst, ref = rmat10 if graph == "rmat10" else cycle1500
        ids = None
    eng = Engine().load_edges(n, src, dst, BOTH, titan_ids=ids)
    rows = ids is None
    first = check(eng, ref, rows)[0]
    for wave_row, tail, trim, pivot in itertools.product((1, 4, -1), (0, 64, -1), (0, 1), (0, 1)):
        lab, info = check(tune(eng, wave_row, tail, trim, pivot), ref, rows)
        assert lab.tobytes() == first.tobytes(), (wave_row, tail, trim, pivot)
    for key, bad in ((L.TUNE_SCC_WAVE_ROW, 0), (L.TUNE_SCC_TAIL, 0.5), (L.TUNE_SCC_TRIM, 2), (L.TUNE_SCC_PIVOT, 0.5)):
        with pytest.raises(TitanException) as e:
            eng.set_tuning(key, bad)
        assert e.value.code == L.TGO_E_INVALID
    check(tune(eng, tail=1 << 20), ref, rows)            # larger values mean 4096
    check(tune(eng), ref, rows)


# ------------------------------------------------------------------ fixtures: vertex cuts, rows load
@pytest.mark.parametrize("fixture", ["gotg", "partition_groups"])
def test_fixture_rows_equal_the_reference_over_the_device_lists(fixture):
    rows, vids, sd, npz = load_fixture(fixture)
    eng = Engine().load_rows(rows, Schema.from_dict(sd), BOTH)
    ref = sr.reference_from_lists(eng.graph_csr(0), eng.graph_csr(1), eng.graph_perm(), eng.vertex_ids())
    check(eng, ref, rows=False)
    check(tune(eng, wave_row=1, tail=0, trim=0, pivot=0), ref, rows=False)


# ------------------------------------------------------------------ native equals generic
def test_native_equals_the_generic_program(planted):
    n, src, dst, ids, ref = planted
    rows, vids, sd, npz = load_fixture("gotg")
    for graph in (GpuGraph(edges=(n, src, dst, None)), GpuGraph(rows, sd)):
        native = graph.compute().program(StronglyConnectedComponentsVertexProgram.build().create()).submit().get()
        nids, nlab = native.vertex_properties[COMPONENT]
        generic = graph.compute().program(GenericScc()).submit().get()
        gids, (glab, present) = generic.vertex_properties["scc"]
        assert present.all() and np.array_equal(nids, gids)
        assert np.asarray(glab, np.int64).tobytes() == np.asarray(nlab, np.int64).tobytes()
        assert generic.memory().getIteration() >= 2


# ------------------------------------------------------------------ surfaces
def test_run_to_run_and_fetch_later(rmat10):
    n, src, dst, ref = rmat10
    eng = Engine().load_edges(n, src, dst, BOTH)
    lab, info = eng.scc()
    bytes_after_first = eng.stats()["device_bytes"]
    again, info2 = eng.scc()
    assert np.array_equal(lab, again) and np.array_equal(lab, eng.vertex_ids()[ref[0]])
    assert {k: info2[k] for k in INFO} == {k: info[k] for k in INFO}       # rounds and passes may differ
    assert eng.stats()["device_bytes"] == bytes_after_first
    assert eng.stats()["iterations"] == info2["rounds"]
    none, info3 = eng.scc(fetch=False)
    assert none is None and {k: info3[k] for k in INFO} == {k: info[k] for k in INFO}
    assert np.array_equal(eng.copy_scc(), lab)
    eng.components()                                     # another program: the labels are no longer the last result
    with pytest.raises(TitanException) as e:
        eng.copy_scc()
    assert e.value.code == L.TGO_E_STATE
    assert eng.stats()["device_bytes"] == bytes_after_first     # the Titan ids by index are shared
    check(eng, ref)


def test_through_the_computer_with_the_map_reduce(rmat10):
    n, src, dst, ref = rmat10
    graph = GpuGraph(edges=(n, src, dst, None))
    c = graph.compute().program(StronglyConnectedComponentsVertexProgram.build().create())
    res = c.mapReduce(SccSizeMapReduce.build().create()).submit().get()
    ids, got = res.vertex_properties[COMPONENT]
    want = sr.reference(n, src, dst, ids)[0]
    assert np.array_equal(got, want)
    u, cnt = np.unique(want, return_counts=True)
    assert res.memory().get("sccSizes") == {int(k): int(v) for k, v in zip(u, cnt)}
    assert res.memory().getIteration() >= 1


def test_persist_and_result_rows():
    rows, vids, sd, npz = load_fixture("gotg")
    kc = (7400 << 6) | 5
    graph = GpuGraph(rows, sd, property_keys={COMPONENT: (kc, L.DT_LONG)})
    c = graph.compute()
    c.resultMode(TitanGraphComputer.ResultMode.PERSIST)
    res = c.program(StronglyConnectedComponentsVertexProgram.build().create()).submit().get()
    assert res.graph() is graph
    ids, lab = res.vertex_properties[COMPONENT]
    for vid, x in zip(ids, lab):
        got = graph.read_property(int(vid), kc, L.DT_LONG)
        assert type(got) is int and got == int(x)
    # the device rows: one entry per vertex, byte for byte the oracle encoder's
    eng = Engine().load_rows(rows, Schema.from_dict(sd), BOTH)
    base = 1 << 30
    with pytest.raises(TitanException) as e:
        eng.result_rows(L.RESULT_SCC, [kc], [L.DT_LONG], base)       # no finished program yet
    assert e.value.code == L.TGO_E_STATE
    none, _ = eng.scc(fetch=False)
    assert none is None and np.array_equal(eng.vertex_ids(), ids)
    lib = fr.load()
    for dt, enc in ((L.DT_LONG, lambda x, rel: fr.encode_property(kc, L.DT_LONG, x, rel)),
                    (L.DT_INTEGER, lambda x, rel: fr.encode_property(kc, L.DT_INTEGER, x, rel)),
                    (L.DT_OBJECT, lambda x, rel: fr.encode_property_generic(kc, L.DT_LONG, x, rel))):
        got = eng.result_rows(L.RESULT_SCC, [kc], [dt], base)
        assert got.nrows == eng.n and list(got.entry_begin) == list(range(eng.n + 1))
        for r in range(got.nrows):
            b = bytes(got.data[got.byte_begin[r]:got.byte_begin[r + 1]])
            assert b == enc(int(lab[r]), base + r)[0], (dt, r)
            assert got.keys[r] == lib.fr_key_of(int(ids[r]), 5)
    with pytest.raises(TitanException) as e:
        eng.result_rows(L.RESULT_SCC, [kc], [L.DT_DOUBLE], base)
    assert e.value.code == L.TGO_E_INVALID
    with pytest.raises(TitanException) as e:
        eng.result_rows(L.RESULT_COMPONENT, [kc], [L.DT_LONG], base)     # the other label program's kind
    assert e.value.code == L.TGO_E_STATE
    assert np.array_equal(eng.copy_scc(), lab)                       # the refused calls left the result in place
    # an Integer key cannot hold a Titan id beyond int range
    n, src, dst = sr.cycle(3)
    big = np.array([24, 32, (1 << 33) + 8], np.int64)
    eng = Engine().load_edges(n, src, dst, BOTH, titan_ids=big)
    assert (eng.scc(fetch=False)[1]["components"], eng.copy_scc().tolist()) == (1, [24, 24, 24])
    with pytest.raises(TitanException) as e:
        eng.result_rows(L.RESULT_SCC, [kc], [L.DT_INTEGER], base)
    assert e.value.code == L.TGO_E_INVALID
    assert eng.result_rows(L.RESULT_SCC, [kc], [L.DT_LONG], base).nrows == 3


# ------------------------------------------------------------------ errors
def test_errors_leave_the_ctx_usable():
    n, src, dst = sr.cycle(64)
    good = (np.zeros(n, np.int64), {"components": 1, "largest": n, "singletons": 0})
    eng = Engine().load_edges(n, src, dst, L.SCOPE_OUT_E)           # not bothE
    with pytest.raises(TitanException) as e:
        eng.scc()
    assert e.value.code == L.TGO_E_INVALID
    a = L.SccArgs(BOTH, 0)                                           # bothE, but not the loaded scope
    assert eng.lib.tgo_scc(eng.ctx, C.byref(a), None, None) == L.TGO_E_INVALID
    eng.load_edges(n, src, dst, BOTH)
    check(eng, good)
    eng = Engine()                                                   # before a load
    with pytest.raises(TitanException) as e:
        eng.scc()
    assert e.value.code == L.TGO_E_STATE
    eng.load_edges(n, src, dst, BOTH)
    a = L.SccArgs(BOTH, 1)                                           # flags
    assert eng.lib.tgo_scc(eng.ctx, C.byref(a), None, None) == L.TGO_E_INVALID
    out = np.zeros(n, np.int64)
    assert eng.lib.tgo_copy_scc(eng.ctx, L.ptr(out, C.c_int64)) == L.TGO_E_STATE        # no finished run
    check(eng, good)
    # lists that are not each other's transpose: a triangle 0 -> 1 -> 2 -> 0 whose IN entry of 0 -> 1 is missing
    out_off, out_idx = np.array([0, 1, 2, 3], np.int64), np.array([1, 2, 0], np.int32)
    in_off, in_idx = np.array([0, 1, 1, 2], np.int64), np.array([2, 1], np.int32)
    eng = Engine().load_csr(3, out_off, out_idx, in_off, in_idx, BOTH, titan_ids=np.array([8, 16, 24], np.int64))
    with pytest.raises(TitanException) as e:
        eng.scc()
    assert e.value.code == L.TGO_E_UNSUPPORTED and "strongly connected components" in str(e.value)
    eng.load_edges(n, src, dst, BOTH)
    check(eng, good)
    # a partitioned ctx; the same ctx then takes a one-GPU load and runs
    eng = Engine().load_partition(n, 0, n, src, dst, BOTH)
    with pytest.raises(TitanException) as e:
        eng.scc()
    assert e.value.code == L.TGO_E_UNSUPPORTED
    eng.load_edges(n, src, dst, BOTH)
    check(eng, good)
