"""GPU: native betweenness centrality (tgo_betweenness, titan_amd/csrc/bc.hip).

The reference is always bc_ref.py (Brandes in exact arithmetic; test_bc_cpu.py checks it against closed
forms).  Values are the raw sums over ordered pairs.  Comparison rule: where every exact value is an
integer or a dyadic fraction and sigma < 2^53, array_equal; otherwise |got - exact| <= tol * exact with
tol = (3 D (dmax + 3) + S) 2^-52 from the reference's own D and dmax and the number of seeds S, which
bounds any fp64 summation order (bc_ref.tolerance has the derivation); an exact zero must be 0.0.
rounds is a diagnostic and is only printed.
"""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import bc_ref as br
import fulgora as fr
from conftest import load_fixture
from titan_amd import (BetweennessCentralityVertexProgram, BetweennessRankMapReduce, Engine, GpuGraph, Schema,
                       TitanException, rmat_edges)
from titan_amd import _lib as L

pytestmark = pytest.mark.gpu

BOTH = L.SCOPE_BOTH_E
CENTRALITY = BetweennessCentralityVertexProgram.CENTRALITY
INFO = ("sources", "reached_pairs", "max_depth")
NONE = (np.zeros(0, np.int32), np.zeros(0, np.int32))


def run(eng, ref, seeds=None, directed=False, exact=False, nseeds=None):
    """One run against (bc, info) of the reference: bit for bit when exact, else within the bound.
    seeds are row numbers here (dense)."""
    rbc, rinfo = ref
    bc, info = eng.betweenness(seeds, directed=directed, dense=True)
    assert bc.dtype == np.float64 and len(bc) == eng.n
    for k in INFO:
        assert info[k] == rinfo[k], k
    st = eng.stats()
    assert st["iterations"] == info["sources"] and st["levels"] == info["max_depth"]
    if exact:
        assert np.array_equal(bc, br.as_floats(rbc))
    else:
        S = nseeds if nseeds is not None else (eng.n if seeds is None else len(seeds))
        tol = br.tolerance(rinfo, S)
        print("worst relative error", br.within(bc, rbc, tol), "bound", float(tol), "rounds", info["rounds"])
    assert np.array_equal(eng.copy_betweenness(), bc)
    return bc, info


@pytest.fixture(scope="module")
def gnp301():
    n, src, dst = br.gnp(301, 0.03, 9)
    ids, s2, d2, new = br.relabel(n, src, dst)
    und = br.reference(n, s2, d2)
    dire = br.reference(n, s2, d2, directed=True)
    assert und[1]["D"] >= 4 and und[1]["dmax"] >= 15 and dire[1]["reached_pairs"] < und[1]["reached_pairs"]
    return n, s2, d2, ids, und, dire


# ------------------------------------------------------------------ closed forms, all seeds, undirected
def test_path_of_33():
    n, src, dst = br.path(33)
    bc, info = run(Engine().load_edges(n, src, dst, BOTH), br.reference(n, src, dst), exact=True)
    assert bc.tolist() == [2.0 * i * (32 - i) for i in range(33)] and info["max_depth"] == 32


def test_star_with_64_leaves():
    n, src, dst = br.star(64)
    bc, info = run(Engine().load_edges(n, src, dst, BOTH), br.reference(n, src, dst), exact=True)
    assert bc.tolist() == [64.0 * 63] + [0.0] * 64


@pytest.mark.parametrize("n", [65, 64])
def test_cycles(n):
    _, src, dst = br.cycle(n)
    bc, info = run(Engine().load_edges(n, src, dst, BOTH), br.reference(n, src, dst), exact=True)
    want = (n - 1) * (n - 3) / 4 if n % 2 else (n - 2) ** 2 / 4     # the even cycle has ties: sigma = 2
    assert bc.tolist() == [want] * n


@pytest.mark.parametrize("k", [5, 70])
def test_cliques_are_all_zero(k):
    n, src, dst = br.clique(k)                           # 70: rows longer than a wave
    bc, info = run(Engine().load_edges(n, src, dst, BOTH), br.reference(n, src, dst), exact=True)
    assert bc.tobytes() == np.zeros(k).tobytes() and info["max_depth"] == 1


def test_complete_bipartite_3_70():
    n, src, dst = br.complete_bipartite(3, 70)           # rows longer than a wave; sigma = 3 and 70
    ref = br.reference(n, src, dst)
    assert ref[0] == [Fraction(70 * 69, 3)] * 3 + [Fraction(6, 70)] * 70
    eng = Engine().load_edges(n, src, dst, BOTH)
    run(eng, ref)
    for wave_row in (1, 1 << 30):
        run(eng.set_tuning(L.TUNE_BC_WAVE_ROW, wave_row), ref)


def test_grid_9x9():
    n, src, dst = br.grid(9, 9)                          # binomial sigma
    run(Engine().load_edges(n, src, dst, BOTH), br.reference(n, src, dst))


# ------------------------------------------------------------------ sigma's range
def test_diamond_chains_exact_then_overflow_then_exact():
    n40, s40, d40 = br.diamond_chain(40)
    ref40 = br.reference(n40, s40, d40, seeds=[0])
    eng = Engine().load_edges(n40, s40, d40, BOTH)
    bc, info = run(eng, ref40, seeds=[0], exact=True)    # sigma up to 2^40, every ratio a power of two
    assert info["max_depth"] == 80
    n, src, dst = br.diamond_chain(1030)                 # sigma passes 2^1024
    eng.load_edges(n, src, dst, BOTH)
    ids = eng.vertex_ids()
    with pytest.raises(TitanException) as e:
        eng.betweenness([int(ids[0])])
    assert e.value.code == L.TGO_E_PROGRAM and str(int(ids[0])) in str(e.value)
    with pytest.raises(TitanException) as e:
        eng.copy_betweenness()
    assert e.value.code == L.TGO_E_STATE
    eng.load_edges(n40, s40, d40, BOTH)                  # the same ctx runs on
    run(eng, ref40, seeds=[0], exact=True)


# ------------------------------------------------------------------ the two readings
def test_projection_fixture_collapses_duplicates():
    n, src, dst = br.projection_fixture()
    eng = Engine().load_edges(n, src, dst, BOTH)
    bc, _ = run(eng, br.reference(n, src, dst), exact=True)
    assert bc.tolist() == [1.0, 1.0, 1.0, 1.0, 0.0]      # a count over raw entries gives 2/3 and 1/3 somewhere
    bc, _ = run(eng, br.reference(n, src, dst, directed=True), directed=True, exact=True)
    assert bc.tolist() == [1.0, 0.5, 0.5, 0.0, 0.0]
    for wave_row in (1, 2):                              # the wave path skips duplicates and self-loops alike
        eng.set_tuning(L.TUNE_BC_WAVE_ROW, wave_row)
        assert eng.betweenness()[0].tolist() == [1.0, 1.0, 1.0, 1.0, 0.0]
        assert eng.betweenness(directed=True)[0].tolist() == [1.0, 0.5, 0.5, 0.0, 0.0]


def test_directed_cycle_and_gnp(gnp301):
    n, src, dst = br.cycle(17)
    bc, info = run(Engine().load_edges(n, src, dst, BOTH), br.reference(n, src, dst, directed=True), directed=True,
                   exact=True)
    assert bc.tolist() == [120.0] * 17 and info["max_depth"] == 16
    n, src, dst, ids, und, dire = gnp301
    eng = Engine().load_edges(n, src, dst, BOTH, titan_ids=ids)
    run(eng, dire, directed=True)
    run(eng.set_tuning(L.TUNE_BC_WAVE_ROW, 1), dire, directed=True)


def test_two_components_and_isolated_vertices():
    n, src, dst = br.two_components_and_isolated()
    ref = br.reference(n, src, dst)
    bc, info = run(Engine().load_edges(n, src, dst, BOTH), ref)
    assert bc[14:].tobytes() == np.zeros(3).tobytes()
    assert {k: info[k] for k in INFO} == {"sources": 17, "reached_pairs": 92, "max_depth": 8}


@pytest.mark.parametrize("n", [1, 130])
def test_no_entries(n):
    eng = Engine().load_edges(n, *NONE, BOTH)
    for directed in (False, True):
        bc, info = eng.betweenness(directed=directed)
        assert bc.tobytes() == np.zeros(n).tobytes()
        assert {k: info[k] for k in INFO} == {"sources": n, "reached_pairs": 0, "max_depth": 0}
    bc, info = eng.betweenness([])
    assert bc.tobytes() == np.zeros(n).tobytes() and info["sources"] == 0 and info["reached_pairs"] == 0


def test_no_seeds_gives_zeros():
    n, src, dst = br.path(33)
    bc, info = Engine().load_edges(n, src, dst, BOTH).betweenness([])
    assert bc.tobytes() == np.zeros(n).tobytes()
    assert info == {"sources": 0, "reached_pairs": 0, "max_depth": 0, "rounds": 0}


# ------------------------------------------------------------------ random graphs
def test_gnp_all_seeds_bit_identity_and_tuning(gnp301):
    n, src, dst, ids, und, dire = gnp301
    eng = Engine().load_edges(n, src, dst, BOTH, titan_ids=ids)
    assert np.array_equal(eng.vertex_ids(), ids)
    first, _ = run(eng, und)
    assert eng.betweenness()[0].tobytes() == first.tobytes()
    for wave_row in (1, 1 << 30):
        eng.set_tuning(L.TUNE_BC_WAVE_ROW, wave_row)
        a, _ = run(eng, und)
        assert eng.betweenness()[0].tobytes() == a.tobytes(), wave_row
    eng.set_tuning(L.TUNE_BC_WAVE_ROW, -1)
    assert eng.betweenness()[0].tobytes() == first.tobytes()
    for bad in (0, 0.5, 1.5):
        with pytest.raises(TitanException) as e:
            eng.set_tuning(L.TUNE_BC_WAVE_ROW, bad)
        assert e.value.code == L.TGO_E_INVALID


def test_path_sum_identity(gnp301):
    """sum_v bc[v] = sum over seeds s and reached t != s of (d(s, t) - 1): every shortest s-t path has
    d - 1 inner vertices and the dependencies of a pair add up to one per inner place.  The
    distances come from tgo_bfs on the same engine, not from the reference."""
    n, src, dst, ids, und, dire = gnp301
    eng = Engine().load_edges(n, src, dst, BOTH, titan_ids=ids)
    want = 0
    for s in range(n):
        d = eng.bfs(s, n, BOTH, seed_is_dense=True)
        d = d[(d != L.DIST_ABSENT) & (d > 0)]
        want += int((d - 1).sum())
    bc, info = eng.betweenness()
    total = sum(Fraction(x) for x in bc.tolist())
    tol = br.tolerance(und[1], n)
    print("sum", float(total), "want", want, "relative error", float(abs(total - want) / want), "bound", float(tol))
    assert want > 0 and abs(total - want) <= tol * want


def test_rmat10_sixteen_titan_id_seeds():
    n = 1 << 10
    src, dst, _ = rmat_edges(10, 8, seed=31)             # hubs, duplicates, self-loops
    assert (src == dst).any()
    eng = Engine().load_edges(n, src, dst, BOTH)
    ids = eng.vertex_ids()
    rows = np.random.default_rng(5).choice(n, 16, replace=False)
    ref = br.reference(n, src, dst, seeds=rows)
    assert ref[1]["dmax"] > 64 and ref[1]["reached_pairs"] > 0
    bc, info = eng.betweenness(ids[rows])
    for k in INFO:
        assert info[k] == ref[1][k], k
    tol = br.tolerance(ref[1], 16)
    print("worst relative error", br.within(bc, ref[0], tol), "bound", float(tol))
    for wave_row in (1, 16):
        br.within(eng.set_tuning(L.TUNE_BC_WAVE_ROW, wave_row).betweenness(ids[rows])[0], ref[0], tol)


def test_seed_handling(gnp301):
    n, src, dst, ids, und, dire = gnp301
    eng = Engine().load_edges(n, src, dst, BOTH, titan_ids=ids)
    a = int(ids[7])
    one, info1 = eng.betweenness([a])
    two, info2 = eng.betweenness([a, a])
    assert two.tobytes() == (2.0 * one).tobytes() and info2["sources"] == 2
    assert info2["reached_pairs"] == 2 * info1["reached_pairs"]
    unknown = int(ids[-1]) + 1
    assert unknown not in set(ids.tolist())
    got, info = eng.betweenness([unknown, a, unknown])
    assert got.tobytes() == one.tobytes() and info["sources"] == 1
    none, info = eng.betweenness([unknown])
    assert none.tobytes() == np.zeros(n).tobytes() and info["sources"] == 0
    rows = [7, 100, 3]
    dense, infod = eng.betweenness(rows, dense=True)
    titan, infot = eng.betweenness(ids[rows])
    assert dense.tobytes() == titan.tobytes() and {k: infod[k] for k in INFO} == {k: infot[k] for k in INFO}
    with pytest.raises(TitanException) as e:
        eng.betweenness([n], dense=True)                 # as tgo_bfs: a dense seed out of range
    assert e.value.code == L.TGO_E_INVALID


# ------------------------------------------------------------------ fixtures: vertex cuts, rows load
@pytest.mark.parametrize("fixture", ["gotg", "partition_groups"])
def test_fixture_rows_are_sorted_and_equal_the_reference(fixture):
    rows, vids, sd, npz = load_fixture(fixture)
    eng = Engine().load_rows(rows, Schema.from_dict(sd), BOTH)
    n = eng.n
    out, inn, perm = eng.graph_csr(0), eng.graph_csr(1), np.asarray(eng.graph_perm(), np.int64)
    for c in (out, inn):                                 # what the directed reading's duplicate skip relies on
        off, adj = np.asarray(c["off"], np.int64), np.asarray(c["adj"], np.int64)
        rising = np.diff(adj) >= 0
        starts = off[1:-1]
        rising[starts[(starts > 0) & (starts < len(adj))] - 1] = True       # a row's first entry
        assert rising.all()
    row_of = np.empty(n, np.int64)
    row_of[perm] = np.arange(n)                          # internal id -> row
    off = np.asarray(out["off"], np.int64)
    src = row_of[np.repeat(np.arange(n), np.diff(off))]
    dst = row_of[np.asarray(out["adj"], np.int64)]
    for directed in (False, True):
        ref = br.reference(n, src, dst, directed=directed)
        for wave_row in (-1, 1):
            run(eng.set_tuning(L.TUNE_BC_WAVE_ROW, wave_row), ref, directed=directed)


# ------------------------------------------------------------------ errors
def test_errors_leave_the_ctx_usable():
    n, src, dst = br.path(33)
    ref = br.reference(n, src, dst)
    eng = Engine().load_edges(n, src, dst, L.SCOPE_IN_E)               # not bothE
    with pytest.raises(TitanException) as e:
        eng.betweenness()
    assert e.value.code == L.TGO_E_INVALID
    a = L.BcArgs(BOTH, 0, 0, 0)                                        # bothE, but not the loaded scope
    assert eng.lib.tgo_betweenness(eng.ctx, C.byref(a), None, -1, None, None) == L.TGO_E_INVALID
    eng.load_edges(n, src, dst, BOTH)
    for bad, nseeds in ((L.BcArgs(BOTH, 1, 0, 0), -1), (L.BcArgs(BOTH, 0, 2, 0), -1), (L.BcArgs(BOTH, 0, -1, 0), -1),
                        (L.BcArgs(BOTH, 0, 0, 0), -2), (L.BcArgs(BOTH, 0, 0, 0), 3)):      # the last: seeds NULL
        assert eng.lib.tgo_betweenness(eng.ctx, C.byref(bad), None, nseeds, None, None) == L.TGO_E_INVALID
    out = np.zeros(n, np.float64)
    assert eng.lib.tgo_copy_betweenness(eng.ctx, L.ptr(out, C.c_double)) == L.TGO_E_STATE    # no finished run
    run(eng, ref, exact=True)
    eng.kcore()
    with pytest.raises(TitanException) as e:
        eng.copy_betweenness()                                         # another program ran since
    assert e.value.code == L.TGO_E_STATE
    # lists that are not each other's transpose: a triangle 0 -> 1 -> 2 -> 0 whose IN entry of 0 -> 1 is missing
    out_off, out_idx = np.array([0, 1, 2, 3], np.int64), np.array([1, 2, 0], np.int32)
    in_off, in_idx = np.array([0, 1, 1, 2], np.int64), np.array([2, 1], np.int32)
    eng = Engine().load_csr(3, out_off, out_idx, in_off, in_idx, BOTH, titan_ids=np.array([8, 16, 24], np.int64))
    with pytest.raises(TitanException) as e:
        eng.betweenness()
    assert e.value.code == L.TGO_E_UNSUPPORTED
    run(Engine().load_edges(n, src, dst, BOTH), ref, exact=True)      # a fresh load runs
    n, src, dst = br.cycle(64)                                        # (a partition holds a multiple of 64 rows)
    eng = Engine().load_partition(n, 0, n, src, dst, BOTH)            # a partitioned ctx
    with pytest.raises(TitanException) as e:
        eng.betweenness()
    assert e.value.code == L.TGO_E_UNSUPPORTED
    eng.load_edges(n, src, dst, BOTH)
    run(eng, br.reference(n, src, dst), exact=True)


# ------------------------------------------------------------------ surfaces
def test_the_simple_adjacency_is_cached_with_the_graph(gnp301):
    n, src, dst, ids, und, dire = gnp301
    eng = Engine().load_edges(n, src, dst, BOTH, titan_ids=ids)
    eng.betweenness([0], directed=True, dense=True)                    # the directed reading builds nothing
    before = eng.stats()["device_bytes"]
    pred, succ = br.adjacency(n, src, dst)
    entries = sum(len(r) for r in succ)
    eng.betweenness([0], dense=True)
    first = eng.stats()["device_bytes"]
    assert first - before == 4 * entries + 8 * (n + 1)
    eng.betweenness([1], dense=True)
    eng.betweenness([1], directed=True, dense=True)
    assert eng.stats()["device_bytes"] == first
    none, info = eng.betweenness([1], dense=True, fetch=False)
    assert none is None and info["sources"] == 1
    assert np.array_equal(eng.copy_betweenness(), eng.betweenness([1], dense=True)[0])


def test_result_rows_match_the_oracle_encoder():
    rows, vids, sd, npz = load_fixture("gotg")
    kc = (7600 << 6) | 5
    eng = Engine().load_rows(rows, Schema.from_dict(sd), BOTH)
    base = 1 << 30
    with pytest.raises(TitanException) as e:
        eng.result_rows(L.RESULT_BETWEENNESS, [kc], [L.DT_DOUBLE], base)       # no finished program yet
    assert e.value.code == L.TGO_E_STATE
    none, info = eng.betweenness(fetch=False)
    assert none is None and info["sources"] == eng.n
    bc = eng.copy_betweenness()
    ids = eng.vertex_ids()
    assert (bc > 0).any()
    lib = fr.load()
    for dt, enc in ((L.DT_DOUBLE, lambda x, rel: fr.encode_property_f64(kc, x, rel)),
                    (L.DT_OBJECT, lambda x, rel: fr.encode_property_generic(kc, L.DT_DOUBLE, x, rel))):
        got = eng.result_rows(L.RESULT_BETWEENNESS, [kc], [dt], base)
        assert got.nrows == eng.n and list(got.entry_begin) == list(range(eng.n + 1))
        for r in range(got.nrows):
            b = bytes(got.data[got.byte_begin[r]:got.byte_begin[r + 1]])
            want, vp = enc(float(bc[r]), base + r)
            assert b == want, (dt, r)
            assert got.limit_valpos[r] == (len(want) << 32) | vp
            assert got.keys[r] == lib.fr_key_of(int(ids[r]), 5)
    with pytest.raises(TitanException) as e:
        eng.result_rows(L.RESULT_BETWEENNESS, [kc], [L.DT_LONG], base)
    assert e.value.code == L.TGO_E_INVALID
    with pytest.raises(TitanException) as e:
        eng.result_rows(L.RESULT_PAGERANK, [kc, kc + 64], [L.DT_DOUBLE, L.DT_DOUBLE], base)   # another program's kind
    assert e.value.code == L.TGO_E_STATE
    assert np.array_equal(eng.copy_betweenness(), bc)                  # the refused calls left the result in place


def test_through_the_computer_with_the_rank_map_reduce():
    n, src, dst = br.grid(9, 9)
    graph = GpuGraph(edges=(n, src, dst, None))
    c = graph.compute().program(BetweennessCentralityVertexProgram.build().create())
    res = c.mapReduce(BetweennessRankMapReduce(top=3)).submit().get()
    ids, got = res.vertex_properties[CENTRALITY]
    ref = br.reference(n, src, dst)
    br.within(got, ref[0], br.tolerance(ref[1], n))
    top = list(res.memory().get("betweennessRank"))
    assert len(top) == 3 and top[0].key == int(ids[40]) and top[0].value == got[40]
    near = {int(ids[v]) for v in (31, 39, 41, 49)}                     # then two of the centre's four neighbours
    assert top[1].key in near and top[2].key in near and top[1].value >= top[2].value
    assert res.memory().getIteration() == n
    seeds = [int(ids[0]), int(ids[80])]
    res = (graph.compute().program(BetweennessCentralityVertexProgram.build().seeds(seeds).directed(True).create())
           .submit().get())
    want = br.reference(n, src, dst, seeds=[0, 80], directed=True)
    br.within(res.vertex_properties[CENTRALITY][1], want[0], br.tolerance(want[1], 2))
    assert res.memory().getIteration() == 2
