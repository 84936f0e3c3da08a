"""GPU: native peer-pressure clustering (tgo_peer_pressure, titan_amd/csrc/pp.hip).

The reference is always pp_ref.py (dict tallies of Python ints; test_pp_cpu.py checks it against closed
forms).  Tallies are exact integers and ties go to the smallest Titan id, so the result is unique:
every comparison is array_equal on int64 labels, and info is compared whole — rounds included, which
for this program is deterministic.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

import fulgora as fr
import pp_ref as pr
from conftest import load_fixture
from pp_generic import GenericPeerPressure
from titan_amd import (ClusterCountMapReduce, ClusterPopulationMapReduce, Engine, GpuGraph, PeerPressureVertexProgram,
                       Schema, TitanException, TitanGraphComputer, rmat_edges)
from titan_amd import _lib as L

pytestmark = pytest.mark.gpu

OUT, IN, BOTH = L.SCOPE_OUT_E, L.SCOPE_IN_E, L.SCOPE_BOTH_E
CLUSTER = PeerPressureVertexProgram.CLUSTER
NONE = (np.zeros(0, np.int32), np.zeros(0, np.int32))
SCOPES = {OUT: "outE", IN: "inE", BOTH: "bothE"}
CASES = list(itertools.product((OUT, IN, BOTH), (0, 1)))
MIN_SLOTS = 16


def rows_by_id(ids, src, dst):
    """The same graph with its vertices renumbered in increasing id order: load_edges takes the
    rows in the order a scan delivers them, strictly increasing Titan ids."""
    ids = np.asarray(ids, np.int64)
    rank = np.empty(len(ids), np.int32)
    rank[np.argsort(ids)] = np.arange(len(ids), dtype=np.int32)
    return np.sort(ids), rank[src], rank[dst]


def tune(eng, wave_row=-1, block_row=-1, slots=-1):
    eng.set_tuning(L.TUNE_PP_WAVE_ROW, wave_row).set_tuning(L.TUNE_PP_BLOCK_ROW, block_row)
    return eng.set_tuning(L.TUNE_PP_SLOTS, slots)


def check(eng, ref, **kw):
    """One run against (cluster, info) of the reference, the result taken both ways."""
    rlab, rinfo = ref
    lab, info = eng.peer_pressure(**kw)
    assert lab.dtype == np.int64 and np.array_equal(lab, rlab)
    assert info == rinfo
    assert np.array_equal(eng.copy_peer_pressure(), lab)
    assert eng.stats()["iterations"] == info["rounds"]
    return lab, info


def run_all(graph, ids=None, cases=CASES, max_rounds=30, tunings=((-1, -1, -1),)):
    """Every (vote_scope, distribute) of `cases` on one load, against the reference: {case: (labels,
    info, the labels as row numbers)}."""
    n, src, dst = graph
    eng = Engine().load_edges(n, src, dst, BOTH, titan_ids=ids)
    ids = eng.vertex_ids()
    out = {}
    for scope, d in cases:
        ref = pr.reference(n, src, dst, ids, scope, d, max_rounds)
        for t in tunings:
            lab, info = check(tune(eng, *t), ref, vote_scope=scope, distribute=bool(d), max_rounds=max_rounds)
            assert (np.diff(ids) > 0).all()
            out[scope, d] = lab, info, np.searchsorted(ids, lab).tolist()
    return out


@pytest.fixture(scope="module")
def rmat10():
    n = 1 << 10
    src, dst, _ = rmat_edges(10, 8, seed=31)            # hubs, duplicates, self-loops
    assert (src == dst).any() and len(np.unique(src.astype(np.int64) * n + dst)) < len(src)
    ids = Engine().load_edges(n, src, dst, BOTH).vertex_ids()
    refs = {c: pr.reference(n, src, dst, ids, *c) for c in CASES}
    assert all(1 < r[1]["clusters"] < n for r in refs.values())
    assert refs[OUT, 0][1]["converged"] == 1 and refs[BOTH, 1][1]["rounds"] == 30     # one case runs into the round limit
    return n, src, dst, refs


# ------------------------------------------------------------------ closed forms
def test_cycles_and_the_round_limit():
    for (scope, d), (lab, info, rows) in run_all(pr.cycle(3, 2), cases=[(OUT, 0), (OUT, 1)], max_rounds=7).items():
        assert rows == [2, 0, 1]
        assert info == {"clusters": 3, "largest": 1, "changed_last": 3, "rounds": 7, "converged": 0}
    for (scope, d), (lab, info, rows) in run_all(pr.cycle(3), cases=[(OUT, 0), (OUT, 1)]).items():
        assert rows == [0, 0, 0] and info["rounds"] == 3 and info["converged"] == 1
    got = run_all(pr.cycle(3), ids=np.array([8, 16, 24], np.int64), cases=[(OUT, 0)], max_rounds=0)
    assert got[OUT, 0][0].tolist() == [8, 16, 24]
    assert got[OUT, 0][1] == {"clusters": 3, "largest": 1, "changed_last": 0, "rounds": 0, "converged": 0}


def test_cliques_bridge_and_path():
    got = run_all(pr.two_cliques_bridge(5), cases=[(BOTH, 0), (BOTH, 1)])
    assert got[BOTH, 0][2] == [0] * 5 + [5] * 5 and got[BOTH, 0][1]["rounds"] == 3
    assert got[BOTH, 1][2] == [0] * 5 + [6] * 5 and got[BOTH, 1][1]["rounds"] == 2
    got = run_all(pr.path(9), cases=[(BOTH, 0)])
    assert got[BOTH, 0][2] == [0] * 9 and got[BOTH, 0][1]["rounds"] == 9


def test_star_of_64_leaves():
    got = run_all(pr.star(64))
    assert [got[c][1]["rounds"] for c in CASES] == [2, 1, 1, 1, 2, 2]
    assert got[IN, 0][2] == list(range(65))                    # IN without distribute moves nobody


@pytest.mark.parametrize("n", [1, 130])
def test_no_entries(n):
    for (scope, d), (lab, info, rows) in run_all((n, *NONE)).items():
        assert rows == list(range(n))
        assert info == {"clusters": n, "largest": 1, "changed_last": 0, "rounds": 1, "converged": 1}


def test_multiplicity_self_loops_and_the_fixed_point_pin():
    e = np.array([(0, 1), (0, 1), (2, 1)], np.int32)                    # a -> b twice, c -> b once; ids a > b > c
    ids, s, t = rows_by_id([240, 160, 80], e[:, 0], e[:, 1])
    got = run_all((3, s, t), ids=ids, cases=[(OUT, 0)], max_rounds=1)
    assert got[OUT, 0][0].tolist() == [80, 240, 240]                    # rows in id order: c, b, a
    e = np.array([(1, 1), (1, 1), (0, 1)], np.int32)                    # b with two self-loops keeps b
    assert run_all((2, e[:, 0], e[:, 1]), cases=[(OUT, 0)], max_rounds=1)[OUT, 0][2] == [0, 1]
    got = run_all(pr.fixed_point_pin(), cases=[(OUT, 0), (OUT, 1)], max_rounds=1)
    assert got[OUT, 1][2][2] == 1 and got[OUT, 0][2][2] == 0            # 3 floor(2^32 / 3) < 2^32


def test_sinks_keep_their_id_under_distribute():
    n, src, dst = pr.star(5)
    ids, s, t = rows_by_id([400, 80, 160, 240, 320, 480], src, dst)
    got = run_all((n, s, t), ids=ids, cases=[(OUT, 1), (OUT, 0)])
    assert got[OUT, 1][0].tolist() == ids.tolist()
    assert got[OUT, 0][0].tolist() == [80, 160, 240, 320, 400, 400]     # each leaf ties with the hub (400): the smaller id


# ------------------------------------------------------------------ ties by Titan id
def test_gnp_with_permuted_ids_every_scope():
    n, src, dst = pr.gnp_digraph(1001, 0.05, 5)
    ids = np.random.default_rng(23).permutation(4 * n)[:n].astype(np.int64) * 8 + 24
    ids_sorted, s2, d2 = rows_by_id(ids, src, dst)
    got = run_all((n, s2, d2), ids=ids_sorted)
    assert all(info["rounds"] >= 2 for _, info, _ in got.values())


# ------------------------------------------------------------------ every tier at its smallest shape
def test_clique_70_and_star_1500():
    run_all(pr.clique(70))                                              # rows longer than a wave
    run_all(pr.star(1500), cases=[(OUT, 0), (IN, 0), (BOTH, 0), (BOTH, 1)])
    n, src, dst = pr.star(1500)
    run_all((n, dst, src), cases=[(OUT, 0), (BOTH, 1)], tunings=[(-1, -1, -1), (8, 512, MIN_SLOTS)])


@pytest.mark.parametrize("leaves", [3000, 6000])
def test_fan_overflows_the_tables_after_round_1(leaves):
    n, src, dst = pr.fan(leaves)
    ids = np.arange(n, dtype=np.int64) * 8 + 8
    ids[0] = 8 * (n + 1)                                                # the hub's id is the largest
    ids_sorted, s2, d2 = rows_by_id(ids, src, dst)
    ref = pr.reference(n, s2, d2, ids_sorted, OUT, 0, 2)
    # after round 1 the hub's row holds leaves / 2 clusters: more than a wave's table at every
    # value, more than a workgroup's default table (2048) at 6000 leaves
    after1 = pr.reference(n, s2, d2, ids_sorted, OUT, 0, 1)[0]
    assert len(np.unique(after1[:-1])) == leaves // 2
    # default, the hub on the wave tier, the hub on the workgroup tier with the smallest table
    got = run_all((n, s2, d2), ids=ids_sorted, cases=[(OUT, 0), (OUT, 1), (BOTH, 0)],
                  tunings=[(-1, -1, -1), (16, 1 << 30, -1), (16, 1024, MIN_SLOTS), (16, 1 << 30, MIN_SLOTS)])
    assert got[OUT, 0][0].tobytes() == ref[0].tobytes() and got[OUT, 0][1]["rounds"] == 2       # round 2 tallies that row


def pp_class(rank):
    """pp.hip's second hash, which sorts a row's labels into the classes of its hashed passes."""
    return ((rank * 0x85EBCA6B) & 0xFFFFFFFF) >> 10


def one_class_star(leaves, m):
    """A star whose leaves all vote for the hub (row 0), on rows whose ranks fall in one hash class of
    the table kernel: pp_class(rank) % K = 0 for K = ceil(2 (l + 1) / m), l = the hub's row.  Two more
    rows of that class: p sends the hub three parallel edges, q sends p two.  The other rows have no
    edge.  Under OUT without distribute: round 1 moves the hub to p (three votes) and p to q; in round
    2 the hub's row holds leaves + 1 labels of one class — more than a table of m slots, which neither
    the hashed table nor the hashed classes can hold, only the rank-range passes — and p's three
    votes now name q, where the hub has to move: neither its own label nor the smallest of the row.
    (n, src, dst, the leaves' rows, p, q, K)"""
    K = (2 * (leaves + 4) + m - 1) // m                                 # l = leaves + 3 entries under OUT
    rows, r = [], 2
    while len(rows) < leaves + 2:
        if pp_class(r) % K == 0:
            rows.append(r)
        r += 1
    q, p = rows.pop(leaves // 2), rows.pop(leaves // 3)
    src = np.array(rows + [p, p, p, q, q], np.int32)
    dst = np.array([0] * (leaves + 3) + [p, p], np.int32)
    return r, src, dst, rows, p, q, K


@pytest.mark.parametrize("tier", ["wave", "block"])
def test_one_hash_class_reaches_the_rank_range_passes(tier):
    m = MIN_SLOTS if tier == "wave" else 4 * MIN_SLOTS                  # a wave's table, a workgroup's
    leaves = 100 if tier == "wave" else 160
    n, src, dst, rows, p, q, K = one_class_star(leaves, m)
    assert leaves > m and K >= 2 and n > 8 * m                          # several classes, several range passes
    # the precondition, on the reference's own labels: after round 1 the hub's senders are leaves + 1
    # clusters, all of hash class 0 (labels are ranks = rows: the ids rise with the rows)
    ids = Engine().load_edges(n, src, dst, BOTH).vertex_ids()
    for d in (0, 1):
        after1 = np.searchsorted(ids, pr.reference(n, src, dst, ids, OUT, d, 1)[0])
        senders = after1[rows + [p]].tolist()
        assert senders == rows + [q] and all(pp_class(c) % K == 0 for c in senders)
    by_round = [np.searchsorted(ids, pr.reference(n, src, dst, ids, OUT, 0, k)[0])[0] for k in (1, 2, 3)]
    assert by_round == [p, q, q] and q not in (0, min(rows))           # round 2 decides, in that row
    tuning = (1, 1 << 30, MIN_SLOTS) if tier == "wave" else (1 << 30, 1, MIN_SLOTS)
    got = run_all((n, src, dst), cases=[(OUT, 0), (OUT, 1), (BOTH, 0)], tunings=[tuning, (-1, -1, -1)])
    assert got[OUT, 0][2][0] == q and got[OUT, 0][1]["rounds"] == 3 and got[OUT, 1][1]["rounds"] >= 2


def test_rmat10_at_the_smallest_table_on_each_tier(rmat10):
    # BOTH with distribute keeps hundreds of clusters in the hubs' rows round after round: at 16 slots
    # classes outgrow the table too (a replay of the reference's labels through the kernel's hashes
    # counts 29 such row-rounds in 30 rounds); four rounds of it on each tier
    n, src, dst, refs = rmat10
    eng = Engine().load_edges(n, src, dst, BOTH)
    ref = pr.reference(n, src, dst, eng.vertex_ids(), BOTH, 1, 4)
    assert ref[1]["rounds"] == 4 and ref[1]["converged"] == 0
    for t in ((1, 1 << 30, MIN_SLOTS), (1 << 30, 1, MIN_SLOTS), (8, 64, MIN_SLOTS)):
        check(tune(eng, *t), ref, vote_scope=BOTH, distribute=True, max_rounds=4)


def test_rmat10_every_scope(rmat10):
    n, src, dst, refs = rmat10
    eng = Engine().load_edges(n, src, dst, BOTH)
    for scope, d in CASES:
        lab, info = check(eng, refs[scope, d], vote_scope=scope, distribute=bool(d))
        print(SCOPES[scope], d, info)


# ------------------------------------------------------------------ tuning invariance
@pytest.mark.parametrize("scope,d", [(OUT, 0), (IN, 1), (BOTH, 0)])       # (BOTH, 1) runs 30 rounds: once, above
def test_every_tuning_gives_the_same_bits(rmat10, scope, d):
    n, src, dst, refs = rmat10
    eng = Engine().load_edges(n, src, dst, BOTH)
    first = check(eng, refs[scope, d], vote_scope=scope, distribute=bool(d))[0]
    for t in itertools.product((1, 8, -1, 1 << 30), (1, -1, 1 << 30), (MIN_SLOTS, -1)):
        lab, info = check(tune(eng, *t), refs[scope, d], vote_scope=scope, distribute=bool(d))
        assert lab.tobytes() == first.tobytes(), t
    for key, bad in ((L.TUNE_PP_WAVE_ROW, 0), (L.TUNE_PP_BLOCK_ROW, 0.5), (L.TUNE_PP_SLOTS, MIN_SLOTS - 1),
                     (L.TUNE_PP_SLOTS, 1025)):
        with pytest.raises(TitanException) as e:
            eng.set_tuning(key, bad)
        assert e.value.code == L.TGO_E_INVALID
    check(tune(eng), refs[scope, d], vote_scope=scope, distribute=bool(d))


def test_run_to_run_and_fetch_later(rmat10):
    n, src, dst, refs = rmat10
    eng = Engine().load_edges(n, src, dst, BOTH)
    lab, info = eng.peer_pressure()
    bytes_after_first = eng.stats()["device_bytes"]
    again, info2 = eng.peer_pressure()
    assert lab.tobytes() == again.tobytes() and info == info2 == refs[OUT, 0][1]
    assert eng.stats()["device_bytes"] == bytes_after_first             # the ranks are built once
    none, info3 = eng.peer_pressure(fetch=False)
    assert none is None and info3 == info
    assert np.array_equal(eng.copy_peer_pressure(), lab)
    eng.kcore()                                                         # another program: no longer the last result
    with pytest.raises(TitanException) as e:
        eng.copy_peer_pressure()
    assert e.value.code == L.TGO_E_STATE
    check(eng, refs[BOTH, 1], vote_scope=BOTH, distribute=True)


# ------------------------------------------------------------------ rows, the computer, write-back
@pytest.mark.parametrize("fixture", ["gotg", "partition_groups"])
def test_fixture_rows_equal_the_reference_over_their_edges(fixture):
    """The fixtures hold encoded rows, not an edge list, so the reference's edges are read back from
    the engine's own lists: this checks the kernels on what was loaded (and that a vertex cut is one
    vertex), not the decode, which test_gpu_parity.py pins against the oracle."""
    rows, vids, sd, npz = load_fixture(fixture)
    eng = Engine().load_rows(rows, Schema.from_dict(sd), BOTH)
    src, dst = pr.edges_from_lists(eng.graph_csr(0), eng.graph_perm())
    ids = eng.vertex_ids()
    assert len(set(ids.tolist())) == eng.n                              # vertex cuts appear once, canonically
    for scope, d in CASES:
        ref = pr.reference(eng.n, src, dst, ids, scope, d)
        check(tune(eng), ref, vote_scope=scope, distribute=bool(d))
        check(tune(eng, 1, 4, MIN_SLOTS), ref, vote_scope=scope, distribute=bool(d))


def test_through_the_computer_with_the_map_reduces(rmat10):
    n, src, dst, refs = rmat10
    graph = GpuGraph(edges=(n, src, dst, None))
    for scope, d in ((OUT, 0), (BOTH, 1)):
        prog = PeerPressureVertexProgram.build().edges(SCOPES[scope]).distributeVote(bool(d)).create()
        c = graph.compute().program(prog).mapReduce(ClusterCountMapReduce.build().create())
        res = c.mapReduce(ClusterPopulationMapReduce.build().create()).submit().get()
        ids, got = res.vertex_properties[CLUSTER]
        want, info = pr.reference(n, src, dst, ids, scope, d)
        assert np.array_equal(got, want)
        assert res.memory().get("clusterCount") == info["clusters"]
        pop = res.memory().get("clusterPopulation")
        assert len(pop) == info["clusters"] and max(pop.values()) == info["largest"] and sum(pop.values()) == n
        assert res.memory().getIteration() == info["rounds"]
    res = graph.compute().program(PeerPressureVertexProgram.build().maxIterations(1).create()).submit().get()
    assert res.memory().getIteration() == 1


def test_result_rows_are_the_component_encoding():
    rows, vids, sd, npz = load_fixture("gotg")
    kc = (7500 << 6) | 5
    eng = Engine().load_rows(rows, Schema.from_dict(sd), BOTH)
    base = 1 << 30
    with pytest.raises(TitanException) as e:
        eng.result_rows(L.RESULT_PEER_PRESSURE, [kc], [L.DT_LONG], base)        # no finished program yet
    assert e.value.code == L.TGO_E_STATE
    none, _ = eng.peer_pressure(vote_scope=BOTH, fetch=False)
    lab, ids = eng.copy_peer_pressure(), eng.vertex_ids()
    lib = fr.load()
    for dt, enc in ((L.DT_LONG, lambda x, rel: fr.encode_property(kc, L.DT_LONG, x, rel)),
                    (L.DT_INTEGER, lambda x, rel: fr.encode_property(kc, L.DT_INTEGER, x, rel)),
                    (L.DT_OBJECT, lambda x, rel: fr.encode_property_generic(kc, L.DT_LONG, x, rel))):
        got = eng.result_rows(L.RESULT_PEER_PRESSURE, [kc], [dt], base)
        assert got.nrows == eng.n and list(got.entry_begin) == list(range(eng.n + 1))
        for r in range(got.nrows):
            b = bytes(got.data[got.byte_begin[r]:got.byte_begin[r + 1]])
            assert b == enc(int(lab[r]), base + r)[0], (dt, r)
            assert got.keys[r] == lib.fr_key_of(int(ids[r]), 5)
    with pytest.raises(TitanException) as e:
        eng.result_rows(L.RESULT_PEER_PRESSURE, [kc], [L.DT_DOUBLE], base)
    assert e.value.code == L.TGO_E_INVALID
    with pytest.raises(TitanException) as e:
        eng.result_rows(L.RESULT_COMPONENT, [kc], [L.DT_LONG], base)            # the other label program's kind
    assert e.value.code == L.TGO_E_STATE
    # kind 9 is kind 4's encoding: the same Long values under tgo_components' kind give the same bytes
    n, src, dst = pr.cycle(3)
    eng = Engine().load_edges(n, src, dst, BOTH, titan_ids=np.array([24, 32, 40], np.int64))
    assert eng.peer_pressure()[0].tolist() == [24, 24, 24] == eng.components()[0].tolist()
    comp = eng.result_rows(L.RESULT_COMPONENT, [kc], [L.DT_LONG], base)
    eng.peer_pressure(fetch=False)
    mine = eng.result_rows(L.RESULT_PEER_PRESSURE, [kc], [L.DT_LONG], base)
    assert bytes(mine.data) == bytes(comp.data) and list(mine.byte_begin) == list(comp.byte_begin)
    assert list(mine.keys) == list(comp.keys)
    # write-back through the computer
    graph = GpuGraph(rows, sd, property_keys={CLUSTER: (kc, L.DT_LONG)})
    c = graph.compute()
    c.resultMode(TitanGraphComputer.ResultMode.PERSIST)
    res = c.program(PeerPressureVertexProgram.build().create()).submit().get()
    ids, lab = res.vertex_properties[CLUSTER]
    for vid, x in zip(ids, lab):
        assert graph.read_property(int(vid), kc, L.DT_LONG) == int(x)


# ------------------------------------------------------------------ native equals generic
def test_native_equals_the_generic_program():
    n = 1 << 8
    src, dst, _ = rmat_edges(8, 8, seed=31)
    graph = GpuGraph(edges=(n, src, dst, None))
    for scope, d in CASES:
        prog = PeerPressureVertexProgram.build().edges(SCOPES[scope]).distributeVote(bool(d)).create()
        native = graph.compute().program(prog).submit().get()
        nids, nlab = native.vertex_properties[CLUSTER]
        generic_prog = GenericPeerPressure(SCOPES[scope], bool(d))
        generic = graph.compute().program(generic_prog).submit().get()
        gids, (glab, present) = generic.vertex_properties["cluster"]
        assert present.all() and np.array_equal(nids, gids)
        assert np.asarray(glab, np.int64).tobytes() == np.asarray(nlab, np.int64).tobytes()
        assert generic_prog.rounds == native.memory().getIteration()


# ------------------------------------------------------------------ errors
def test_errors_leave_the_ctx_usable():
    n, src, dst = pr.cycle(64)
    good = pr.reference(n, src, dst, Engine().load_edges(n, src, dst, BOTH).vertex_ids())
    eng = Engine().load_edges(n, src, dst, OUT)                          # not bothE
    with pytest.raises(TitanException) as e:
        eng.peer_pressure()
    assert e.value.code == L.TGO_E_INVALID
    a = L.PpArgs(BOTH, 0, OUT, 0, 30, 0)                                 # bothE, but not the loaded scope
    assert eng.lib.tgo_peer_pressure(eng.ctx, C.byref(a), None, None) == L.TGO_E_INVALID
    eng.load_edges(n, src, dst, BOTH)
    check(eng, good)
    eng = Engine()                                                       # before a load
    with pytest.raises(TitanException) as e:
        eng.peer_pressure()
    assert e.value.code == L.TGO_E_STATE
    eng.load_edges(n, src, dst, BOTH)
    out = np.zeros(n, np.int64)
    assert eng.lib.tgo_copy_peer_pressure(eng.ctx, L.ptr(out, C.c_int64)) == L.TGO_E_STATE      # no finished run
    for bad in (L.PpArgs(BOTH, 1, OUT, 0, 30, 0),                        # flags
                L.PpArgs(BOTH, 0, OUT, 0, 30, 1),                        # pad
                L.PpArgs(BOTH, 0, 3, 0, 30, 0), L.PpArgs(BOTH, 0, -1, 0, 30, 0),    # vote_scope
                L.PpArgs(BOTH, 0, OUT, 2, 30, 0), L.PpArgs(BOTH, 0, OUT, -1, 30, 0),   # distribute
                L.PpArgs(BOTH, 0, OUT, 0, -1, 0),                        # max_rounds
                L.PpArgs(OUT, 0, OUT, 0, 30, 0)):                        # scope
        assert eng.lib.tgo_peer_pressure(eng.ctx, C.byref(bad), None, None) == L.TGO_E_INVALID
        check(eng, good)
    assert eng.lib.tgo_peer_pressure(eng.ctx, None, None, None) == L.TGO_E_INVALID
    eng.kcore()
    assert eng.lib.tgo_copy_peer_pressure(eng.ctx, L.ptr(out, C.c_int64)) == L.TGO_E_STATE      # after another program
    check(eng, good)
    # lists that are not each other's transpose: a triangle 0 -> 1 -> 2 -> 0 whose IN entry of 0 -> 1 is missing
    out_off, out_idx = np.array([0, 1, 2, 3], np.int64), np.array([1, 2, 0], np.int32)
    in_off, in_idx = np.array([0, 1, 1, 2], np.int64), np.array([2, 1], np.int32)
    eng = Engine().load_csr(3, out_off, out_idx, in_off, in_idx, BOTH, titan_ids=np.array([8, 16, 24], np.int64))
    with pytest.raises(TitanException) as e:
        eng.peer_pressure()
    assert e.value.code == L.TGO_E_UNSUPPORTED and "votes" in str(e.value)
    eng.load_edges(n, src, dst, BOTH)
    check(eng, good)
    eng = Engine().load_partition(n, 0, n, src, dst, BOTH)               # a partitioned ctx
    with pytest.raises(TitanException) as e:
        eng.peer_pressure()
    assert e.value.code == L.TGO_E_UNSUPPORTED
    eng.load_edges(n, src, dst, BOTH)
    check(eng, good)
