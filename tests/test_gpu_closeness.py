"""GPU: native closeness and harmonic centrality (tgo_closeness, titan_amd/csrc/cl.hip).

The reference is cl_ref.py (one BFS per seed, integer far / reach / ecc, the harmonic sum folded in the
contractual order; test_cl_cpu.py checks it against closed forms and exact Fraction sums).  Comparison
rule: far / reach / ecc / info array_equal, closeness and harmonic tobytes() equality — the device
folds in the same order with IEEE fp64 division and addition, so every value matches bit for bit.
tgo_copy_multi_distances after a closeness run returns the distances of the LAST batch (documented in
the header); test_the_sweep_state_afterwards pins that.
"""
import ctypes as C

import numpy as np
import pytest

import bc_ref as br
import cl_ref as cr
import fulgora as fr
from conftest import load_fixture
from titan_amd import (ClosenessCentralityVertexProgram, ClosenessRankMapReduce, Engine, GpuGraph, Schema,
                       TitanException, rmat_edges)
from titan_amd import _lib as L

pytestmark = pytest.mark.gpu

OUT, IN, BOTH = L.SCOPE_OUT_E, L.SCOPE_IN_E, L.SCOPE_BOTH_E
ABSENT = L.DIST_ABSENT
INTS = ("far", "reach", "ecc")
FLOATS = ("closeness", "harmonic")
NONE = (np.zeros(0, np.int32), np.zeros(0, np.int32))
ZERO_INFO = {"sources": 0, "reached_pairs": 0, "batches": 0, "max_depth": 0}


def run(eng, ref, seeds=None, scope=BOTH, dense=True, max_depth=None):
    """One run against (arrays, info) of the reference, bit for bit.  seeds are row numbers (dense)
    unless dense is False."""
    want, winfo = ref
    res, info = eng.closeness(seeds, dense=dense, max_depth=max_depth, scope=scope)
    got = eng.copy_closeness()
    print("info", info, "far sum", int(got["far"].sum()), "harmonic sum", float(got["harmonic"].sum()))
    assert info == winfo
    for k in INTS:
        assert got[k].dtype == np.int64 and np.array_equal(got[k], want[k]), k
    for k in FLOATS:
        assert res[k].dtype == np.float64 and len(res[k]) == eng.n
        assert got[k].tobytes() == want[k].tobytes(), k
        assert res[k].tobytes() == want[k].tobytes(), k
    st = eng.stats()
    assert st["iterations"] == info["batches"] and st["levels"] == info["max_depth"]
    return got, info


@pytest.fixture(scope="module")
def gnp301():
    n, src, dst = br.gnp(301, 0.03, 9)
    ids, s2, d2, new = br.relabel(n, src, dst)
    return n, s2, d2, ids


@pytest.fixture(scope="module")
def path300():
    return br.path(300)


@pytest.fixture(scope="module")
def rmat10():
    n = 1 << 10
    src, dst, _ = rmat_edges(10, 8, seed=31)             # hubs, duplicates, self-loops
    assert (src == dst).any()
    return n, src, dst, cr.reference(n, src, dst, BOTH)


# ------------------------------------------------------------------ batch edges
@pytest.mark.parametrize("count", [1, 63, 64, 65, 129])
def test_batch_edges_with_a_duplicate_and_an_unknown_seed(gnp301, count):
    n, src, dst, ids = gnp301
    rows = np.random.default_rng(count).choice(n, count, replace=False)
    if count > 1:
        rows[-1] = rows[0]                                # a duplicate counts twice
    unknown = int(ids[-1]) + 1
    assert unknown not in set(ids.tolist())
    given = ids[rows].tolist()
    given.insert(len(given) // 2, unknown)                # contributes nothing, is not counted
    given.append(unknown)
    eng = Engine().load_edges(n, src, dst, BOTH, titan_ids=ids)
    assert np.array_equal(eng.vertex_ids(), ids)
    ref = cr.reference(n, src, dst, BOTH, seeds=rows)
    assert ref[1]["sources"] == count and ref[1]["batches"] == (count + 63) // 64
    got, _ = run(eng, ref, seeds=given, dense=False)
    assert got["reach"].max() <= count


# ------------------------------------------------------------------ 64 distinct levels, plane boundaries
@pytest.mark.parametrize("first", [0, 236])
def test_path_of_300_sees_64_distinct_levels_over_nine_planes(path300, first):
    n, src, dst = path300
    seeds = list(range(first, first + 64))
    ref = cr.reference(n, src, dst, BOTH, seeds=seeds)
    far_end = 299 if first == 0 else 0
    assert ref[0]["reach"][far_end] == 64 and ref[0]["ecc"][far_end] == 299      # levels cross 255 / 256
    got, info = run(Engine().load_edges(n, src, dst, BOTH), ref, seeds=seeds)
    assert info["max_depth"] == 299 and info["batches"] == 1
    assert got["far"][far_end] == sum(range(236, 300))


# ------------------------------------------------------------------ level 0, closed forms, all seeds
def test_path_of_33_all_seeds():
    n, src, dst = br.path(33)
    got, info = run(Engine().load_edges(n, src, dst, BOTH), cr.reference(n, src, dst, BOTH))
    assert got["far"].tolist() == [i * (i + 1) // 2 + (32 - i) * (33 - i) // 2 for i in range(33)]
    assert (got["reach"] == 32).all() and info["max_depth"] == 32


def test_star_with_64_leaves_all_seeds():
    n, src, dst = br.star(64)
    got, info = run(Engine().load_edges(n, src, dst, BOTH), cr.reference(n, src, dst, BOTH))
    assert got["far"].tolist() == [64] + [127] * 64 and got["closeness"][0] == 1.0
    assert got["harmonic"].tolist() == [64.0] + [32.5] * 64 and info["batches"] == 2


@pytest.mark.parametrize("n", [64, 65])
def test_cycles_all_seeds(n):
    _, src, dst = br.cycle(n)
    got, info = run(Engine().load_edges(n, src, dst, BOTH), cr.reference(n, src, dst, BOTH))
    assert got["far"].tolist() == [(n * n - 1) // 4 if n % 2 else n * n // 4] * n
    assert got["ecc"].tolist() == [n // 2] * n and info["reached_pairs"] == n * (n - 1)


def test_clique_of_70_all_seeds():
    n, src, dst = br.clique(70)
    got, info = run(Engine().load_edges(n, src, dst, BOTH), cr.reference(n, src, dst, BOTH))
    assert got["closeness"].tolist() == [1.0] * 70 and got["harmonic"].tolist() == [69.0] * 70
    assert info == {"sources": 70, "reached_pairs": 70 * 69, "batches": 2, "max_depth": 1}


def test_one_vertex():
    eng = Engine().load_edges(1, *NONE, BOTH)
    got, info = run(eng, cr.reference(1, *NONE, BOTH))
    assert info == {"sources": 1, "reached_pairs": 0, "batches": 1, "max_depth": 0}
    for k in FLOATS:
        assert got[k].tobytes() == np.zeros(1).tobytes()
    run(eng, cr.reference(1, *NONE, BOTH, seeds=[]), seeds=[])


def test_no_vertices():
    import edgestore as es
    _, _, sd, _ = load_fixture("gotg")
    rows = es.Rows(np.zeros(0, np.int64), np.zeros(1, np.int64), np.zeros(1, np.int64), np.zeros(0, np.uint8),
                   np.zeros(0, np.int64))
    eng = Engine().load_rows(rows, Schema.from_dict(sd), BOTH)
    assert eng.n == 0
    res, info = eng.closeness()
    assert info == ZERO_INFO and all(len(res[k]) == 0 for k in FLOATS)
    assert all(len(v) == 0 for v in eng.copy_closeness().values())
    st = eng.stats()
    assert st["iterations"] == 0 and st["levels"] == 0


# ------------------------------------------------------------------ unreached vertices
def test_two_components_and_isolated_vertices_n65():
    _, s1, d1 = br.path(30)
    _, s2, d2 = br.cycle(20)
    n = 65                                               # 30 + 20 + 15 vertices without an entry
    src, dst = np.concatenate([s1, s2 + 30]).astype(np.int32), np.concatenate([d1, d2 + 30]).astype(np.int32)
    eng = Engine().load_edges(n, src, dst, BOTH)
    got, info = run(eng, cr.reference(n, src, dst, BOTH))
    assert info["reached_pairs"] == 30 * 29 + 20 * 19 and info["batches"] == 2 and info["max_depth"] == 29
    for k in INTS:
        assert not got[k][50:].any()
    for k in FLOATS:
        assert got[k][50:].tobytes() == np.zeros(15).tobytes()           # 0.0 means exactly 0.0
    run(eng, cr.reference(n, src, dst, BOTH, seeds=[64, 3, 40]), seeds=[64, 3, 40])   # an isolated seed reaches nobody


# ------------------------------------------------------------------ direction, weights
@pytest.fixture(scope="module")
def directed_refs(gnp301):
    n, src, dst, ids = gnp301
    seeds = list(range(0, n, 3))
    refs = {s: cr.reference(n, src, dst, s, seeds=seeds) for s in (OUT, IN, BOTH)}
    fars = [refs[s][0]["far"] for s in (OUT, IN, BOTH)]
    assert not np.array_equal(fars[0], fars[1]) and not np.array_equal(fars[0], fars[2])
    assert not np.array_equal(fars[1], fars[2])
    return seeds, refs


@pytest.mark.parametrize("scope", [OUT, IN, BOTH])
def test_directed_gnp_per_scope(gnp301, directed_refs, scope):
    n, src, dst, ids = gnp301
    seeds, refs = directed_refs
    eng = Engine().load_edges(n, src, dst, scope, titan_ids=ids)
    run(eng, refs[scope], seeds=seeds, scope=scope)


def test_weights_are_ignored(gnp301, directed_refs):
    n, src, dst, ids = gnp301
    seeds, refs = directed_refs
    w = np.random.default_rng(2).integers(1, 9, len(src)).astype(np.int32)
    eng = Engine().load_edges(n, src, dst, BOTH, weight=w, titan_ids=ids)
    run(eng, refs[BOTH], seeds=seeds)


# ------------------------------------------------------------------ max_depth
@pytest.mark.parametrize("depth", [0, 1, 3])
def test_max_depth_cut(gnp301, path300, depth):
    n, src, dst = path300
    seeds = [0, 150, 299, 150]
    _, info = run(Engine().load_edges(n, src, dst, BOTH), cr.reference(n, src, dst, BOTH, seeds=seeds, max_depth=depth),
                  seeds=seeds, max_depth=depth)
    assert info["max_depth"] == depth and info["reached_pairs"] == (0 if depth == 0 else 2 * depth + 2 * 2 * depth)
    n, src, dst, ids = gnp301
    _, info = run(Engine().load_edges(n, src, dst, BOTH, titan_ids=ids),
                  cr.reference(n, src, dst, BOTH, max_depth=depth), max_depth=depth)
    assert info["max_depth"] == depth and info["batches"] == 5


# ------------------------------------------------------------------ exactness at size
def test_rmat10_all_seeds(rmat10):
    n, src, dst, ref = rmat10
    assert ref[1]["batches"] == 16 and ref[1]["sources"] == n
    run(Engine().load_edges(n, src, dst, BOTH), ref)


def test_rmat12_two_hundred_seeds():
    n = 1 << 12
    src, dst, _ = rmat_edges(12, 8, seed=7)
    eng = Engine().load_edges(n, src, dst, BOTH)
    ids = eng.vertex_ids()
    rows = np.random.default_rng(12).choice(n, 200, replace=False)
    ref = cr.reference(n, src, dst, BOTH, seeds=rows)
    assert ref[1]["batches"] == 4 and ref[1]["reached_pairs"] > 0
    run(eng, ref, seeds=ids[rows], dense=False)


@pytest.mark.parametrize("key,value", [(L.TUNE_MS_SPARSE, 0), (L.TUNE_MS_SPLIT, 0), (L.TUNE_MS_STAY, 0),
                                       (L.TUNE_MS_COLD, 2)])
def test_tuning_independence(rmat10, key, value):
    n, src, dst, ref = rmat10
    eng = Engine().load_edges(n, src, dst, BOTH)
    eng.closeness(fetch=False)
    base = eng.copy_closeness()
    eng.set_tuning(key, value)
    run(eng, ref)
    tuned = eng.copy_closeness()
    for k in INTS + FLOATS:
        assert tuned[k].tobytes() == base[k].tobytes(), k


# ------------------------------------------------------------------ oracle pin
def oracle_sums(o, seeds, scope, n):
    far, reach = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for s in seeds:
        d, _ = o.shortest_distance(int(s), 1 << 20, scope)
        at = (d != ABSENT) & (d > 0)
        far += np.where(at, d, 0)
        reach += at
    return far, reach


@pytest.mark.parametrize("fixture,scope,limit", [("gotg", BOTH, 100000), ("degree_random100", IN, 5)])
def test_far_and_reach_equal_the_oracles_shortest_distance_sums(fixture, scope, limit):
    rows, vids, sd, npz = load_fixture(fixture)
    osch = fr.OracleSchema(sd["edge_types"], [tuple(x) for x in sd["property_keys"]])
    o = fr.OracleGraph.from_rows(rows, osch, scope, hard_limit=limit)
    eng = Engine(hard_query_limit=limit).load_rows(rows, Schema.from_dict(sd), scope)
    ids = eng.vertex_ids()
    assert np.array_equal(ids, o.vertex_ids())
    assert eng.stats()["truncated_results"] == o.stats.truncated_results
    if fixture != "gotg":
        assert o.stats.truncated_results > 0              # the inE cap cuts rows
    far, reach = oracle_sums(o, ids, scope, eng.n)
    res, info = eng.closeness(scope=scope)
    got = eng.copy_closeness()
    assert np.array_equal(got["far"], far) and np.array_equal(got["reach"], reach)
    assert info["sources"] == eng.n and info["reached_pairs"] == int(reach.sum()) and reach.sum() > 0
    some = far > 0
    assert np.array_equal(got["closeness"][some], reach[some] / far[some]) and not got["closeness"][~some].any()


# ------------------------------------------------------------------ interaction with the sweep
def test_the_sweep_state_afterwards(gnp301):
    n, src, dst, ids = gnp301
    eng = Engine().load_edges(n, src, dst, BOTH, titan_ids=ids)
    seeds = list(range(70))                              # the last batch holds rows 64..69
    eng.closeness(seeds, dense=True)
    out = np.zeros(n, np.int64)
    for r, row in ((0, 64), (5, 69)):
        assert eng.lib.tgo_copy_multi_distances(eng.ctx, r, L.ptr(out, C.c_int64)) == L.TGO_OK
        assert np.array_equal(out, eng.bfs(row, n, BOTH, seed_is_dense=True)), r
        eng.closeness(seeds, dense=True)                 # tgo_bfs ran: fold the sweeps again
    assert eng.lib.tgo_copy_multi_distances(eng.ctx, 6, L.ptr(out, C.c_int64)) == L.TGO_E_INVALID
    multi = eng.bfs_multi([3, 200, 3, 77], n, BOTH, seed_is_dense=True)
    for i, row in enumerate((3, 200, 3, 77)):
        assert np.array_equal(multi[i], eng.bfs(row, n, BOTH, seed_is_dense=True)), row
    with pytest.raises(TitanException) as e:
        eng.copy_closeness()                             # other programs ran since
    assert e.value.code == L.TGO_E_STATE


# ------------------------------------------------------------------ errors
def test_errors_leave_the_ctx_usable():
    n, src, dst = br.path(33)
    ref = cr.reference(n, src, dst, BOTH)
    eng = Engine().load_edges(n, src, dst, IN)
    with pytest.raises(TitanException) as e:
        eng.closeness()                                  # bothE is not the loaded scope
    assert e.value.code == L.TGO_E_INVALID
    eng.load_edges(n, src, dst, BOTH)
    one, past = np.array([8], np.int64), np.array([33], np.int64)
    for bad, seeds, nseeds in ((L.ClArgs(IN, 0, 5, 0), None, -1), (L.ClArgs(3, 0, 5, 0), None, -1),
                               (L.ClArgs(BOTH, 1, 5, 0), None, -1), (L.ClArgs(BOTH, 0, -1, 0), None, -1),
                               (L.ClArgs(BOTH, 0, 5, 0), None, -2), (L.ClArgs(BOTH, 0, 5, 0), None, 3),
                               (L.ClArgs(BOTH, 0, 5, 1), L.ptr(past, C.c_int64), 1)):      # a dense seed out of range
        assert eng.lib.tgo_closeness(eng.ctx, C.byref(bad), seeds, nseeds, None, None, None) == L.TGO_E_INVALID
    assert eng.lib.tgo_closeness(eng.ctx, None, L.ptr(one, C.c_int64), 1, None, None, None) == L.TGO_E_INVALID
    assert eng.lib.tgo_copy_closeness(eng.ctx, None, None, None, None, None) == L.TGO_E_STATE     # no finished run
    run(eng, ref)
    assert eng.lib.tgo_copy_closeness(eng.ctx, None, None, None, None, None) == L.TGO_OK          # each may be NULL
    eng.bfs(0, n, BOTH, seed_is_dense=True)
    with pytest.raises(TitanException) as e:
        eng.copy_closeness()                             # tgo_bfs ran since
    assert e.value.code == L.TGO_E_STATE
    run(eng, ref)
    n, src, dst = br.cycle(64)                           # (a partition holds a multiple of 64 rows)
    eng = Engine().load_partition(n, 0, n, src, dst, BOTH)
    with pytest.raises(TitanException) as e:
        eng.closeness()
    assert e.value.code == L.TGO_E_UNSUPPORTED
    eng.load_edges(n, src, dst, BOTH)
    run(eng, cr.reference(n, src, dst, BOTH))


# ------------------------------------------------------------------ surfaces
def test_result_rows_match_the_oracle_encoder():
    from test_gpu_writeback import assert_rows_equal, expected_rows, BASE
    rows, vids, sd, npz = load_fixture("gotg")
    kc, kh = (7600 << 6) | 5, (7601 << 6) | 5
    eng = Engine().load_rows(rows, Schema.from_dict(sd), BOTH)
    with pytest.raises(TitanException) as e:
        eng.result_rows(L.RESULT_CLOSENESS, [kc, kh], [L.DT_DOUBLE, L.DT_DOUBLE], BASE)   # no finished program yet
    assert e.value.code == L.TGO_E_STATE
    none, info = eng.closeness(fetch=False)
    assert none == {"closeness": None, "harmonic": None} and info["sources"] == eng.n
    got5 = eng.copy_closeness()
    cl, ha = got5["closeness"], got5["harmonic"]
    assert (cl > 0).any() and (ha > 0).any()
    ids = eng.vertex_ids()

    def col(kv):
        return fr.buf_bytes("fr_write_relation_type", kv[0], 0, 0, 0)

    for keys in ((kc, kh), (kh + (5 << 6), kc)):         # either column order
        for dts, enc in (((L.DT_DOUBLE, L.DT_DOUBLE), lambda k, x, rel: fr.encode_property_f64(k, x, rel)),
                         ((L.DT_OBJECT, L.DT_OBJECT), lambda k, x, rel: fr.encode_property_generic(k, L.DT_DOUBLE, x, rel))):
            def entries(i, rel):
                kvs = sorted([(keys[0], float(cl[i])), (keys[1], float(ha[i]))], key=col)
                return [enc(k, v, rel + j) for j, (k, v) in enumerate(kvs)]
            got = eng.result_rows(L.RESULT_CLOSENESS, list(keys), list(dts), BASE)
            assert got.nrows == eng.n
            assert_rows_equal(got, expected_rows(ids, entries))
    for dts in ((L.DT_INTEGER, L.DT_DOUBLE), (L.DT_DOUBLE, L.DT_INTEGER), (L.DT_LONG, L.DT_LONG)):
        with pytest.raises(TitanException) as e:
            eng.result_rows(L.RESULT_CLOSENESS, [kc, kh], list(dts), BASE)
        assert e.value.code == L.TGO_E_INVALID
    with pytest.raises(TitanException) as e:
        eng.result_rows(L.RESULT_PAGERANK, [kc, kh], [L.DT_DOUBLE, L.DT_DOUBLE], BASE)    # another program's kind
    assert e.value.code == L.TGO_E_STATE
    assert eng.copy_closeness()["harmonic"].tobytes() == ha.tobytes()    # the refused calls left the result in place


def test_through_the_computer_with_the_rank_map_reduce(gnp301):
    n, src, dst, ids = gnp301
    P = ClosenessCentralityVertexProgram
    graph = GpuGraph(edges=(n, src, dst, None))
    res = (graph.compute().program(P.build().create())
           .mapReduce(ClosenessRankMapReduce(top=5))
           .mapReduce(ClosenessRankMapReduce.build().by(P.HARMONIC).top(3).memoryKey("harmonicRank").create())
           .submit().get())
    want, winfo = cr.reference(n, src, dst, BOTH)
    gids, cl = res.vertex_properties[P.CLOSENESS]
    _, ha = res.vertex_properties[P.HARMONIC]
    assert cl.tobytes() == want["closeness"].tobytes() and ha.tobytes() == want["harmonic"].tobytes()
    assert res.memory().getIteration() == winfo["batches"] == 5
    for key, vals, top in (("closenessRank", cl, 5), ("harmonicRank", ha, 3)):
        order = np.lexsort((gids, -vals))[:top]
        got = list(res.memory().get(key))
        assert [(kv.key, kv.value) for kv in got] == [(int(gids[i]), float(vals[i])) for i in order]
    seeds = [int(gids[0]), int(gids[80])]
    res = graph.compute().program(P.build().seeds(seeds).maxDepth(2).edges("outE").create()).submit().get()
    want, winfo = cr.reference(n, src, dst, OUT, seeds=[0, 80], max_depth=2)
    assert res.vertex_properties[P.HARMONIC][1].tobytes() == want["harmonic"].tobytes()
    assert res.memory().getIteration() == 1
