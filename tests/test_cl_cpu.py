"""CPU: the host-side surface of the native closeness / harmonic centrality program — struct layouts of
the C-ABI mirror, the declarations in the header / JNI shim / TgoNative.java, the program builder and its
map-reduce, the computer's wiring tables, the Python-side argument checks that need no device — and
the reference the GPU tests compare with (cl_ref.py), checked against closed forms and against exact
Fraction sums.  A vertex accumulates its distances from the seeds; nothing is normalised."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import bc_ref as br
import cl_ref as cr
import titan_amd
from titan_amd import TitanException
from titan_amd import _lib as L
from titan_amd import computer as cp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT, IN, BOTH = L.SCOPE_OUT_E, L.SCOPE_IN_E, L.SCOPE_BOTH_E


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_struct_sizes_and_constants():
    assert C.sizeof(L.ClArgs) == 16
    assert C.sizeof(L.ClInfo) == 24
    assert [f[0] for f in L.ClArgs._fields_] == ["scope", "flags", "max_depth", "seed_is_dense"]
    assert [f[0] for f in L.ClInfo._fields_] == ["sources", "reached_pairs", "batches", "max_depth"]
    assert L.RESULT_CLOSENESS == 10
    assert "tgo_closeness" in L.EXPORTS and "tgo_copy_closeness" in L.EXPORTS


def test_header_shim_and_java_name_the_entry_points():
    hdr = _read("include", "titan_gpu_olap.h")
    assert re.search(r"int\s+tgo_closeness\(tgo_ctx\*[^;]*const tgo_cl_args\*[^;]*const int64_t\*[^;]*int64_t[^;]*"
                     r"double\*[^;]*double\*[^;]*tgo_cl_info\*[^;]*\);", hdr)
    assert re.search(r"int\s+tgo_copy_closeness\(tgo_ctx\*[^;]*int64_t\*[^;]*int64_t\*[^;]*int64_t\*[^;]*double\*[^;]*"
                     r"double\*[^;]*\);", hdr)
    assert "typedef struct { int32_t scope; int32_t flags; int32_t max_depth; int32_t seed_is_dense; } tgo_cl_args;" in hdr
    assert "typedef struct { int64_t sources, reached_pairs; int32_t batches, max_depth; } tgo_cl_info;" in hdr
    assert "TGO_RESULT_CLOSENESS = 10" in hdr
    block = hdr[hdr.index("Closeness and harmonic centrality"):hdr.index("tgo_cl_args;")]
    # the contract: the fold order, the reading, who normalises
    assert "HARMONIC FOLD ORDER" in block and "ascending" in block and "h = h + (double)c / (double)L" in block
    assert "in-closeness" in block and "UNNORMALISED" in block and "left to" in block
    assert "bit-identical" in block and "TGO_TUNE_MS_*" in block
    shim = _read("java", "jni", "titan_gpu_olap_jni.c")
    assert re.search(r"JNIEXPORT\s+jobjectArray\s+JNICALL\s+JFN\(closeness\)", shim) and "tgo_closeness(" in shim
    java = os.path.join("java", "src", "main", "java", "com", "thinkaurelius", "titan", "graphdb", "olap")
    native = _read(java, "gpu", "TgoNative.java")
    assert re.search(r"public static native double\[\]\[\] closeness\(long ctx, long\[\] seeds, int scope, int maxDepth\);",
                     native)
    assert "RESULT_CLOSENESS = 10" in native
    comp = _read(java, "computer", "GpuGraphComputer.java")
    assert "ClosenessCentralityVertexProgram" in comp and "titan.closeness.closeness" in comp
    assert "titan.closeness.harmonic" in comp


def test_program_builder_map_reduce_and_wiring():
    P = titan_amd.ClosenessCentralityVertexProgram
    assert P.CLOSENESS == "titan.closeness.closeness" and P.HARMONIC == "titan.closeness.harmonic"
    assert P.compute_keys == (P.CLOSENESS, P.HARMONIC)
    sib = titan_amd.BetweennessCentralityVertexProgram
    assert (P.preferred_result_graph, P.preferred_persist) == (sib.preferred_result_graph, sib.preferred_persist)
    p = P.build().create()
    assert p.seeds is None and p.max_depth is None and p.scope_name == "bothE"
    p = P.build().seeds([24, 8, 8]).maxDepth(3).edges("outE").create()
    assert p.seeds == [24, 8, 8] and p.max_depth == 3 and p.scope_name == "outE"
    assert cp.GpuGraphComputer._RESULT_KEYS[P] == (L.RESULT_CLOSENESS, (P.CLOSENESS, P.HARMONIC))
    for bad in (dict(edges="sideways"), dict(max_depth=-1), dict(max_depth=1 << 31)):
        with pytest.raises(TitanException) as e:
            P(**bad)
        assert e.value.code == L.TGO_E_INVALID
    with pytest.raises(TitanException) as e:
        titan_amd.ClosenessRankMapReduce(by="titan.betweenness.centrality")
    assert e.value.code == L.TGO_E_INVALID


def test_rank_map_reduce_ordering():
    P = titan_amd.ClosenessCentralityVertexProgram
    mr = titan_amd.ClosenessRankMapReduce(top=3)
    assert mr.memory_key == "closenessRank" and mr.by == P.CLOSENESS
    ids = np.array([40, 8, 16, 24, 32], np.int64)
    props = {P.CLOSENESS: np.array([0.25, 0.5, 0.25, 0.75, 0.25]), P.HARMONIC: np.array([9.0, 1.0, 9.0, 2.0, 3.0])}
    got = mr.emit(ids, props)
    assert [(kv.key, kv.value) for kv in got] == [(24, 0.75), (8, 0.5), (16, 0.25)]    # the tie goes to the smaller id
    by_h = titan_amd.ClosenessRankMapReduce.build().top(2).by(P.HARMONIC).memoryKey("m").create()
    assert by_h.memory_key == "m"
    assert [(kv.key, kv.value) for kv in by_h.emit(ids, props)] == [(16, 9.0), (40, 9.0)]
    assert by_h.emit(ids, {}) == []
    assert len(titan_amd.ClosenessRankMapReduce(top=9).emit(ids, props)) == 5
    assert titan_amd.ClosenessRankMapReduce(top=0).emit(ids, props) == []


# ----------------------------------------------------------------------------- the reference, closed forms
def test_path_from_an_end_and_from_every_vertex():
    n, src, dst = br.path(33)
    res, info = cr.reference(n, src, dst, BOTH, seeds=[0])
    assert res["far"].tolist() == list(range(33)) and int(res["far"].sum()) == 33 * 32 // 2
    assert res["reach"].tolist() == [0] + [1] * 32 and res["ecc"].tolist() == list(range(33))
    assert res["closeness"][0] == 0.0 and res["closeness"][4] == 0.25 and res["harmonic"][4] == 0.25
    assert info == {"sources": 1, "reached_pairs": 32, "batches": 1, "max_depth": 32}
    res, info = cr.reference(n, src, dst, BOTH)
    assert res["far"][0] == res["far"][32] == 33 * 32 // 2                # n (n - 1) / 2 at an end
    assert res["far"].tolist() == [i * (i + 1) // 2 + (32 - i) * (33 - i) // 2 for i in range(33)]
    assert res["ecc"].tolist() == [max(i, 32 - i) for i in range(33)] and (res["reach"] == 32).all()
    assert info == {"sources": 33, "reached_pairs": 33 * 32, "batches": 1, "max_depth": 32}


def test_star_cycles_and_clique():
    res, info = cr.reference(*br.star(64), BOTH)
    assert res["far"].tolist() == [64] + [1 + 2 * 63] * 64 and (res["reach"] == 64).all()
    assert res["ecc"].tolist() == [1] + [2] * 64 and info["batches"] == 2 and info["max_depth"] == 2
    assert res["closeness"][0] == 1.0 and res["harmonic"][0] == 64.0 and res["harmonic"][1] == 1.0 + 63 / 2
    for n in (64, 65):
        res, info = cr.reference(*br.cycle(n), BOTH)
        want = (n * n - 1) // 4 if n % 2 else n * n // 4
        assert res["far"].tolist() == [want] * n and res["ecc"].tolist() == [n // 2] * n
        assert (res["reach"] == n - 1).all() and info["reached_pairs"] == n * (n - 1)
        assert len(set(res["closeness"].tolist())) == 1
    res, info = cr.reference(*br.clique(70), BOTH)
    assert (res["far"] == 69).all() and (res["reach"] == 69).all() and (res["ecc"] == 1).all()
    assert res["closeness"].tolist() == [1.0] * 70 and res["harmonic"].tolist() == [69.0] * 70
    assert info == {"sources": 70, "reached_pairs": 70 * 69, "batches": 2, "max_depth": 1}


def test_directed_path_out_scope_against_in_scope():
    n, src, dst = br.path(20)                                # arcs i -> i + 1
    out, _ = cr.reference(n, src, dst, OUT, seeds=[0])       # messages run along the arcs
    assert out["far"].tolist() == list(range(20))
    inn, info = cr.reference(n, src, dst, IN, seeds=[0])     # ... against them: vertex 0 reaches nobody
    assert not inn["far"].any() and not inn["reach"].any() and info["reached_pairs"] == 0
    assert inn["closeness"].tobytes() == np.zeros(20).tobytes() and inn["harmonic"].tobytes() == np.zeros(20).tobytes()
    inn, _ = cr.reference(n, src, dst, IN, seeds=[19])
    assert inn["far"].tolist() == list(range(19, -1, -1))
    # every vertex a seed: OUT accumulates over the predecessors, IN over the successors
    out, _ = cr.reference(n, src, dst, OUT)
    inn, _ = cr.reference(n, src, dst, IN)
    assert out["far"].tolist() == [i * (i + 1) // 2 for i in range(20)] and out["far"].tolist() == inn["far"][::-1].tolist()
    assert out["harmonic"].tobytes() == inn["harmonic"][::-1].tobytes()
    both, _ = cr.reference(n, src, dst, BOTH)
    assert (both["far"] == out["far"] + inn["far"]).all()


def test_unreached_depth_cut_and_seed_handling():
    n, src, dst = br.two_components_and_isolated()
    res, info = cr.reference(n, src, dst, BOTH)
    for k in ("far", "reach", "ecc"):
        assert res[k][14:].tolist() == [0, 0, 0]
    assert res["closeness"][14:].tobytes() == np.zeros(3).tobytes() and res["harmonic"][14:].tobytes() == np.zeros(3).tobytes()
    assert info == {"sources": 17, "reached_pairs": 9 * 8 + 5 * 4, "batches": 1, "max_depth": 8}
    cut, info = cr.reference(n, src, dst, BOTH, max_depth=3)
    assert info["max_depth"] == 3 and (cut["ecc"] <= 3).all() and cut["far"][0] == 1 + 2 + 3
    zero, info = cr.reference(n, src, dst, BOTH, max_depth=0)
    assert not zero["reach"].any() and info["max_depth"] == 0 and info["sources"] == 17
    one, _ = cr.reference(n, src, dst, BOTH, seeds=[3])
    two, info = cr.reference(n, src, dst, BOTH, seeds=[3, 3])
    assert (two["far"] == 2 * one["far"]).all() and (two["reach"] == 2 * one["reach"]).all() and info["sources"] == 2
    assert (two["ecc"] == one["ecc"]).all() and two["closeness"].tobytes() == one["closeness"].tobytes()
    none, info = cr.reference(n, src, dst, BOTH, seeds=[])
    assert not none["far"].any() and info == {"sources": 0, "reached_pairs": 0, "batches": 0, "max_depth": 0}


def test_the_fold_order_is_per_batch_levels_ascending():
    """Three seeds at distances 3, 1, 3 and, in a second batch, one more at distance 1: the fold is
    ((0 + 1/1) + 2/3) + 1/1, not the seed-order sum."""
    dist = np.full((65, 1), -1, np.int64)
    dist[0, 0], dist[1, 0], dist[2, 0], dist[64, 0] = 3, 1, 3, 1
    res, info = cr.fold(dist)
    want = ((np.float64(0) + np.float64(1) / np.float64(1)) + np.float64(2) / np.float64(3)) + np.float64(1) / np.float64(1)
    assert res["harmonic"][0] == want and res["far"][0] == 8 and res["reach"][0] == 4 and res["ecc"][0] == 3
    assert info["batches"] == 2 and info["sources"] == 65
    assert res["closeness"][0] == 0.5


@pytest.mark.parametrize("graph", ["gnp", "path", "rmat"])
def test_harmonic_against_exact_fractions(graph):
    if graph == "gnp":
        n, src, dst = br.gnp(301, 0.03, 9)
        seeds = list(range(n))
    elif graph == "path":
        n, src, dst = br.path(300)
        seeds = list(range(64))
    else:
        n = 1 << 10
        src, dst, _ = titan_amd.rmat_edges(10, 8, seed=31)
        seeds = list(range(0, n, 5))
    dist = cr.distances(n, src, dst, BOTH, seeds)
    res, info = cr.fold(dist)
    exact = cr.exact_harmonic(dist)
    S = len(seeds)
    worst = Fraction(0)
    for v in range(n):
        got = Fraction(float(res["harmonic"][v]))
        if exact[v] == 0:
            assert res["harmonic"][v].tobytes() == np.float64(0.0).tobytes()
            continue
        err = abs(got - exact[v]) / exact[v]
        worst = max(worst, err)
        assert err <= Fraction(S, 1 << 52), (v, float(err))
    print("worst relative error", float(worst), "bound", S / 2.0 ** 52)
    # closeness is one division of exact integers
    for v in range(n):
        if res["far"][v]:
            assert res["closeness"][v] == int(res["reach"][v]) / int(res["far"][v])
    assert info["reached_pairs"] == int((dist > 0).sum())


def test_engine_argument_checks_need_no_device():
    """Engine.closeness validates max_depth and the seeds' shape before it touches the library."""
    from titan_amd import Engine
    eng = Engine.__new__(Engine)                             # no ctx: a check that reached the library would fail
    eng.ctx = None
    eng.n = 0
    for bad in (-1, 1 << 31):
        with pytest.raises(ValueError):
            eng.closeness(max_depth=bad)
    with pytest.raises(ValueError):
        eng.closeness(seeds=[[1, 2], [3, 4]])
