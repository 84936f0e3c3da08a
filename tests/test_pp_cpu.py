"""CPU: the host-side surface of the native peer-pressure program — the C-ABI mirror, the declarations
in the header / JNI shim / TgoNative.java, the program builder, the map-reduces' key choice — and the
plain-Python reference the GPU tests compare with (pp_ref.py), checked against closed forms."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pp_ref as pr
import titan_amd
from titan_amd import _lib as L
from titan_amd import computer as cp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


# ------------------------------------------------------------------ the boundary
def test_exports_structs_and_constants():
    assert "tgo_peer_pressure" in L.EXPORTS and "tgo_copy_peer_pressure" in L.EXPORTS
    assert C.sizeof(L.PpArgs) == 24 and C.sizeof(L.PpInfo) == 32
    assert [f[0] for f in L.PpArgs._fields_] == ["scope", "flags", "vote_scope", "distribute", "max_rounds", "pad"]
    assert [f[0] for f in L.PpInfo._fields_] == ["clusters", "largest", "changed_last", "rounds", "converged"]
    assert L.RESULT_PEER_PRESSURE == 9
    assert (L.TUNE_PP_WAVE_ROW, L.TUNE_PP_BLOCK_ROW, L.TUNE_PP_SLOTS) == (22, 23, 24)
    assert (pr.OUT, pr.IN, pr.BOTH) == (L.SCOPE_OUT_E, L.SCOPE_IN_E, L.SCOPE_BOTH_E)
    lib = L.load()
    assert hasattr(lib, "tgo_peer_pressure") and hasattr(lib, "tgo_copy_peer_pressure")


def test_header_shim_and_java_name_the_entry_points():
    hdr = _read("include", "titan_gpu_olap.h")
    assert re.search(r"int\s+tgo_peer_pressure\(tgo_ctx\*[^;]*const tgo_pp_args\*[^;]*int64_t\*[^;]*tgo_pp_info\*[^;]*\);", hdr)
    assert re.search(r"int\s+tgo_copy_peer_pressure\(tgo_ctx\*[^;]*int64_t\*[^;]*\);", hdr)
    assert ("typedef struct { int32_t scope; int32_t flags; int32_t vote_scope; int32_t distribute; int32_t max_rounds; "
            "int32_t pad; } tgo_pp_args;") in hdr
    assert "typedef struct { int64_t clusters, largest, changed_last; int32_t rounds, converged; } tgo_pp_info;" in hdr
    assert "TGO_RESULT_PEER_PRESSURE = 9" in hdr
    assert "TGO_TUNE_PP_WAVE_ROW = 22, TGO_TUNE_PP_BLOCK_ROW = 23, TGO_TUNE_PP_SLOTS = 24" in hdr
    block = hdr[hdr.index("Peer-pressure clustering"):hdr.index("tgo_pp_args;")]
    for phrase in ("EVERY ENTRY IS ONE EDGE", "SMALLEST TITAN ID", "DEVIATION", "DETERMINISTIC", "floor(2^32 / d(v))"):
        assert phrase in block, phrase
    shim = _read("java", "jni", "titan_gpu_olap_jni.c")
    assert re.search(r"JNIEXPORT\s+jlongArray\s+JNICALL\s+JFN\(peerPressure\)", shim) and "tgo_peer_pressure(" in shim
    java = os.path.join("java", "src", "main", "java", "com", "thinkaurelius", "titan", "graphdb", "olap")
    native = _read(java, "gpu", "TgoNative.java")
    assert re.search(r"public static native long\[\] peerPressure\(long ctx, int voteScope, boolean distribute, int maxRounds\);",
                     native)
    assert "RESULT_PEER_PRESSURE = 9" in native
    comp = _read(java, "computer", "GpuGraphComputer.java")
    assert "PeerPressureVertexProgram" in comp and "gremlin.peerPressureVertexProgram.cluster" in comp


def test_program_builder_and_wiring():
    P = titan_amd.PeerPressureVertexProgram
    assert P.CLUSTER == "gremlin.peerPressureVertexProgram.cluster" and P.compute_keys == (P.CLUSTER,)
    assert P.scope_name == "bothE"
    p = P.build().create()
    assert (p.distribute, p.max_iterations, p.edges) == (False, 30, "outE")
    p = P.build().distributeVote(True).maxIterations(7).edges("bothE").create()
    assert (p.distribute, p.max_iterations, p.edges) == (True, 7, "bothE")
    with pytest.raises(titan_amd.TitanException):
        P.build().edges("sideways").create()
    assert cp.GpuGraphComputer._RESULT_KEYS[P] == (L.RESULT_PEER_PRESSURE, (P.CLUSTER,))
    assert "PeerPressureVertexProgram" in titan_amd.__all__


def test_cluster_map_reduces_read_the_cluster_key_first():
    ids = np.array([8, 16, 24, 32], np.int64)
    comp = {cp.ConnectedComponentVertexProgram.COMPONENT: np.array([8, 8, 8, 32], np.int64)}
    clus = {titan_amd.PeerPressureVertexProgram.CLUSTER: np.array([8, 8, 24, 24], np.int64)}
    pop, cnt = titan_amd.ClusterPopulationMapReduce(), titan_amd.ClusterCountMapReduce()
    assert pop.emit(ids, comp) == {8: 3, 32: 1} and cnt.emit(ids, comp) == 2        # exactly as before
    assert pop.emit(ids, clus) == {8: 2, 24: 2} and cnt.emit(ids, clus) == 2
    assert pop.emit(ids, {**comp, **clus}) == {8: 2, 24: 2}
    assert pop.emit(ids, {}) == {} and cnt.emit(ids, {}) == 0


# ------------------------------------------------------------------ pp_ref against closed forms
def run(graph, **kw):
    lab, info = pr.reference(*graph, **kw)
    return lab.tolist(), info


@pytest.mark.parametrize("distribute", [0, 1])
def test_doubled_directed_3_cycle_never_converges(distribute):
    lab, info = run(pr.cycle(3, 2), distribute=distribute, max_rounds=7)
    assert lab == [2, 0, 1]
    assert info == {"clusters": 3, "largest": 1, "changed_last": 3, "rounds": 7, "converged": 0}


@pytest.mark.parametrize("distribute", [0, 1])
def test_single_3_cycle(distribute):
    lab, info = run(pr.cycle(3), distribute=distribute)
    assert lab == [0, 0, 0] and info["rounds"] == 3 and info["converged"] == 1 and info["changed_last"] == 0


def test_two_k5_and_a_bridge():
    lab, info = run(pr.two_cliques_bridge(5), vote_scope=pr.BOTH, distribute=0)
    assert lab == [0] * 5 + [5] * 5 and info["rounds"] == 3 and info["clusters"] == 2 and info["largest"] == 5
    lab, info = run(pr.two_cliques_bridge(5), vote_scope=pr.BOTH, distribute=1)
    assert lab == [0] * 5 + [6] * 5 and info["rounds"] == 2


def test_path_of_9():
    lab, info = run(pr.path(9), vote_scope=pr.BOTH)
    assert lab == [0] * 9 and info["rounds"] == 9 and info["converged"] == 1


def test_star_of_64_leaves():
    got = [run(pr.star(64), vote_scope=s, distribute=d) for s in (pr.OUT, pr.IN, pr.BOTH) for d in (0, 1)]
    assert [info["rounds"] for _, info in got] == [2, 1, 1, 1, 2, 2]
    assert all(info["converged"] == 1 for _, info in got)
    own = list(range(65))
    # OUT: every leaf hears the hub alone, a 1-1 tie that the hub's smaller id wins; with the vote
    # split in 64 the leaf's own whole vote wins instead.  IN: the hub hears 64 leaves, each tied
    # with its own vote, and keeps the smallest id, its own; with distribute it sends over no entry.
    assert got[0][0] == [0] * 65 and got[1][0] == own and got[2][0] == own and got[3][0] == own
    # BOTH with distribute: a leaf's whole vote beats the hub's 64th, so the hub joins the smallest leaf
    assert got[4][0] == [0] * 65 and got[5][0] == [1] + own[1:]


@pytest.mark.parametrize("n", [1, 130])
def test_no_edge(n):
    none = np.zeros(0, np.int32)
    for d in (0, 1):
        lab, info = run((n, none, none), distribute=d)
        assert lab == list(range(n))
        assert info == {"clusters": n, "largest": 1, "changed_last": 0, "rounds": 1, "converged": 1}


def test_no_round():
    lab, info = run(pr.cycle(3), ids=[24, 8, 16], max_rounds=0)
    assert lab == [24, 8, 16]
    assert info == {"clusters": 3, "largest": 1, "changed_last": 0, "rounds": 0, "converged": 0}


def test_multiplicity_self_loops_and_titan_id_ties():
    # a -> b twice, c -> b once, a has the largest id: b joins a (a deduplicating tally would tie and pick c)
    e = np.array([(0, 1), (0, 1), (2, 1)], np.int32)
    assert run((3, e[:, 0], e[:, 1]), ids=[30, 20, 10], max_rounds=1)[0] == [30, 30, 10]
    # b with two self-loops keeps b: they vote for b's own cluster, three against one
    e = np.array([(1, 1), (1, 1), (0, 1)], np.int32)
    assert run((2, e[:, 0], e[:, 1]), ids=[10, 20], max_rounds=1)[0] == [10, 20]
    # ties go to the smaller Titan id, not the smaller row
    e = np.array([(0, 2), (1, 2)], np.int32)
    assert run((3, e[:, 0], e[:, 1]), ids=[30, 20, 40], max_rounds=1)[0] == [30, 20, 20]


def test_fixed_point_pin():
    # three votes of floor(2^32 / 3) are 2^32 - 1: the single whole vote wins, although the rationals
    # tie (and the doubles 3 * (1.0 / 3) == 1.0 tie too), which the smaller id a = 0 would win
    assert 3 * (pr.ONE // 3) == pr.ONE - 1 and 3 * (1.0 / 3) == 1.0
    lab, info = run(pr.fixed_point_pin(), distribute=1, max_rounds=1)
    assert lab[2] == 1
    assert run(pr.fixed_point_pin(), distribute=0, max_rounds=1)[0][2] == 0       # three whole votes against one


def test_sinks_keep_their_id_under_distribute():
    n, src, dst = pr.star(5)                # the leaves send over no OUT entry
    lab, _ = run((n, src, dst), ids=[50, 10, 20, 30, 40, 60], distribute=1)
    assert lab == [50, 10, 20, 30, 40, 60]
    lab, _ = run((n, src, dst), ids=[5, 10, 20, 30, 40, 60], distribute=0)
    assert lab == [5] * 6
