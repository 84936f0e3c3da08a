"""CPU: the host-side surface of the native betweenness program — struct layouts of the C-ABI mirror,
the declarations in the header / JNI shim / TgoNative.java, the program builder and its map-reduce,
the computer's wiring tables — and the exact reference the GPU tests compare with (bc_ref.py),
checked against closed forms.  All values are raw sums over ordered pairs."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np

import bc_ref as br
import titan_amd
from titan_amd import _lib as L
from titan_amd import computer as cp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_struct_sizes_and_constants():
    assert C.sizeof(L.BcArgs) == 16
    assert C.sizeof(L.BcInfo) == 24
    assert [f[0] for f in L.BcArgs._fields_] == ["scope", "flags", "directed", "seed_is_dense"]
    assert [f[0] for f in L.BcInfo._fields_] == ["sources", "reached_pairs", "max_depth", "rounds"]
    assert L.RESULT_BETWEENNESS == 8 and L.TUNE_BC_WAVE_ROW == 21
    assert "tgo_betweenness" in L.EXPORTS and "tgo_copy_betweenness" in L.EXPORTS


def test_header_shim_and_java_name_the_entry_points():
    hdr = _read("include", "titan_gpu_olap.h")
    assert re.search(r"int\s+tgo_betweenness\(tgo_ctx\*[^;]*const tgo_bc_args\*[^;]*const int64_t\*[^;]*int64_t[^;]*"
                     r"double\*[^;]*tgo_bc_info\*[^;]*\);", hdr)
    assert re.search(r"int\s+tgo_copy_betweenness\(tgo_ctx\*[^;]*double\*[^;]*\);", hdr)
    assert "typedef struct { int32_t scope; int32_t flags; int32_t directed; int32_t seed_is_dense; } tgo_bc_args;" in hdr
    assert "typedef struct { int64_t sources, reached_pairs; int32_t max_depth, rounds; } tgo_bc_info;" in hdr
    assert "TGO_RESULT_BETWEENNESS = 8" in hdr and "TGO_TUNE_BC_WAVE_ROW = 21" in hdr
    block = hdr[hdr.index("Betweenness centrality"):hdr.index("tgo_bc_args;")]
    assert "DIAGNOSTIC" in block and "not halved" in block and "not normalised" in block
    tune = hdr[hdr.index("TGO_TUNE_BC_WAVE_ROW (tgo_betweenness)"):hdr.index("enum { TGO_TUNE_MS_SPLIT")]
    assert "not bit for bit" in tune
    shim = _read("java", "jni", "titan_gpu_olap_jni.c")
    assert re.search(r"JNIEXPORT\s+jdoubleArray\s+JNICALL\s+JFN\(betweenness\)", shim) and "tgo_betweenness(" in shim
    java = os.path.join("java", "src", "main", "java", "com", "thinkaurelius", "titan", "graphdb", "olap")
    native = _read(java, "gpu", "TgoNative.java")
    assert re.search(r"public static native double\[\] betweenness\(long ctx, long\[\] seeds, boolean directed\);", native)
    assert "RESULT_BETWEENNESS = 8" in native
    comp = _read(java, "computer", "GpuGraphComputer.java")
    assert "BetweennessCentralityVertexProgram" in comp and "titan.betweenness.centrality" in comp


def test_program_builder_map_reduce_and_wiring():
    P = titan_amd.BetweennessCentralityVertexProgram
    assert P.CENTRALITY == "titan.betweenness.centrality" and P.compute_keys == (P.CENTRALITY,)
    assert P.scope_name == "bothE"
    sib = titan_amd.KCoreVertexProgram
    assert (P.preferred_result_graph, P.preferred_persist) == (sib.preferred_result_graph, sib.preferred_persist)
    p = P.build().create()
    assert p.seeds is None and p.directed is False
    p = P.build().seeds([24, 8, 8]).directed(True).create()
    assert p.seeds == [24, 8, 8] and p.directed is True
    assert cp.GpuGraphComputer._RESULT_KEYS[P] == (L.RESULT_BETWEENNESS, (P.CENTRALITY,))
    mr = titan_amd.BetweennessRankMapReduce(top=3)
    assert mr.memory_key == "betweennessRank"
    ids = np.array([40, 8, 16, 24, 32], np.int64)
    got = mr.emit(ids, {P.CENTRALITY: np.array([2.0, 5.0, 2.0, 7.5, 2.0])})
    assert [(kv.key, kv.value) for kv in got] == [(24, 7.5), (8, 5.0), (16, 2.0)]    # the tie goes to the smaller id
    assert titan_amd.BetweennessRankMapReduce.build().top(1).memoryKey("m").create().emit(ids, {}) == []
    assert len(titan_amd.BetweennessRankMapReduce(top=9).emit(ids, {P.CENTRALITY: np.zeros(5)})) == 5


# ----------------------------------------------------------------------------- the reference, closed forms
def test_path_star_and_cycles():
    bc, info = br.reference(*br.path(33))
    assert bc == [2 * i * (32 - i) for i in range(33)]
    assert info == {"sources": 33, "reached_pairs": 33 * 32, "max_depth": 32, "D": 32, "dmax": 2}
    bc, info = br.reference(*br.star(64))
    assert bc == [64 * 63] + [0] * 64 and info["dmax"] == 64 and info["D"] == 2
    bc, info = br.reference(*br.cycle(65))
    assert bc == [Fraction(64 * 62, 4)] * 65 and info["D"] == 32
    bc, info = br.reference(*br.cycle(64))
    assert bc == [Fraction(62 * 62, 4)] * 64 and info["D"] == 32


def test_cliques_bipartite_and_grid():
    assert br.reference(*br.clique(5))[0] == [0] * 5
    bc, info = br.reference(*br.clique(70))
    assert bc == [0] * 70 and info["dmax"] == 69 and info["D"] == 1
    bc, info = br.reference(*br.complete_bipartite(3, 70))
    assert bc == [Fraction(70 * 69, 3)] * 3 + [Fraction(3 * 2, 70)] * 70 and info["dmax"] == 70
    n, src, dst = br.grid(9, 9)
    bc, info = br.reference(n, src, dst)
    assert max(range(n), key=lambda v: bc[v]) == 40 and info["D"] == 16 and info["dmax"] == 4
    assert bc[0] == bc[8] == bc[72] == bc[80] and bc[1] == bc[9]
    # every shortest path between two vertices at distance d has d - 1 inner vertices
    dist = sum(abs(a % 9 - b % 9) + abs(a // 9 - b // 9) - 1 for a in range(n) for b in range(n) if a != b)
    assert sum(bc) == dist


def test_diamonds_projection_and_directed():
    n, src, dst = br.diamond_chain(40)
    bc, info = br.reference(n, src, dst, seeds=[0])
    assert info["max_depth"] == 80 and info["reached_pairs"] == n - 1 and info["sources"] == 1
    assert bc[3] == 3 * 39 and bc[1] == bc[2] == Fraction(1 + 3 * 39, 2) and bc[0] == 0 and bc[120] == 0
    br.as_floats(bc)                                     # every value is a double
    n, src, dst = br.projection_fixture()
    assert br.reference(n, src, dst)[0] == [1, 1, 1, 1, 0]
    assert br.reference(n, src, dst, directed=True)[0] == [1, Fraction(1, 2), Fraction(1, 2), 0, 0]
    bc, info = br.reference(*br.cycle(17), directed=True)
    assert bc == [120] * 17 and info["D"] == 16 and info["dmax"] == 1
    n, src, dst = br.two_components_and_isolated()
    bc, info = br.reference(n, src, dst)
    assert bc[14:] == [0, 0, 0] and info["sources"] == 17 and info["reached_pairs"] == 9 * 8 + 5 * 4
    assert info["max_depth"] == 8
    # a seed twice counts twice; the order of the seeds does not matter to the exact sum
    one = br.reference(n, src, dst, seeds=[3])[0]
    assert br.reference(n, src, dst, seeds=[3, 3])[0] == [2 * x for x in one]


def test_tolerance_and_comparison_helpers():
    info = {"D": 16, "dmax": 4}
    assert br.tolerance(info, 81) == Fraction(3 * 16 * 7 + 81, 1 << 52)
    exact = [Fraction(1, 3), Fraction(0), Fraction(5)]
    assert br.within([1 / 3, 0.0, 5.0], exact, br.tolerance(info, 1)) < 1e-15
    for bad in ([1 / 3, 1e-300, 5.0], [0.3333, 0.0, 5.0]):
        try:
            br.within(bad, exact, br.tolerance(info, 1))
        except AssertionError:
            continue
        raise AssertionError("within() accepted " + repr(bad))
    ids, s2, d2, new = br.relabel(*br.path(5))
    assert (np.diff(ids) > 0).all() and sorted(new.tolist()) == list(range(5)) and len(s2) == 4
