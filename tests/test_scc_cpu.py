"""CPU: the host-side surface of the native strongly-connected-components program — struct layouts
of the C-ABI mirror, the declarations in the header / JNI shim / TgoNative.java, the program
builder, the map-reduce — and the host reference the GPU tests compare with (scc_ref.py), checked
against closed forms, a reachability closure and, where it imports, scipy."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import titan_amd
from titan_amd import _lib as L
import scc_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


# ------------------------------------------------------------------ surfaces
def test_struct_sizes_and_constants():
    assert C.sizeof(L.SccArgs) == 8
    assert C.sizeof(L.SccInfo) == 32
    assert [f[0] for f in L.SccInfo._fields_] == ["components", "largest", "singletons", "rounds", "passes"]
    assert L.RESULT_SCC == 7
    assert (L.TUNE_SCC_WAVE_ROW, L.TUNE_SCC_TAIL, L.TUNE_SCC_TRIM, L.TUNE_SCC_PIVOT) == (17, 18, 19, 20)
    assert "tgo_scc" in L.EXPORTS and "tgo_copy_scc" in L.EXPORTS
    assert L.ABI_VERSION == 2


def test_header_shim_and_java_name_the_entry_points():
    hdr = _read("include", "titan_gpu_olap.h")
    assert re.search(r"int\s+tgo_scc\(tgo_ctx\*[^;]*const tgo_scc_args\*[^;]*int64_t\*[^;]*tgo_scc_info\*[^;]*\);", hdr)
    assert re.search(r"int\s+tgo_copy_scc\(tgo_ctx\*[^;]*int64_t\*[^;]*\);", hdr)
    assert re.search(r"typedef struct \{ int32_t scope; int32_t flags; \} tgo_scc_args;", hdr)
    assert re.search(r"typedef struct \{ int64_t components, largest, singletons;\s*int32_t rounds, passes; \} tgo_scc_info;", hdr)
    assert "TGO_RESULT_SCC = 7" in hdr and "#define TGO_ABI_VERSION 2" in hdr
    for name, value in (("WAVE_ROW", 17), ("TAIL", 18), ("TRIM", 19), ("PIVOT", 20)):
        assert re.search(rf"TGO_TUNE_SCC_{name} = {value}\b", hdr)
    # rounds and passes are diagnostics, and the header says so
    block = hdr[hdr.index("Strongly connected components"):hdr.index("tgo_scc_args;")]
    assert "rounds" in block and "passes" in block and "DIAGNOSTICS" in block and "may differ" in block
    shim = _read("java", "jni", "titan_gpu_olap_jni.c")
    assert re.search(r"JNIEXPORT\s+jlongArray\s+JNICALL\s+JFN\(scc\)", shim) and "tgo_scc(" in shim
    java = os.path.join("java", "src", "main", "java", "com", "thinkaurelius", "titan", "graphdb", "olap")
    native = _read(java, "gpu", "TgoNative.java")
    assert re.search(r"public static native long\[\] scc\(long ctx\);", native)
    assert re.search(r"RESULT_SCC = 7", native)
    comp = _read(java, "computer", "GpuGraphComputer.java")
    assert "StronglyConnectedComponentsVertexProgram" in comp and "TgoNative.scc(ctx)" in comp
    assert "titan.scc.component" in comp and "TgoNative.RESULT_SCC" in comp
    assert "scc.hip" in _read("titan_amd", "csrc", "Makefile")


def test_program_builder_and_attributes():
    P = titan_amd.StronglyConnectedComponentsVertexProgram
    p = P.build().create()
    assert isinstance(p, P)
    assert P.COMPONENT == "titan.scc.component"
    assert p.compute_keys == (P.COMPONENT,)
    assert p.scope_name == "bothE"
    sd = titan_amd.ShortestDistanceVertexProgram
    assert p.preferred_result_graph == sd.preferred_result_graph
    assert p.preferred_persist == sd.preferred_persist
    kind, names = titan_amd.GpuGraphComputer._RESULT_KEYS[P]
    assert kind == L.RESULT_SCC and names == (P.COMPONENT,)


def test_map_reduce_on_a_hand_written_vector():
    P = titan_amd.StronglyConnectedComponentsVertexProgram
    ids = np.array([8, 16, 24, 32, 40], np.int64)
    props = {P.COMPONENT: np.array([8, 8, 24, 8, 40], np.int64)}
    mr = titan_amd.SccSizeMapReduce.build().create()
    assert mr.memory_key == "sccSizes"
    sizes = mr.emit(ids, props)
    assert sizes == {8: 3, 24: 1, 40: 1}
    assert all(type(k) is int and type(v) is int for k, v in sizes.items())
    assert titan_amd.SccSizeMapReduce.build().memoryKey("s").create().memory_key == "s"
    assert mr.emit(ids, {}) == {}


def test_package_exports():
    for name in ("StronglyConnectedComponentsVertexProgram", "SccSizeMapReduce"):
        assert name in titan_amd.__all__ and hasattr(titan_amd, name)
    assert hasattr(titan_amd.Engine, "scc") and hasattr(titan_amd.Engine, "copy_scc")


# ------------------------------------------------------------------ the reference: closed forms
def test_cycles_paths_cliques_and_stars():
    for n, src, dst in (sr.cycle(7), sr.random_cycle(300), sr.bidirected_clique(9)):
        lab, info = sr.reference(n, src, dst)
        assert (lab == 0).all() and info == {"components": 1, "largest": n, "singletons": 0}
    for n, src, dst in (sr.random_dipath(300), sr.in_out_star(40)):
        lab, info = sr.reference(n, src, dst)
        assert np.array_equal(lab, np.arange(n)) and info == {"components": n, "largest": 1, "singletons": n}
    assert sr.in_out_star(40)[0] == 81


def test_bridge_and_chain():
    for forward in (True, False):
        n, src, dst = sr.two_cycles_bridge(4, 7, forward)
        lab, info = sr.reference(n, src, dst)
        assert lab.tolist() == [0] * 4 + [4] * 7 and info == {"components": 2, "largest": 7, "singletons": 0}
    want = None
    for asc in (True, False):
        n, src, dst = sr.cycle_chain(5, 3, asc)
        lab, info = sr.reference(n, src, dst)
        assert n == 15 and info == {"components": 5, "largest": 3, "singletons": 0}
        assert np.array_equal(lab, np.repeat(np.arange(0, 15, 3), 3))
        want = lab


def test_projection_rules_and_no_entries():
    e = np.array([(0, 1), (0, 1), (1, 0), (1, 2), (2, 2), (3, 3)])
    lab, info = sr.reference(5, e[:, 0], e[:, 1])
    assert lab.tolist() == [0, 0, 2, 3, 4] and info == {"components": 4, "largest": 2, "singletons": 3}
    none = np.zeros(0, np.int32)
    lab, info = sr.reference(130, none, none)
    assert np.array_equal(lab, np.arange(130)) and info == {"components": 130, "largest": 1, "singletons": 130}
    ids = np.array([80, 16, 24, 8, 40], np.int64)
    lab, _ = sr.reference(5, e[:, 0], e[:, 1], ids)
    assert lab.tolist() == [16, 16, 24, 8, 40]


def test_planted_equals_its_construction():
    n, src, dst, comp = sr.planted(range(1, 61), 3000, 3)
    assert n == 1830 and (src == dst).any()
    assert len(np.unique(src.astype(np.int64) * n + dst)) < len(src)
    lab, info = sr.reference(n, src, dst)
    want, winfo = sr.labels_of(comp)
    assert np.array_equal(lab, want) and info == winfo == {"components": 60, "largest": 60, "singletons": 1}
    assert sorted(np.unique(lab, return_counts=True)[1].tolist()) == list(range(1, 61))


# ------------------------------------------------------------------ the reference: a second method
@pytest.mark.parametrize("case", ["planted", "gnp", "bridge", "chain"])
def test_reference_equals_the_reachability_closure(case):
    if case == "planted":
        n, src, dst, _ = sr.planted([1, 1, 1, 2, 3, 5, 8, 13, 1, 21, 30], 150, 9)
    elif case == "gnp":
        n, src, dst = sr.gnp_digraph(200, 0.008, 4)
    elif case == "bridge":
        n, src, dst = sr.two_cycles_bridge(40, 70)
    else:
        n, src, dst = sr.cycle_chain(40, 3, False)
    assert n <= 200
    lab, info = sr.reference(n, src, dst)
    want, winfo = sr.labels_of(sr.closure_components(n, src, dst))
    assert np.array_equal(lab, want) and info == winfo


def test_reference_equals_scipy():
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components
    for n, src, dst in (sr.gnp_digraph(1001, 0.0012, 7), sr.gnp_digraph(1001, 0.002, 8),
                        sr.planted(range(1, 61), 3000, 3)[:3]):
        m = sp.csr_matrix((np.ones(len(src)), (src, dst)), shape=(n, n))
        k, comp = connected_components(m, directed=True, connection="strong")
        lab, info = sr.reference(n, src, dst)
        want, winfo = sr.labels_of(comp)
        assert info["components"] == k and np.array_equal(lab, want) and info == winfo
