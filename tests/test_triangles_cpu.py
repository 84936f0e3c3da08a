"""CPU: the host-side surface of the native triangle-counting program — struct layouts of the
C-ABI mirror, the declarations in the header / JNI shim / TgoNative.java, the program builder,
the two map-reduces on hand-written vectors, and the numpy reference the GPU tests compare with."""
import ctypes as C
import os
import re

import numpy as np

import titan_amd
from titan_amd import _lib as L
from triangles_ref import lcc_of, reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_struct_sizes_and_constants():
    assert C.sizeof(L.TriArgs) == 8
    assert C.sizeof(L.TriInfo) == 32
    assert [f[0] for f in L.TriInfo._fields_] == ["triangles", "wedges", "simple_edges", "max_forward"]
    assert L.RESULT_TRIANGLES == 5
    assert (L.TUNE_TRI_WAVE_ROW, L.TUNE_TRI_BLOCK_ROW) == (11, 12)
    assert "tgo_triangles" in L.EXPORTS and "tgo_copy_triangles" in L.EXPORTS


def test_header_shim_and_java_name_the_entry_points():
    hdr = _read("include", "titan_gpu_olap.h")
    assert re.search(r"int\s+tgo_triangles\(tgo_ctx\*[^;]*const tgo_tri_args\*[^;]*int64_t\*[^;]*tgo_tri_info\*[^;]*\);", hdr)
    assert re.search(r"int\s+tgo_copy_triangles\(tgo_ctx\*[^;]*int64_t\*[^;]*int64_t\*[^;]*double\*[^;]*\);", hdr)
    assert re.search(r"typedef struct \{ int32_t scope; int32_t flags; \} tgo_tri_args;", hdr)
    assert re.search(r"typedef struct \{ int64_t triangles, wedges, simple_edges, max_forward; \} tgo_tri_info;", hdr)
    assert "TGO_RESULT_TRIANGLES = 5" in hdr and "#define TGO_ABI_VERSION 2" in hdr
    assert "TGO_TUNE_TRI_WAVE_ROW = 11" in hdr and re.search(r"TGO_TUNE_TRI_BLOCK_ROW = 12", hdr)
    shim = _read("java", "jni", "titan_gpu_olap_jni.c")
    assert re.search(r"JNIEXPORT\s+jlongArray\s+JNICALL\s+JFN\(triangles\)", shim) and "tgo_triangles(" in shim
    java = os.path.join("java", "src", "main", "java", "com", "thinkaurelius", "titan", "graphdb", "olap")
    native = _read(java, "gpu", "TgoNative.java")
    assert re.search(r"public static native long\[\] triangles\(long ctx\);", native)
    assert re.search(r"RESULT_TRIANGLES = 5", native)
    comp = _read(java, "computer", "GpuGraphComputer.java")
    assert "TriangleCountVertexProgram" in comp and "TgoNative.triangles(ctx)" in comp
    assert "titan.triangleCount.triangles" in comp and "titan.triangleCount.clusteringCoefficient" in comp
    assert "tri.hip" in _read("titan_amd", "csrc", "Makefile")


def test_program_builder_and_attributes():
    P = titan_amd.TriangleCountVertexProgram
    p = P.build().create()
    assert isinstance(p, P)
    assert P.TRIANGLES == "titan.triangleCount.triangles"
    assert P.CLUSTERING == "titan.triangleCount.clusteringCoefficient"
    assert p.compute_keys == (P.TRIANGLES, P.CLUSTERING)        # the degree is not persisted
    assert P.DEGREE not in p.compute_keys
    assert p.scope_name == "bothE"
    sd = titan_amd.ShortestDistanceVertexProgram
    assert p.preferred_result_graph == sd.preferred_result_graph
    assert p.preferred_persist == sd.preferred_persist
    kind, names = titan_amd.GpuGraphComputer._RESULT_KEYS[P]
    assert kind == L.RESULT_TRIANGLES and names == (P.TRIANGLES, P.CLUSTERING)


def test_map_reduces_on_hand_written_vectors():
    P = titan_amd.TriangleCountVertexProgram
    ids = np.array([8, 16, 24, 32, 40], np.int64)
    # a triangle 0-1-2 with a tail 2-3 and an isolated vertex: wedges 1 + 1 + 3 + 0 + 0
    props = {P.TRIANGLES: np.array([1, 1, 1, 0, 0], np.int64), P.DEGREE: np.array([2, 2, 3, 1, 0], np.int64),
             P.CLUSTERING: np.array([1.0, 1.0, 1 / 3, 0.0, 0.0])}
    cnt = titan_amd.TriangleCountMapReduce.build().create()
    tr = titan_amd.TransitivityMapReduce.build().create()
    assert cnt.memory_key == "triangleCount" and tr.memory_key == "transitivity"
    assert cnt.emit(ids, props) == 1
    assert tr.emit(ids, props) == 3 * 1 / 5
    assert titan_amd.TriangleCountMapReduce.build().memoryKey("k").create().memory_key == "k"
    assert titan_amd.TransitivityMapReduce.build().memoryKey("t").create().memory_key == "t"
    assert cnt.emit(ids, {}) == 0 and tr.emit(ids, {}) == 0.0
    # no wedge: 0.0, not a division by zero
    assert tr.emit(ids[:2], {P.TRIANGLES: np.zeros(2, np.int64), P.DEGREE: np.ones(2, np.int64)}) == 0.0
    # K4: 4 triangles, 12 wedges
    k4 = {P.TRIANGLES: np.full(4, 3, np.int64), P.DEGREE: np.full(4, 3, np.int64)}
    assert cnt.emit(ids[:4], k4) == 4 and tr.emit(ids[:4], k4) == 1.0


def test_package_exports():
    for name in ("TriangleCountVertexProgram", "TriangleCountMapReduce", "TransitivityMapReduce"):
        assert name in titan_amd.__all__ and hasattr(titan_amd, name)
    assert hasattr(titan_amd.Engine, "triangles") and hasattr(titan_amd.Engine, "copy_triangles")


def test_numpy_reference_on_k4_and_the_projection_case():
    s, d = np.triu_indices(4, 1)
    tri, deg, lcc, info = reference(4, s, d)
    assert tri.tolist() == [3] * 4 and deg.tolist() == [3] * 4 and lcc.tolist() == [1.0] * 4
    assert info == {"triangles": 4, "wedges": 12, "simple_edges": 6}
    # duplicates, both directions of a pair, a self-loop and an isolated vertex
    e = np.array([(0, 1), (0, 1), (1, 0), (1, 2), (2, 0), (2, 2)])
    tri, deg, lcc, info = reference(4, e[:, 0], e[:, 1])
    assert tri.tolist() == [1, 1, 1, 0] and deg.tolist() == [2, 2, 2, 0] and lcc.tolist() == [1.0, 1.0, 1.0, 0.0]
    assert info == {"triangles": 1, "wedges": 3, "simple_edges": 3}
    assert lcc_of([2], [4]).tolist() == [4.0 / 12.0] and lcc_of([0, 0], [1, 0]).tolist() == [0.0, 0.0]
