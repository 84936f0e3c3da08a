"""CPU: the host-side surface of the native k-truss program — struct layouts of the C-ABI mirror, the
entry points' null-ctx answers, the declarations in the header / JNI shim / TgoNative.java, the
program builder, the two map-reduces on hand-written vectors — and the host restatement the GPU
tests compare with, checked against the definitional fixed point and against closed forms."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import titan_amd
from titan_amd import _lib as L
import kcore_ref as kr
import truss_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def both(n, src, dst):
    """(vtruss, info, edges): the peel and the definitional fixed point agree on every edge."""
    vtruss, info, edges = tr.reference(n, src, dst)
    want = tr.definitional_fixed_point(n, src, dst)
    assert len(edges) == len(want)
    assert {(int(u), int(v)): int(t) for u, v, t, _ in edges} == want
    assert vtruss.dtype == np.int64 and len(vtruss) == n and edges.dtype == np.int64
    return vtruss, info, edges


# ------------------------------------------------------------------ the ABI without a device
def test_struct_sizes_and_constants():
    assert C.sizeof(L.TrussArgs) == 24
    assert C.sizeof(L.TrussInfo) == 40
    assert [f[0] for f in L.TrussArgs._fields_] == ["scope", "flags", "k", "wave_row", "block_row", "peel_wave_row"]
    assert [f[0] for f in L.TrussInfo._fields_] == ["max_truss", "innermost_edges", "triangles", "simple_edges",
                                                    "levels", "rounds"]
    assert L.RESULT_TRUSS == 11
    for name in ("tgo_ktruss", "tgo_copy_truss", "tgo_copy_truss_edges"):
        assert name in L.EXPORTS
    assert L.ABI_VERSION == 2


def test_null_ctx_is_invalid():
    lib = L.load()
    a = L.TrussArgs(L.SCOPE_BOTH_E, 0, 0, 0, 0, 0)
    info = L.TrussInfo()
    assert lib.tgo_ktruss(None, C.byref(a), None, C.byref(info)) == L.TGO_E_INVALID
    out = np.zeros(4, np.int64)
    assert lib.tgo_copy_truss(None, L.ptr(out, C.c_int64)) == L.TGO_E_INVALID
    assert lib.tgo_copy_truss_edges(None, None, None, None, None) == L.TGO_E_INVALID


def test_header_shim_and_java_name_the_entry_points():
    hdr = _read("include", "titan_gpu_olap.h")
    assert re.search(r"int\s+tgo_ktruss\(tgo_ctx\*[^;]*const tgo_truss_args\*[^;]*int64_t\*[^;]*tgo_truss_info\*[^;]*\);", hdr)
    assert re.search(r"int\s+tgo_copy_truss\(tgo_ctx\*[^;]*int64_t\*[^;]*\);", hdr)
    assert re.search(r"int\s+tgo_copy_truss_edges\(tgo_ctx\*[^;]*int64_t\*[^;]*int64_t\*[^;]*int64_t\*[^;]*int64_t\*[^;]*\);", hdr)
    assert re.search(r"typedef struct \{ int32_t scope; int32_t flags; int32_t k;\s*int32_t wave_row; int32_t block_row; "
                     r"int32_t peel_wave_row; \} tgo_truss_args;", hdr)
    assert re.search(r"typedef struct \{ int64_t max_truss, innermost_edges, triangles, simple_edges;\s*"
                     r"int32_t levels, rounds; \} tgo_truss_info;", hdr)
    assert "TGO_RESULT_TRUSS = 11" in hdr and "#define TGO_ABI_VERSION 2" in hdr
    # rounds is a diagnostic, and the header says so; the tuning keys did not grow
    block = hdr[hdr.index("k-truss decomposition"):hdr.index("tgo_truss_args;")]
    assert "rounds" in block and "DIAGNOSTIC" in block and "may differ" in block
    assert "TGO_TUNE_TRUSS" not in hdr
    shim = _read("java", "jni", "titan_gpu_olap_jni.c")
    assert re.search(r"JNIEXPORT\s+jlongArray\s+JNICALL\s+JFN\(ktruss\)", shim) and "tgo_ktruss(" in shim
    java = os.path.join("java", "src", "main", "java", "com", "thinkaurelius", "titan", "graphdb", "olap")
    native = _read(java, "gpu", "TgoNative.java")
    assert re.search(r"public static native long\[\] ktruss\(long ctx, int k\);", native)
    assert re.search(r"RESULT_TRUSS = 11", native)
    comp = _read(java, "computer", "GpuGraphComputer.java")
    assert "com.thinkaurelius.titan.olap.KTrussVertexProgram" in comp and "TgoNative.ktruss(ctx" in comp
    assert "titan.kTruss.trussNumber" in comp and "TgoNative.RESULT_TRUSS" in comp
    mk = _read("titan_amd", "csrc", "Makefile")
    assert "truss.hip" in mk and "api_truss.cpp" in mk


def test_program_builder_and_attributes():
    P = titan_amd.KTrussVertexProgram
    p = P.build().create()
    assert isinstance(p, P) and p.k == 0
    assert P.build().k(5).create().k == 5
    assert P.TRUSS == "titan.kTruss.trussNumber"
    assert p.compute_keys == (P.TRUSS,)
    assert p.scope_name == "bothE"
    sd = titan_amd.ShortestDistanceVertexProgram
    assert p.preferred_result_graph == sd.preferred_result_graph
    assert p.preferred_persist == sd.preferred_persist
    kind, names = titan_amd.GpuGraphComputer._RESULT_KEYS[P]
    assert kind == L.RESULT_TRUSS and names == (P.TRUSS,)
    assert titan_amd.GpuGraphComputer._RESULT_KEYS[titan_amd.KCoreVertexProgram][0] == L.RESULT_CORE


def test_map_reduces_on_hand_written_vectors():
    P = titan_amd.KTrussVertexProgram
    ids = np.array([8, 16, 24, 32, 40, 48], np.int64)
    # a triangle with a tail of two and an isolated vertex
    props = {P.TRUSS: np.array([3, 3, 3, 2, 2, 0], np.int64)}
    mt = titan_amd.MaxTrussMapReduce.build().create()
    ts = titan_amd.TrussSizeMapReduce.build().create()
    assert mt.memory_key == "maxTruss" and ts.memory_key == "trussSizes"
    assert mt.emit(ids, props) == 3 and type(mt.emit(ids, props)) is int
    sizes = ts.emit(ids, props)
    assert sizes == {0: 1, 2: 2, 3: 3}
    assert all(type(k) is int and type(v) is int for k, v in sizes.items())
    assert titan_amd.MaxTrussMapReduce.build().memoryKey("m").create().memory_key == "m"
    assert titan_amd.TrussSizeMapReduce.build().memoryKey("s").create().memory_key == "s"
    assert mt.emit(ids, {}) == 0 and ts.emit(ids, {}) == {}
    assert mt.emit(ids[:0], {P.TRUSS: np.zeros(0, np.int64)}) == 0


def test_package_exports():
    for name in ("KTrussVertexProgram", "MaxTrussMapReduce", "TrussSizeMapReduce"):
        assert name in titan_amd.__all__ and hasattr(titan_amd, name)
    for name in ("ktruss", "copy_truss", "copy_truss_edges"):
        assert hasattr(titan_amd.Engine, name)


# ------------------------------------------------------------------ the restatement
def test_gnp_300_equals_the_definition():
    n, src, dst, _ = kr.gnp(300, 0.08, 12)
    vtruss, info, edges = both(n, src, dst)
    assert info["simple_edges"] == len(edges) and info["max_truss"] >= 3
    assert info["triangles"] * 3 == int(edges[:, 3].sum())


def test_book_equals_the_definition_and_its_closed_form():
    m = 200
    n, src, dst = tr.book(m)
    vtruss, info, edges = both(n, src, dst)
    assert (edges[:, 2] == 3).all() and (vtruss == 3).all()
    assert edges[0].tolist() == [0, 1, 3, m] and (edges[1:, 3] == 1).all()     # the spine's support is m
    assert info == {"max_truss": 3, "innermost_edges": 2 * m + 1, "triangles": m, "simple_edges": 2 * m + 1, "levels": 1}


def test_clique_chain_equals_the_definition():
    n, src, dst, core = kr.clique_chain(2, 12)
    vtruss, info, edges = both(n, src, dst)
    # K_2 and every bridge: 2; K_j: j.  A vertex carries its clique's value.
    assert np.array_equal(vtruss, core + 1)
    assert info["max_truss"] == 12 and info["innermost_edges"] == 66 and info["levels"] == 11


def test_shared_edge_cliques_equal_the_definition():
    n, src, dst = tr.two_cliques_sharing_an_edge(5, 4)
    vtruss, info, edges = both(n, src, dst)
    assert n == 7 and info["simple_edges"] == 10 + 6 - 1
    by = {(int(u), int(v)): (int(t), int(s)) for u, v, t, s in edges}
    assert by[(3, 4)] == (5, 3 + 2)                     # the shared edge: K5's value, both cliques' triangles
    assert sorted(set(edges[:, 2].tolist())) == [4, 5] and info["innermost_edges"] == 10
    assert vtruss.tolist() == [5, 5, 5, 5, 5, 4, 4]


@pytest.mark.parametrize("k", [3, 4, 5, 70])
def test_cliques(k):
    n, src, dst = kr.clique(k)
    vtruss, info, edges = tr.reference(n, src, dst)
    assert (edges[:, 2] == k).all() and (edges[:, 3] == k - 2).all() and (vtruss == k).all()
    assert info == {"max_truss": k, "innermost_edges": k * (k - 1) // 2, "triangles": k * (k - 1) * (k - 2) // 6,
                    "simple_edges": k * (k - 1) // 2, "levels": 1}


def test_triangle_free_graphs_and_graphs_without_an_edge():
    n, src, dst = kr.star(64)
    vtruss, info, edges = both(n, src, dst)
    assert (edges[:, 2] == 2).all() and (edges[:, 3] == 0).all() and (vtruss == 2).all()
    assert info == {"max_truss": 2, "innermost_edges": 64, "triangles": 0, "simple_edges": 64, "levels": 1}
    ring = np.arange(10, dtype=np.int32)                # an even cycle
    _, info, edges = both(10, ring, np.roll(ring, -1))
    assert (edges[:, 2] == 2).all() and info["levels"] == 1
    none = np.zeros(0, np.int32)
    vtruss, info, edges = tr.reference(5, none, none)
    assert not vtruss.any() and edges.shape == (0, 4) and info == dict.fromkeys(tr.INFO, 0)


def test_projection_collapses_duplicates_directions_and_self_loops():
    e = np.array([(0, 1), (0, 1), (1, 0), (1, 2), (2, 0), (2, 2)], np.int32)
    vtruss, info, edges = both(4, e[:, 0], e[:, 1])
    assert vtruss.tolist() == [3, 3, 3, 0] and edges.tolist() == [[0, 1, 3, 1], [0, 2, 3, 1], [1, 2, 3, 1]]


def test_a_k_truss_is_a_k_minus_one_core():
    for n, src, dst in (kr.gnp(300, 0.08, 12)[:3], kr.clique_chain(2, 12)[:3], tr.book(50), kr.wheel(30),
                        tr.two_cliques_sharing_an_edge(6, 4)):
        vtruss = tr.reference(n, src, dst)[0]
        core = kr.reference(n, src, dst)[0]
        has = core > 0
        assert (vtruss[has] <= core[has] + 1).all() and (vtruss[has] >= 2).all() and not vtruss[~has].any()


def test_k_clamps_the_values_and_the_info():
    n, src, dst, _ = kr.clique_chain(2, 12)
    full = tr.reference(n, src, dst)
    for k in (2, 3, 7, 40):
        vtruss, info, edges = tr.reference(n, src, dst, k=k)
        assert np.array_equal(edges[:, 2], np.minimum(full[2][:, 2], k)) and np.array_equal(edges[:, 3], full[2][:, 3])
        assert np.array_equal(vtruss, np.minimum(full[0], k))
        assert info["max_truss"] == min(12, k) and info["levels"] == len(np.unique(edges[:, 2]))
        assert info["innermost_edges"] == int((full[2][:, 2] >= min(12, k)).sum())
        again = tr.clamp(full, k)
        assert np.array_equal(again[0], vtruss) and again[1] == info and np.array_equal(again[2], edges)


def test_reference_from_lists_renumbers_and_reorders():
    n, src, dst = tr.two_cliques_sharing_an_edge(5, 4)
    rng = np.random.default_rng(3)
    perm = rng.permutation(n)                           # row -> internal
    s, d = perm[src], perm[dst]
    order = np.argsort(s, kind="stable")
    out = {"off": np.concatenate([[0], np.cumsum(np.bincount(s, minlength=n))]), "adj": d[order].astype(np.int32)}
    order = np.argsort(d, kind="stable")
    inn = {"off": np.concatenate([[0], np.cumsum(np.bincount(d, minlength=n))]), "adj": s[order].astype(np.int32)}
    vtruss, info, edges = tr.reference_from_lists(out, inn, perm)
    want = tr.reference(n, src, dst)
    assert np.array_equal(vtruss, want[0]) and info == want[1] and np.array_equal(edges, want[2])
