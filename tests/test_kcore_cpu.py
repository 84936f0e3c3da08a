"""CPU: the host-side surface of the native k-core program — struct layouts of the C-ABI mirror,
the declarations in the header / JNI shim / TgoNative.java, the program builder, the two
map-reduces on hand-written vectors — and the two host restatements the GPU tests compare with,
checked against closed forms and against each other."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import titan_amd
from titan_amd import _lib as L
import kcore_ref as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def both(n, src, dst):
    """(core, info, sweeps): the peel and the H-index fixed point agree."""
    core, info = kr.reference(n, src, dst)
    off, adj = kr.projection(n, src, dst)
    h, sweeps = kr.hindex_fixed_point(off, adj)
    assert np.array_equal(core, h)
    assert core.dtype == np.int64 and len(core) == n
    return core, info, sweeps


def test_struct_sizes_and_constants():
    assert C.sizeof(L.CoreArgs) == 8
    assert C.sizeof(L.CoreInfo) == 32
    assert [f[0] for f in L.CoreInfo._fields_] == ["degeneracy", "innermost", "simple_edges", "levels", "rounds"]
    assert L.RESULT_CORE == 6
    assert (L.TUNE_CORE_WAVE_ROW, L.TUNE_CORE_TAIL) == (14, 15)
    assert L.TUNE_CORE_LDS_QUEUE == 16
    assert "tgo_kcore" in L.EXPORTS and "tgo_copy_cores" in L.EXPORTS
    assert L.ABI_VERSION == 2


def test_header_shim_and_java_name_the_entry_points():
    hdr = _read("include", "titan_gpu_olap.h")
    assert re.search(r"int\s+tgo_kcore\(tgo_ctx\*[^;]*const tgo_core_args\*[^;]*int64_t\*[^;]*tgo_core_info\*[^;]*\);", hdr)
    assert re.search(r"int\s+tgo_copy_cores\(tgo_ctx\*[^;]*int64_t\*[^;]*\);", hdr)
    assert re.search(r"typedef struct \{ int32_t scope; int32_t flags; \} tgo_core_args;", hdr)
    assert re.search(r"typedef struct \{ int64_t degeneracy, innermost, simple_edges;\s*int32_t levels, rounds; \} tgo_core_info;", hdr)
    assert "TGO_RESULT_CORE = 6" in hdr and "#define TGO_ABI_VERSION 2" in hdr
    assert "TGO_TUNE_CORE_WAVE_ROW = 14" in hdr and re.search(r"TGO_TUNE_CORE_TAIL = 15", hdr)
    assert "TGO_TUNE_CORE_LDS_QUEUE = 16" in hdr
    # rounds is a diagnostic, and the header says so
    block = hdr[hdr.index("k-core decomposition"):hdr.index("tgo_core_args;")]
    assert "rounds" in block and "DIAGNOSTIC" in block and "may differ" in block
    shim = _read("java", "jni", "titan_gpu_olap_jni.c")
    assert re.search(r"JNIEXPORT\s+jlongArray\s+JNICALL\s+JFN\(kcore\)", shim) and "tgo_kcore(" in shim
    java = os.path.join("java", "src", "main", "java", "com", "thinkaurelius", "titan", "graphdb", "olap")
    native = _read(java, "gpu", "TgoNative.java")
    assert re.search(r"public static native long\[\] kcore\(long ctx\);", native)
    assert re.search(r"RESULT_CORE = 6", native)
    comp = _read(java, "computer", "GpuGraphComputer.java")
    assert "KCoreVertexProgram" in comp and "TgoNative.kcore(ctx)" in comp
    assert "titan.kCore.coreNumber" in comp and "TgoNative.RESULT_CORE" in comp
    assert "core.hip" in _read("titan_amd", "csrc", "Makefile")


def test_program_builder_and_attributes():
    P = titan_amd.KCoreVertexProgram
    p = P.build().create()
    assert isinstance(p, P)
    assert P.CORE == "titan.kCore.coreNumber"
    assert p.compute_keys == (P.CORE,)
    assert p.scope_name == "bothE"
    sd = titan_amd.ShortestDistanceVertexProgram
    assert p.preferred_result_graph == sd.preferred_result_graph
    assert p.preferred_persist == sd.preferred_persist
    kind, names = titan_amd.GpuGraphComputer._RESULT_KEYS[P]
    assert kind == L.RESULT_CORE and names == (P.CORE,)


def test_map_reduces_on_hand_written_vectors():
    P = titan_amd.KCoreVertexProgram
    ids = np.array([8, 16, 24, 32, 40, 48], np.int64)
    # a triangle with a tail of two and an isolated vertex
    props = {P.CORE: np.array([2, 2, 2, 1, 1, 0], np.int64)}
    dg = titan_amd.DegeneracyMapReduce.build().create()
    cs = titan_amd.CoreSizeMapReduce.build().create()
    assert dg.memory_key == "degeneracy" and cs.memory_key == "coreSizes"
    assert dg.emit(ids, props) == 2 and type(dg.emit(ids, props)) is int
    sizes = cs.emit(ids, props)
    assert sizes == {0: 1, 1: 2, 2: 3}
    assert all(type(k) is int and type(v) is int for k, v in sizes.items())
    assert titan_amd.DegeneracyMapReduce.build().memoryKey("d").create().memory_key == "d"
    assert titan_amd.CoreSizeMapReduce.build().memoryKey("s").create().memory_key == "s"
    assert dg.emit(ids, {}) == 0 and cs.emit(ids, {}) == {}
    assert dg.emit(ids[:0], {P.CORE: np.zeros(0, np.int64)}) == 0


def test_package_exports():
    for name in ("KCoreVertexProgram", "DegeneracyMapReduce", "CoreSizeMapReduce"):
        assert name in titan_amd.__all__ and hasattr(titan_amd, name)
    assert hasattr(titan_amd.Engine, "kcore") and hasattr(titan_amd.Engine, "copy_cores")


# ------------------------------------------------------------------ the restatements
@pytest.mark.parametrize("k", [4, 5, 70])
def test_cliques(k):
    core, info, _ = both(*kr.clique(k))
    assert (core == k - 1).all()
    assert info == {"degeneracy": k - 1, "innermost": k, "simple_edges": k * (k - 1) // 2, "levels": 1}


def test_wheel_star_path_and_empty_graphs():
    core, info, _ = both(*kr.wheel(1500))
    assert (core == 3).all() and info == {"degeneracy": 3, "innermost": 1501, "simple_edges": 3000, "levels": 1}
    core, info, _ = both(*kr.star(64))
    assert len(core) == 65 and (core == 1).all()
    assert info == {"degeneracy": 1, "innermost": 65, "simple_edges": 64, "levels": 1}
    n, src, dst = kr.random_path(4097)
    core, info = kr.reference(n, src, dst)              # (the fixed point needs ~2048 sweeps here: the peel alone)
    assert (core == 1).all() and info == {"degeneracy": 1, "innermost": n, "simple_edges": n - 1, "levels": 1}
    n, src, dst = kr.random_path(129)
    assert (both(n, src, dst)[0] == 1).all()
    for n in (1, 130):
        core, info, sweeps = both(n, np.zeros(0, np.int32), np.zeros(0, np.int32))
        assert not core.any() and len(core) == n and sweeps == 1
        assert info == {"degeneracy": 0, "innermost": 0, "simple_edges": 0, "levels": 0}


def test_clique_chain():
    n, src, dst, want = kr.clique_chain(2, 40)
    assert n == 819
    core, info, _ = both(n, src, dst)
    assert np.array_equal(core, want)
    assert info["levels"] == 39 and info["degeneracy"] == 39 and info["innermost"] == 40
    assert info["simple_edges"] == sum(j * (j - 1) // 2 for j in range(2, 41)) + 38


def test_clique_beside_a_star_has_two_levels():
    _, s1, d1 = kr.clique(70)
    _, s2, d2 = kr.star(64, base=70)
    core, info, _ = both(135, np.concatenate([s1, s2]), np.concatenate([d1, d2]))
    assert (core[:70] == 69).all() and (core[70:] == 1).all()
    assert info == {"degeneracy": 69, "innermost": 70, "simple_edges": 70 * 69 // 2 + 64, "levels": 2}


def test_projection_case():
    e = np.array([(0, 1), (0, 1), (1, 0), (1, 2), (2, 0), (2, 2)])
    core, info, _ = both(4, e[:, 0], e[:, 1])            # vertex 3 is isolated
    assert core.tolist() == [2, 2, 2, 0]
    assert info == {"degeneracy": 2, "innermost": 3, "simple_edges": 3, "levels": 2}
    # what a peel over the raw entries would start from: 0 has four raw entries, two neighbours
    off, adj = kr.projection(4, e[:, 0], e[:, 1])
    assert np.diff(off).tolist() == [2, 2, 2, 0] and adj.tolist() == [1, 2, 0, 2, 0, 1]


def test_the_two_restatements_agree_on_gnp():
    n, src, dst, _ = kr.gnp(1001, 0.05, 12)
    core, info, sweeps = both(n, src, dst)
    assert info["degeneracy"] == core.max() and info["levels"] == len(np.unique(core)) and sweeps >= 2
    # k-core property, checked directly: inside {core >= k} every vertex keeps at least k neighbours,
    # for the innermost core and one in the middle
    off, adj = kr.projection(n, src, dst)
    rows = np.repeat(np.arange(n), np.diff(off))
    for k in (int(core.max()), int(np.median(core))):
        inside = core >= k
        d = np.bincount(rows[inside[rows] & inside[adj]], minlength=n)
        assert (d[inside] >= k).all()


def test_reference_from_lists_takes_internal_ids():
    # a triangle 0-1-2 with a tail 2-3, the lists in internal ids under the permutation row -> internal
    perm = np.array([2, 0, 3, 1])
    e = [(0, 1), (1, 2), (2, 0), (2, 3)]
    src = np.array([perm[a] for a, _ in e])
    dst = np.array([perm[b] for _, b in e])

    def csr(rows, cols):
        o = np.argsort(rows, kind="stable")
        off = np.zeros(5, np.int64)
        np.add.at(off, rows + 1, 1)
        return {"off": np.cumsum(off), "adj": cols[o].astype(np.int32)}

    core, info = kr.reference_from_lists(csr(src, dst), csr(dst, src), perm)
    assert core.tolist() == [2, 2, 2, 1] and info["levels"] == 2 and info["simple_edges"] == 4
