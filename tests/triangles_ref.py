"""numpy restatement of tgo_triangles for the tests: the simple undirected projection of an edge
list as a dense boolean matrix.  Exact while every count stays below 2^53 (fp64 BLAS product of
0/1 matrices); keep n <= ~2100 so the product is cheap."""
import numpy as np


def lcc_of(tri, deg):
    """The contract's expression: one IEEE division of two integers below 2^53."""
    tri = np.asarray(tri, np.int64)
    deg = np.asarray(deg, np.int64)
    den = deg * (deg - 1)
    out = np.zeros(len(tri), np.float64)
    m = deg >= 2
    out[m] = (2 * tri[m]).astype(np.float64) / den[m].astype(np.float64)
    return out


def reference(n, src, dst):
    """(tri, deg, lcc, info) of the projection of the edges src[i] -> dst[i] over vertices 0..n-1:
    parallel edges, both directions of a pair and self-loops collapse."""
    a = np.zeros((n, n), bool)
    src = np.asarray(src, np.int64)
    dst = np.asarray(dst, np.int64)
    a[src, dst] = True
    a[dst, src] = True
    a[np.arange(n), np.arange(n)] = False
    f = a.astype(np.float64)
    tri2 = ((f @ f) * f).sum(1)                         # twice the pairs of neighbours that are adjacent
    tri = (tri2 / 2).astype(np.int64)
    assert np.array_equal(tri * 2, tri2.astype(np.int64))
    deg = a.sum(1).astype(np.int64)
    s = int(tri.sum())
    assert s % 3 == 0 and int(deg.sum()) % 2 == 0
    info = {"triangles": s // 3, "wedges": int((deg * (deg - 1) // 2).sum()), "simple_edges": int(deg.sum()) // 2}
    return tri, deg, lcc_of(tri, deg), info


def reference_from_lists(out, inn, perm):
    """The same from assembled device lists (Engine.graph_csr(0), graph_csr(1), graph_perm()):
    rows and entries in internal ids, results in row order."""
    n = len(perm)
    rows = np.concatenate([np.repeat(np.arange(n), np.diff(out["off"])), np.repeat(np.arange(n), np.diff(inn["off"]))])
    nbrs = np.concatenate([out["adj"], inn["adj"]]).astype(np.int64)
    tri, deg, lcc, info = reference(n, rows, nbrs)
    perm = np.asarray(perm, np.int64)
    return tri[perm], deg[perm], lcc[perm], info
