"""Host restatements of tgo_ktruss for the tests, over the simple undirected projection of an edge
list (parallel edges, both directions of a pair and self-loops collapse).

Two independent ones: `reference` peels edges level by level over Python sets (an edge whose
remaining support is at most l gets truss l + 2 and takes its triangles with it);
`definitional_fixed_point` deletes, for k = 3, 4, ..., the edges in fewer than k - 2 remaining
triangles until nothing changes, which is the definition read aloud.  Both are exact integer
computations; the tests compare with array_equal.

info follows the C-ABI: max_truss = the largest reported value, innermost_edges = the edges at it,
triangles = sum(support) / 3, simple_edges, levels = distinct reported values.  With k >= 2 every
value is min(truss, k) and info is computed from the clamped values.  A projection without any edge
is not peeled: its info is all zero."""
import numpy as np

from kcore_ref import clique, clique_chain, gnp, projection, star, wheel  # noqa: F401  (the tests' graphs)

INFO = ("max_truss", "innermost_edges", "triangles", "simple_edges", "levels")


def neighbour_sets(n, src, dst):
    off, adj = projection(n, src, dst)
    offl, adjl = off.tolist(), adj.tolist()
    return [set(adjl[offl[v]:offl[v + 1]]) for v in range(n)]


def supports(nbr):
    """{(u, v): |N(u) ∩ N(v)|} over the edges u < v."""
    return {(u, v): len(nbr[u] & nbr[v]) for u in range(len(nbr)) for v in nbr[u] if u < v}


def peel(nbr):
    """({(u, v): truss}, {(u, v): support}); nbr is consumed."""
    sup0 = supports(nbr)
    sup = dict(sup0)
    truss = {}
    key = lambda a, b: (a, b) if a < b else (b, a)
    while sup:
        l = min(sup.values())
        stack = [e for e, s in sup.items() if s <= l]
        queued = set(stack)
        while stack:
            e = stack.pop()
            u, v = e
            for w in nbr[u] & nbr[v]:
                for t in (key(u, w), key(v, w)):
                    if t in queued:
                        continue
                    sup[t] -= 1
                    if sup[t] <= l:
                        queued.add(t)
                        stack.append(t)
            nbr[u].discard(v)
            nbr[v].discard(u)
            truss[e] = l + 2
            del sup[e]
    return truss, sup0


def definitional_fixed_point(n, src, dst):
    """{(u, v): truss} by the definition: the k-truss is what is left after deleting, again and
    again, every edge in fewer than k - 2 remaining triangles; an edge's value is the last k whose
    truss holds it."""
    nbr = neighbour_sets(n, src, dst)
    edges = {(u, v) for u in range(n) for v in nbr[u] if u < v}
    truss = {e: 2 for e in edges}
    k = 3
    while edges:
        while True:
            gone = [(u, v) for (u, v) in edges if len(nbr[u] & nbr[v]) < k - 2]
            if not gone:
                break
            for u, v in gone:
                nbr[u].discard(v)
                nbr[v].discard(u)
            edges.difference_update(gone)
        for e in edges:
            truss[e] = k
        k += 1
    return truss


def assemble(n, truss, sup0, k=0):
    """(vtruss, info, edges) from the per-edge dictionaries."""
    rows = np.array(sorted((u, v, truss[(u, v)], sup0[(u, v)]) for (u, v) in truss), np.int64).reshape(-1, 4)
    if k >= 2:
        rows[:, 2] = np.minimum(rows[:, 2], k)
    vtruss = np.zeros(n, np.int64)
    if len(rows) == 0:
        return vtruss, dict.fromkeys(INFO, 0), rows
    np.maximum.at(vtruss, rows[:, 0], rows[:, 2])
    np.maximum.at(vtruss, rows[:, 1], rows[:, 2])
    top = int(rows[:, 2].max())
    info = {"max_truss": top, "innermost_edges": int((rows[:, 2] == top).sum()), "triangles": int(rows[:, 3].sum()) // 3,
            "simple_edges": len(rows), "levels": len(np.unique(rows[:, 2]))}
    return vtruss, info, rows


def reference(n, src, dst, k=0):
    """(vtruss, info, edges) of the projection of the edges src[i] -> dst[i] over vertices 0..n-1;
    edges = the (u, v, truss, support) rows with u < v, sorted."""
    truss, sup0 = peel(neighbour_sets(n, src, dst))
    return assemble(n, truss, sup0, k)


def clamp(ref, k):
    """What reference(..., k=k) returns, from the full reference."""
    n = len(ref[0])
    rows = ref[2]
    return assemble(n, {(int(u), int(v)): int(t) for u, v, t, _ in rows}, {(int(u), int(v)): int(s) for u, v, _, s in rows}, k)


def edge_rows(u, v, truss, support):
    """Four edge columns as rows sorted by (u, v), each pair ordered."""
    u, v = np.asarray(u, np.int64), np.asarray(v, np.int64)
    rows = np.stack([np.minimum(u, v), np.maximum(u, v), np.asarray(truss, np.int64), np.asarray(support, np.int64)], 1)
    return rows[np.lexsort((rows[:, 1], rows[:, 0]))].reshape(-1, 4)


def with_ids(edges, ids):
    """The reference's rows with vertex i named ids[i], ordered and sorted again."""
    ids = np.asarray(ids, np.int64)
    return edge_rows(ids[edges[:, 0]], ids[edges[:, 1]], edges[:, 2], edges[:, 3])


def reference_from_lists(out, inn, perm, k=0):
    """The same from assembled device lists (Engine.graph_csr(0), graph_csr(1), graph_perm()): rows
    and entries in internal ids; vtruss in row order, the edges' endpoints as row indices."""
    n = len(perm)
    rows = np.concatenate([np.repeat(np.arange(n), np.diff(out["off"])), np.repeat(np.arange(n), np.diff(inn["off"]))])
    nbrs = np.concatenate([out["adj"], inn["adj"]]).astype(np.int64)
    vtruss, info, edges = reference(n, rows, nbrs, k)
    perm = np.asarray(perm, np.int64)
    row_of = np.empty(n, np.int64)
    row_of[perm] = np.arange(n)
    return vtruss[perm], info, with_ids(edges, row_of)


# ------------------------------------------------------------------ the tests' graphs: (n, src, dst)
def book(m):
    """m triangles sharing the spine edge {0, 1}: pages 2 .. m + 1."""
    page = np.arange(2, m + 2, dtype=np.int32)
    src = np.concatenate([np.zeros(1, np.int32), np.zeros(m, np.int32), np.ones(m, np.int32)])
    dst = np.concatenate([np.ones(1, np.int32), page, page])
    return m + 2, src, dst


def two_cliques_sharing_an_edge(a, b):
    """K_a and K_b with exactly two vertices (one edge) in common."""
    _, s1, d1 = clique(a)
    _, s2, d2 = clique(b, base=a - 2)
    return a + b - 2, np.concatenate([s1, s2]), np.concatenate([d1, d2])
