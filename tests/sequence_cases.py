"""Call sequences on one context: the graph, the named calls with their references, and the walk.

A tgo_ctx carries one Scratch that every program reinterprets for itself, and the drivers keep lazy
invariants from one call to the next (planes "still zero", counters "zero again afterwards", a cached
light / heavy split, cached forward lists).  A program can therefore be wrong only when it follows some
other program.  DESIGN.md states that every program is bit-identical from run to run, so "B after A"
has an exact expected value: B's reference, and bit for bit what B gives on a fresh context.

Pure numpy, the oracle and the per-program reference helpers: no device here.  test_sequence_cpu.py
checks this module; test_gpu_sequence.py drives an Engine with it.

The graph.  sequence_graph(n, seed) is ragged.ragged_graph(n, seed) (zero weights, isolated vertices,
self-loops, duplicates, the degree ladder) with 28 more vertices at the dense indices n..n+27:
  * a bidirected path of 20 vertices hanging off info["hub"]: a sweep from its far end runs >= 20
    levels, so it writes level planes 0..4 of the multi-source sweep;
  * two disjoint directed cycles of 3 and 5 vertices that nothing else touches: extra weak and strong
    components.
The Titan ids stay strictly increasing multiples of 8 and the new weights are drawn like the old ones.

The calls.  calls(scope) is the ordered list of the named calls of a bothE (2) or an inE (1) load.  A
Call runs on (engine, Case) and returns (values, same): `values` is compared with Call.ref(case) by
Call.check, and values and same together must equal, bit for bit, the same call on a fresh context
(assert_same).  `same` holds what is deterministic but what no reference restates (the level count of
a sweep).  What is documented to vary from run to run is in neither: the phase count of DELTA mode
(test_gpu_program_stats.py), the `rounds` / `passes` diagnostics of the analytics.  tgo_stats.iterations
is compared wherever test_gpu_program_stats.py compares it.

Two calls of each scope fail: the integer division by a zero weight of
test_integer_division_by_zero_fails_the_program (TGO_E_PROGRAM, raised by a kernel mid-run through
Counters::err), and a call whose opening check refuses the load's scope (TGO_E_INVALID).  On the bothE
load the latter is walkcount(3): DegreeCounter runs on inE loads only, so on a bothE load that call IS
the wrong-scope call; on the inE load it is components().  The directed betweenness call sums over 8
seeds like the undirected one (another draw): the exact-arithmetic reference over every vertex of the
n = 1001 graph would take minutes.  pagerank(.., 0) sets no PAGE_RANK property: its result is NaN at
every vertex by contract, the one reference that cannot vary over the vertices (constant_by_contract).

The walk.  pair_walk(k) is an Eulerian circuit of the complete digraph on k nodes with self-loops:
k * k + 1 node indices in which every ordered pair (A, B), A = B included, is adjacent exactly once.
"""
import numpy as np

import bc_ref
import cl_ref
import fulgora as fr
import kcore_ref
import pp_ref
import scc_ref
import triangles_ref
import truss_ref
from ragged import draw_seeds, ragged_graph
from titan_amd import _lib as L

OUT, IN, BOTH = L.SCOPE_OUT_E, L.SCOPE_IN_E, L.SCOPE_BOTH_E
SEED = 7
PATH_LEN = 20
CYCLES = (3, 5)
EXTRA = PATH_LEN + sum(CYCLES)
HOP_DEPTH = 25                  # past the path into the base graph, short of convergence
PR_L1_TOL = 1e-6                # BASELINE.json north_star, as in test_gpu_ragged.py
VALUE_KEY = (7700 << 6) | 5     # a user property key id for the generic result rows
RELATION_BASE = 1 << 40
SCOPE_NAMES = {BOTH: "bothE", IN: "inE"}


# ----------------------------------------------------------------------------- the graph
def sequence_graph(n, seed=SEED):
    """(N, src, dst, w, ids, info): ragged_graph(n, seed) plus the path and the two cycles, N = n + 28.
    info gains n_base, path (dense indices, nearest the hub first), path_end and cycles."""
    src, dst, w, ids, info = ragged_graph(n, seed)
    rng = np.random.default_rng([n, seed, 1])
    path = n + np.arange(PATH_LEN, dtype=np.int64)
    first = n + PATH_LEN
    cycles = []
    for c in CYCLES:
        cycles.append(first + np.arange(c, dtype=np.int64))
        first += c
    chain = np.concatenate([[info["hub"]], path])
    add_src = np.concatenate([chain[:-1], chain[1:]] + cycles)
    add_dst = np.concatenate([chain[1:], chain[:-1]] + [np.roll(c, -1) for c in cycles])
    add_w = rng.integers(0, 41, len(add_src))
    add_ids = ids[-1] + 8 * np.cumsum(rng.integers(1, 5, EXTRA))
    info = dict(info, n_base=n, path=path, path_end=int(path[-1]), cycles=cycles)
    return (n + EXTRA, np.concatenate([src, add_src]).astype(np.int32), np.concatenate([dst, add_dst]).astype(np.int32),
            np.concatenate([w, add_w]).astype(np.int32), np.concatenate([ids, add_ids]).astype(np.int64), info)


def marks_of(info, seed=SEED):
    """The vertices the calls name, as dense indices: ints, or int64 arrays for seed lists."""
    n = info["n_base"]
    end, hub = info["path_end"], info["hub"]
    rng = np.random.default_rng([n, seed, 2])
    mid = int(info["path"][PATH_LEN // 2])
    pick = rng.choice(info["base"], 12, replace=False).astype(np.int64)
    return {"path_end": end, "hub": hub, "isolated": int(info["isolated"][0]),
            "seeds64": draw_seeds(n, info, 64, seed),
            "seeds3": np.array([end, hub, int(info["cycles"][1][0])], np.int64),
            "bc_und": np.concatenate([[end, mid], pick[:6]]).astype(np.int64),
            "bc_dir": np.concatenate([[hub, int(info["cycles"][1][2])], pick[6:]]).astype(np.int64)}


class Case:
    """One graph in one row order with the oracle loaded from it, and the references of the calls,
    each computed once and never written to."""

    def __init__(self, N, src, dst, w, ids, marks, oracle=None):
        self.N = int(N)
        self.src, self.dst, self.w = (np.ascontiguousarray(a, np.int32) for a in (src, dst, w))
        self.ids = np.ascontiguousarray(ids, np.int64)
        self.marks = marks
        self.oracle = oracle if oracle is not None else fr.OracleGraph.from_edges(self.N, src, dst, w, titan_ids=ids)
        self._ref = {}
        self._sd = {}
        self._rows = {}

    @classmethod
    def make(cls, n, seed=SEED):
        N, src, dst, w, ids, info = sequence_graph(n, seed)
        return cls(N, src, dst, w, ids, marks_of(info, seed))

    def reordered(self, new_of_old, ids, oracle=None):
        """The same graph with vertex v at row new_of_old[v], rows named ids[row]."""
        p = np.asarray(new_of_old, np.int64)
        marks = {k: (int(p[v]) if np.isscalar(v) or isinstance(v, int) else p[np.asarray(v, np.int64)])
                 for k, v in self.marks.items()}
        return Case(self.N, p[self.src], p[self.dst], self.w, ids, marks, oracle)

    def sd(self, v, depth, scope, weighted=False):
        key = (int(v), int(depth), scope, weighted)
        if key not in self._sd:
            d = self.oracle.shortest_distance(int(self.ids[v]), int(depth), scope, weighted=weighted)[0]
            d.setflags(write=False)
            self._sd[key] = d
        return self._sd[key]

    def ref(self, call):
        key = (call.scope, call.name)
        if key not in self._ref:
            want = call.ref(self)
            for a in want.values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            self._ref[key] = want
        return self._ref[key]

    def csr(self):
        """(out_off, out_idx, out_w, in_off, in_idx, in_w) of the edge list, entries in edge order."""
        src, dst = self.src.astype(np.int64), self.dst.astype(np.int64)
        oo, io = np.argsort(src, kind="stable"), np.argsort(dst, kind="stable")
        out_off = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=self.N))]).astype(np.int64)
        in_off = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=self.N))]).astype(np.int64)
        return out_off, dst[oo], self.w[oo], in_off, src[io], self.w[io]

    def rows(self, other_ids=False):
        """(rows, vids, schema dict, weight key): edgestore rows of the graph built by edgestore.build_rows,
        the weight an Integer property in the label's signature; vertex i is named vids[i].  other_ids: the
        same vertices under other Titan ids that sort differently (so the rows come in another order)."""
        import edgestore as es
        if other_ids not in self._rows:
            label = es.user_edge_label(1)
            wkey = (1 << 6) | 5
            sd = {"edge_types": [{"type_id": label, "multiplicity": 0, "signature": [wkey]}], "property_keys": [[wkey, 3]]}
            spec = es.GraphSpec(n=self.N, edges=[(int(a), int(b), label, [(wkey, int(x))])
                                                 for a, b, x in zip(self.src, self.dst, self.w)])
            if other_ids:
                p = np.random.default_rng([self.N, 6]).permutation(self.N)
                spec.vids = [es.vertex_id(int(i) + 1000) for i in p]
            rows, vids = es.build_rows(spec, fr.OracleSchema(sd["edge_types"], [(wkey, 3)]))
            self._rows[other_ids] = rows, vids, sd, wkey
        return self._rows[other_ids]


def reached(d):
    return int((d != L.DIST_ABSENT).sum())


# ----------------------------------------------------------------------------- comparisons
def _bits_equal(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        a, b = np.asarray(a), np.asarray(b)
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    return bool(a == b)


def check_exact(got, want):
    """Every entry of the reference, bit for bit (fp64 arrays too: the closeness module's comparison, one
    IEEE division for the clustering coefficients, send order for the combiners)."""
    for k, x in want.items():
        assert k in got, k
        assert _bits_equal(got[k], x), (k, got[k], x)


def check_pagerank(got, want):
    """test_gpu_ragged.py's comparison: equal finite masks, L1 over the finite entries within 1e-6."""
    pr, opr = got["pr"], want["pr"]
    fin = np.isfinite(opr)
    assert pr.dtype == np.float64 and np.array_equal(np.isfinite(pr), fin)
    l1 = float(np.abs(pr[fin] - opr[fin]).sum())
    assert l1 <= PR_L1_TOL, l1
    check_exact(got, {k: v for k, v in want.items() if k != "pr"})


def check_betweenness(got, want):
    """test_gpu_betweenness.py's comparison: bc_ref.tolerance from the reference's own D and dmax and the
    number of seeds; an exact zero must be 0.0."""
    bc_ref.within(got["bc"], want["exact"], bc_ref.tolerance(want["bound"], want["nseeds"]))
    check_exact(got, {k: v for k, v in want.items() if k not in ("exact", "bound", "nseeds")})


def assert_same(got, fresh):
    """(values, same) of a call against the same call on a fresh context: the documented determinism."""
    for part_got, part_fresh in zip(got, fresh):
        assert sorted(part_got) == sorted(part_fresh)
        for k in part_fresh:
            assert _bits_equal(part_got[k], part_fresh[k]), (k, part_got[k], part_fresh[k])


def varies(want):
    """Whether some array of a reference differs between two vertices."""
    return any(isinstance(a, np.ndarray) and a.size > 1 and len(np.unique(a.view(np.int64) if a.dtype == np.float64
                                                                          else a)) > 1 for a in want.values())


# ----------------------------------------------------------------------------- the calls
class Call:
    def __init__(self, scope, name, run, ref=None, check=check_exact, fails=None, constant_by_contract=False):
        self.scope, self.name, self.run, self.ref, self.check = scope, name, run, ref, check
        self.fails = fails                            # the TitanException code of a failing call
        self.constant_by_contract = constant_by_contract

    def __repr__(self):
        return f"{SCOPE_NAMES[self.scope]}:{self.name}"


def _seed(g, mark, by_id):
    v = g.marks[mark]
    return int(g.ids[v]) if by_id else int(v)


def _bfs(scope, mark, by_id):
    def run(eng, g):
        d = eng.bfs(_seed(g, mark, by_id), g.N, scope, seed_is_dense=not by_id, stats=True)
        st = eng.stats()
        return {"dist": d, "reached": int(st["reached"]), "iterations": int(st["iterations"])}, {"levels": int(st["levels"])}

    def ref(g):
        d = g.sd(g.marks[mark], g.N, scope)
        return {"dist": d.copy(), "reached": reached(d), "iterations": g.N}
    return run, ref


def _bfs_multi(scope, mark, by_id):
    def run(eng, g):
        v = g.marks[mark]
        d = eng.bfs_multi(g.ids[v] if by_id else v, g.N, scope, seed_is_dense=not by_id, stats=True)
        r, _ = eng.multi_stats(len(v))
        st = eng.stats()
        return {"dist": d, "reached": r, "iterations": int(st["iterations"])}, {"levels": int(st["levels"])}

    def ref(g):
        d = np.stack([g.sd(int(v), g.N, scope) for v in g.marks[mark]])
        return {"dist": d, "reached": np.array([reached(x) for x in d], np.int64), "iterations": g.N}
    return run, ref


def _sssp(scope, mark, by_id, mode, delta, depth):
    def run(eng, g):
        d = eng.sssp(_seed(g, mark, by_id), depth or g.N, scope, mode=mode, seed_is_dense=not by_id, stats=True,
                     delta=delta)
        st = eng.stats()
        same = {} if mode == L.SSSP_DELTA else {"levels": int(st["levels"])}      # DELTA's phase count varies
        return {"dist": d, "reached": int(st["reached"]), "iterations": int(st["iterations"])}, same

    def ref(g):
        d = g.sd(g.marks[mark], depth or g.N, scope, weighted=True)
        return {"dist": d.copy(), "reached": reached(d), "iterations": depth or g.N}
    return run, ref


def _pagerank(iters):
    def run(eng, g):
        pr = eng.pagerank(0.85, g.N, iters)
        return {"pr": pr, "iterations": int(eng.stats()["iterations"]), "exact_reruns": int(eng.stats()["exact_reruns"])}, {}

    def ref(g):
        return {"pr": g.oracle.pagerank(0.85, g.N, iters)[0], "iterations": iters, "exact_reruns": 0}
    return run, ref


def _walkcount(k):
    def run(eng, g):
        return {"count": eng.walkcount(k), "iterations": int(eng.stats()["iterations"])}, {}

    def ref(g):
        return {"count": g.oracle.degree_counter(k)[0], "iterations": k}
    return run, ref


def _components():
    def run(eng, g):
        lab, info = eng.components()
        assert eng.stats()["iterations"] == info["rounds"]
        return {"label": lab, "components": info["components"]}, {"path": info["path"]}

    def ref(g):
        """MIN label propagation over bothE through the oracle's gather until nothing changes."""
        lab = g.ids.copy()
        every = np.ones(g.N, bool)
        while True:
            got, has = g.oracle.gather(BOTH, L.VAL_INT64, L.COMBINE_MIN, L.EDGE_IDENTITY, lab, every)
            new = np.where(has, np.minimum(lab, got), lab)
            if np.array_equal(new, lab):
                return {"label": lab, "components": int(len(np.unique(lab)))}
            lab = new
    return run, ref


def _triangles():
    def run(eng, g):
        tri, info = eng.triangles()
        ctri, deg, lcc = eng.copy_triangles()
        assert np.array_equal(ctri, tri)
        return ({"tri": tri, "deg": deg, "lcc": lcc, "iterations": int(eng.stats()["iterations"]),
                 **{k: info[k] for k in ("triangles", "wedges", "simple_edges")}}, {"max_forward": info["max_forward"]})

    def ref(g):
        tri, deg, lcc, info = triangles_ref.reference(g.N, g.src, g.dst)
        return {"tri": tri, "deg": deg, "lcc": lcc, "iterations": 1, **info}
    return run, ref


def _kcore():
    def run(eng, g):
        core, info = eng.kcore()
        return ({"core": core, "iterations": int(eng.stats()["iterations"]),
                 **{k: info[k] for k in ("degeneracy", "innermost", "simple_edges", "levels")}}, {})

    def ref(g):
        core, info = kcore_ref.reference(g.N, g.src, g.dst)
        return {"core": np.asarray(core, np.int64), "iterations": info["levels"], **info}
    return run, ref


def _ktruss(k):
    def run(eng, g):
        vt, info = eng.ktruss(k=k)
        edges = truss_ref.edge_rows(*eng.copy_truss_edges())
        return ({"vtruss": vt, "edges": edges, "iterations": int(eng.stats()["iterations"]),
                 **{key: info[key] for key in truss_ref.INFO}}, {})

    def ref(g):
        full = g.ref(ALL[(BOTH, "ktruss0")]) if k else None
        if full is None:
            vt, info, edges = truss_ref.reference(g.N, g.src, g.dst)
            raw = edges
        else:
            vt, info, raw = truss_ref.clamp((full["vtruss"], None, full["raw"]), k)
        return {"vtruss": vt, "edges": truss_ref.with_ids(raw, g.ids), "raw": raw, "iterations": info["levels"], **info}
    return run, ref


def check_truss(got, want):
    check_exact(got, {k: v for k, v in want.items() if k != "raw"})


def _scc():
    def run(eng, g):
        lab, info = eng.scc()
        return {"label": lab, **{k: info[k] for k in ("components", "largest", "singletons")}}, {}

    def ref(g):
        lab, info = scc_ref.reference(g.N, g.src, g.dst, g.ids)
        return {"label": lab, **info}
    return run, ref


def _betweenness(mark, directed):
    keys = ("sources", "reached_pairs", "max_depth")

    def run(eng, g):
        bc, info = eng.betweenness(g.ids[g.marks[mark]], directed=directed)
        st = eng.stats()
        assert st["iterations"] == info["sources"] and st["levels"] == info["max_depth"]
        return {"bc": bc, **{k: info[k] for k in keys}}, {}

    def ref(g):
        seeds = g.marks[mark]
        exact, info = bc_ref.reference(g.N, g.src, g.dst, seeds=seeds, directed=directed)
        return {"bc": np.array([float(x) for x in exact]), "exact": exact, "bound": info, "nseeds": len(seeds),
                **{k: info[k] for k in keys}}
    return run, ref


def check_bc(got, want):
    check_betweenness(got, {k: v for k, v in want.items() if k != "bc"})


def _peer_pressure(distribute):
    def run(eng, g):
        lab, info = eng.peer_pressure(distribute=distribute)
        assert eng.stats()["iterations"] == info["rounds"]
        return {"cluster": lab, **info}, {}

    def ref(g):
        lab, info = pp_ref.reference(g.N, g.src, g.dst, g.ids, vote_scope=OUT, distribute=int(distribute))
        return {"cluster": lab, **info}
    return run, ref


def _closeness(scope):
    def run(eng, g):
        res, info = eng.closeness(scope=scope)
        five = eng.copy_closeness()
        assert all(res[k].tobytes() == five[k].tobytes() for k in res)
        st = eng.stats()
        assert st["iterations"] == info["batches"] and st["levels"] == info["max_depth"]
        return {**five, **info}, {}

    def ref(g):
        five, info = cl_ref.reference(g.N, g.src, g.dst, scope)
        return {**five, **info}
    return run, ref


def _messages(g, value_type):
    rng = np.random.default_rng([g.N, value_type, 3])
    has = rng.random(g.N) >= 1.0 / 3
    msg = rng.integers(-(1 << 40), 1 << 40, g.N) if value_type == L.VAL_INT64 else rng.standard_normal(g.N)
    return msg, has


def _gather(scope, value_type, combiner, edge_fn):
    def fold(out, has):
        return {"has": np.asarray(has, bool), "value": np.where(has, out, 0).astype(out.dtype)}

    def run(eng, g):
        return fold(*eng.gather(scope, value_type, combiner, edge_fn, *_messages(g, value_type))), {}

    def ref(g):
        return fold(*g.oracle.gather(scope, value_type, combiner, edge_fn, *_messages(g, value_type)))
    return run, ref


def _global_messages(g):
    rng = np.random.default_rng([g.N, 4])
    m = 5 * g.N
    targets = rng.integers(0, g.N, m)
    targets[::7] = rng.integers(0, min(16, g.N), len(targets[::7]))           # a few hot targets
    return targets, rng.integers(-(1 << 50), 1 << 50, m)


def _combine_global():
    def fold(out, has):
        return {"has": np.asarray(has, bool), "value": np.where(has, out, 0).astype(out.dtype)}

    def run(eng, g):
        return fold(*eng.combine_global(L.VAL_INT64, L.COMBINE_SUM, *_global_messages(g))), {}

    def ref(g):
        return fold(*fr.combine_global(g.N, L.VAL_INT64, L.COMBINE_SUM, *_global_messages(g)))
    return run, ref


def encoded_rows(ids, entries_of, base=RELATION_BASE):
    """The oracle encoder's rows for every vertex (row order) that holds a value, as test_gpu_writeback.py
    builds them: dict(keys, entry_begin, byte_begin, data, limit_valpos); the relation ids run on from base."""
    keys, eb, bb, data, lv = [], [0], [0], bytearray(), []
    rel = base
    lib = fr.load()
    for i, vid in enumerate(ids):
        ents = entries_of(i, rel)
        if not ents:
            continue
        rel += len(ents)
        start = len(data)
        for b, vp in sorted(ents, key=lambda e: e[0][:e[1]]):
            data += b
            lv.append(((len(data) - start) << 32) | vp)
        keys.append(lib.fr_key_of(int(vid), 5))
        eb.append(len(lv))
        bb.append(len(data))
    return {"keys": np.array(keys, np.int64), "entry_begin": np.array(eb, np.int64), "byte_begin": np.array(bb, np.int64),
            "data": np.frombuffer(bytes(data), np.uint8).copy(), "limit_valpos": np.array(lv, np.int64)}


def rows_dict(rows):
    """An Engine result (Rows) in encoded_rows' form."""
    return {"keys": np.asarray(rows.keys, np.int64), "entry_begin": np.asarray(rows.entry_begin, np.int64),
            "byte_begin": np.asarray(rows.byte_begin, np.int64), "data": np.asarray(rows.data, np.uint8),
            "limit_valpos": np.asarray(rows.limit_valpos, np.int64)}


def _row_values(g):
    """One distinct value per row and a ragged present mask."""
    rng = np.random.default_rng([g.N, 5])
    values = (np.arange(g.N, dtype=np.int64) * 2654435761 + 12345) - (1 << 33)
    present = rng.random(g.N) < 0.6
    present[:3] = [True, False, True]
    return values, present


def _result_rows_values():
    def run(eng, g):
        values, present = _row_values(g)
        return rows_dict(eng.result_rows_values(VALUE_KEY, L.DT_LONG, L.VAL_INT64, values, present, RELATION_BASE)), {}

    def ref(g):
        values, present = _row_values(g)
        return encoded_rows(g.ids, lambda i, rel: [fr.encode_property(VALUE_KEY, L.DT_LONG, int(values[i]), rel)]
                            if present[i] else [])
    return run, ref


def _division_by_zero(scope):
    """test_integer_division_by_zero_fails_the_program's call: some entry the gather reads weighs 0."""
    def run(eng, g):
        eng.gather(scope, L.VAL_INT64, L.COMBINE_SUM, L.EDGE_DIV_WEIGHT, np.ones(g.N, np.int64))
        return {}, {}
    return run, None


def _wrong_scope(scope):
    def run(eng, g):
        if scope == BOTH:
            eng.walkcount(3)          # DegreeCounter runs on inE loads only
        else:
            eng.components()          # the analytics run on bothE loads only
        return {}, {}
    return run, None


def _build(scope):
    H, D = L.SSSP_HOP_BOUNDED, L.SSSP_DELTA
    c = [("bfs_path_end", _bfs(scope, "path_end", True), {}),
         ("bfs_multi_64", _bfs_multi(scope, "seeds64", False), {}),
         ("bfs_multi_3", _bfs_multi(scope, "seeds3", True), {}),
         ("sssp_hop", _sssp(scope, "path_end", False, H, 0, HOP_DEPTH), {}),
         ("sssp_delta9", _sssp(scope, "hub", False, D, 9, 0), {}),
         ("sssp_delta3", _sssp(scope, "path_end", True, D, 3, 0), {})]
    if scope == BOTH:
        c += [("bfs_isolated", _bfs(scope, "isolated", False), {}),
              ("components", _components(), {}),
              ("triangles", _triangles(), {}),
              ("kcore", _kcore(), {}),
              ("ktruss0", _ktruss(0), {"check": check_truss}),
              ("ktruss4", _ktruss(4), {"check": check_truss}),
              ("scc", _scc(), {}),
              ("betweenness_8", _betweenness("bc_und", False), {"check": check_bc}),
              ("betweenness_directed_8", _betweenness("bc_dir", True), {"check": check_bc}),
              ("peer_pressure", _peer_pressure(False), {}),
              ("peer_pressure_distribute", _peer_pressure(True), {}),
              ("closeness_all", _closeness(BOTH), {}),
              ("gather_int64_sum", _gather(BOTH, L.VAL_INT64, L.COMBINE_SUM, L.EDGE_IDENTITY), {}),
              ("gather_fp64_min_add_weight", _gather(BOTH, L.VAL_FP64, L.COMBINE_MIN, L.EDGE_ADD_WEIGHT), {}),
              ("combine_global", _combine_global(), {}),
              ("result_rows_values", _result_rows_values(), {})]
    else:
        c += [("pagerank_5", _pagerank(5), {"check": check_pagerank}),
              ("pagerank_0", _pagerank(0), {"check": check_pagerank, "constant_by_contract": True}),
              ("walkcount_3", _walkcount(3), {}),
              ("closeness_all", _closeness(IN), {}),
              ("gather_int64_sum_add_weight", _gather(IN, L.VAL_INT64, L.COMBINE_SUM, L.EDGE_ADD_WEIGHT), {})]
    c += [("fails_division_by_zero", _division_by_zero(scope), {"fails": L.TGO_E_PROGRAM}),
          ("fails_wrong_scope", _wrong_scope(scope), {"fails": L.TGO_E_INVALID})]
    return [Call(scope, name, run, ref, **kw) for name, (run, ref), kw in c]


_CALLS = {scope: _build(scope) for scope in (BOTH, IN)}
ALL = {(c.scope, c.name): c for cs in _CALLS.values() for c in cs}


def calls(scope):
    """The ordered named calls of a load of `scope` (BOTH or IN)."""
    return list(_CALLS[scope])


# ----------------------------------------------------------------------------- the walk
def pair_walk(k):
    """Hierholzer's algorithm on the complete digraph on k nodes with self-loops, every node's arcs taken
    in ascending order of their heads, from node 0: k * k + 1 nodes, every ordered pair adjacent once."""
    nxt = [0] * k                                # the next unused arc of node a goes to nxt[a]
    stack, circuit = [0], []
    while stack:
        a = stack[-1]
        if nxt[a] < k:
            stack.append(nxt[a])
            nxt[a] += 1
        else:
            circuit.append(stack.pop())
    return circuit[::-1]
