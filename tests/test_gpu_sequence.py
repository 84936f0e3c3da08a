"""GPU: every program held to its reference after every other program on one context.

A tgo_ctx carries one Scratch that every program reinterprets for itself, and the drivers keep lazy
invariants between calls (tests/sequence_cases.py names them).  Three families:

  1. every ordered pair: one Engine per scope (bothE, inE) makes the named calls of sequence_cases.calls
     in sequence_cases.pair_walk order, k * k + 1 calls in which every ordered pair (A, B), A = B included,
     is adjacent exactly once.  Every call is compared with its reference (oracle, *_ref helpers) under
     the rule of its own module, and bit for bit with the same call on a fresh context (every
     program is bit-identical from run to run).  The two failing calls must fail with their codes, and
     the call after them is held to its reference like any other.
  2. results that stay on the device: X(fetch=False), copy_X, another program Y over X's result array,
     after which copy_X and result_rows of X's kind refuse and result_rows of Y's kind gives the oracle
     encoder's bytes for Y's values.
  3. reloads on one engine: grow, shrink, a CSR load, an edgestore load and the same rows under another
     id set (both unsorted, one vertex count: seeds given as Titan ids resolve through the id index, peer
     pressure ranks the ids itself); every call of the scope after every load, and
     tgo_stats.device_bytes equal to a context that loaded nothing else.
"""
import ctypes as C

import numpy as np
import pytest

import fulgora as fr
import sequence_cases as sc
from sequence_cases import BOTH, IN
from titan_amd import Engine, Schema, TitanException
from titan_amd import _lib as L

pytestmark = pytest.mark.gpu

N_BASE = 129
CHUNKS = 1                      # contiguous chunks of a walk, one test each (a walk takes about a second)
SCOPES = [BOTH, IN]


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(n):
        if n not in made:
            made[n] = sc.Case.make(n)
        return made[n]
    return get


def load(eng, g, scope, how="edges"):
    """Loads Case g into eng: the rows come in g's own order."""
    if how == "edges":
        eng.load_edges(g.N, g.src, g.dst, scope, weight=g.w, titan_ids=g.ids)
    else:
        oo, oi, ow, io, ii, iw = g.csr()
        eng.load_csr(g.N, oo, oi, io, ii, scope, out_w=ow, in_w=iw, titan_ids=g.ids)
    assert eng.n == g.N and np.array_equal(eng.vertex_ids(), g.ids)
    return eng


def run_call(eng, g, c):
    """(values, same) of one call, checked against its reference; None for a call that must fail."""
    if c.fails is not None:
        with pytest.raises(TitanException) as e:
            c.run(eng, g)
        assert e.value.code == c.fails, (c, str(e.value))
        return None
    got = c.run(eng, g)
    c.check(got[0], g.ref(c))
    return got


@pytest.fixture(scope="module")
def fresh(cases):
    """Per scope {name: (values, same)}: every call on a context of its own, held to its reference."""
    g = cases(N_BASE)
    out = {}
    for scope in SCOPES:
        out[scope] = {}
        for c in sc.calls(scope):
            eng = load(Engine(), g, scope)
            out[scope][c.name] = run_call(eng, g, c)
            eng.close()
    return out


# ----------------------------------------------------------------------------- 1. every ordered pair
def chunk_bounds(k):
    return [k * k * i // CHUNKS for i in range(CHUNKS + 1)]


def chunk_pairs(walk, lo, hi):
    """The ordered pairs (previous call, call) that the chunk of walk positions lo + 1 .. hi compares."""
    return list(zip(walk[lo:hi], walk[lo + 1:hi + 1]))


def walk_params():
    out = []
    for scope in SCOPES:
        k = len(sc.calls(scope))
        b = chunk_bounds(k)
        assert b[0] == 0 and b[-1] == k * k and all(x < y for x, y in zip(b, b[1:]))
        # the chunks' pairs together are the k * k ordered pairs, each once, however many chunks there are
        walk = sc.pair_walk(k)
        assigned = [pair for i in range(CHUNKS) for pair in chunk_pairs(walk, b[i], b[i + 1])]
        assert len(assigned) == k * k and set(assigned) == {(x, y) for x in range(k) for y in range(k)}
        for i in range(CHUNKS):
            out.append(pytest.param(scope, i, id=f"{sc.SCOPE_NAMES[scope]}-chunk{i}-pairs{b[i + 1] - b[i]}-of-{k * k}"))
    return out


@pytest.mark.parametrize("scope,chunk", walk_params())
def test_every_ordered_pair_on_one_context(cases, fresh, scope, chunk):
    g = cases(N_BASE)
    cs = sc.calls(scope)
    k = len(cs)
    walk = sc.pair_walk(k)
    lo, hi = chunk_bounds(k)[chunk:chunk + 2]
    eng = load(Engine(), g, scope)
    prev = cs[walk[lo]]                       # chunk 0: the walk's first call; later: the previous chunk's last
    run_call(eng, g, prev)
    compared = []                             # (previous, current) of every call that was held to its reference
    for p in range(lo, hi):
        cur = cs[walk[p + 1]]
        try:
            got = run_call(eng, g, cur)
            if got is not None:
                sc.assert_same(got, fresh[scope][cur.name])
        except (AssertionError, TitanException) as err:
            raise AssertionError(f"{cur} after {prev} at position {p + 1} of the walk: {err!r}") from err
        compared.append((cs.index(prev), cs.index(cur)))
        prev = cur
    eng.close()
    print(f"{sc.SCOPE_NAMES[scope]} chunk {chunk}: {len(compared)} ordered pairs compared, k = {k}, k * k = {k * k}")
    # what ran is this chunk's share of the k * k pairs (walk_params checks that the shares add up to all
    # of them), every pair distinct; with one chunk that is all k * k
    assert compared == chunk_pairs(walk, lo, hi) and len(set(compared)) == hi - lo


# ----------------------------------------------------------------------------- 2. results on the device
KEY_A, KEY_B = (7800 << 6) | 5, (7801 << 6) | 5


def copy_distances(eng):
    out = np.zeros(eng.n, np.int64)
    rc = eng.lib.tgo_copy_distances(eng.ctx, L.ptr(out, C.c_int64))
    if rc != L.TGO_OK:
        raise TitanException(rc, eng.lib.tgo_last_error(eng.ctx).decode(errors="replace"))
    return out


def _truss_copy(eng):
    return {"vtruss": eng.copy_truss(), "edges": sc.truss_ref.edge_rows(*eng.copy_truss_edges())}


def _tri_copy(eng):
    tri, deg, lcc = eng.copy_triangles()
    return {"tri": tri, "deg": deg, "lcc": lcc}


def _hop(scope):
    return lambda e, g: e.sssp(g.marks["path_end"], sc.HOP_DEPTH, scope, seed_is_dense=True, fetch=False)


# X: (load scope, call name, X(fetch=False), copy_X as the reference's entries, kind, datatypes of its keys, Y).
# tgo_bfs, tgo_sssp and tgo_pagerank share tgo_copy_distances (the ranks come as the bits of the doubles).
RESIDENT = [
    (IN, "pagerank_5", lambda e, g: e.pagerank(0.85, g.N, 5, fetch=False),
     lambda e: {"pr": copy_distances(e).view(np.float64)}, L.RESULT_PAGERANK, [L.DT_DOUBLE, L.DT_DOUBLE], "walkcount_3"),
    (IN, "sssp_hop", _hop(IN), lambda e: {"dist": copy_distances(e)}, L.RESULT_DISTANCE, [L.DT_LONG], "walkcount_3"),
    (BOTH, "sssp_delta9", lambda e, g: e.sssp(g.marks["hub"], g.N, BOTH, mode=L.SSSP_DELTA, seed_is_dense=True,
                                              fetch=False, delta=9),
     lambda e: {"dist": copy_distances(e)}, L.RESULT_DISTANCE, [L.DT_LONG], "scc"),
    (BOTH, "bfs_path_end", lambda e, g: e.bfs(int(g.ids[g.marks["path_end"]]), g.N, BOTH, fetch=False),
     lambda e: {"dist": copy_distances(e)}, L.RESULT_DISTANCE, [L.DT_LONG], "components"),
    (BOTH, "components", lambda e, g: e.components(fetch=False), lambda e: {"label": e.copy_components()},
     L.RESULT_COMPONENT, [L.DT_LONG], "bfs_path_end"),
    (BOTH, "triangles", lambda e, g: e.triangles(fetch=False), _tri_copy, L.RESULT_TRIANGLES, [L.DT_LONG, L.DT_DOUBLE], "scc"),
    (BOTH, "kcore", lambda e, g: e.kcore(fetch=False), lambda e: {"core": e.copy_cores()}, L.RESULT_CORE, [L.DT_LONG],
     "bfs_path_end"),
    (BOTH, "ktruss0", lambda e, g: e.ktruss(fetch=False), _truss_copy, L.RESULT_TRUSS, [L.DT_LONG], "kcore"),
    (BOTH, "scc", lambda e, g: e.scc(fetch=False), lambda e: {"label": e.copy_scc()}, L.RESULT_SCC, [L.DT_LONG], "kcore"),
    (BOTH, "betweenness_8", lambda e, g: e.betweenness(g.ids[g.marks["bc_und"]], fetch=False),
     lambda e: {"bc": e.copy_betweenness()}, L.RESULT_BETWEENNESS, [L.DT_DOUBLE], "scc"),
    (BOTH, "peer_pressure", lambda e, g: e.peer_pressure(fetch=False), lambda e: {"cluster": e.copy_peer_pressure()},
     L.RESULT_PEER_PRESSURE, [L.DT_LONG], "components"),
    (BOTH, "closeness_all", lambda e, g: e.closeness(fetch=False), lambda e: e.copy_closeness(), L.RESULT_CLOSENESS,
     [L.DT_DOUBLE, L.DT_DOUBLE], "betweenness_8"),
]

# Y: kind, the datatype of its key, its values in the call's result, whether ABSENT rows hold no property
OVERWRITERS = {
    "components": (L.RESULT_COMPONENT, L.DT_LONG, "label", False),
    "bfs_path_end": (L.RESULT_DISTANCE, L.DT_LONG, "dist", True),
    "scc": (L.RESULT_SCC, L.DT_LONG, "label", False),
    "kcore": (L.RESULT_CORE, L.DT_LONG, "core", False),
    "betweenness_8": (L.RESULT_BETWEENNESS, L.DT_DOUBLE, "bc", False),
    "walkcount_3": (L.RESULT_DEGREE, L.DT_INTEGER, "count", False),
}


def encoded(g, dt, values, skip_absent):
    def entries(i, rel):
        if skip_absent and values[i] == L.DIST_ABSENT:
            return []
        if dt == L.DT_DOUBLE:
            return [fr.encode_property_f64(KEY_A, float(values[i]), rel)]
        return [fr.encode_property(KEY_A, dt, int(values[i]), rel)]
    return sc.encoded_rows(g.ids, entries)


@pytest.fixture(scope="module")
def resident_engines(cases):
    engines = {scope: load(Engine(), cases(N_BASE), scope) for scope in SCOPES}
    yield engines
    for eng in engines.values():
        eng.close()


@pytest.mark.parametrize("x", RESIDENT, ids=[f"{sc.SCOPE_NAMES[r[0]]}-{r[1]}" for r in RESIDENT])
def test_a_result_left_on_the_device(cases, resident_engines, x):
    scope, name, run_x, copy_x, kind, dts, y_name = x
    g, eng = cases(N_BASE), resident_engines[scope]
    want = g.ref(sc.ALL[(scope, name)])
    run_x(eng, g)                                           # nothing is fetched
    got = copy_x(eng)
    if name == "betweenness_8":
        sc.bc_ref.within(got["bc"], want["exact"], sc.bc_ref.tolerance(want["bound"], want["nseeds"]))
    elif name == "pagerank_5":
        sc.check_pagerank(got, {"pr": want["pr"]})
    else:
        sc.check_exact(got, {k: want[k] for k in got})
    keys = [KEY_A, KEY_B][:len(dts)]
    assert eng.result_rows(kind, keys, dts, sc.RELATION_BASE).nrows > 0
    # Y runs over X's result array and is itself held to its reference
    y = sc.ALL[(scope, y_name)]
    y_kind, y_dt, y_key, skip_absent = OVERWRITERS[y_name]
    assert y_kind != kind
    values = run_call(eng, g, y)[0]
    with pytest.raises(TitanException) as e:
        copy_x(eng)
    assert e.value.code == L.TGO_E_STATE
    with pytest.raises(TitanException) as e:
        eng.result_rows(kind, keys, dts, sc.RELATION_BASE)
    assert e.value.code == L.TGO_E_STATE
    rows = sc.rows_dict(eng.result_rows(y_kind, [KEY_A], [y_dt], sc.RELATION_BASE))
    sc.check_exact(rows, encoded(g, y_dt, values[y_key], skip_absent))


# ----------------------------------------------------------------------------- 3. reloads on one engine
def rows_case(eng, g, scope, other_ids=False):
    """Loads g's edgestore rows (edgestore.build_rows) and returns g in the rows' order under the rows'
    ids, with the oracle loaded from the same rows."""
    rows, vids, sd, wkey = g.rows(other_ids)
    eng.load_rows(rows, Schema.from_dict(sd), scope, weight_key=wkey)
    o = fr.OracleGraph.from_rows(rows, fr.OracleSchema(sd["edge_types"], [(wkey, 3)]), scope, weight_key=wkey)
    eids = eng.vertex_ids()
    assert eng.n == g.N and np.array_equal(o.vertex_ids(), eids) and sorted(eids.tolist()) == sorted(vids.tolist())
    row_of = {int(v): r for r, v in enumerate(eids)}
    return g.reordered(np.array([row_of[int(v)] for v in vids], np.int64), eids, o)


def run_every_call(eng, g, scope, order_seed, what):
    order = np.random.default_rng([order_seed, scope]).permutation(len(sc.calls(scope)))
    prev = "the load"
    for i in order:
        c = sc.calls(scope)[i]
        try:
            run_call(eng, g, c)
        except (AssertionError, TitanException) as err:
            raise AssertionError(f"{what}: {c} after {prev}: {err!r}") from err
        prev = c


def fresh_bytes(g, scope, how):
    eng = Engine()
    if how.startswith("rows"):
        rows_case(eng, g, scope, how == "rows, other ids")
    else:
        load(eng, g, scope, how)
    b = eng.stats()["device_bytes"]
    eng.close()
    return b


@pytest.mark.parametrize("scope", SCOPES, ids=[sc.SCOPE_NAMES[s] for s in SCOPES])
def test_reloads_on_one_engine(cases, scope):
    g129, g1001, g65 = cases(129), cases(1001), cases(65)
    # edge and CSR loads take strictly increasing ids only: the rows of an edgestore load come in key
    # order, which is not id order, so the two row loads are the unsorted id sets of one vertex count
    steps = [("edges 129", g129, "edges"), ("edges 1001 (grow)", g1001, "edges"), ("edges 65 (shrink)", g65, "edges"),
             ("csr 129", g129, "csr"), ("rows 129", g129, "rows"), ("rows 129, other ids", g129, "rows, other ids"),
             ("edges 129 again", g129, "edges")]
    eng = Engine()
    after_load, after_calls = {}, {}
    previous_ids = None
    for i, (what, g, how) in enumerate(steps):
        if how.startswith("rows"):
            loaded = rows_case(eng, g, scope, how == "rows, other ids")
            assert not (np.diff(loaded.ids) > 0).all()                 # seeds given as ids go through the id index
            if previous_ids is not None:
                assert len(previous_ids) == loaded.N and not np.array_equal(previous_ids, loaded.ids)
            previous_ids = loaded.ids
        else:
            load(eng, g, scope, how)
            loaded = g
        b = eng.stats()["device_bytes"]
        want = fresh_bytes(g, scope, how)
        print(f"{what}: device_bytes {b} after the load, {want} on a context of its own")
        assert b == want, what
        after_load.setdefault((id(g), how), []).append(b)
        run_every_call(eng, loaded, scope, 20261021, what)             # the same order at every step
        after_calls.setdefault((id(g), how), []).append(eng.stats()["device_bytes"])
    eng.close()
    first, again = after_load[(id(g129), "edges")], after_calls[(id(g129), "edges")]
    assert len(first) == 2 and first[0] == first[1] and again[0] == again[1], (first, again)
