"""Test helper: what a row load holds, entry for entry, from both sides.

An Engine's assembled OUT / IN lists (graph_csr, graph_perm, vertex_ids) and an OracleGraph's
decoded adjacency (export) are each turned into one int64 array of
    (row Titan id, direction 0 OUT / 1 IN, other Titan id, weight)
sorted lexicographically, so the two can be compared with array_equal: nothing sampled, nothing
left out.  The weight column is the load's 32-bit column (Float: the IEEE bits), MISSING
(INT32_MIN) for an entry without the weight property, and 0 where weights are not compared.

An entry whose other endpoint has no live row (a ghost, a filtered schema vertex, a vertex the
scan never returned) is represented the same way by both sides: not at all.  The assembly drops
it (graph_build.cpp assemble_from_rows: dense[k] < 0), fr_export drops it (entry_vertex < 0), and
neither keeps a tombstone, so the kept entries of a row are the comparison: their number per row
is part of the array equality, every kept id is asserted to be a live vertex, and the oracle's
own count of such entries is oracle_dangling().

Long / Double weight keys: the engine's column holds positions in a 64-bit value table, not
values, so those loads compare topology here and values through weight_lists(): a combiner-less
receive of zero messages with EDGE_ADD_WEIGHT, which hands every vertex exactly its entries'
weights.
"""
import numpy as np

from titan_amd import _lib as L

MISSING = -(1 << 31)
COUNTERS = ("out_entries", "in_entries")


def _sorted_rows(a):
    a = np.asarray(a, np.int64).reshape(-1, 4)
    return a[np.lexsort((a[:, 3], a[:, 2], a[:, 1], a[:, 0]))]


def engine_entries(eng, weights=True):
    """{direction: sorted (E, 4) array} for each direction list the load holds."""
    n = eng.n
    tid = np.empty(n, np.int64)
    tid[np.asarray(eng.graph_perm(), np.int64)] = eng.vertex_ids()      # internal id -> Titan id
    out = {}
    for d in (0, 1):
        g = eng.graph_csr(d)
        if g is None:
            continue
        row = np.repeat(np.arange(n, dtype=np.int64), np.diff(g["off"]))
        w = g["w"].astype(np.int64) if weights else np.zeros(len(row), np.int64)
        out[d] = _sorted_rows(np.stack([tid[row], np.full(len(row), d, np.int64), tid[g["adj"].astype(np.int64)], w], 1))
    return out


def oracle_entries(o, weights=True):
    """The same two arrays from OracleGraph.export: OUT entries [off, mid), IN entries [mid, off[v+1])."""
    off, mid, adj, w = o.export(weighted=True)
    ids = o.vertex_ids()
    n = len(ids)
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(off))
    k = np.arange(len(row), dtype=np.int64)
    d = (k >= mid[row]).astype(np.int64) if len(row) else np.zeros(0, np.int64)
    ww = w.astype(np.int64) if weights else np.zeros(len(row), np.int64)
    a = np.stack([ids[row], d, ids[adj.astype(np.int64)], ww], 1) if len(row) else np.zeros((0, 4), np.int64)
    return {x: _sorted_rows(a[a[:, 1] == x]) for x in (0, 1)}


def oracle_dangling(o):
    """Entries the oracle decoded whose other endpoint has no live row (dropped by export)."""
    return int(o.stats.num_entries) - len(o.export()[2])


def assert_lists_equal(eng, o, weights=True):
    """Every entry of every list the engine holds equals the oracle's; returns the number compared,
    which is the load's own out_entries + in_entries."""
    assert np.array_equal(np.sort(eng.vertex_ids()), np.sort(o.vertex_ids()))
    got, want = engine_entries(eng, weights), oracle_entries(o, weights)
    st = eng.stats()
    ids = o.vertex_ids()
    total = 0
    for d, a in got.items():
        assert len(a) == st[COUNTERS[d]], (d, len(a), st[COUNTERS[d]])
        assert len(want[d]) == len(a), (d, len(want[d]), len(a))
        assert np.array_equal(a, want[d]), (d, _first_difference(a, want[d]))
        assert np.isin(a[:, 2], ids).all()
        total += len(a)
    assert total == st["out_entries"] + st["in_entries"]
    return total


def _first_difference(a, b):
    bad = np.flatnonzero((a != b).any(1))
    return (int(bad[0]), a[bad[0]].tolist(), b[bad[0]].tolist(), len(bad)) if len(bad) else None


STAT_PAIRS = (("num_vertices", None), ("ghost_vertices", "ghost_vertices"), ("truncated_results", "truncated_results"),
              ("skipped_rows", "skipped_rows"), ("partitioned_vertices", "partitioned_vertices"),
              ("partition_rows", "partition_rows"), ("ghost_partition_rows", "ghost_partition_rows"))


def assert_counters_equal(eng, o):
    """ScanMetrics counters of the load against OracleGraph.stats."""
    st = eng.stats()
    for mine, theirs in STAT_PAIRS:
        want = o.n if theirs is None else getattr(o.stats, theirs)
        assert st[mine] == want, (mine, st[mine], want)


def _pairs(ids, off, vals):
    """(vertex id, value) sorted by id, then value: every vertex's received list, sorted."""
    row = np.repeat(np.asarray(ids, np.int64), np.diff(off))
    order = np.lexsort((vals, row))
    return row[order], np.asarray(vals)[order]


def weight_lists(side, scope, value_type, present_ids=None):
    """Every vertex's entry weights as (ids, values) sorted per vertex: gather_lists over an all-zero
    message vector with EDGE_ADD_WEIGHT.  side: an Engine or an OracleGraph; present_ids: the Titan
    ids of the vertices that hold a message (None: every vertex).  A load in which a read entry
    lacks the weight fails here as the program does (TitanException / RuntimeError)."""
    ids = side.vertex_ids()
    msg = np.zeros(len(ids), np.int64 if value_type == L.VAL_INT64 else np.float64)
    has = np.ones(len(ids), bool) if present_ids is None else np.isin(ids, present_ids)
    off, vals = side.gather_lists(scope, value_type, L.EDGE_ADD_WEIGHT, msg, has)
    return _pairs(ids, off, vals)


def assert_weight_lists_equal(eng, o, scope, value_type, present_ids=None):
    gi, gv = weight_lists(eng, scope, value_type, present_ids)
    wi, wv = weight_lists(o, scope, value_type, present_ids)
    assert np.array_equal(gi, wi), (len(gi), len(wi))
    bits = (lambda x: x.view(np.int64)) if value_type == L.VAL_FP64 else (lambda x: x)
    assert np.array_equal(bits(gv), bits(wv)), int(np.flatnonzero(bits(gv) != bits(wv))[0])
    return len(gi)


# ------------------------------------------------------------------ expected lists of a GraphSpec
def spec_entries(spec, vids, weight_key, labels=(), dead=()):
    """The entries a load of build_rows(spec) must hold when nothing is cut: every edge once as
    OUT on its source row and once as IN on its target row, MISSING for an absent weight; edges of
    other labels (typed scope) and edges touching a vertex without a live row (dead) are absent."""
    dead = set(dead)
    rows = []
    for (s, d, label, props) in spec.edges:
        if (labels and label not in labels) or s in dead or d in dead:
            continue
        w = dict(props).get(weight_key, MISSING) if weight_key else 0
        rows.append((int(vids[s]), 0, int(vids[d]), w))
        rows.append((int(vids[d]), 1, int(vids[s]), w))
    a = _sorted_rows(np.asarray(rows, np.int64)) if rows else np.zeros((0, 4), np.int64)
    return {x: a[a[:, 1] == x] for x in (0, 1)}


# ------------------------------------------------------------------ the mixed schema
def mixed_schema():
    """One label per multiplicity over three property keys, the weight key's id the largest so that
    the String and the Double precede it among the remaining properties:
      MULTI     sort key DESC [String, Double, weight]
      SIMPLE    signature [String, weight]
      MANY2ONE  signature [String, weight]
      ONE2MANY  no signature: String, Double and weight among the remaining properties
      ONE2ONE   signature [weight]
    Returns (schema dict, OracleSchema, weight key, [label ids by multiplicity])."""
    import fulgora as fr
    lib = fr.load()
    ks, kd, w = (lib.fr_schema_id(0, c) for c in (1, 2, 3))
    labels = [lib.fr_schema_id(2, c) for c in (1, 2, 3, 4, 5)]
    pkeys = [(ks, L.DT_STRING), (kd, L.DT_DOUBLE), (w, L.DT_INTEGER)]
    ets = [{"type_id": labels[0], "multiplicity": L.MULTI, "sort_key": [ks, kd, w], "signature": [], "order": "DESC"},
           {"type_id": labels[1], "multiplicity": L.SIMPLE, "sort_key": [], "signature": [ks, w], "order": "ASC"},
           {"type_id": labels[2], "multiplicity": L.MANY2ONE, "sort_key": [], "signature": [ks, w], "order": "ASC"},
           {"type_id": labels[3], "multiplicity": L.ONE2MANY, "sort_key": [], "signature": [], "order": "ASC"},
           {"type_id": labels[4], "multiplicity": L.ONE2ONE, "sort_key": [], "signature": [w], "order": "ASC"}]
    sd = {"edge_types": ets, "property_keys": [list(p) for p in pkeys]}
    return sd, fr.OracleSchema(ets, pkeys), w, labels


def mixed_edges(rnd, n, m, absent=0.15):
    """m random edges over the mixed schema, all labels on the same rows (self-loops and parallel
    edges included); every property absent now and then, the weight on `absent` of the edges."""
    sd, osch, w, labels = mixed_schema()
    ks, kd = sd["property_keys"][0][0], sd["property_keys"][1][0]
    edges = []
    for _ in range(m):
        props = []
        if rnd.random() >= 0.1:         # "" / ASCII digits / full UTF (oracle fr_string_of)
            props.append((ks, rnd.choice([0, rnd.randrange(1, 10 ** 9), -rnd.randrange(1, 10 ** 6)])))
        if rnd.random() >= 0.1:
            props.append((kd, rnd.randrange(-(1 << 50), 1 << 50)))
        if rnd.random() >= absent:
            props.append((w, rnd.choice([rnd.randrange(-(1 << 31) + 1, 1 << 31), rnd.randrange(-50, 50)])))
        edges.append((rnd.randrange(n), rnd.randrange(n), rnd.choice(labels), props))
    return edges
