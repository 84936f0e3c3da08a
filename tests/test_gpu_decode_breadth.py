"""GPU: the device compile of the edgestore codec (decode.hip: dec_rows / dec_entries) and the host
decoder (TGO_HOST_DECODE=1) each against the ORACLE, entry for entry.

test_gpu_decode.py compares the two compiles of codec.hpp with each other, through distances; a
mistake they share, or one wrong weight, is invisible there.  Here every load's assembled lists
(tests/loaded_lists.py) must equal the oracle's decoded adjacency, and its counters the oracle's
stats, over the codec's breadth: the eight layouts of test_codec_types, one label per
multiplicity, every 32-bit weight datatype in every position, Long / Double weights (values
through a combiner-less receive) including those whose low 32 bits equal the missing-weight
value, the per-row rules of dec_rows at a small hard limit, and malformed rows.

Every case has more than 256 live rows and more than 256 kept entries (kBlock = 256: more than
one workgroup and a ragged tail in both kernels)."""
import functools
import random

import numpy as np
import pytest

import edgestore as es
import fulgora as fr
import loaded_lists as ll
from test_codec_types import K, LAYOUTS, PKEYS, W, random_props, schema_dict
from titan_amd import Engine, Schema, TitanException
from titan_amd import _lib as L

pytestmark = pytest.mark.gpu
OUT, IN, BOTH = L.SCOPE_OUT_E, L.SCOPE_IN_E, L.SCOPE_BOTH_E
BYTE, SHORT, INTEGER, LONG, FLOAT, DOUBLE, BOOLEAN, DATE, CHARACTER, STRING = range(1, 11)
HOSTS = pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
BATCHES = (None, 1, 77)
N = 300
lib = fr.load()


def osch_of(sd):
    return fr.OracleSchema(sd["edge_types"], [tuple(p) for p in sd["property_keys"]])


def decoder(monkeypatch, host):
    monkeypatch.setenv("TGO_HOST_DECODE", "1" if host else "0")


def check(eng, o, weights=True):
    """Counters and every entry against the oracle; the case is large enough for two workgroups."""
    ll.assert_counters_equal(eng, o)
    compared = ll.assert_lists_equal(eng, o, weights)
    assert eng.n > 256 and compared > 256
    return compared


@functools.lru_cache(maxsize=None)
def oracle(case, args, scope, labels=(), limit=100000):
    """The reference load of case(*args), made once and shared by the device and the host test."""
    rows, sd, wkey = case(*args)[:3]
    return fr.OracleGraph.from_rows(rows, osch_of(sd), scope, hard_limit=limit, labels=labels, weight_key=wkey)


# ------------------------------------------------------------------ (a) the eight layouts
@functools.lru_cache(maxsize=None)
def layout_rows(layout):
    mult, sk, sig, order = LAYOUTS[layout]
    sd = schema_dict(mult, sk, sig, order)
    rnd = random.Random(400 + layout)
    keys = [k for k, _ in PKEYS]
    edges = []
    for _ in range(3000):
        props = [(k, v) for k, v in random_props(rnd, keys) if not (k == W and v == ll.MISSING)]
        edges.append((rnd.randrange(N), rnd.randrange(N), sd["edge_types"][0]["type_id"], props))
    rows, vids = es.build_rows(es.GraphSpec(n=N, edges=edges, schema_rows=2), osch_of(sd))
    return rows, sd, W, vids


@HOSTS
@pytest.mark.parametrize("layout", range(len(LAYOUTS)))
def test_layouts_match_oracle(monkeypatch, layout, host):
    decoder(monkeypatch, host)
    rows, sd, wkey, _ = layout_rows(layout)
    eng = Engine()
    for scope in (IN, BOTH):
        o = oracle(layout_rows, (layout,), scope)
        for batch in BATCHES:
            eng.load_rows(rows, Schema.from_dict(sd), scope, weight_key=wkey, batch_rows=batch)
            assert check(eng, o) == 6000          # both entries of every edge, none sampled


# ------------------------------------------------------------------ (b) multiplicities
@functools.lru_cache(maxsize=None)
def mixed_rows():
    sd, osch, w, labels = ll.mixed_schema()
    rnd = random.Random(31)
    spec = es.GraphSpec(n=N, edges=ll.mixed_edges(rnd, N, 3500), schema_rows=2, pv_ghost=[17, 150])
    rows, vids = es.build_rows(spec, osch)
    return rows, sd, w, labels


@HOSTS
def test_multiplicities_match_oracle(monkeypatch, host):
    """Five labels, one per multiplicity (both branches of unique_in, the forward and the backward
    read of the other-vertex id), mixed on the same rows; sort-key / signature / remaining weights
    behind Strings and a Double; null inline values; untyped and typed scopes."""
    decoder(monkeypatch, host)
    rows, sd, w, labels = mixed_rows()
    eng = Engine()
    loads = [(OUT, ()), (IN, ()), (BOTH, ())] + [(IN, (lab,)) for lab in labels] + \
            [(OUT, (labels[0], labels[3])), (BOTH, (labels[2], labels[4]))]
    for scope, chosen in loads:
        o = oracle(mixed_rows, (), scope, chosen)
        eng.load_rows(rows, Schema.from_dict(sd), scope, labels=chosen, weight_key=w, batch_rows=77)
        compared = check(eng, o)
        assert chosen or compared > 6000
        assert eng.stats()["ghost_vertices"] == 2 and eng.stats()["skipped_rows"] == 2


# ------------------------------------------------------------------ (c) 32-bit weight datatypes
VALUES32 = {BYTE: [-128, -1, 0, 5, 127], SHORT: [-32768, -3, 0, 7, 32767], CHARACTER: [0, 65, 65535], BOOLEAN: [0, 1],
            INTEGER: [-2147483647, -65537, -1, 0, 7, 2147483647], FLOAT: [-16777216, -7, -1, 0, 3, 1000, 16777216]}


def position_labels(key):
    """Four labels holding `key` in every position: sort key ASC, sort key DESC behind a String,
    signature behind a String, remaining properties."""
    ids = [lib.fr_schema_id(2, c) for c in (3, 4, 5, 6)]
    return ids, [{"type_id": ids[0], "multiplicity": L.MULTI, "sort_key": [key], "signature": [], "order": "ASC"},
                 {"type_id": ids[1], "multiplicity": L.MULTI, "sort_key": [K[STRING], key], "signature": [], "order": "DESC"},
                 {"type_id": ids[2], "multiplicity": L.SIMPLE, "sort_key": [], "signature": [K[STRING], key], "order": "ASC"},
                 {"type_id": ids[3], "multiplicity": L.MULTI, "sort_key": [], "signature": [], "order": "ASC"}]


@functools.lru_cache(maxsize=None)
def narrow_rows(dt):
    key = W if dt == INTEGER else K[dt]
    ids, ets = position_labels(key)
    sd = {"edge_types": ets, "property_keys": [list(p) for p in PKEYS]}
    rnd = random.Random(500 + dt)
    edges = []
    for i in range(1600):                              # 400 edges per position
        props = [(K[STRING], rnd.choice([0, 77, -9]))] if rnd.random() < 0.8 else []
        if rnd.random() >= 0.1:
            props.append((key, VALUES32[dt][i // 4 % len(VALUES32[dt])]))
        edges.append((rnd.randrange(N), rnd.randrange(N), ids[i % 4], props))
    rows, vids = es.build_rows(es.GraphSpec(n=N, edges=edges), osch_of(sd))
    return rows, sd, key, vids


@HOSTS
@pytest.mark.parametrize("dt", sorted(VALUES32))
def test_32_bit_weight_datatypes_match_oracle(monkeypatch, dt, host):
    decoder(monkeypatch, host)
    rows, sd, key, _ = narrow_rows(dt)
    eng = Engine()
    for scope, batch in ((BOTH, None), (IN, 77)):
        o = oracle(narrow_rows, (dt,), scope)
        eng.load_rows(rows, Schema.from_dict(sd), scope, weight_key=key, batch_rows=batch)
        assert check(eng, o) == 3200
    # the column holds the values the test chose (a Float as its IEEE bits), or the missing value
    want = set(VALUES32[dt]) if dt != FLOAT else {int(np.float32(x).view(np.int32)) for x in VALUES32[dt]}
    got = set(np.unique(eng.graph_csr(1)["w"]).tolist())
    assert got == want | {ll.MISSING}


# ------------------------------------------------------------------ (d) Long / Double weights
# values whose low 32 bits are 0x80000000 (the 32-bit column's missing value) first, then ordinary
# ones on both sides of 2^32
VALUES64 = {LONG: [2147483648, -2147483648, 6442450944, -6442450944,
                   0, 1, -1, 7, 4294967295, 4294967296, 4294967297, -4294967297, 5_000_000_000, -(1 << 40) - 3,
                   (1 << 62) + 5, -(1 << 62)],
            DOUBLE: [2097153, -2097153, 4503601774854144,
                     0, 1, -2, 3, 2097152, 2097154, 4294967296, -4294967297, 1 << 53, -1099511627779]}
WHERE = ("sort_key_asc", "sort_key_desc", "signature", "remaining")
QUIET = [i for i in range(N) if i % 5 < 2]        # an edge between two quiet vertices has no weight: 16 %


@functools.lru_cache(maxsize=None)
def wide_rows(dt, where, absent):
    ids, ets = position_labels(K[dt])
    label, et = ids[WHERE.index(where)], ets[WHERE.index(where)]
    sd = {"edge_types": [et], "property_keys": [list(p) for p in PKEYS]}
    rnd = random.Random(600 + 10 * dt + WHERE.index(where))
    quiet = set(QUIET)
    edges, n_absent = [], 0
    for i in range(2500):
        s, d = rnd.randrange(N), rnd.randrange(N)
        props = [(K[STRING], rnd.choice([0, 77, -9]))] if rnd.random() < 0.8 else []
        if absent and s in quiet and d in quiet:
            n_absent += 1
        else:
            props.append((K[dt], VALUES64[dt][i % len(VALUES64[dt])]))
        edges.append((s, d, label, props))
    rows, vids = es.build_rows(es.GraphSpec(n=N, edges=edges), osch_of(sd))
    return rows, sd, K[dt], vids, n_absent


@HOSTS
@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("dt", [LONG, DOUBLE], ids=["Long", "Double"])
def test_wide_weights_match_oracle(monkeypatch, dt, where, host):
    """Each vertex's received list under EDGE_ADD_WEIGHT over zero messages is its entries' 64-bit
    weights: equal to the oracle's, per vertex.  In the loads where some entries lack the weight
    the program fails on both sides when every vertex sends (e.value(key) throws), and the lists
    are compared with only the loud vertices sending: every entry a loud vertex sends over has one."""
    decoder(monkeypatch, host)
    vt = L.VAL_INT64 if dt == LONG else L.VAL_FP64
    eng = Engine()
    for absent in (False, True):
        rows, sd, key, vids, n_absent = wide_rows(dt, where, absent)
        loud = np.delete(vids, QUIET)
        assert (n_absent > 300) == absent
        for scope in (IN, BOTH):
            o = oracle(wide_rows, (dt, where, absent), scope)
            for batch in BATCHES:
                eng.load_rows(rows, Schema.from_dict(sd), scope, weight_key=key, batch_rows=batch)
                assert check(eng, o, weights=False) == 5000
                missing = sum(int((eng.graph_csr(d)["w"] == ll.MISSING).sum()) for d in (0, 1))
                assert missing == 2 * n_absent
                try:
                    ll.weight_lists(o, scope, vt)
                    oracle_fails = False
                except RuntimeError:
                    oracle_fails = True
                assert oracle_fails == absent
                if oracle_fails:
                    with pytest.raises(TitanException) as e:
                        ll.weight_lists(eng, scope, vt)
                    assert e.value.code == L.TGO_E_PROGRAM
                    assert ll.assert_weight_lists_equal(eng, o, scope, vt, present_ids=loud) > 256
                else:
                    per_edge = 1 if scope == IN else 2
                    assert ll.assert_weight_lists_equal(eng, o, scope, vt) == 2500 * per_edge


# ------------------------------------------------------------------ (e) row rules of dec_rows
LIMIT = 12
KNOWS = lib.fr_schema_id(2, 1)
PLAIN = {"edge_types": [{"type_id": KNOWS, "multiplicity": 0}], "property_keys": [[W, 3]]}


def plain_edges(rnd, lo, hi, m):
    return [(rnd.randrange(lo, hi), rnd.randrange(lo, hi), KNOWS, [(W, rnd.randrange(-99, 99))] if rnd.random() > 0.15 else [])
            for _ in range(m)]


@functools.lru_cache(maxsize=None)
def ruled_rows():
    """Vertices 0..9 are placed by hand, 10..N-1 carry random edges (degrees around the limit)."""
    rnd = random.Random(77)
    edges = plain_edges(rnd, 10, N, 1700)
    far = iter(rnd.sample(range(10, N), 60))
    for v, cnt in ((0, LIMIT - 1), (1, LIMIT), (2, LIMIT + 1)):        # exactly L-1, L, L+1 user edges
        for j in range(cnt):
            u = next(far)
            edges.append((v, u, KNOWS, [(W, j)]) if j % 2 else (u, v, KNOWS, [(W, -j)]))
    edges += [(4, 4, KNOWS, [(W, 5)]), (4, 4, KNOWS, []), (4, 4, KNOWS, [(W, 6)])]      # only self-loops
    edges += [(5, next(far), KNOWS, [(W, 1)]), (9, next(far), KNOWS, []), (next(far), 9, KNOWS, [(W, 2)])]
    spec = es.GraphSpec(n=N, edges=edges, vprops={3: [(lib.fr_schema_id(0, 40), 5)], 5: [(lib.fr_schema_id(0, 40), 6)]},
                        ghost_rows=[(es.vertex_id(N + 7), [(0, es.vertex_id(20), KNOWS), (1, es.vertex_id(21), KNOWS)])],
                        schema_rows=3, pv_ghost=[9])            # vertex 3: properties only; 9: a ghost with edges
    rows, vids = es.build_rows(spec, osch_of(PLAIN))
    return rows, PLAIN, W, vids


@functools.lru_cache(maxsize=None)
def cut_rows():
    """Vertex cuts: four hubs and a small vertex stored as representatives, one of them a ghost."""
    rnd = random.Random(78)
    edges = plain_edges(rnd, 0, N, 2200)
    for hub in (0, 1, 2, 3):
        edges += [(hub, rnd.randrange(N), KNOWS, [(W, rnd.randrange(9))]) for _ in range(60)]
        edges += [(rnd.randrange(N), hub, KNOWS, [(W, rnd.randrange(9))]) for _ in range(60)]
    rows, vids = es.build_rows(es.GraphSpec(n=N, edges=edges, partitioned=[0, 1, 2, 3, 9], pv_ghost=[3]), osch_of(PLAIN))
    return rows, PLAIN, W, vids


def entries_of_row(rows, r):
    """Number of user-edge entries (first column byte in [0x60, 0x80)) of row r."""
    e0, e1 = int(rows.entry_begin[r]), int(rows.entry_begin[r + 1])
    base = int(rows.byte_begin[r])
    starts = [0] + [int(x) >> 32 for x in rows.limit_valpos[e0:e1 - 1]]
    return sum(0x60 <= int(rows.data[base + s]) < 0x80 for s in starts)


@HOSTS
@pytest.mark.parametrize("scope", [IN, OUT], ids=["inE", "outE"])
def test_row_rules_match_oracle(monkeypatch, scope, host):
    decoder(monkeypatch, host)
    rows, sd, w, vids = ruled_rows()
    by_key = {int(k): r for r, k in enumerate(rows.keys)}
    counts = [entries_of_row(rows, by_key[es.key_of(int(vids[v]))]) for v in (0, 1, 2, 3, 4)]
    assert counts == [LIMIT - 1, LIMIT, LIMIT + 1, 0, 6]
    o = oracle(ruled_rows, (), scope, (), LIMIT)
    eng = Engine(hard_query_limit=LIMIT)
    for batch in BATCHES:
        eng.load_rows(rows, Schema.from_dict(sd), scope, weight_key=w, batch_rows=batch)
        check(eng, o)
        st = eng.stats()
        assert st["truncated_results"] == o.stats.truncated_results > 100
        assert (st["ghost_vertices"], st["skipped_rows"]) == (2, 3)
    before = ll.engine_entries(eng)
    # the same rows in three work blocks, the middle one empty
    a = rows.nrows // 2 + 3
    for block in (rows.slice(0, a), rows.slice(a, a), rows.slice(a, rows.nrows)):
        eng.append_rows(block, Schema.from_dict(sd), scope, weight_key=w)
    eng.finish_rows()
    check(eng, o)
    after = ll.engine_entries(eng)
    assert all(np.array_equal(before[d], after[d]) for d in (0, 1))


@HOSTS
@pytest.mark.parametrize("scope", [IN, OUT], ids=["inE", "outE"])
def test_vertex_cut_rows_match_oracle(monkeypatch, scope, host):
    decoder(monkeypatch, host)
    rows, sd, w, vids = cut_rows()
    o = oracle(cut_rows, (), scope, (), LIMIT)
    eng = Engine(hard_query_limit=LIMIT)
    for batch in (None, 77):
        eng.load_rows(rows, Schema.from_dict(sd), scope, weight_key=w, batch_rows=batch)
        check(eng, o)
        st = eng.stats()
        assert st["partitioned_vertices"] == 4 and st["partition_rows"] > 60 and st["ghost_partition_rows"] > 0
        assert st["truncated_results"] == o.stats.truncated_results > 100


# ------------------------------------------------------------------ (f) malformed rows
SORTED = {"edge_types": [{"type_id": KNOWS, "multiplicity": 0, "sort_key": [W], "order": "ASC"}],
          "property_keys": [[W, 3], [K[SHORT], SHORT], [K[INTEGER], INTEGER]]}


@functools.lru_cache(maxsize=None)
def sorted_rows():
    """One MULTI label with the weight as its sort key, a Short and then an Integer among the
    remaining properties; the last row is a vertex row and its last entry a user edge."""
    rnd = random.Random(79)
    edges = [(rnd.randrange(N), rnd.randrange(N), KNOWS, [(W, rnd.randrange(-99, 99)), (K[SHORT], rnd.randrange(99)), (K[INTEGER], rnd.randrange(99))])
             for _ in range(2500)]
    rows, vids = es.build_rows(es.GraphSpec(n=N, edges=edges), osch_of(SORTED))
    return rows, SORTED, W, vids


def copy_rows(rows):
    return es.Rows(*(x.copy() for x in (rows.keys, rows.entry_begin, rows.byte_begin, rows.data, rows.limit_valpos)))


def last_entry(rows):
    """(index of the last entry, its first byte's index in data, its length)."""
    r, k = rows.nrows - 1, int(rows.entry_begin[-1]) - 1
    start = 0 if k == rows.entry_begin[r] else int(rows.limit_valpos[k - 1]) >> 32
    return k, int(rows.byte_begin[r]) + start, (int(rows.limit_valpos[k]) >> 32) - start


def corrupt(name):
    """(rows, schema dict, weight key, expected code).  Every offset stays inside the arrays handed over."""
    rows, sd, wkey, _ = sorted_rows()
    bad = copy_rows(rows)
    code = L.TGO_E_CODEC
    mid = rows.nrows // 2
    k, first, length = last_entry(bad)
    if name == "unknown_label":                 # the last entry of the last row names no label
        assert 0x60 <= bad.data[first] < 0x80
        bad.data[first] = 0x7E
    elif name == "key_suffix_6":
        bad.keys[mid] = (int(bad.keys[mid]) & ~7) | 6
    elif name == "empty_row":                   # one more row, without entries or bytes
        bad.keys = np.insert(bad.keys, mid, int(bad.keys[mid]) - 8)
        bad.entry_begin = np.insert(bad.entry_begin, mid, bad.entry_begin[mid])
        bad.byte_begin = np.insert(bad.byte_begin, mid, bad.byte_begin[mid])
    elif name == "first_column":                # type count 0: not a relation type
        bad.data[int(bad.byte_begin[mid])] = 0x00
    elif name == "short_sort_key":              # the final entry ends two bytes into its sort key
        cut = length - 3
        assert length > 6 and int(bad.limit_valpos[k]) & 0x7FFFFFFF > 3
        bad.limit_valpos[k] = ((int(bad.limit_valpos[k]) >> 32) - cut) << 32 | 3
        bad.byte_begin[-1] -= cut
        bad.data = bad.data[:int(bad.byte_begin[-1])].copy()
    elif name == "value_position":              # valuePos three past the entry's end
        bad.limit_valpos[k] = (int(bad.limit_valpos[k]) >> 32) << 32 | (length + 3)
    elif name == "unknown_property":            # the Short ahead of the weight is stored inline, its key no schema key
        sd = dict(sd, property_keys=[[W, 3], [K[INTEGER], INTEGER]])
        wkey = K[INTEGER]
        code = L.TGO_E_UNSUPPORTED
    else:
        raise ValueError(name)
    return bad, sd, wkey, code


CORRUPTIONS = ("unknown_label", "key_suffix_6", "empty_row", "first_column", "short_sort_key", "value_position",
               "unknown_property")


@HOSTS
@pytest.mark.parametrize("name", CORRUPTIONS)
def test_malformed_rows_fail_alike(monkeypatch, name, host):
    """Each corruption fails the load with the code the other decoder gives (a fixed one), the
    oracle refuses the same rows, and the same Engine then loads the good rows correctly."""
    decoder(monkeypatch, host)
    rows, good_sd, w, _ = sorted_rows()
    bad, sd, bad_w, code = corrupt(name)
    with pytest.raises(RuntimeError) as refused:
        fr.OracleGraph.from_rows(bad, osch_of(sd), BOTH, weight_key=bad_w)
    assert f"rc={code}" in str(refused.value)            # FR_E_CODEC / FR_E_UNSUPPORTED: the same numbers
    eng = Engine()
    with pytest.raises(TitanException) as e:
        eng.load_rows(bad, Schema.from_dict(sd), BOTH, weight_key=bad_w)
    assert e.value.code == code
    eng.load_rows(rows, Schema.from_dict(good_sd), BOTH, weight_key=w, batch_rows=77)
    assert check(eng, oracle(sorted_rows, (), BOTH)) == 5000
