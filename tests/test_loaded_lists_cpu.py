"""CPU: the reference half of tests/loaded_lists.py against edges the test chose itself.

The GPU tests compare a load's lists with OracleGraph.export through that helper; here the
helper's oracle side is pinned to the GraphSpec the rows were built from, so the reference cannot
agree with a wrong decoder by being wrong the same way: every edge once as OUT on its source row
and once as IN on its target row, its Integer weight or INT32_MIN, for the mixed schema (one label
per multiplicity, sort key / signature / remaining weights, typed scopes) and for an untyped
single-direction load cut at a small hard limit."""
import random

import numpy as np
import pytest

import edgestore as es
import fulgora as fr
import loaded_lists as ll
from titan_amd import _lib as L

OUT, IN, BOTH = L.SCOPE_OUT_E, L.SCOPE_IN_E, L.SCOPE_BOTH_E


def mixed_case():
    rnd = random.Random(11)
    n = 300
    sd, osch, w, labels = ll.mixed_schema()
    spec = es.GraphSpec(n=n, edges=ll.mixed_edges(rnd, n, 3000), schema_rows=2, pv_ghost=[17, 150])
    rows, vids = es.build_rows(spec, osch)
    return spec, rows, vids, osch, w, labels


MIXED = mixed_case()


@pytest.mark.parametrize("scope", [OUT, IN, BOTH])
@pytest.mark.parametrize("typed", [0, 1, 2])
def test_oracle_lists_of_the_mixed_schema_are_the_spec(scope, typed):
    spec, rows, vids, osch, w, labels = MIXED
    chosen = tuple([(), (labels[2],), (labels[0], labels[3])][typed])
    o = fr.OracleGraph.from_rows(rows, osch, scope, labels=chosen, weight_key=w)
    assert o.n == spec.n - 2 and o.stats.ghost_vertices == 2 and o.stats.skipped_rows == 2
    assert o.stats.truncated_results == 0            # typed or bothE: no limit; untyped at 100000: none reached
    got = ll.oracle_entries(o)
    want = ll.spec_entries(spec, vids, w, labels=chosen, dead=spec.pv_ghost)
    kept = 0
    for d in (0, 1):
        assert np.array_equal(got[d], want[d]), ll._first_difference(got[d], want[d])
        kept += len(got[d])
    absent = (want[0][:, 3] == ll.MISSING).sum()            # absent weights are among the compared entries
    assert 0.1 * len(want[0]) < absent < 0.2 * len(want[0])
    # every entry of a chosen label on a live row was decoded; those towards the two ghosts are dropped
    live = [(s, d) for (s, d, lab, _) in spec.edges if not chosen or lab in chosen]
    dangling = sum((s in spec.pv_ghost) != (d in spec.pv_ghost) for s, d in live)
    assert ll.oracle_dangling(o) == dangling > 0
    assert o.stats.num_entries == kept + dangling


def column_order(entries):
    """One MULTI label without a sort key: a row's columns sort by (direction, other id, relation id)
    (IDHandler.writeRelationType keeps the direction in the type varint; EdgeSerializer.java:255-259
    writes other id and relation id in an order-preserving form)."""
    return sorted(entries, key=lambda e: (e[1], e[2], e[4]))


@pytest.mark.parametrize("scope", [IN, OUT])
def test_oracle_lists_of_a_cut_untyped_load_are_the_spec(scope):
    lib = fr.load()
    knows, w = lib.fr_schema_id(2, 1), lib.fr_schema_id(0, 1)
    ets = [{"type_id": knows, "multiplicity": 0}]
    osch = fr.OracleSchema(ets, [(w, 3)])
    rnd = random.Random(23)
    n, limit = 60, 5
    edges = [(rnd.randrange(n), rnd.randrange(n), knows, [(w, rnd.randrange(-99, 99))] if rnd.random() > 0.15 else [])
             for _ in range(400)]
    spec = es.GraphSpec(n=n, edges=edges, pv_ghost=[7], schema_rows=1)
    rows, vids = es.build_rows(spec, osch)
    o = fr.OracleGraph.from_rows(rows, osch, scope, hard_limit=limit, weight_key=w)
    # per row: every entry in column order (relation ids follow the edge index), cut at the limit,
    # then the entries towards the ghost dropped
    per_row = {int(v): [] for i, v in enumerate(vids) if i != 7}
    for k, (s, d, _, props) in enumerate(edges):
        x = dict(props).get(w, ll.MISSING)
        if s != 7:
            per_row[int(vids[s])].append((int(vids[s]), 0, int(vids[d]), x, k))
        if d != 7:
            per_row[int(vids[d])].append((int(vids[d]), 1, int(vids[s]), x, k))
    want, cut = [], 0
    for v, ents in per_row.items():
        cut += len(ents) >= limit
        want += [e[:4] for e in column_order(ents)[:limit] if e[2] != int(vids[7])]
    want = ll._sorted_rows(np.asarray(want, np.int64))
    assert o.stats.truncated_results == cut > 40 and o.stats.ghost_vertices == 1
    got = ll.oracle_entries(o)
    for d in (0, 1):
        assert np.array_equal(got[d], want[want[:, 1] == d]), d
    assert len(got[0]) + len(got[1]) == len(want) < 2 * len(edges)
    assert (want[:, 3] == ll.MISSING).any()
