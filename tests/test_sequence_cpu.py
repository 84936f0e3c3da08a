"""CPU checks of tests/sequence_cases.py: the walk covers every ordered pair once, the graph keeps the
properties test_gpu_sequence.py relies on (asserted from the references alone), and every named call has
a reference that varies over the vertices, so a result left over from another program cannot pass for it."""
import numpy as np
import pytest

import sequence_cases as sc
from sequence_cases import BOTH, IN

N_BASE = 129
COUNTS = sorted({len(sc.calls(BOTH)), len(sc.calls(IN))})


@pytest.fixture(scope="module")
def case():
    return sc.Case.make(N_BASE)


@pytest.mark.parametrize("k", [1, 2, 3] + COUNTS)
def test_pair_walk_is_an_eulerian_circuit(k):
    walk = sc.pair_walk(k)
    assert len(walk) == k * k + 1 and walk[0] == walk[-1]
    pairs = list(zip(walk, walk[1:]))
    assert len(set(pairs)) == k * k
    assert set(pairs) == {(a, b) for a in range(k) for b in range(k)}
    assert walk == sc.pair_walk(k)


def test_the_call_lists_hold_what_the_sequences_need():
    both = [c.name for c in sc.calls(BOTH)]
    ine = [c.name for c in sc.calls(IN)]
    assert len(set(both)) == len(both) == 24 and len(set(ine)) == len(ine) == 13
    for names in (both, ine):
        assert [n for n in names if n.startswith("fails_")] == ["fails_division_by_zero", "fails_wrong_scope"]
    for scope in (BOTH, IN):
        for c in sc.calls(scope):
            assert (c.ref is None) == (c.fails is not None), c


def test_ids_are_strictly_increasing_multiples_of_8(case):
    assert case.N == N_BASE + sc.EXTRA
    assert (np.diff(case.ids) > 0).all() and (case.ids % 8 == 0).all() and case.ids[0] > 0


@pytest.mark.parametrize("scope", [BOTH, IN])
def test_a_sweep_from_the_path_end_is_deep(case, scope):
    d = case.ref(sc.ALL[(scope, "bfs_path_end")])["dist"]
    depth = int(d[d != sc.L.DIST_ABSENT].max())
    print("depth from the path end", depth)
    assert depth >= 17
    multi = case.ref(sc.ALL[(scope, "bfs_multi_3")])["dist"]
    assert np.array_equal(multi[0], d)


def test_components_weak_and_strong(case):
    weak = case.ref(sc.ALL[(BOTH, "components")])
    assert weak["components"] >= 3
    lab = case.ref(sc.ALL[(BOTH, "scc")])["label"]
    _, cnt = np.unique(lab, return_counts=True)
    print("weak", weak["components"], "strong with more than one vertex", int((cnt > 1).sum()))
    assert (cnt > 1).sum() >= 3


def test_triangles_cores_and_trusses(case):
    assert case.ref(sc.ALL[(BOTH, "triangles")])["triangles"] > 0
    core = case.ref(sc.ALL[(BOTH, "kcore")])["core"]
    assert len(np.unique(core)) >= 3
    truss = case.ref(sc.ALL[(BOTH, "ktruss0")])
    assert truss["max_truss"] >= 4
    clamped = case.ref(sc.ALL[(BOTH, "ktruss4")])
    assert clamped["max_truss"] == 4 and np.array_equal(clamped["vtruss"], np.minimum(truss["vtruss"], 4))


def test_the_failing_gather_reads_a_zero_weight(case):
    # bothE reads every entry of both lists, inE every edge once over its head's IN list
    assert (case.w == 0).any()
    d = case.ref(sc.ALL[(BOTH, "bfs_isolated")])
    assert d["reached"] == 1                                  # an isolated vertex
    deg = np.bincount(case.src, minlength=case.N) + np.bincount(case.dst, minlength=case.N)
    assert deg[case.marks["isolated"]] == 0


@pytest.mark.parametrize("scope", [BOTH, IN])
def test_every_call_has_a_reference_that_varies(case, scope):
    for c in sc.calls(scope):
        if c.fails is not None:
            continue
        want = case.ref(c)
        if c.constant_by_contract:                            # pagerank(.., 0): no PAGE_RANK property anywhere
            assert np.isnan(want["pr"]).all()
            continue
        assert sc.varies(want), c
        c.check(want, want)                                   # a reference passes its own comparison


def test_the_graph_in_another_row_order_has_the_same_results(case):
    """Case.reordered (the row order of an edgestore load) renames the vertices and nothing else."""
    rng = np.random.default_rng(11)
    p = rng.permutation(case.N)
    ids = np.empty(case.N, np.int64)
    ids[p] = case.ids
    other = case.reordered(p, ids)
    for name in ("bfs_path_end", "components", "kcore", "scc"):
        a, b = case.ref(sc.ALL[(BOTH, name)]), other.ref(sc.ALL[(BOTH, name)])
        key = "dist" if name == "bfs_path_end" else [k for k in a if isinstance(a[k], np.ndarray)][0]
        assert np.array_equal(a[key], b[key][p]), name
