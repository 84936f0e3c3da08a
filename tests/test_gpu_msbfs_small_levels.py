"""Multi-source BFS levels that find little: the sparse push form (TGO_TUNE_MS_SPARSE: the push
queues the vertices it touches and the settle runs over that queue, no pass over every mask),
the stay-in-pull rule (TGO_TUNE_MS_STAY: after a pull level the next one pulls too while the
still-open vertices' list entries are at most gamma x the frontier's entries) and the counters
published and zeroed in one launch.  All of it is policy: every case compares the sweep level
for level with each seed's own single-source run and with the same sweep under
TUNE_MS_SPARSE = 0, TUNE_MS_STAY = 0 (every level dense, the frontier's entries alone decide).
"""
import numpy as np
import pytest

from titan_amd import Engine, TitanException, pick_roots, rmat_edges
from titan_amd import _lib as L

pytestmark = pytest.mark.gpu

OUT, IN, BOTH = L.SCOPE_OUT_E, L.SCOPE_IN_E, L.SCOPE_BOTH_E
HUGE = 1.0e9                      # a sparse fraction no frontier exceeds: every push level sparse
GAMMAS = (1.0, 4.0, 12.0)         # the stay rule's values of the committed A/B


def sweep(eng, seeds, depth, scope, sparse, stay, split=None):
    """One sweep under the given policy: (levels per seed, reached, reached entries, level count)."""
    eng.set_tuning(L.TUNE_MS_SPARSE, sparse).set_tuning(L.TUNE_MS_STAY, stay)
    if split is not None:
        eng.set_tuning(L.TUNE_MS_SPLIT, split)
    d = eng.bfs_multi(seeds, depth, scope, seed_is_dense=True, stats=True)
    r, e = eng.multi_stats(len(seeds))
    return d, r, e, eng.stats()["levels"]


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]


def singles(eng, seeds, depth, scope):
    return np.stack([eng.bfs(int(s), depth, scope, seed_is_dense=True) for s in seeds])


# ----------------------------------------------------------------------------- deep and thin
PATH, ISOLATED = 600, 37


@pytest.mark.parametrize("scope", [BOTH, IN, OUT])
def test_deep_thin_path_every_level_sparse(scope):
    """A 600-vertex path plus 37 entry-less vertices (n = 637, no multiple of 64): every level
    has one or two frontier vertices, so every push level is sparse and the depth crosses several
    level planes.  Seeds at both ends and the middle, a duplicate, and one entry-less vertex."""
    n = PATH + ISOLATED
    src = np.arange(PATH - 1, dtype=np.int32)
    dst = src + 1
    seeds = [0, PATH - 1, PATH // 2, 0, PATH + 20]
    eng = Engine().load_edges(n, src, dst, scope)
    ref = singles(eng, seeds, n, scope)
    assert ref[0].max() == PATH - 1 or ref[1].max() == PATH - 1        # the whole path from one end
    base = sweep(eng, seeds, n, scope, 0.0, 0.0)
    assert np.array_equal(base[0], ref)
    for sparse, stay in ((-1.0, -1.0), (HUGE, 4.0), (HUGE, 0.0)):
        first = sweep(eng, seeds, n, scope, sparse, stay)
        assert same(first, base), (sparse, stay)
        # the sweep ended on an empty sparse level: the next one starts from masks left zero
        assert same(sweep(eng, seeds, n, scope, sparse, stay), base), (sparse, stay)
        # a sweep cut at depth 5 leaves frontier masks behind; the full one after it must not see them
        cut = sweep(eng, seeds, 5, scope, sparse, stay)
        assert np.array_equal(cut[0], singles(eng, seeds, 5, scope)), (sparse, stay)
        assert same(sweep(eng, seeds, n, scope, sparse, stay), base), (sparse, stay)
        # other seeds on the same engine after a clean end
        other = [PATH // 3, PATH + 1, 7]
        got = sweep(eng, other, n, scope, sparse, stay)
        assert np.array_equal(got[0], singles(eng, other, n, scope)), (sparse, stay)
        assert same(sweep(eng, seeds, n, scope, sparse, stay), base), (sparse, stay)


# ----------------------------------------------------------------------------- RMAT-12
@pytest.fixture(scope="module")
def rmat12():
    n = 1 << 12
    src, dst, _ = rmat_edges(12, 16, seed=0x54495441)
    eng = Engine().load_edges(n, src, dst, BOTH)
    seeds = pick_roots(n, src, dst, 64, seed=29)
    deg = np.bincount(src, minlength=n) + np.bincount(dst, minlength=n)
    top = np.argsort(deg, kind="stable")[-64:]
    return n, src, dst, eng, seeds, singles(eng, seeds, n, BOTH), top, singles(eng, top, n, BOTH)


@pytest.mark.parametrize("split", [0.0, -1.0])
def test_rmat12_sparse_fraction_is_policy_only(rmat12, split):
    """64 seeds, sparse fraction 0 / default / huge with the source split off and on.  The huge
    fraction makes the hub level sparse too: thousands of contributions to one mask word go
    through the returning atomic and exactly one of them queues the vertex, and the touched list
    (longer than a block) is appended wave by wave.  Levels, per-source stats and the level count
    are identical."""
    n, src, dst, eng, seeds, ref, _, _ = rmat12
    base = sweep(eng, seeds, n, BOTH, 0.0, 0.0, split)
    assert np.array_equal(base[0], ref)
    for sparse in (-1.0, HUGE):
        for stay in (0.0, -1.0):
            assert same(sweep(eng, seeds, n, BOTH, sparse, stay, split), base), (sparse, stay, split)
    eng.set_tuning(L.TUNE_MS_SPLIT, -1.0)


@pytest.mark.parametrize("scope", [IN, OUT])
def test_rmat12_directed_scopes(rmat12, scope):
    n, src, dst, _, seeds, _, _, _ = rmat12
    eng = Engine().load_edges(n, src, dst, scope)
    base = sweep(eng, seeds, n, scope, 0.0, 0.0)
    assert np.array_equal(base[0], singles(eng, seeds, n, scope))
    for sparse, stay in ((-1.0, -1.0), (HUGE, 12.0)):
        assert same(sweep(eng, seeds, n, scope, sparse, stay), base), (sparse, stay)


def test_top_degree_seeds_sparse_level0(rmat12):
    """The 64 top-degree vertices as seeds: level 0 is sparse by definition and touches most of the
    graph (a large touched list from a 64-entry queue)."""
    n, src, dst, eng, _, _, top, ref = rmat12
    base = sweep(eng, top, n, BOTH, 0.0, 0.0)
    assert np.array_equal(base[0], ref)
    for sparse in (-1.0, HUGE):
        assert same(sweep(eng, top, n, BOTH, sparse, -1.0), base), sparse


# ----------------------------------------------------------------------------- tail and dead source
TAIL = 40


@pytest.fixture(scope="module")
def tailed():
    """RMAT-12 with a 40-vertex path hung on its top-degree vertex (many tiny levels after the
    dense ones) and a separate 3-vertex component; n = 4139."""
    n0 = 1 << 12
    src, dst, _ = rmat_edges(12, 16, seed=0x54495441)
    deg = np.bincount(src, minlength=n0) + np.bincount(dst, minlength=n0)
    hub = int(np.argmax(deg))
    tail = np.arange(n0, n0 + TAIL, dtype=np.int32)
    comp = np.arange(n0 + TAIL, n0 + TAIL + 3, dtype=np.int32)
    src2 = np.concatenate([src, [hub], tail[:-1], comp[:-1]]).astype(np.int32)
    dst2 = np.concatenate([dst, [tail[0]], tail[1:], comp[1:]]).astype(np.int32)
    n = n0 + TAIL + 3
    eng = Engine().load_edges(n, src2, dst2, BOTH)
    seeds = [int(s) for s in pick_roots(n0, src, dst, 63, seed=31)]
    return n, eng, seeds, int(comp[1]), int(tail[-1])


@pytest.mark.parametrize("with_dead", [False, True])
def test_tail_levels_under_the_stay_rule(tailed, with_dead):
    """After the dense pull levels the sweep walks the 40-vertex tail one vertex a level: the
    stay rule decides each of those levels (mu against gamma x mf), for every gamma of the A/B.
    with_dead: one seed sits in the separate 3-vertex component, so every vertex of the giant
    component stays open for that source for the whole sweep and mu stays large — the rule must
    not fire wrongly, and the result is the same."""
    n, eng, seeds, dead, tail_end = tailed
    sd = seeds + [dead if with_dead else tail_end]
    ref = singles(eng, sd, n, BOTH)
    assert ref[:63].max() >= TAIL                       # the tail is walked to its end
    if with_dead:
        assert (ref[63] >= 0).sum() == 3
    base = sweep(eng, sd, n, BOTH, 0.0, 0.0)
    assert np.array_equal(base[0], ref)
    for gamma in GAMMAS + (HUGE,):
        for sparse in (0.0, -1.0, HUGE):
            assert same(sweep(eng, sd, n, BOTH, sparse, gamma), base), (gamma, sparse)
    # cut inside the tail, then full: the stay rule and the clean flags across sweeps
    cut = sweep(eng, sd, 9, BOTH, -1.0, -1.0)
    assert np.array_equal(cut[0], singles(eng, sd, 9, BOTH))
    assert same(sweep(eng, sd, n, BOTH, -1.0, -1.0), base)


def test_new_tuning_keys_reject_out_of_range(rmat12):
    eng = rmat12[3]
    for key in (L.TUNE_MS_STAY, L.TUNE_MS_SPARSE):
        for bad in (-0.5, -2.0, float("nan"), float("inf")):
            with pytest.raises(TitanException):
                eng.set_tuning(key, bad)
        eng.set_tuning(key, 0.0).set_tuning(key, 3.5).set_tuning(key, -1.0)
    with pytest.raises(TitanException):
        eng.set_tuning(99, 0.0)
