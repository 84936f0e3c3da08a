"""GPU: what every program's epilogue leaves in tgo_stats (iterations, levels, last_kernel_ms),
and the copy-out of a result that stayed on the device.

The graph is the smallest at which these paths differ from trivial: 67 vertices (one past a
wave) and 300 random weighted edges from a fixed seed, loaded once bothE and once inE.  The
iteration counts are those of the programs' definitions (rounds, levels, max_iterations, k); the
traversals' iterations and levels are literals read once from the library of the commit that
introduced this file, before the epilogue code was unified (but for the phase count of DELTA mode,
which no library reproduces: see TRAVERSALS).  last_kernel_ms is only required to be a finite
positive time.
"""
import ctypes as C
import math

import numpy as np
import pytest

from titan_amd import Engine
from titan_amd import _lib as L

pytestmark = pytest.mark.gpu

N, M, SEED = 67, 300, 20261020
SCOPES = {"bothE": L.SCOPE_BOTH_E, "inE": L.SCOPE_IN_E}

# (iterations, levels) of tgo_bfs / tgo_sssp HOP_BOUNDED / tgo_sssp DELTA (delta 9) from ROOT with
# max_depth N, per load scope.  DELTA's levels are the phases of the device loop, whose concurrent
# relaxations make the count vary from run to run on one library (15 and 16, 24 and 25 were seen for
# the same call; the loop's bucket and extraction counts differ between two runs of the library these
# literals were read from): None stands for "at least one phase", and the distances are compared
# with the converged HOP_BOUNDED ones instead.
TRAVERSALS = {
    ("bothE", "bfs"): (67, 4),
    ("bothE", "sssp_hop"): (67, 9),
    ("bothE", "sssp_delta"): (67, None),
    ("inE", "bfs"): (67, 6),
    ("inE", "sssp_hop"): (67, 7),
    ("inE", "sssp_delta"): (67, None),
}


def graph():
    rng = np.random.default_rng(SEED)
    src = rng.integers(0, N, M).astype(np.int32)
    dst = rng.integers(0, N, M).astype(np.int32)
    w = rng.integers(1, 41, M).astype(np.int32)
    return src, dst, w


def root():
    src, dst, _ = graph()
    return int(np.argmax(np.bincount(src, minlength=N) + np.bincount(dst, minlength=N)))


ROOT = root()


@pytest.fixture(scope="module", params=sorted(SCOPES))
def loaded(request):
    src, dst, w = graph()
    eng = Engine().load_edges(N, src, dst, SCOPES[request.param], weight=w)
    assert eng.n == N
    yield request.param, eng
    eng.close()


@pytest.fixture(scope="module")
def both():
    src, dst, w = graph()
    eng = Engine().load_edges(N, src, dst, L.SCOPE_BOTH_E, weight=w)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def ine():
    src, dst, w = graph()
    eng = Engine().load_edges(N, src, dst, L.SCOPE_IN_E, weight=w)
    yield eng
    eng.close()


def stats_of(eng, what):
    st = eng.stats()
    print(f"{what}: iterations {st['iterations']} levels {st['levels']} last_kernel_ms {st['last_kernel_ms']!r}")
    assert math.isfinite(st["last_kernel_ms"]) and st["last_kernel_ms"] > 0, what
    return st


def copy_distances(eng, dtype=np.int64):
    out = np.zeros(eng.n, np.int64)
    assert eng.lib.tgo_copy_distances(eng.ctx, L.ptr(out, C.c_int64)) == 0
    return out.view(dtype)


def traversal(eng, scope, name, fetch=True):
    if name == "bfs":
        return eng.bfs(ROOT, N, scope, seed_is_dense=True, fetch=fetch)
    mode, delta = (L.SSSP_DELTA, 9) if name == "sssp_delta" else (L.SSSP_HOP_BOUNDED, 0)
    return eng.sssp(ROOT, N, scope, mode=mode, seed_is_dense=True, fetch=fetch, delta=delta)


# ------------------------------------------------------------------ the analytics (bothE)
def test_components_iterations_are_its_rounds(both):
    label, info = both.components()
    assert stats_of(both, "components")["iterations"] == info["rounds"]
    _, again = both.components(fetch=False)
    assert again["components"] == info["components"]
    assert np.array_equal(both.copy_components(), label)


def test_triangles_is_one_iteration(both):
    tri, info = both.triangles()
    assert stats_of(both, "triangles")["iterations"] == 1
    _, again = both.triangles(fetch=False)
    assert again == info
    assert np.array_equal(both.copy_triangles()[0], tri)


def test_kcore_iterations_are_its_levels(both):
    core, info = both.kcore()
    assert stats_of(both, "kcore")["iterations"] == info["levels"]
    _, again = both.kcore(fetch=False)
    assert again["levels"] == info["levels"]
    assert np.array_equal(both.copy_cores(), core)


# ------------------------------------------------------------------ PageRank, DegreeCounter (inE)
@pytest.mark.parametrize("iters", [0, 1, 5])
def test_pagerank_iterations(ine, iters):
    pr = ine.pagerank(0.85, N, iters)
    assert stats_of(ine, f"pagerank({iters})")["iterations"] == iters
    assert ine.pagerank(0.85, N, iters, fetch=False) is None
    assert stats_of(ine, f"pagerank({iters}, on the device)")["iterations"] == iters
    # the ranks stay in the distance scratch; bit patterns, so iteration 0's NaNs compare too
    assert np.array_equal(copy_distances(ine), pr.view(np.int64))
    assert np.isfinite(pr).all() if iters else np.isnan(pr).all()


def test_walkcount_iterations(ine):
    out = ine.walkcount(3)
    assert stats_of(ine, "walkcount(3)")["iterations"] == 3
    assert out.dtype == np.int32 and (out >= 0).all()


# ------------------------------------------------------------------ the traversals (both loads)
@pytest.mark.parametrize("name", ["bfs", "sssp_hop", "sssp_delta"])
def test_traversal_iterations_and_levels(loaded, name):
    key, eng = loaded
    iterations, levels = TRAVERSALS[(key, name)]

    def check_stats(what):
        st = stats_of(eng, what)
        assert st["iterations"] == iterations
        assert st["levels"] == levels if levels is not None else st["levels"] >= 1

    dist = traversal(eng, SCOPES[key], name)
    check_stats(f"{key} {name}")
    assert dist[ROOT] == 0
    assert traversal(eng, SCOPES[key], name, fetch=False) is None
    check_stats(f"{key} {name} (on the device)")
    assert np.array_equal(copy_distances(eng), dist)
    if name == "sssp_delta":        # N hops reach every shortest path of 67 vertices
        assert np.array_equal(dist, traversal(eng, SCOPES[key], "sssp_hop"))
