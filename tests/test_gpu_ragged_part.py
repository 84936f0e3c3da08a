"""GPU: the partitioned (multi-GPU) path at ragged partitions, and the PageRank job whose ranks
would each pick another fixed-point range.

Ranks are threads of one process over one device (test_gpu_distributed.Ranks / RowRanks); the
inputs and every property the assertions rest on are proven on the CPU by
test_ragged_part_cpu.py.

  * The cross-rank range (tests/ragged.py range_fixture): rank 0 holds one in-row of 32769
    entries, rank 1 holds rows of one entry.  The blocked layout's fixed-point passes are exact
    below 2^7 for the first and below 2^11 for the second, and the sources on rank 1 emit
    contributions in [2^7, 2^11) from update 69 on.  The range is a property of the job (the
    longest in-row of any rank, all-reduced before the layout is built), so every rank flags the
    message, the job re-runs on the fp64 gather and equals exact rational arithmetic — as one GPU
    does with its single range.
  * Ragged partitions (padded_ragged / part_cases): vertices without entries, n_active below
    n_local, rows on every length threshold, a rank of one bitmap word, a rank of the final word,
    a rank with no entry at all, long rows fed from several ranks — BFS, multi-source BFS and
    delta-stepping bit-exact, PageRank within 1e-6 L1 (BASELINE.json north_star).

Paths of the partitioned code these cases reach that test_gpu_distributed.py's on-grid RMAT
graphs never did, and what shows that they ran:
  * the blocked layout built on a rank with no entry (tgo_part_pr_blocked -> sort_rows_device,
    build_cold_blocks_device, pack_supertiles_device with nnz = 0): test_part_pagerank_l1[empty]
    asserts that the last rank holds no entry and no active row and still reports the layout
    (hot 64, the job's span) its peers report, then runs the blocked updates on it;
  * the frontier extraction of a rank that owns one bitmap word (k_bfs_queue over n_active <= 64
    after a bottom-up level): test_part_bfs_extracts_a_one_word_frontier reads the driver's level
    trace and finds a top-down level after a bottom-up one;
  * a long row gathered from ghosts of several ranks (part_ghost.hip): the CPU file proves that
    the 4097-entry in-row draws sources from two ranks or more at every multi-rank partition, and
    test_part_pagerank_l1 asserts that the ghost exchange moved bytes, fewer than the slices.
"""
import functools

import numpy as np
import pytest

import fulgora as fr
from ragged import (BIG, RANGE_S, draw_seeds, padded_ragged, part_case, part_cases, range_contributions, range_fixture,
                    range_reference)
from test_gpu_distributed import Ranks, RowRanks
from test_gpu_ragged import sssp_seeds
from titan_amd import Engine, Schema, trace
from titan_amd import _lib as L
from titan_amd.distributed import (NativeExchange, PR_EXCHANGE_ALLGATHER, PR_EXCHANGE_GHOST, distributed_bfs,
                                   distributed_bfs_native, distributed_msbfs_native, distributed_pagerank,
                                   distributed_pagerank_native, distributed_sssp, distributed_sssp_native,
                                   pagerank_layout)

pytestmark = pytest.mark.gpu

OUT, IN, BOTH = L.SCOPE_OUT_E, L.SCOPE_IN_E, L.SCOPE_BOTH_E
ABSENT = L.DIST_ABSENT
PR_L1_TOL = 1e-6      # north_star: PageRank within 1e-6 L1
SEED = 7


# ----------------------------------------------------------------------------- the cross-rank range
RANGE_ALPHA = 2.5
RANGE_RTOL = 1e-9     # as test_partitioned_pagerank_out_of_range_reruns_plain


@functools.lru_cache(maxsize=None)
def range_ranks():
    n, src, dst, _ = range_fixture()
    return Ranks(2, n, src, dst, IN, layout=True), NativeExchange.local_group(2)


def range_runs(ranks, xs, n, iters):
    """{name: (ranks, exact_reruns per rank, bytes received over all ranks)} of the three drivers."""
    out = {}
    for name, mode in (("allgather", PR_EXCHANGE_ALLGATHER), ("ghost", PR_EXCHANGE_GHOST)):
        res = ranks.run(lambda be, comm: distributed_pagerank_native(be, RANGE_ALPHA, n, iters, xs[comm.rank], mode=mode))
        out[name] = (np.concatenate([x[0] for x in res]), {be.e.stats()["exact_reruns"] for be in ranks.backends},
                     sum(x[1] for x in res))
    py = ranks.run(lambda be, comm: distributed_pagerank(be, RANGE_ALPHA, n, iters, comm=comm))
    out["python"] = (np.concatenate(py), {be.e.stats()["exact_reruns"] for be in ranks.backends}, None)
    return out


def assert_range_values(pr, ref, what):
    assert np.array_equal(np.isfinite(pr), np.isfinite(ref)), what
    fin = np.isfinite(ref)
    worst = float(np.max(np.abs(pr[fin] - ref[fin]) / np.abs(ref[fin])))
    print(f"{what}: p_t = {pr[0]!r} (exact {ref[0]!r}), p_s = {pr[RANGE_S]!r} (exact {ref[RANGE_S]!r}), "
          f"worst relative error {worst:.3e}")
    assert np.allclose(pr[fin], ref[fin], rtol=RANGE_RTOL, atol=0), (what, worst)


def test_range_is_agreed_across_ranks(monkeypatch):
    """T = 80: rank 0 reads c_69 .. c_79 above its own limit 2^7 while every one of them is
    inside rank 1's own limit 2^11 (test_ragged_part_cpu.py proves both).  With a range per rank
    nothing flagged them: the split sums of the 32769-entry row wrapped past 2^63, exact_reruns
    was 0 on both ranks in all three drivers and p_t came back as 12850342.47 where exact
    arithmetic gives -112978777.53 (measured on an MI355X before the fix).  With the agreed range
    every rank re-runs and p_t = -112978777.52780546 (worst relative error 6.6e-16)."""
    monkeypatch.setenv("TGO_PR_HOT", "512")
    monkeypatch.delenv("TGO_PR_SEG", raising=False)       # 256-source segments would cut the row too short to wrap
    n, src, dst, t = range_fixture()
    iters = 80
    ref = range_reference(iters)
    ranks, xs = range_ranks()
    runs = range_runs(ranks, xs, n, iters)
    for name, (pr, reruns, _) in runs.items():
        print(f"{name}: exact_reruns {sorted(reruns)}, p_t = {pr[t]!r} (exact {ref[t]!r})")
    for name, (pr, reruns, _) in runs.items():
        assert reruns == {1}, (name, reruns)
        assert_range_values(pr, ref, name)
    assert np.array_equal(runs["allgather"][0], runs["ghost"][0])
    # one GPU has a single range, from the same 32769-entry row: it already re-runs
    one = Engine().load_edges(n, src, dst, IN)
    pr1 = one.pagerank(RANGE_ALPHA, n, iters)
    assert one.stats()["exact_reruns"] == 1
    assert_range_values(pr1, ref, "one GPU")
    # the re-run is a plain rank-major all-gather per update in either mode: the bytes of the
    # discarded blocked run are not reported, so the job moved what ranks that never had a
    # blocked layout move
    monkeypatch.setenv("TGO_PR_BLOCKED", "0")
    plain_ranks = Ranks(2, n, src, dst, IN, layout=True)
    res = plain_ranks.run(lambda be, comm: distributed_pagerank_native(be, RANGE_ALPHA, n, iters, xs[comm.rank],
                                                                        mode=PR_EXCHANGE_ALLGATHER))
    assert {be.e.stats()["exact_reruns"] for be in plain_ranks.backends} == {0}
    assert_range_values(np.concatenate([x[0] for x in res]), ref, "plain layout")
    plain_bytes = sum(x[1] for x in res)
    assert plain_bytes == 2 * (iters - 1) * RANGE_S * 8
    print(f"exchanged bytes: plain {plain_bytes}, allgather {runs['allgather'][2]}, ghost {runs['ghost'][2]}")
    assert runs["allgather"][2] == plain_bytes and runs["ghost"][2] == plain_bytes


def test_range_control_stays_blocked(monkeypatch):
    """T = 60: no contribution reaches 2^7, so the agreed range flags nothing and the job stays
    on the blocked fixed-point passes (the agreement does not simply force every job onto fp64)."""
    monkeypatch.setenv("TGO_PR_HOT", "512")
    monkeypatch.delenv("TGO_PR_SEG", raising=False)
    n, src, dst, t = range_fixture()
    iters = 60
    assert max(abs(c) for c in range_contributions(iters)) < 2 ** 7
    ref = range_reference(iters)
    ranks, xs = range_ranks()
    runs = range_runs(ranks, xs, n, iters)
    for name, (pr, reruns, _) in runs.items():
        assert reruns == {0}, (name, reruns)
        assert_range_values(pr, ref, name)
    assert np.array_equal(runs["allgather"][0], runs["ghost"][0])
    assert 0 < runs["ghost"][2] < runs["allgather"][2]    # the blocked layout and its ghost lists ran


# ----------------------------------------------------------------------------- ragged partitions
WORLD = {"equal2": 2, "equal4": 4, "single": 1, "one_word": 2, "last_word": 3, "balanced4": 4, "empty": 3}
# (n, partition, degree-grouped layout): every partition with the layout the bench loads, and
# the world-2 ones in plain slot order too
PARTS = [(n, name, True) for n in BIG for name, _ in part_cases(padded_ragged(n, SEED)[0], *padded_ragged(n, SEED)[1:3])]
PARTS += [(n, name, False) for n, name, _ in PARTS if WORLD[name] == 2]


class PartGraph:
    """padded_ragged(n) with its oracles (one per vertex count: the `empty` partition appends a
    word of pads) and their results, computed once and never written to."""

    def __init__(self, n):
        self.n = n
        self.P, self.src, self.dst, self.w, self.info = padded_ragged(n, SEED)
        self._og, self._sd, self._pr = {}, {}, {}

    def part(self, name):
        return part_case(self.P, self.src, self.dst, name)

    def oracle(self, N):
        if N not in self._og:
            self._og[N] = fr.OracleGraph.from_edges(N, self.src, self.dst, self.w)
        return self._og[N]

    def sd(self, N, v, scope, weighted=False):
        key = (N, int(v), scope, weighted)
        if key not in self._sd:
            d = self.oracle(N).shortest_distance((int(v) + 1) << 3, N, scope, weighted=weighted)[0]
            d.setflags(write=False)
            self._sd[key] = d
        return self._sd[key]

    def pr(self, N, iters):
        if (N, iters) not in self._pr:
            p = self.oracle(N).pagerank(0.85, self.n, iters)[0]
            p.setflags(write=False)
            self._pr[(N, iters)] = p
        return self._pr[(N, iters)]

    def top_rungs(self):
        r = self.info["rungs"]
        return list(r[max(r)])

    def bfs_seeds(self, N):
        s = [self.info["hub"], int(self.info["isolated"][0])] + self.top_rungs() + [self.n - 1, N - 1]
        assert N - 1 >= self.n                                 # the last seed is a pad
        return list(dict.fromkeys(s))


@functools.lru_cache(maxsize=None)
def graph(n):
    return PartGraph(n)


@functools.lru_cache(maxsize=None)
def ranks_for(n, name, scope, weighted, layout, device_counts=False):
    g = graph(n)
    part = g.part(name)
    return Ranks(part.world, part.n, g.src, g.dst, scope, weight=g.w if weighted else None, layout=layout,
                 device_counts=device_counts, part=part)


@functools.lru_cache(maxsize=None)
def exchange(world):
    return NativeExchange.local_group(world)


def cut(part, per_rank):
    """The ranks' slot-local results in caller order (real vertices, then the pads)."""
    out = np.concatenate([part.slot_results(r, x) for r, x in enumerate(per_rank)])
    assert len(out) == part.n
    return out


def slots(part, vs):
    return [int(s) for s in part.to_slots(np.asarray(vs, np.int64))]


def reached(d):
    return int((d != ABSENT).sum())


@pytest.mark.parametrize("n,name,layout", PARTS)
def test_part_bfs_bit_exact(n, name, layout):
    g = graph(n)
    part = g.part(name)
    N, ns = part.n, part.n_slots
    ranks, xs = ranks_for(n, name, BOTH, False, layout), exchange(part.world)
    assert any(be.active_rows() < be.n_local for be in ranks.backends)
    for v in g.bfs_seeds(N):
        od = g.sd(N, v, BOTH)
        s, = slots(part, [v])
        for alpha in (15.0, 1e9):                              # direction-optimizing, and top-down only
            res = ranks.run(lambda be, comm: distributed_bfs_native(be, s, ns, xs[comm.rank], alpha=alpha))
            py = ranks.run(lambda be, comm: distributed_bfs(be, s, ns, alpha=alpha, comm=comm))
            for drv, out in (("native", res), ("python", py)):
                assert np.array_equal(cut(part, [x[0] for x in out]), od), (drv, v, alpha)
                assert all(x[1][0] == reached(od) for x in out), (drv, v, alpha)
                assert len({x[2] for x in out}) == 1, (drv, v, alpha)
            assert res[0][2] == py[0][2], (v, alpha)           # the same levels
    assert reached(g.sd(N, N - 1, BOTH)) == 1 == reached(g.sd(N, int(g.info["isolated"][0]), BOTH))


def test_part_bfs_extracts_a_one_word_frontier(tmp_path):
    """From the hub with beta = 2 the native loop runs bottom-up levels and then turns top-down
    again, so every rank extracts its frontier bitmap into a queue over its active rows — on the
    rank that owns one word that is a scan of a single, partly filled bitmap word."""
    n, name = 4099, "one_word"
    g = graph(n)
    part = g.part(name)
    ranks, xs = ranks_for(n, name, BOTH, False, True), exchange(part.world)
    assert 0 < ranks.backends[0].active_rows() <= 64 < ranks.backends[1].active_rows()
    s, = slots(part, [g.info["hub"]])
    path = str(tmp_path / "trace.json")
    trace.enable(path)
    trace.clear()
    try:
        res = ranks.run(lambda be, comm: distributed_bfs_native(be, s, part.n_slots, xs[comm.rank], alpha=15.0, beta=2.0))
        trace.flush()
    finally:
        trace.disable()
    assert np.array_equal(cut(part, [x[0] for x in res]), g.sd(part.n, g.info["hub"], BOTH))
    by_level = {}
    for e in trace.load_events(path):
        if e["name"] == "part.bfs.level":
            by_level.setdefault(e["args"]["level"], set()).add(e["args"]["bottom_up"])
    assert all(len(v) == 1 for v in by_level.values()), by_level       # the ranks agree on each level's direction
    bu = [by_level[k].copy().pop() for k in sorted(by_level)]
    assert len(bu) == res[0][2]
    assert any(a == 1 and b == 0 for a, b in zip(bu, bu[1:])), bu


def check_part_msbfs(g, part, ranks, xs, seeds):
    N, ns = part.n, part.n_slots
    ss = slots(part, seeds)

    def body(be, comm):
        r, _, lv = distributed_msbfs_native(be, ss, ns, xs[comm.rank])
        return r, lv, [be.ms_levels(i) for i in range(len(ss))]
    res = ranks.run(body)
    assert len({x[1] for x in res}) == 1
    for i, v in enumerate(seeds):
        od = g.sd(N, int(v), BOTH)
        assert np.array_equal(cut(part, [x[2][i] for x in res]), od), (i, int(v))
        assert all(x[0][i] == reached(od) for x in res), (i, int(v))


@pytest.mark.parametrize("n,name,layout", PARTS)
def test_part_multi_source_bfs_bit_exact(n, name, layout):
    g = graph(n)
    part = g.part(name)
    xs = exchange(part.world)
    for dc in ((False, True) if part.world == 2 else (False,)):
        ranks = ranks_for(n, name, BOTH, False, layout, dc)
        for nseeds in (1, 63, 64):
            check_part_msbfs(g, part, ranks, xs, draw_seeds(n, g.info, nseeds, SEED))


@pytest.mark.parametrize("n,name,layout,scope", [(n, name, lay, s) for n, name, lay in PARTS
                                                 for s in (IN, OUT) + ((BOTH,) if WORLD[name] == 2 else ())])
def test_part_delta_stepping_bit_exact(n, name, layout, scope):
    g = graph(n)
    part = g.part(name)
    N = part.n
    ranks, xs = ranks_for(n, name, scope, True, layout), exchange(part.world)
    for v in sssp_seeds(g):
        od = g.sd(N, v, scope, weighted=True)
        s, = slots(part, [v])
        for delta in (0, 9):
            res = ranks.run(lambda be, comm: distributed_sssp_native(be, s, xs[comm.rank], delta=delta))
            py = ranks.run(lambda be, comm: distributed_sssp(be, s, delta, comm=comm))
            for drv, out in (("native", res), ("python", py)):
                assert np.array_equal(cut(part, [x[0] for x in out]), od), (drv, v, delta)
                assert all(x[1][0] == reached(od) for x in out), (drv, v, delta)
                assert len({x[2] for x in out}) == 1, (drv, v, delta)    # the same phases on every rank


@pytest.mark.parametrize("n,name,layout", PARTS)
def test_part_pagerank_l1(n, name, layout, monkeypatch):
    g = graph(n)
    part = g.part(name)
    N, W = part.n, part.world
    ranks, xs = ranks_for(n, name, IN, True, layout), exchange(W)
    for env in ({"TGO_PR_HOT": 64 * W, "TGO_PR_SEG": 256}, {"TGO_PR_BLOCKED": 0}):
        for k, v in env.items():
            monkeypatch.setenv(k, str(v))
        lays = set(ranks.run(lambda be, comm: pagerank_layout(be, comm=comm)))
        # every rank agrees on the layout (the empty rank builds the blocked one from no entry)
        span = max(be.active_rows() for be in ranks.backends)
        assert lays == ({(0, part.slot)} if "TGO_PR_BLOCKED" in env else {(64, span)}), (env, lays)
        if name == "empty":                                    # ... which is what its last rank holds
            assert ranks.backends[-1].total_entries == 0 and ranks.backends[-1].active_rows() == 0
        for iters in (2, 20):
            opr = g.pr(N, iters)
            fin = np.isfinite(opr)
            got, moved = {}, {}
            for drv in ("allgather", "ghost", "python"):
                for again in (False, True):
                    if drv == "python":
                        res = ranks.run(lambda be, comm: distributed_pagerank(be, 0.85, n, iters, comm=comm))
                    else:
                        mode = PR_EXCHANGE_GHOST if drv == "ghost" else PR_EXCHANGE_ALLGATHER
                        nat = ranks.run(lambda be, comm: distributed_pagerank_native(be, 0.85, n, iters, xs[comm.rank],
                                                                                    mode=mode))
                        res, moved[drv] = [x[0] for x in nat], sum(x[1] for x in nat)
                    pr = cut(part, res)
                    assert {be.e.stats()["exact_reruns"] for be in ranks.backends} == {0}, (env, iters, drv)
                    assert np.array_equal(np.isfinite(pr), fin), (env, iters, drv)
                    l1 = float(np.abs(pr[fin] - opr[fin]).sum())
                    assert l1 <= PR_L1_TOL, (env, iters, drv, l1)
                    if again:
                        assert np.array_equal(pr, got[drv]), (env, iters, drv)      # bitwise repeatable
                    got[drv] = pr
            assert np.array_equal(got["allgather"], got["ghost"]), (env, iters)
            # the ghost lists ran, and carry less than the slices: the 4097-entry row's sources
            # sit on several ranks (test_ragged_part_cpu.py), so its gather reads ghosts of each
            assert moved["allgather"] == W * (W - 1) * (iters - 1) * lays.copy().pop()[1] * 8, (env, iters)
            if W > 1:
                assert 0 < moved["ghost"] < moved["allgather"], (env, iters, moved)
        for k in env:
            monkeypatch.delenv(k)


# ----------------------------------------------------------------------------- partition from rows
@functools.lru_cache(maxsize=None)
def ragged_rows():
    """Edgestore rows of the padded 1001 graph: one weighted MULTI label, a row per vertex (the
    isolated vertices and the pads hold their VertexExists entry only), weights 1..41."""
    import edgestore as es
    g = graph(1001)
    label, wkey = es.user_edge_label(1), es.user_property_key(1)
    sd = {"edge_types": [{"type_id": label, "multiplicity": 0, "signature": [wkey]}], "property_keys": [[wkey, 3]]}
    osch = fr.OracleSchema(sd["edge_types"], [tuple(x) for x in sd["property_keys"]])
    edges = [(int(s), int(d), label, [(wkey, int(x) + 1)]) for s, d, x in zip(g.src, g.dst, g.w)]
    rows, vids = es.build_rows(es.GraphSpec(n=g.P, edges=edges), osch)
    return rows, vids, sd, osch, wkey


@pytest.mark.parametrize("world", [2, 3])
def test_part_rows_match_one_gpu_rows(world, monkeypatch):
    """tgo_load_partition_rows on the ragged rows (row ranges balanced by entries: the ladder's
    long rows make them unequal, the slots past a rank's live rows are pads): BFS, weighted
    delta-stepping and PageRank equal the one-GPU tgo_load_rows load of the same rows and the
    oracle."""
    monkeypatch.setenv("TGO_PR_HOT", str(64 * world))
    monkeypatch.setenv("TGO_PR_SEG", "256")
    g = graph(1001)
    rows, vids, sd, osch, wkey = ragged_rows()
    n, limit = len(vids), 100000
    seeds = [int(vids[v]) for v in g.bfs_seeds(g.P)]
    for scope in (BOTH, IN):
        one = Engine(hard_query_limit=limit).load_rows(rows, Schema.from_dict(sd), scope, weight_key=wkey)
        o = fr.OracleGraph.from_rows(rows, osch, scope, hard_limit=limit, weight_key=wkey)
        ids1 = one.vertex_ids()
        rr = RowRanks(world, rows, sd, scope, limit, weight_key=wkey)
        assert sum(rr.live) == len(ids1) == n and len(set(rr.live)) > 1       # unequal live rows
        assert one.stats()["truncated_results"] == o.stats.truncated_results == 0
        for s in seeds:
            if scope == BOTH:
                want = one.bfs(s, n, scope)
                assert np.array_equal(want, o.shortest_distance(s, n, scope)[0])
                res = rr.run(lambda be, comm, x: distributed_bfs_native(be, rr.slot[s], rr.n_global, x))
            else:
                want = one.sssp(s, n, scope, mode=L.SSSP_DELTA)
                assert np.array_equal(want, o.shortest_distance(s, n, scope, weighted=True)[0])
                res = rr.run(lambda be, comm, x: distributed_sssp_native(be, rr.slot[s], x))
            assert np.array_equal(rr.gather([r[0] for r in res], ids1), want), (scope, s)
        if scope == IN:
            opr = o.pagerank(0.85, n, 20)[0]
            want = one.pagerank(0.85, n, 20)
            fin = np.isfinite(opr)
            for mode in (PR_EXCHANGE_ALLGATHER, PR_EXCHANGE_GHOST):
                res = rr.run(lambda be, comm, x: distributed_pagerank_native(be, 0.85, n, 20, x, mode=mode))
                got = rr.gather([r[0] for r in res], ids1)
                assert np.array_equal(np.isfinite(got), fin) and np.array_equal(np.isfinite(want), fin)
                assert float(np.abs(got[fin] - opr[fin]).sum()) <= PR_L1_TOL
                assert float(np.abs(want[fin] - opr[fin]).sum()) <= PR_L1_TOL
                assert {be.e.stats()["exact_reruns"] for be in rr.backends} == {0}
