"""CPU: what the partitioned device tests (test_gpu_ragged_part.py) rest on, proven without a
device.

  * The cross-rank range fixture (ragged.range_fixture): the limits the two ranks would each
    derive from their own rows, where the sources' contributions lie relative to both (from the
    exact recurrence), and the oracle against exact rational arithmetic.
  * The ragged partitions (ragged.padded_ragged / part_cases): per partition, which rank holds
    the hub, an isolated vertex and the largest rungs, that the longest rows cross ranks, that
    the one-word rank, the final-word rank and the empty rank hold what they are named for, and
    that some rank has active rows short of its slots.  The Python drivers then run over the numpy
    backend (test_distributed.NumpyPartBackend) and thread ranks on a world-2 partition and on
    the empty-rank partition against the oracle: expected values and the slot mapping are right
    before anything runs on a device.
"""
import functools

import numpy as np
import pytest

import fulgora as fr
from ragged import (BIG, RANGE_ALPHA, RANGE_D, RANGE_S, owner, padded_ragged, part_case, part_cases,
                    range_contributions, range_fixture, range_reference)
from test_distributed import NumpyPartBackend
from titan_amd.distributed import InProcessGroup, distributed_bfs, distributed_pagerank, distributed_sssp

OUT, IN, BOTH = 0, 1, 2
ABSENT = fr.FR_ABSENT
PR_L1_TOL = 1e-6      # north_star: PageRank within 1e-6 L1
SEED = 7


# ----------------------------------------------------------------------------- the cross-rank range
def fx_limit_log2(max_len):
    """titan_amd/csrc/api_load.cpp fx_range, restated: with 2^c the first power of two that holds
    the longest in-row, the fixed-point sums are exact for |v| < 2^ehi, ehi = min(47 - c (a row's
    sum below 2^47), 23 - min(c, 22) (a tile's split high words below 2^63), 11 (the entry
    conversion)); the floor is 2^-53 whatever the rows."""
    c = 0
    while (1 << c) < max_len and c < 47:
        c += 1
    return min(47 - c, 23 - min(c, 22), 11)


FX_FLOOR_LOG2 = -53


def test_range_fixture_limits_differ_by_rank():
    n, src, dst, t = range_fixture()
    assert n == 2 * RANGE_S and RANGE_S % 64 == 0 and RANGE_S // 64 == 513
    indeg = np.bincount(dst, minlength=n)
    outdeg = np.bincount(src, minlength=n)
    own = [indeg[:RANGE_S], indeg[RANGE_S:]]
    assert own[0].max() == indeg[t] == RANGE_D and (np.delete(own[0], t) == 0).all()
    assert (outdeg[:RANGE_S] == 0).all()                          # rank 0: t, and vertices without entries
    assert own[1].max() == 1 and int(own[1].sum()) == RANGE_D
    assert (outdeg[RANGE_S:RANGE_S + RANGE_D] == 2).all()         # edgeCount 2: c_k = x_k / 2
    assert 2 ** 15 < RANGE_D <= 2 ** 16                           # c = 16
    assert fx_limit_log2(int(own[0].max())) == 7                  # rank 0 alone: |v| < 2^7
    assert fx_limit_log2(int(own[1].max())) == 11                 # rank 1 alone: |v| < 2^11
    assert fx_limit_log2(int(indeg.max())) == 7                   # the job (and one GPU): 2^7
    # the rule's corners: the entry conversion binds up to 4096 entries, the split words after
    assert [fx_limit_log2(x) for x in (0, 1, 2, 4096, 4097, 8192, 8193, 1 << 22, (1 << 22) + 1, 1 << 40)] == \
        [11, 11, 11, 11, 10, 10, 9, 1, 1, 1]


def test_range_contributions_sit_between_the_two_limits():
    """T = 80: everything a source emits is inside rank 1's own limit, the first update's entries
    pass rank 0's entry check, and rank 0 then reads eleven contributions above its limit — the
    last ones within a factor 2 of rank 1's.  T = 60: nothing reaches rank 0's limit."""
    T = 80
    c = [abs(x) for x in range_contributions(T + 1)]              # c[k - 1] = |c_k|
    assert max(c[:T]) < 2 ** 11                                   # c_1 .. c_T, the last one emitted included
    assert min(c[:T]) >= 2.0 ** FX_FLOOR_LOG2
    assert float(min(c[:T])) == pytest.approx(1.9e-6, rel=0.01)
    assert c[0] < 2 ** 7                                          # what the first update's entry check sees
    assert max(c[1:T - 1]) >= 2 ** 10                             # c_2 .. c_{T-1}: read by later updates
    first = {lim: next(k + 1 for k, x in enumerate(c) if x >= 2 ** lim) for lim in (7, 10)}
    assert first == {7: 69, 10: 78} and c[T] >= 2 ** 11           # c_81 would leave rank 1's range too
    assert sum(x >= 2 ** 7 for x in c[:T - 1]) == 11              # c_69 .. c_79
    assert max(c[:60]) < 2 ** 7                                   # the control job


@pytest.mark.parametrize("iters", [60, 80])
def test_range_oracle_equals_rational_arithmetic(iters):
    n, src, dst, t = range_fixture()
    ref = range_reference(iters)
    assert np.isfinite(ref).all()
    base = float((1 - RANGE_ALPHA) / n)
    assert ref[t] != base and (ref[1:RANGE_S] == base).all() and (ref[RANGE_S + RANGE_D:] == base).all()
    opr, _ = fr.OracleGraph.from_edges(n, src, dst).pagerank(float(RANGE_ALPHA), n, iters)
    assert np.array_equal(np.isfinite(opr), np.isfinite(ref))
    assert np.allclose(opr, ref, rtol=1e-9, atol=0)


# ----------------------------------------------------------------------------- ragged partitions
@functools.lru_cache(maxsize=None)
def padded(n):
    return padded_ragged(n, SEED)


CASES = [(1001, "equal2"), (1001, "equal4"), (4099, "single"), (4099, "one_word"), (4099, "last_word"),
         (4099, "balanced4"), (4099, "empty")]
# (hub, first isolated vertex, largest IN rung, largest OUT rung) -> owning rank
OWNERS = {(1001, "equal2"): (1, 0, 1, 0), (1001, "equal4"): (2, 0, 3, 1), (4099, "single"): (0, 0, 0, 0),
          (4099, "one_word"): (1, 1, 1, 1), (4099, "last_word"): (0, 0, 0, 0), (4099, "balanced4"): (1, 0, 1, 1),
          (4099, "empty"): (0, 0, 0, 0)}


def test_part_cases_are_the_named_ones():
    assert [(n, name) for n in BIG for name, _ in part_cases(padded(n)[0], *padded(n)[1:3])] == CASES
    assert padded(1001)[0] == 1024 and padded(4099)[0] == 4160


@pytest.mark.parametrize("n,name", CASES)
def test_partition_claims(n, name):
    P, src, dst, w, info = padded(n)
    part = part_case(P, src, dst, name)
    N = part.n
    assert N == (P + 64 if name == "empty" else P) and part.slot % 64 == 0
    assert src.max() < n and dst.max() < n                         # n .. N-1 are pads: no entry
    deg = np.bincount(src, minlength=N) + np.bincount(dst, minlength=N)
    top = max(info["rungs"])
    vin, vout = info["rungs"][top]
    assert top == 4097
    marks = (info["hub"], int(info["isolated"][0]), vin, vout)
    assert tuple(owner(part, v) for v in marks) == OWNERS[(n, name)]
    if part.world > 1:
        feeders = {owner(part, int(s)) for s in src[dst == vin]}
        reached = {owner(part, int(d)) for d in dst[src == vout]}
        assert len(src[dst == vin]) == len(dst[src == vout]) == 4097
        assert len(feeders) >= 2 and len(reached) >= 2
    # the slot mapping is a bijection from the caller ids onto the non-pad slots
    slots = part.to_slots(np.arange(N))
    assert len(np.unique(slots)) == N and np.array_equal(part.from_slots(slots), np.arange(N))
    short = 0
    for r in range(part.world):
        lo, hi = part.range(r)
        act = np.nonzero(deg[lo:hi])[0]
        n_active = int(act[-1]) + 1 if len(act) else 0
        short += n_active < part.slot
    assert short >= 1                                              # n_active < n_local on some rank
    if name == "one_word":
        assert part.range(0) == (0, 64) and part.slot == 4096 and deg[:64].sum() > 0
    if name == "last_word":
        assert part.range(2) == (4096, 4160) and n - 4096 == 3
        assert (deg[4096:n] > 0).any() and (deg[n:] == 0).all()
    if name == "empty":
        assert part.range(2) == (P, P + 64) and deg[P:].sum() == 0
        assert not ((src >= P) | (dst >= P)).any()
    if name == "balanced4":
        assert len(set(np.diff(part.bounds))) > 1                  # unequal ranges


class NumpyRanks:
    """One NumpyPartBackend per rank over the partition's slot ids, run as thread ranks."""

    def __init__(self, part, src, dst, w, scope):
        s, d = part.to_slots(src).astype(np.int64), part.to_slots(dst).astype(np.int64)
        self.part = part
        self.backends = [NumpyPartBackend(part.n_slots, *part.slot_range(r), s, d, np.asarray(w, np.int64), scope)
                         for r in range(part.world)]

    def run(self, fn):
        return InProcessGroup(self.part.world).run(lambda rank, comm: fn(self.backends[rank], comm))

    def cut(self, per_rank):
        return np.concatenate([self.part.slot_results(r, x) for r, x in enumerate(per_rank)])


def reached(d):
    return int((d != ABSENT).sum())


@pytest.mark.parametrize("n,name", [(1001, "equal2"), (4099, "one_word"), (4099, "empty")])
def test_python_drivers_over_the_numpy_backend(n, name):
    P, src, dst, w, info = padded(n)
    part = part_case(P, src, dst, name)
    N, ns = part.n, part.n_slots
    og = fr.OracleGraph.from_edges(N, src, dst, w)
    tid = lambda v: (int(v) + 1) << 3                              # noqa: E731 — the partitioned load's implied ids
    slot = lambda v: int(part.to_slots(np.asarray([v]))[0])        # noqa: E731
    seeds = [info["hub"], int(info["isolated"][0]), *info["rungs"][max(info["rungs"])], n - 1, N - 1]
    assert N - 1 >= n                                              # the last seed is a pad
    ranks = NumpyRanks(part, src, dst, w, BOTH)
    for v in seeds:
        od = og.shortest_distance(tid(v), N, BOTH)[0]
        for alpha in (15.0, 1e9):
            res = ranks.run(lambda be, comm: distributed_bfs(be, slot(v), ns, alpha=alpha, comm=comm))
            assert np.array_equal(ranks.cut([x[0] for x in res]), od), (v, alpha)
            assert all(x[1][0] == reached(od) for x in res)
    assert reached(og.shortest_distance(tid(N - 1), N, BOTH)[0]) == 1
    for scope in (IN, OUT):
        wr = NumpyRanks(part, src, dst, w, scope)
        for v in seeds[:3]:
            od = og.shortest_distance(tid(v), N, scope, weighted=True)[0]
            for delta in (0, 9):
                res = wr.run(lambda be, comm: distributed_sssp(be, slot(v), delta, comm=comm))
                assert np.array_equal(wr.cut([x[0] for x in res]), od), (scope, v, delta)
                assert len({x[2] for x in res}) == 1
    for hot in (0, 64):
        for be in ranks.backends:
            be.pr_hot = hot
        for iters in (2, 20):
            opr = og.pagerank(0.85, N, iters)[0]
            pr = ranks.cut(ranks.run(lambda be, comm: distributed_pagerank(be, 0.85, N, iters, comm=comm)))
            fin = np.isfinite(opr)
            assert np.array_equal(np.isfinite(pr), fin)
            assert float(np.abs(pr[fin] - opr[fin]).sum()) <= PR_L1_TOL, (hot, iters)
    assert {be.job_row for be in ranks.backends} == {int(np.bincount(dst).max())}   # the agreed longest in-row
