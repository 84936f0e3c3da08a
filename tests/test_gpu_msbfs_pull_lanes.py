"""Multi-source BFS pull levels, long lists: the head probe (TGO_TUNE_MS_HEAD = H: a lane whose
lists hold more than 64 entries first walks the first H entries of its own lists, then the whole
wave goes on from where the head stopped).  It is policy: every case compares the sweep with each
seed's own single-source run, with the same sweep at H = 0 and with the sweep at the default H —
levels per seed, the per-source reached vertices and entries, and the level count.

The boundary graph pins where a long list is covered.  The degree-grouped relabel keeps row
order among vertices of equal degree and lists are sorted by the new ids, so a hub whose
neighbours all have degree 2 keeps them in creation order: neighbour j is entry j of its
concatenated lists.  Every entry of a hub is therefore a vertex of its own (n is about 2 600, not
the few hundred a multigraph would need).  One neighbour (F) brings every common source, one
(the key) brings the last source X, both at the same level, which pulls; the rest are never in a
frontier before the hub.  A walk that skips the entry where the head ends loses X at the hub.
"""
import numpy as np
import pytest

from titan_amd import Engine, TitanException, pick_roots, rmat_edges, trace
from titan_amd import _lib as L

pytestmark = pytest.mark.gpu

OUT, IN, BOTH = L.SCOPE_OUT_E, L.SCOPE_IN_E, L.SCOPE_BOTH_E
HEADS = (1, 4, 5, 16, 64)
# the key at H - 1, H, H + 1 for every H above, and at 63, 64, 65 (the whole-wave trip's edges)
POSITIONS = sorted({h + o for h in HEADS for o in (-1, 0, 1)} | {63, 64, 65})
HUB_DEGREES = (65, 66, 200, 1000)
LEAD = 6                          # vertices between the seeds' collector and the core's top vertex
HUB_LEVEL = LEAD + 4              # seed -> collector -> LEAD vertices -> top -> F -> hub


def sweep(eng, seeds, depth, scope, head, split=None, stay=None):
    """One sweep under the given policy: (levels per seed, reached, reached entries, level count)."""
    eng.set_tuning(L.TUNE_MS_HEAD, head)
    if split is not None:
        eng.set_tuning(L.TUNE_MS_SPLIT, split)
    if stay is not None:
        eng.set_tuning(L.TUNE_MS_STAY, stay)
    d = eng.bfs_multi(seeds, depth, scope, seed_is_dense=True, stats=True)
    r, e = eng.multi_stats(len(seeds))
    return d, r, e, eng.stats()["levels"]


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]


def singles(eng, seeds, depth, scope):
    return np.stack([eng.bfs(int(s), depth, scope, seed_is_dense=True) for s in seeds])


class Boundary:
    """RMAT-10 core; 63 common seeds on one collector, LEAD vertices from it to the core's top
    vertex T; seed X at the start of a path of its own; hubs whose entry `pos` is the key (fed by
    X's path) and whose entry 0 (1 when pos = 0) is F (fed by T); a separate 3-vertex component.
    Extra edges point the way the scope travels; under BOTH_E a hub's first `l0` entries are
    out-edges (list 0), the rest in-edges (list 1)."""

    def __init__(self, scope, pos):
        n0 = 1 << 10
        src, dst, _ = rmat_edges(10, 16, seed=0x54495441)
        es, ed = [], []
        self.next = n0

        def new(k=1):
            v = np.arange(self.next, self.next + k, dtype=np.int64)
            self.next += k
            return v if k > 1 else int(v[0])

        def edge(a, b):
            es.append(a)
            ed.append(b)

        fan = np.bincount(dst if scope == IN else src, minlength=n0)
        if scope == BOTH:
            fan = np.bincount(src, minlength=n0) + np.bincount(dst, minlength=n0)
        top = int(np.argmax(fan))
        coll = new()
        self.common = [int(v) for v in new(63)]
        for s in self.common:
            edge(s, coll)
        prev = coll
        for _ in range(LEAD):
            v = new()
            edge(prev, v)
            prev = v
        edge(prev, top)
        self.x = new()
        prev = self.x
        for _ in range(HUB_LEVEL - 2):      # X -> ... -> feeder -> key -> hub: the key at HUB_LEVEL - 1
            v = new()
            edge(prev, v)
            prev = v
        feeder = prev
        sink = new()
        self.hubs = []
        self.entries = []                   # every hub's neighbours, in creation order
        # (degree, entries in list 0 under BOTH_E): the plain hubs, one whose list 0 is shorter than
        # most heads, one whose list 0 is empty
        shapes = [(d, d // 3) for d in HUB_DEGREES] + [(70, 3), (72, 0)]
        for deg, l0 in shapes:
            hub = new()
            self.hubs.append(hub)
            nb = new(deg)
            self.entries.append(nb)
            key_at = min(pos, deg - 1)      # position 65 of a 65-entry hub is its last entry
            f_at = 1 if key_at == 0 else 0
            for j, v in enumerate(nb):
                v = int(v)
                if scope == BOTH and j < l0:
                    edge(hub, v)            # the hub's out-list
                else:
                    edge(v, hub)
                if j == key_at:
                    edge(feeder, v)
                elif j == f_at:
                    edge(top, v)
                else:
                    edge(v, sink)           # degree 2 like the others, in no frontier before the hub
        comp = new(3)
        edge(int(comp[0]), int(comp[1]))
        edge(int(comp[1]), int(comp[2]))
        self.dead = int(comp[0])
        while self.next % 64 in (0, 1):     # a ragged last word
            new()
        self.n = self.next
        es, ed = np.asarray(es, np.int32), np.asarray(ed, np.int32)
        # what pins the positions: every neighbour of a hub has degree 2 (one relabel group, which
        # keeps row order) and ascending ids, so it is entry j of the hub's sorted, concatenated lists
        degree = np.bincount(es, minlength=self.n) + np.bincount(ed, minlength=self.n)
        for nb in self.entries:
            assert (degree[nb] == 2).all() and (np.diff(nb) == 1).all()
        if scope == IN:
            es, ed = ed, es
        self.eng = Engine().load_edges(self.n, np.concatenate([src, es]), np.concatenate([dst, ed]), scope)
        self.scope = scope


def pull_levels(eng, seeds, n, scope, tmp_path):
    """The levels of one sweep that pulled (the msbfs.level spans' attribute)."""
    path = str(tmp_path / "trace.json")
    trace.enable(path)
    trace.clear()
    try:
        eng.bfs_multi(seeds, n, scope, seed_is_dense=True, fetch=False)
        trace.flush()
    finally:
        trace.disable()
    return {e["args"]["level"] for e in trace.load_events(path) if e["name"] == "msbfs.level" and e["args"]["pull"]}


@pytest.mark.parametrize("pos", POSITIONS)
@pytest.mark.parametrize("scope", [BOTH, IN, OUT])
def test_head_boundary(scope, pos, tmp_path):
    g = Boundary(scope, pos)
    eng, n = g.eng, g.n
    assert n % 64 != 0
    rungs = {
        "64": g.common + [g.x],                         # 64 distinct bits
        "63": g.common[:62] + [g.x],
        "dup": g.common[:62] + [g.common[0], g.x],      # two bits on one vertex
        "dead": g.common[:62] + [g.dead, g.x],          # no hub is ever covered: one source never arrives
    }
    for name, seeds in rungs.items():
        ref = singles(eng, seeds, n, scope)
        # the construction: every hub is reached at HUB_LEVEL by X and by the common sources alike
        for hub in g.hubs:
            assert ref[-1, hub] == HUB_LEVEL and ref[0, hub] == HUB_LEVEL, (name, hub)
        for split in (0.0, -1.0):                       # split off: X is pulled, the key's entry decides
            base = sweep(eng, seeds, n, scope, 0, split)
            assert np.array_equal(base[0], ref), (name, split)
            dflt = sweep(eng, seeds, n, scope, -1, split)
            assert same(dflt, base), (name, split)
            for head in HEADS:
                got = sweep(eng, seeds, n, scope, head, split)
                assert same(got, base), (name, split, head)
                if name == "64":                        # back to back
                    assert same(sweep(eng, seeds, n, scope, head, split), base), (name, split, head, "again")
        if name == "64":
            # the level that finds the hubs pulls, so the hubs' lists are walked by ms_pull
            eng.set_tuning(L.TUNE_MS_HEAD, -1).set_tuning(L.TUNE_MS_SPLIT, 0.0)
            assert HUB_LEVEL - 1 in pull_levels(eng, seeds, n, scope, tmp_path)
            # a depth-cut sweep (ending on the pull level that finds the hubs, and one before it),
            # then the full one
            for depth in (HUB_LEVEL, HUB_LEVEL - 1):
                cut = sweep(eng, seeds, depth, scope, 16, 0.0)
                assert np.array_equal(cut[0], singles(eng, seeds, depth, scope)), depth
                assert same(sweep(eng, seeds, n, scope, 16, 0.0), sweep(eng, seeds, n, scope, 0, 0.0)), depth
    eng.set_tuning(L.TUNE_MS_SPLIT, -1.0).set_tuning(L.TUNE_MS_HEAD, -1)


# ----------------------------------------------------------------------------- RMAT-12, tail, dead source
TAIL = 40
HUGE = 1.0e9


@pytest.fixture(scope="module")
def tailed():
    """RMAT-12 with a 40-vertex path hung on its top-degree vertex and a separate 3-vertex
    component; n = 4139 (the small-levels test's shape)."""
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
@pytest.mark.parametrize("split", [0.0, -1.0])
def test_rmat12_tail_head_is_policy_only(tailed, with_dead, split):
    """RMAT-12's own long lists (hundreds of rows above 64 entries) under every head length, with
    the stay rule holding the tail levels in pull (gamma huge: the long rows that stay open for the
    dead source are walked to their end level after level) and without it."""
    n, eng, seeds, dead, tail_end = tailed
    sd = seeds + [dead if with_dead else tail_end]
    ref = singles(eng, sd, n, BOTH)
    for stay in (-1.0, 0.0, HUGE):
        base = sweep(eng, sd, n, BOTH, 0, split, stay)
        assert np.array_equal(base[0], ref), stay
        assert same(sweep(eng, sd, n, BOTH, -1, split, stay), base), stay
        for head in HEADS + (1000,):
            assert same(sweep(eng, sd, n, BOTH, head, split, stay), base), (stay, head)
    cut = sweep(eng, sd, 3, BOTH, -1, split, -1.0)
    assert np.array_equal(cut[0], singles(eng, sd, 3, BOTH))
    assert same(sweep(eng, sd, n, BOTH, -1, split, -1.0), sweep(eng, sd, n, BOTH, 0, split, -1.0))
    eng.set_tuning(L.TUNE_MS_SPLIT, -1.0).set_tuning(L.TUNE_MS_STAY, -1.0).set_tuning(L.TUNE_MS_HEAD, -1)


def test_head_key_rejects_out_of_range(tailed):
    eng = tailed[1]
    for bad in (-0.5, -2.0, 2.5, float(1 << 21), float("nan"), float("inf")):
        with pytest.raises(TitanException):
            eng.set_tuning(L.TUNE_MS_HEAD, bad)
    eng.set_tuning(L.TUNE_MS_HEAD, 0).set_tuning(L.TUNE_MS_HEAD, 5).set_tuning(L.TUNE_MS_HEAD, float(1 << 20))
    eng.set_tuning(L.TUNE_MS_HEAD, -1)
