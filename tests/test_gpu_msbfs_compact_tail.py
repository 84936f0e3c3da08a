"""Multi-source BFS, the compact form of the tail pull levels (ms_pull_compact): a pull level that
counts mu — the level after the frontier's peak and every stay-rule level after it — scans the
reached masks a chunk of vertices per wave, compacts the open vertices' ids inside the wave and walks
only those.  It is a form, not a result: every case compares the sweep under the default policy
with each seed's own single-source run (Engine.bfs), with the same sweep at TUNE_MS_STAY = 0 (the
word form at every level) and at TUNE_MS_STAY = 1e9 (pull, hence compact, for as long as the
frontier keeps shrinking) — levels per seed, the per-source reached vertices and entries, the
level count — and reads the msbfs.level spans: the levels a case was built for ran with
compact = 1, and none did at STAY = 0.

The graphs hang a fan of layers with strictly decreasing widths on the top vertex of an RMAT-10
core, each vertex of a layer attached to one vertex of the layer before: the frontier's entries
shrink level after level, and the open vertices of a level are the layers still ahead, which puts
0, 1, 2, 63, 64, 65, ... open vertices into a chunk.  The seeds reach the top vertex together
(through one collector) or in two groups one level apart, so the levels of the fan are known.

Chunk sizes: the candidates are 512, 1024 and 2048 vertices (8, 16 and 32 words of 64 rows, which
a wave takes a grid stride apart), and the tests do not depend on the one chosen.  The fan and the
core alone hold about 5 000 rows with entries, so the rows with entries (n_active) are padded with
degree-2 filler to 3 * 2048 + r for r in -1, 0, 1, 63, 64, 65: behind more than two chunks' worth of
rows, the words then fill the chunks exactly (r = 0), with a last word one row short (r = -1), or
leave one or two words over — a 1-row word, a 63-row word, a full word, a full word and a 1-row
word — so that most chunks of the last stride have a word missing, for every candidate at once
(2048 = 2 * 1024 = 4 * 512).  n itself is never a multiple of 64.
"""
import numpy as np
import pytest

import cl_ref as cr
from titan_amd import Engine, rmat_edges, trace
from titan_amd import _lib as L

pytestmark = pytest.mark.gpu

OUT, IN, BOTH = L.SCOPE_OUT_E, L.SCOPE_IN_E, L.SCOPE_BOTH_E
HUGE = 1.0e9
WIDTHS = (2048 + 65, 1025, 513, 129, 65, 64, 63, 2, 1)
ROWS = tuple(3 * 2048 + r for r in (-1, 0, 1, 63, 64, 65))
POLICIES = (-1.0, 0.0, HUGE)      # TUNE_MS_STAY: default, the word form everywhere, compact while shrinking


def sweep(eng, seeds, depth, scope, stay, head=None):
    """One sweep under the given policy: (levels per seed, reached, reached entries, level count)."""
    eng.set_tuning(L.TUNE_MS_STAY, stay)
    if head is not None:
        eng.set_tuning(L.TUNE_MS_HEAD, head)
    d = eng.bfs_multi(seeds, depth, scope, seed_is_dense=True, stats=True)
    r, e = eng.multi_stats(len(seeds))
    return d, r, e, eng.stats()["levels"]


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]


def singles(eng, seeds, depth, scope):
    return np.stack([eng.bfs(int(s), depth, scope, seed_is_dense=True) for s in seeds])


def level_spans(eng, seeds, n, scope, stay, tmp_path):
    """The msbfs.level spans of one sweep at TUNE_MS_STAY = stay: (levels that pulled, levels that
    ran compact, number of levels)."""
    path = str(tmp_path / "trace.json")
    eng.set_tuning(L.TUNE_MS_STAY, stay)
    trace.enable(path)
    trace.clear()
    try:
        eng.bfs_multi(seeds, n, scope, seed_is_dense=True, fetch=False)
        trace.flush()
    finally:
        trace.disable()
    ev = [e["args"] for e in trace.load_events(path) if e["name"] == "msbfs.level"]
    assert all("compact" in a for a in ev)
    return {a["level"] for a in ev if a["pull"]}, {a["level"] for a in ev if a["compact"]}, len(ev)


def check(eng, seeds, n, scope, ref, tmp_path, built_for):
    """The three policies against the singles and each other; the spans: compact only on pull
    levels, on every level of built_for at STAY = 1e9, on none at STAY = 0."""
    base = sweep(eng, seeds, n, scope, 0.0)
    assert np.array_equal(base[0], ref)
    for stay in POLICIES:
        assert same(sweep(eng, seeds, n, scope, stay), base), stay
    pulls, compact, count = level_spans(eng, seeds, n, scope, 0.0, tmp_path)
    assert not compact and count == base[3]
    pulls, compact, count = level_spans(eng, seeds, n, scope, HUGE, tmp_path)
    print("levels", count, "pull", sorted(pulls), "compact", sorted(compact), "built for", sorted(built_for))
    assert count == base[3] and compact <= pulls
    assert set(built_for) <= compact, (sorted(built_for), sorted(compact))
    pulls, compact, count = level_spans(eng, seeds, n, scope, -1.0, tmp_path)
    assert count == base[3] and compact <= pulls
    eng.set_tuning(L.TUNE_MS_STAY, -1.0)
    return base


class Tapered:
    """RMAT-10 core with a fan of WIDTHS on its top vertex T.  Seeds: `near` of them on a collector
    next to T (T at distance 2), the others on a collector one vertex further (distance 3).  Extra
    edges point the way the scope travels.  A separate 3-vertex component (dead), degree-2 filler
    between T and a sink up to `rows` rows with entries, isolated vertices up to a ragged n."""

    def __init__(self, scope, near=32, count=64, seed=0x54495441, base=0):
        self.scope = scope
        self.n0 = 1 << 10
        src, dst, _ = rmat_edges(10, 16, seed=seed)
        self.core = (src.astype(np.int64) + base, dst.astype(np.int64) + base)
        self.es, self.ed = [], []
        self.next = base + self.n0
        fan = np.bincount(dst if scope == IN else src, minlength=self.n0)
        if scope == BOTH:
            fan = np.bincount(src, minlength=self.n0) + np.bincount(dst, minlength=self.n0)
        self.top = base + int(np.argmax(fan))
        self.seeds = []
        if count:
            coll = self.new()
            self.edge(coll, self.top)
            far = self.new()
            hop = self.new()
            self.edge(far, hop)
            self.edge(hop, self.top)
            for i in range(count):
                s = self.new()
                self.seeds.append(s)
                self.edge(s, coll if i < near else far)
        self.near = near

    def new(self, k=1):
        v = np.arange(self.next, self.next + k, dtype=np.int64)
        self.next += k
        return v if k > 1 else int(v[0])

    def edge(self, a, b):
        self.es.append(int(a))
        self.ed.append(int(b))

    def fan(self, root, widths=WIDTHS):
        """The layers; layer i at distance i + 1 from root."""
        layers, prev = [], np.asarray([root], np.int64)
        for w in widths:
            cur = self.new(w) if w > 1 else np.asarray([self.new()], np.int64)
            for j, v in enumerate(cur):
                self.edge(prev[j % len(prev)], v)
            layers.append(cur)
            prev = cur
        return layers

    def dead_component(self):
        comp = self.new(3)
        self.edge(comp[0], comp[1])
        self.edge(comp[1], comp[2])
        return int(comp[0])

    def edges(self):
        es, ed = np.asarray(self.es, np.int64), np.asarray(self.ed, np.int64)
        if self.scope == IN:
            es, ed = ed, es
        return np.concatenate([self.core[0], es]), np.concatenate([self.core[1], ed])

    def rows_with_entries(self):
        s, d = self.edges()
        return len(np.union1d(s, d))

    def pad(self, rows):
        have = self.rows_with_entries()
        assert rows - have >= 2, (rows, have)
        sink = self.new()
        for _ in range(rows - have - 1):
            f = self.new()
            self.edge(self.top, f)
            self.edge(f, sink)
        assert self.rows_with_entries() == rows

    def load(self, others=()):
        self.new()                                       # at least one row without entries
        while self.next % 64 == 0:
            self.new()
        self.n = self.next
        s, d = self.edges()
        for o in others:
            so, do = o.edges()
            s, d = np.concatenate([s, so]), np.concatenate([d, do])
        self.src, self.dst = s.astype(np.int32), d.astype(np.int32)
        self.eng = Engine().load_edges(self.n, self.src, self.dst, self.scope)
        return self.eng


def fan_levels(first, layers=len(WIDTHS)):
    """The sweep levels at which the last source discovers the fan's layers 2 .. last: a frontier of
    one layer, narrower than the one before it.  `first` = the distance of layer 0 from the last
    group of seeds; level L discovers distance L + 1."""
    return range(first + 1, first + layers - 1)


# ----------------------------------------------------------------------------- 1. tapering layers
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("scope", [BOTH, IN, OUT])
def test_tapering_layers(scope, rows, tmp_path):
    """Every layer level past the peak counts mu and runs compact; 64 seeds, 63, and a duplicate."""
    g = Tapered(scope)
    layers = g.fan(g.top)
    g.pad(rows)
    eng = g.load()
    n = g.n
    assert n % 64 != 0
    ref = singles(eng, g.seeds, n, scope)
    assert ref[0, g.top] == 2 and ref[-1, g.top] == 3
    assert ref[-1, layers[-1][0]] == 3 + len(WIDTHS)
    # the far group finds layer 0 at distance 4
    built_for = fan_levels(4)
    check(eng, g.seeds, n, scope, ref, tmp_path, built_for)
    check(eng, g.seeds[:63], n, scope, ref[:63], tmp_path, built_for)
    dup = g.seeds[:62] + [g.seeds[0], g.seeds[63]]
    check(eng, dup, n, scope, np.concatenate([ref[:62], ref[:1], ref[63:]]), tmp_path, built_for)


# ----------------------------------------------------------------------------- 2. a dead seed
@pytest.mark.parametrize("scope", [BOTH, IN, OUT])
def test_dead_seed_keeps_every_vertex_open(scope, tmp_path):
    """One seed sits in a separate 3-vertex component: every vertex of the giant component stays
    open for the whole sweep, so the compacted list is the whole chunk at every compact level."""
    g = Tapered(scope)
    g.fan(g.top)
    dead = g.dead_component()
    g.pad(ROWS[5])
    eng = g.load()
    seeds = g.seeds[:40] + [dead] + g.seeds[41:]
    ref = singles(eng, seeds, g.n, scope)
    assert (ref[40] >= 0).sum() == 3
    check(eng, seeds, g.n, scope, ref, tmp_path, fan_levels(4))


# ----------------------------------------------------------------------------- 3. long lists
HUB_SHAPES = ((65, 21), (66, 22), (200, 66), (1000, 333), (70, 3), (72, 0))   # (degree, entries of list 0 under BOTH_E)
HEADS = (0, 4, 64)
KEY_AT = (0, 3, 4, 63, 64, -1)    # entry 0, H - 1 and H of the heads above, the last entry
FEED = 2                          # the fan layer that feeds the hubs' entry F
HUB_DIST = 3 + FEED + 2           # seed, collector, T, layers 0 .. FEED, F, hub


@pytest.mark.parametrize("key_at", KEY_AT)
@pytest.mark.parametrize("scope", [BOTH, IN, OUT])
def test_long_lists_from_a_compacted_lane(scope, key_at, tmp_path):
    """Hubs of 65, 66, 200 and 1000 entries, still open at a compact level, covered there by entry
    F (every common source, fed by a fan layer) and by the key entry (the last source X, on a path
    of its own) at the same level — or never, with a dead seed.  Every neighbour of a hub has
    degree 2 and ascending ids, which pins it as entry j of the hub's sorted, concatenated lists
    (the construction of test_gpu_msbfs_pull_lanes.py).  Under BOTH_E one hub's list 0 is empty and
    one's is shorter than the head."""
    g = Tapered(scope, near=63, count=63)
    layers = g.fan(g.top)
    x = g.new()
    prev = x
    for _ in range(HUB_DIST - 2):                         # X -> ... -> feeder -> key -> hub
        v = g.new()
        g.edge(prev, v)
        prev = v
    feeder, sink, hubs, entries = prev, g.new(), [], []
    for deg, l0 in HUB_SHAPES:
        hub = g.new()
        hubs.append(hub)
        nb = g.new(deg)
        entries.append(nb)
        k_at = deg - 1 if key_at < 0 else min(key_at, deg - 1)
        f_at = 1 if k_at == 0 else 0
        for j, v in enumerate(nb):
            if scope == BOTH and j < l0:
                g.edge(hub, v)
            else:
                g.edge(v, hub)
            if j == k_at:
                g.edge(feeder, v)
            elif j == f_at:
                g.edge(layers[FEED][j % len(layers[FEED])], v)
            else:
                g.edge(v, sink)
    dead = g.dead_component()
    g.pad(3 * 2048 + 2048 + 65)
    eng = g.load()
    n = g.n
    degree = np.bincount(g.src, minlength=n) + np.bincount(g.dst, minlength=n)
    for nb in entries:
        assert (degree[nb] == 2).all() and (np.diff(nb) == 1).all()
    for name, seeds in (("64", g.seeds + [x]), ("dead", g.seeds[:62] + [dead, x])):
        ref = singles(eng, seeds, n, scope)
        for hub in hubs:
            assert ref[-1, hub] == HUB_DIST and ref[0, hub] == HUB_DIST, (name, hub)
        base = sweep(eng, seeds, n, scope, 0.0, 0)
        assert np.array_equal(base[0], ref), name
        for head in HEADS:
            for stay in POLICIES:
                assert same(sweep(eng, seeds, n, scope, stay, head), base), (name, head, stay)
        eng.set_tuning(L.TUNE_MS_HEAD, -1)
        # the level that finds the hubs walks their lists from compacted lanes
        pulls, compact, _ = level_spans(eng, seeds, n, scope, HUGE, tmp_path)
        print(name, "pull", sorted(pulls), "compact", sorted(compact))
        assert HUB_DIST - 1 in compact, (name, sorted(compact))
        assert not level_spans(eng, seeds, n, scope, 0.0, tmp_path)[1]
    eng.set_tuning(L.TUNE_MS_STAY, -1.0)


# ----------------------------------------------------------------------------- 4. compact -> push -> pull
BRIDGE = 4


def test_compact_level_then_push_then_pull(tmp_path):
    """Two cores joined by a thin bridge: the tail of the first runs compact, the bridge (a path:
    its frontier stops shrinking) pushes, and the second core pulls again."""
    g = Tapered(BOTH)
    layers = g.fan(g.top)
    g.next = max(g.next, 1 << 13)
    h = Tapered(BOTH, count=0, seed=0x1234567, base=g.next)
    g.next = h.next
    prev = int(layers[-1][0])
    for _ in range(BRIDGE):
        v = g.new()
        g.edge(prev, v)
        prev = v
    g.edge(prev, h.top)
    eng = g.load(others=[h])
    n = g.n
    ref = singles(eng, g.seeds, n, BOTH)
    assert ref[0, h.top] == 2 + len(WIDTHS) + BRIDGE + 1
    assert (ref[0, h.core[0]] > ref[0, h.top]).any()      # the second core is swept from its top
    check(eng, g.seeds, n, BOTH, ref, tmp_path, fan_levels(4))
    pulls, compact, count = level_spans(eng, g.seeds, n, BOTH, HUGE, tmp_path)
    tail = max(fan_levels(4))
    pushes = [lv for lv in range(count) if lv not in pulls and lv > tail]
    assert pushes and any(lv > pushes[0] for lv in pulls), (sorted(pulls), pushes)
    eng.set_tuning(L.TUNE_MS_STAY, -1.0)


# ----------------------------------------------------------------------------- 5. plane fills across sweeps
PATH, ISOLATED = 600, 37


def test_plane_fills_across_sweeps_on_one_engine():
    """The level planes across sweeps of one engine: a plane filled for a level that found nothing
    is not filled again, a plane a level wrote is, and the rows without entries are zeroed once.
    Deep sweep (10 planes), shallow (1 plane), deep, depth-cut, other seeds, a seed on a row without
    entries; the closeness fold reads the planes after a deep and after a shallow sweep."""
    n = PATH + ISOLATED
    src = np.arange(PATH - 1, dtype=np.int32)
    dst = src + 1
    eng = Engine().load_edges(n, src, dst, BOTH)
    seeds = [0, PATH - 1, PATH // 2, 0, PATH + 20]
    for stay in POLICIES:
        eng.set_tuning(L.TUNE_MS_STAY, stay)
        ref = singles(eng, seeds, n, BOTH)
        assert ref.max() == PATH - 1
        deep = sweep(eng, seeds, n, BOTH, stay)
        assert np.array_equal(deep[0], ref), stay
        shallow = sweep(eng, seeds, 2, BOTH, stay)
        assert np.array_equal(shallow[0], singles(eng, seeds, 2, BOTH)), stay
        assert same(sweep(eng, seeds, n, BOTH, stay), deep), stay
        cut = sweep(eng, seeds, 5, BOTH, stay)
        assert np.array_equal(cut[0], singles(eng, seeds, 5, BOTH)), stay
        other = [PATH // 3, PATH + 1, 7]
        got = sweep(eng, other, n, BOTH, stay)
        assert np.array_equal(got[0], singles(eng, other, n, BOTH)), stay
        lone = sweep(eng, [PATH + 5], n, BOTH, stay)
        assert lone[0][0, PATH + 5] == 0 and (np.delete(lone[0][0], PATH + 5) < 0).all(), stay
        assert same(sweep(eng, seeds, n, BOTH, stay), deep), stay
        # the fold after a deep sweep, then after a shallow one
        for depth in (None, 2, None):
            want, winfo = cr.reference(n, src, dst, BOTH, seeds=np.asarray(seeds), max_depth=depth)
            res, info = eng.closeness(seeds, dense=True, max_depth=depth, scope=BOTH)
            got = eng.copy_closeness()
            assert info == winfo, (stay, depth)
            for k in ("far", "reach", "ecc"):
                assert np.array_equal(got[k], want[k]), (stay, depth, k)
            for k in ("closeness", "harmonic"):
                assert got[k].tobytes() == want[k].tobytes(), (stay, depth, k)
        assert same(sweep(eng, seeds, n, BOTH, stay), deep), stay
    eng.set_tuning(L.TUNE_MS_STAY, -1.0)
