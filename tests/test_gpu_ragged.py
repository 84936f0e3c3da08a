"""GPU parity at ragged sizes (tests/ragged.py): vertex counts off the 64 grid (a partial last
bitmap word, a partial last block, n_active below n) and rows whose length sits one below, on
and one above every row-length threshold of the kernels.  Every case compares the device with
the CPU oracle on the same edge list, bit-exact unless stated; test_ragged_cpu.py checks the
generator and that oracle against plain numpy at the same sizes, and proves the bottom-up
condition the direction assertions below rely on.

Bars (BASELINE.json north_star): BFS levels, reachability and integer distances bit-exact;
PageRank within 1e-6 L1.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import fulgora as fr
from ragged import BIG, SIZES, draw_seeds, edge_fixed_point, low_degree_vertex, numpy_fixed_point, ragged_graph
from titan_amd import Engine, trace
from titan_amd import _lib as L

pytestmark = pytest.mark.gpu

OUT, IN, BOTH = L.SCOPE_OUT_E, L.SCOPE_IN_E, L.SCOPE_BOTH_E
ABSENT = L.DIST_ABSENT
PR_L1_TOL = 1e-6      # north_star: PageRank within 1e-6 L1
SEED = 7
SCOPES = [IN, OUT, BOTH]
SIZE_SCOPES = [(n, s) for n in SIZES for s in SCOPES]
WIDE_N = 20483        # 321 bitmap words: in one block a wave gets 81 / 80 / 80 / 80 of them


class Ragged:
    def __init__(self, n):
        self.n = n
        self.src, self.dst, self.w, self.ids, self.info = ragged_graph(n, SEED)
        self.oracle = fr.OracleGraph.from_edges(n, self.src, self.dst, self.w, titan_ids=self.ids)
        self._sd = {}
        self._pr = {}

    def engine(self, scope, weighted=False):
        eng = Engine().load_edges(self.n, self.src, self.dst, scope, weight=self.w if weighted else None,
                                  titan_ids=self.ids)
        assert np.array_equal(eng.vertex_ids(), self.ids)         # results come in the edge list's dense order
        return eng

    def sd(self, v, depth, scope, weighted=False):
        """The oracle's distances from dense index v, computed once and never written to."""
        key = (int(v), int(depth), scope, weighted)
        if key not in self._sd:
            d = self.oracle.shortest_distance(int(self.ids[v]), int(depth), scope, weighted=weighted)[0]
            d.setflags(write=False)
            self._sd[key] = d
        return self._sd[key]

    def pr(self, iters):
        if iters not in self._pr:
            p = self.oracle.pagerank(0.85, self.n, iters)[0]
            p.setflags(write=False)
            self._pr[iters] = p
        return self._pr[iters]

    def top_rungs(self):
        r = self.info["rungs"]
        return list(r[max(r)]) if r else []

    def bfs_seeds(self):
        s = [self.info["hub"]] + [int(v) for v in self.info["isolated"][:1]] + self.top_rungs() + [self.n - 1, 0]
        return list(dict.fromkeys(s))


@functools.lru_cache(maxsize=None)
def ragged(n):
    return Ragged(n)


def reached(d):
    return int((d != ABSENT).sum())


# ----------------------------------------------------------------------------- BFS
@pytest.mark.parametrize("n,scope", SIZE_SCOPES)
def test_bfs_bit_exact(n, scope):
    g = ragged(n)
    eng = g.engine(scope)
    for i, v in enumerate(g.bfs_seeds()):
        if i % 2:                                          # every other seed by Titan id: a real lookup
            d = eng.bfs(int(g.ids[v]), n, scope, stats=True)
        else:
            d = eng.bfs(v, n, scope, seed_is_dense=True, stats=True)
        od = g.sd(v, n, scope)
        assert np.array_equal(d, od), v
        assert eng.stats()["reached"] == reached(od)
    for v in g.info["isolated"][:1]:
        assert reached(g.sd(int(v), n, scope)) == 1        # an isolated seed reaches only itself
    hub = g.info["hub"]
    assert np.array_equal(eng.bfs(hub, 2, scope, seed_is_dense=True), g.sd(hub, 2, scope))


@pytest.mark.parametrize("n", [n for n in SIZES if n >= 63])
def test_bfs_hub_root_runs_both_directions(n, tmp_path):
    """From the hub in bothE at least one level runs bottom-up (bu_step over n_active < n
    vertices, a partial last word), and at the larger sizes a top-down level precedes it —
    test_ragged_cpu.py proves both conditions on the input."""
    g = ragged(n)
    eng = g.engine(BOTH)
    path = str(tmp_path / "trace.json")
    trace.enable(path)
    trace.clear()
    try:
        d = eng.bfs(g.info["hub"], n, BOTH, seed_is_dense=True)
        trace.flush()
    finally:
        trace.disable()
    assert np.array_equal(d, g.sd(g.info["hub"], n, BOTH))
    bu = [e["args"]["bottom_up"] for e in trace.load_events(path) if e["name"] == "bfs.level"]
    assert len(bu) == eng.stats()["levels"]
    assert 1 in bu
    if n in BIG:
        assert 0 in bu


# ----------------------------------------------------------------------------- multi-source BFS
def check_multi(g, eng, seeds, scope):
    d = eng.bfs_multi(seeds, g.n, scope, seed_is_dense=True, stats=True)
    r, _ = eng.multi_stats(len(seeds))
    for i, s in enumerate(seeds):
        od = g.sd(int(s), g.n, scope)
        assert np.array_equal(d[i], od), (i, int(s))
        assert r[i] == reached(od), (i, int(s))
    return d


@pytest.mark.parametrize("n,scope", SIZE_SCOPES)
def test_multi_source_bfs_bit_exact(n, scope):
    g = ragged(n)
    eng = g.engine(scope)
    check_multi(g, eng, np.array([g.info["hub"]]), scope)
    for nseeds in (1, 63, 64):
        check_multi(g, eng, draw_seeds(n, g.info, nseeds, SEED), scope)
    if n in BIG:
        seeds = draw_seeds(n, g.info, 64, SEED + 1)
        plain = check_multi(g, eng, seeds, scope)
        for split in (0.0, 1.0):
            for cold in (0, 1):
                eng.set_tuning(L.TUNE_MS_SPLIT, split).set_tuning(L.TUNE_MS_COLD, cold)
                assert np.array_equal(check_multi(g, eng, seeds, scope), plain), (split, cold)


# ----------------------------------------------------------------------------- SSSP
def sssp_seeds(g):
    s = [g.info["hub"]] + [int(v) for v in g.info["isolated"][:1]] + g.top_rungs()[1:] + [g.n - 1]
    return list(dict.fromkeys(s))


@pytest.mark.parametrize("n,scope", [(n, s) for n in SIZES for s in (IN, OUT)] + [(n, BOTH) for n in BIG])
def test_sssp_hop_bounded_bit_exact(n, scope):
    g = ragged(n)
    eng = g.engine(scope, weighted=True)
    for v in sssp_seeds(g):
        for depth in (0, 1, 3, n):
            d = eng.sssp(v, depth, scope, seed_is_dense=True)
            assert np.array_equal(d, g.sd(v, depth, scope, weighted=True)), (v, depth)
    hub = g.info["hub"]
    assert np.array_equal(eng.sssp(int(g.ids[hub]), 3, scope), g.sd(hub, 3, scope, weighted=True))


@pytest.mark.parametrize("n,scope", [(n, s) for n in SIZES for s in (IN, OUT)] + [(n, BOTH) for n in BIG])
def test_sssp_delta_bit_exact(n, scope):
    """Delta-stepping (default and width-9 buckets; the binned loop, the binned loop with piles
    of 16 that overflow into the bitmap scan, the done filter and heavy pulls, the bitmap-scan
    loop, and the one-block small steps) gives the oracle's converged distances."""
    g = ragged(n)
    eng = g.engine(scope, weighted=True)
    configs = [(1, 0, 0, 0, 0), (1, 16, 1, 0.001, 0), (0, 0, 0, 0, 0)]
    for bins, cap, done, pull, small in configs + [(1, 0, 0, 0, 1)]:
        eng.set_tuning(L.TUNE_DS_BINS, bins).set_tuning(L.TUNE_DS_PILE_CAP, cap).set_tuning(L.TUNE_DS_DONE, done)
        eng.set_tuning(L.TUNE_DS_PULL, pull).set_tuning(L.TUNE_DS_SMALL, small)
        for delta in ((9,) if small else (0, 9)):
            for v in sssp_seeds(g):
                d = eng.sssp(v, n, scope, mode=L.SSSP_DELTA, seed_is_dense=True, stats=True, delta=delta)
                od = g.sd(v, n, scope, weighted=True)
                assert np.array_equal(d, od), (bins, cap, done, pull, small, delta, v)
                assert eng.stats()["reached"] == reached(od)


# ----------------------------------------------------------------------------- PageRank
def check_pagerank(g, env, monkeypatch, plain=None):
    """The engine loaded under `env` against the oracle at 1, 2 and 20 iterations: equal finite
    masks, L1 over the finite entries, bitwise equal run to run, no exact re-run (these inputs
    stay inside the fixed-point range), and within 1e-12 L1 of `plain` when given."""
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    eng = g.engine(IN)
    out = {}
    for iters in (1, 2, 20):
        pr = eng.pagerank(0.85, g.n, iters)
        opr = g.pr(iters)
        fin = np.isfinite(opr)
        assert np.array_equal(np.isfinite(pr), fin), (env, iters)
        l1 = float(np.abs(pr[fin] - opr[fin]).sum())
        assert l1 <= PR_L1_TOL, (env, iters, l1)
        assert eng.stats()["exact_reruns"] == 0, (env, iters)
        assert np.array_equal(pr, eng.pagerank(0.85, g.n, iters)), (env, iters)
        if plain is not None:
            assert float(np.abs(pr[fin] - plain[iters][fin]).sum()) <= 1e-12, (env, iters)
        out[iters] = pr
    for k in env:
        monkeypatch.delenv(k)
    return out


@pytest.mark.parametrize("n", SIZES)
def test_pagerank_l1(n, monkeypatch):
    g = ragged(n)
    default = check_pagerank(g, {}, monkeypatch)
    if n not in (129, 1001, 4099):
        return
    plain = check_pagerank(g, {"TGO_PR_BLOCKED": 0}, monkeypatch)
    assert all(float(np.abs(default[i] - plain[i]).sum()) <= 1e-12 for i in plain)
    check_pagerank(g, {"TGO_PR_HOT": 64, "TGO_PR_SEG": 256}, monkeypatch, plain)
    check_pagerank(g, {"TGO_PR_FX": 0}, monkeypatch, plain)
    check_pagerank(g, {"TGO_PR_FX": 0, "TGO_PR_HOT": 64, "TGO_PR_SEG": 256}, monkeypatch, plain)
    if n in BIG:
        check_pagerank(g, {"TGO_PR_HOT": 1000, "TGO_PR_SEG": 100, "TGO_PR_WIN": 500}, monkeypatch, plain)


# ----------------------------------------------------------------------------- walk counts
@pytest.mark.parametrize("n", SIZES)
def test_walkcount_exact(n):
    g = ragged(n)
    eng = g.engine(IN)
    for k in (1, 3, 6):
        assert np.array_equal(eng.walkcount(k), g.oracle.degree_counter(k)[0]), k


# ----------------------------------------------------------------------------- components
@pytest.mark.parametrize("n", SIZES)
def test_components_hook_path(n):
    g = ragged(n)
    ref = edge_fixed_point(g.ids, g.src, g.dst)
    eng = g.engine(BOTH)
    lab, info = eng.components()
    assert np.array_equal(lab, ref)
    assert info["components"] == len(np.unique(ref)) and info["path"] == L.CC_HOOK
    for v in g.info["isolated"]:
        assert lab[v] == g.ids[v]
    assert np.array_equal(eng.components()[0], lab)


def hook_threshold_graph(outdeg):
    """Two stars joined only by the tail of one row.  cc_hook unions a row's first two OUT
    entries and first IN entry, then the rest of its OUT entries, and compares the length of the
    slice it is given (not the row's) with kSerialRow — so the ladder's rungs, whose other ends
    all sit in the giant component, cannot pin that comparison.  Here `a` has `outdeg` OUT entries: two
    (duplicates) to hub_a, which sort first, and outdeg - 2 to the targets t, each of which also
    hangs under hub_b, whose higher degree puts it first in t's IN list.  The rest slice of `a`
    (outdeg - 2 entries) is the only thing that joins the two stars.  The last dense index z has
    one OUT entry to t[0] and nothing else: it is the last internal row, and only its own row
    unions it with anything."""
    leaves = 200
    hub_a, hub_b, a = 0, 1, 2
    la = np.arange(3, 3 + leaves)
    lb = np.arange(3 + leaves, 3 + 2 * leaves)
    t = np.arange(3 + 2 * leaves, 3 + 2 * leaves + outdeg - 2)
    z = int(t[-1]) + 1
    src = np.concatenate([[a, a], np.full(len(t), a), np.full(len(t), hub_b), np.full(leaves, hub_a),
                          np.full(leaves, hub_b), [z]]).astype(np.int32)
    dst = np.concatenate([[hub_a, hub_a], t, t, la, lb, [t[0]]]).astype(np.int32)
    n = z + 1
    ids = 8 * np.cumsum(np.random.default_rng(outdeg).integers(1, 5, n)).astype(np.int64)
    return n, src, dst, ids, dict(hub_a=hub_a, hub_b=hub_b, a=a, t=t, z=z)


@pytest.mark.parametrize("outdeg", [33, 34, 35, 36])
def test_components_hook_slice_on_the_serial_threshold(outdeg):
    """Rest slices of 31, 32, 33 and 34 entries: one below, on and above kSerialRow = 32."""
    n, src, dst, ids, v = hook_threshold_graph(outdeg)
    ref = edge_fixed_point(ids, src, dst)
    assert (ref == ids.min()).all() and n % 64 != 0
    eng = Engine().load_edges(n, src, dst, BOTH, titan_ids=ids)
    # the fixture is what the docstring says, in the engine's own row and entry order
    perm = eng.graph_perm()
    out, inn = eng.graph_csr(0), eng.graph_csr(1)
    ra = perm[v["a"]]
    row = out["adj"][out["off"][ra]:out["off"][ra + 1]]
    assert len(row) == outdeg and (row[:2] == perm[v["hub_a"]]).all()
    assert sorted(row[2:]) == sorted(perm[v["t"]])
    for tj in perm[v["t"]]:
        assert inn["adj"][inn["off"][tj]] == perm[v["hub_b"]]
    assert perm[v["z"]] == n - 1
    lab, info = eng.components()
    assert np.array_equal(lab, ref)
    assert info["components"] == 1 and info["path"] == L.CC_HOOK


def test_components_propagate_path():
    """The lists of n = 1001 handed over as a CSR with one IN entry dropped (no longer each
    other's transposes): label propagation over exactly those lists, against numpy."""
    n = 1001
    g = ragged(n)
    src, dst = g.src.astype(np.int64), g.dst.astype(np.int64)
    oo = np.argsort(src, kind="stable")
    io = np.argsort(dst, kind="stable")
    out_idx, in_idx, in_row = dst[oo], src[io], dst[io]
    out_off = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=n))]).astype(np.int64)
    vin = g.info["rungs"][33][0]                          # a 33-entry IN list becomes a 32-entry one
    drop = np.nonzero(in_row == vin)[0][5]
    keep = np.ones(len(in_idx), bool)
    keep[drop] = False
    in_idx, in_row = in_idx[keep], in_row[keep]
    in_off = np.concatenate([[0], np.cumsum(np.bincount(in_row, minlength=n))]).astype(np.int64)
    assert in_off[vin + 1] - in_off[vin] == 32
    recv = np.concatenate([np.repeat(np.arange(n), np.diff(out_off)), in_row])
    send = np.concatenate([out_idx, in_idx])
    ref = numpy_fixed_point(g.ids, recv, send)
    eng = Engine().load_csr(n, out_off, out_idx, in_off, in_idx, BOTH, titan_ids=g.ids)
    lab, info = eng.components()
    assert np.array_equal(lab, ref)
    assert info["components"] == len(np.unique(ref)) and info["path"] == L.CC_PROPAGATE


# ----------------------------------------------------------------------------- generic gather
def test_generic_gather_both_scopes():
    n = 1001
    g = ragged(n)
    eng = g.engine(BOTH, weighted=True)
    rng = np.random.default_rng(3)
    has = rng.random(n) >= 1.0 / 3
    vin, vout = g.info["rungs"][64]
    has[g.src[g.dst == vin]] = False                      # a whole rung hears nothing over its IN entries
    assert 0.25 < 1.0 - has.mean() < 0.45
    imsg = rng.integers(-(1 << 40), 1 << 40, n)
    fmsg = rng.standard_normal(n)
    for vt, comb, fn, msg in ((L.VAL_INT64, L.COMBINE_SUM, L.EDGE_IDENTITY, imsg),
                              (L.VAL_INT64, L.COMBINE_SUM, L.EDGE_ADD_WEIGHT, imsg),
                              (L.VAL_FP64, L.COMBINE_MIN, L.EDGE_IDENTITY, fmsg),
                              (L.VAL_FP64, L.COMBINE_MIN, L.EDGE_ADD_WEIGHT, fmsg)):
        got, gh = eng.gather(BOTH, vt, comb, fn, msg, has)
        exp, eh = g.oracle.gather(BOTH, vt, comb, fn, msg, has)
        assert np.array_equal(gh, eh), (vt, comb, fn)
        assert np.array_equal(got[gh], exp[eh]), (vt, comb, fn)
        assert not gh[g.info["isolated"]].any()


# ----------------------------------------------------------------------------- no edges
@pytest.mark.parametrize("n", [1, 130])
def test_no_edge_graph(n):
    none = np.zeros(0, np.int32)
    ids = 8 * np.cumsum(np.random.default_rng(n).integers(1, 5, n)).astype(np.int64)
    o = fr.OracleGraph.from_edges(n, none, none, None, titan_ids=ids)
    for scope in SCOPES:
        eng = Engine().load_edges(n, none, none, scope, titan_ids=ids)
        for v in (0, n - 1):
            d = eng.bfs(v, n, scope, seed_is_dense=True, stats=True)
            assert np.array_equal(d, o.shortest_distance(int(ids[v]), n, scope)[0])
            assert reached(d) == 1 and eng.stats()["reached"] == 1
    eng = Engine().load_edges(n, none, none, IN, titan_ids=ids)
    for iters in (1, 2, 20):
        pr = eng.pagerank(0.85, n, iters)
        opr = o.pagerank(0.85, n, iters)[0]
        assert np.isfinite(opr).all() and np.array_equal(np.isfinite(pr), np.isfinite(opr))
        assert float(np.abs(pr - opr).sum()) <= PR_L1_TOL
    for k in (1, 3, 6):
        assert np.array_equal(eng.walkcount(k), o.degree_counter(k)[0])


# ----------------------------------------------------------------------------- wide extraction
_WIDE = """
import sys
sys.path.insert(0, "tests")
import numpy as np
from ragged import draw_seeds, low_degree_vertex, ragged_graph
from titan_amd import Engine, trace
from titan_amd import _lib as L
n, out = int(sys.argv[1]), sys.argv[2]
src, dst, w, ids, info = ragged_graph(n, 7)
B = L.SCOPE_BOTH_E
res = {}
trace.enable(out + ".trace.json")
trace.clear()
eng = Engine().load_edges(n, src, dst, B, weight=w, titan_ids=ids)
res["bfs_hub"] = eng.bfs(info["hub"], n, B, seed_is_dense=True)
res["bfs_low"] = eng.bfs(low_degree_vertex(n, src, dst, info), n, B, seed_is_dense=True)
trace.flush()
trace.disable()
res["ms"] = eng.bfs_multi(draw_seeds(n, info, 64, 7), n, B, seed_is_dense=True)
for name, bins, cap in (("ds_bins", 1, 0), ("ds_bins_cap16", 1, 16), ("ds_scan", 0, 0)):
    eng.set_tuning(L.TUNE_DS_BINS, bins).set_tuning(L.TUNE_DS_PILE_CAP, cap)
    res[name] = eng.sssp(info["hub"], n, B, mode=L.SSSP_DELTA, seed_is_dense=True, delta=9)
np.savez(out, **res)
"""


def _wide_child(tmp_path, name, **env):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / (name + ".npz"))
    # TGO_BFS_BETA=2: the level loop turns top-down again below n / 2 frontier vertices, so the
    # frontier bitmap is queued (bfs_queue) after the bottom-up levels
    p = subprocess.run([sys.executable, "-c", _WIDE, str(WIDE_N), out], cwd=root,
                       env=dict(os.environ, TGO_BFS_BETA="2", **env), capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    bu = [e["args"]["bottom_up"] for e in trace.load_events(out + ".trace.json") if e["name"] == "bfs.level"]
    return dict(np.load(out)), bu


def test_wide_extraction_windows(tmp_path):
    """A wave with more than 64 bitmap words takes the wide forms of the two-pass extraction:
    extract_write's `all` walk (ms_queue / ms_settle, the bitmap-scan delta-stepping), the second
    and later windows of live_words_plain (bfs_queue through chunk_extract_live, the staged
    scan of the binned loop's overflowed piles).  TGO_EXTRACT_BLOCKS=1 (read once: a fresh
    process) gives one block all 321 words of n = 20483, 81 / 80 / 80 / 80 a wave, so the second
    window is partial.  Bit-exact against the oracle and equal to the default chunking."""
    n = WIDE_N
    src, dst, w, ids, info = ragged_graph(n, SEED)
    o = fr.OracleGraph.from_edges(n, src, dst, w, titan_ids=ids)
    wide, bu = _wide_child(tmp_path, "wide", TGO_EXTRACT_BLOCKS="1")
    # some top-down level follows a bottom-up one: the frontier bitmap was extracted into a queue
    assert any(a == 1 and b == 0 for a, b in zip(bu, bu[1:])), bu
    hub, low = info["hub"], low_degree_vertex(n, src, dst, info)
    assert np.array_equal(wide["bfs_hub"], o.shortest_distance(int(ids[hub]), n, BOTH)[0])
    assert np.array_equal(wide["bfs_low"], o.shortest_distance(int(ids[low]), n, BOTH)[0])
    for i, s in enumerate(draw_seeds(n, info, 64, SEED)):
        assert np.array_equal(wide["ms"][i], o.shortest_distance(int(ids[s]), n, BOTH)[0]), i
    conv = o.shortest_distance(int(ids[hub]), n, BOTH, weighted=True)[0]
    for name in ("ds_bins", "ds_bins_cap16", "ds_scan"):
        assert np.array_equal(wide[name], conv), name
    default, bu2 = _wide_child(tmp_path, "default")
    assert bu2 == bu and sorted(default) == sorted(wide)
    for name in wide:
        assert np.array_equal(default[name], wide[name]), name
