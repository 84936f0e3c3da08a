#!/usr/bin/env python3
"""Betweenness centrality on the bench's RMAT bothE graph (tgo_betweenness, undirected reading) from
the first --seeds of the bench's BFS roots: the device time of the three per-seed spans
(betweenness.bfs / .sigma / .delta, from the engine's trace), tgo_bfs of the same roots on the same
build, the ratio (sigma + delta) / bfs, and the bytes per second each sweep reaches against its
algorithmic bytes: 4 B per simple-adjacency entry of a reached vertex + 4 B of level per entry + 8 B
of sigma per matching entry (a predecessor for sigma, a successor for delta) + 16 B per reached vertex.

    python scripts/bc_bench.py [--scale 20] [--edge-factor 16] [--seeds 16] [--warmup 1] [--runs 5]
                               [--sweep]

--sweep    repeats the timing at TGO_TUNE_BC_WAVE_ROW = 16, 64, 256 (DESIGN.md 4.8 records it).

Prints one JSON line.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
SPANS = ("bfs", "sigma", "delta")


def simple_adjacency(out, inn, n):
    """(row, neighbour) of the simple undirected projection in internal ids, from the device's lists."""
    def pairs(c):
        return np.repeat(np.arange(n, dtype=np.int64), np.diff(c["off"])), c["adj"].astype(np.int64)
    ro, ao = pairs(out)
    ri, ai = pairs(inn)
    key = np.unique(np.concatenate([ro * n + ao, ri * n + ai]))
    row, nb = key // n, key % n
    keep = row != nb
    return row[keep], nb[keep]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--scale", type=int, default=20)
    p.add_argument("--edge-factor", type=int, default=16)
    p.add_argument("--seeds", type=int, default=16)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--sweep", action="store_true")
    args = p.parse_args()
    if args.runs < 1 or args.seeds < 1:
        p.error("--runs and --seeds must be >= 1")

    from titan_amd import Engine, pick_roots, rmat_edges, trace
    from titan_amd import _lib as L

    n = 1 << args.scale
    src, dst, _ = rmat_edges(args.scale, args.edge_factor, seed=0x54495441)      # the graph of bench.py
    roots = np.asarray(pick_roots(n, src, dst, 64, seed=7)[:args.seeds], np.int64)   # and its roots
    out = {"workload": f"rmat{args.scale}-ef{args.edge_factor}-bothE-betweenness{len(roots)}", "vertices": n,
           "edges": int(len(src)), "seeds": int(len(roots))}
    eng = Engine(device=0).load_edges(n, src, dst, L.SCOPE_BOTH_E, apply_cap=False)
    del src, dst
    loaded = eng.stats()["device_bytes"]
    eng.sync()
    t0 = time.perf_counter()
    eng.betweenness(roots[:1], dense=True, fetch=False)             # builds and caches the simple adjacency
    first_wall = (time.perf_counter() - t0) * 1e3
    out["first_call_ms"] = first_wall
    out["list_build_ms"] = first_wall - eng.stats()["last_kernel_ms"]
    out["device_bytes_lists"] = eng.stats()["device_bytes"] - loaded

    tmp = tempfile.mkdtemp(prefix="bc_bench_")

    def spans_of(run_once, names, count):
        """Median over --runs of each seed's span durations (ms): {name: array of count}."""
        got = {k: [] for k in names}
        for r in range(args.warmup + args.runs):
            path = os.path.join(tmp, f"trace_{r}.json")
            trace.clear()
            trace.enable(path)
            run_once()
            trace.flush(path)
            trace.disable()
            if r < args.warmup:
                continue
            ev = trace.load_events(path)
            for k in names:
                d = [e["dur"] / 1e3 for e in ev if e["name"] == k and e["cat"] == "device"]
                assert len(d) == count, (k, len(d), count)
                got[k].append(d)
        return {k: np.median(np.asarray(v), axis=0) for k, v in got.items()}

    def bc_point():
        info = {}

        def once():
            info.update(eng.betweenness(roots, dense=True, fetch=False)[1])
            info["ms"] = eng.stats()["last_kernel_ms"]
        t = spans_of(once, ["betweenness." + k for k in SPANS], len(roots))
        return {k: t["betweenness." + k] for k in SPANS}, info

    def summary(t):
        s = {k + "_ms_per_seed": float(t[k].mean()) for k in SPANS}
        s["sweeps_over_bfs"] = float((t["sigma"] + t["delta"]).sum() / t["bfs"].sum())
        return s

    t, info = bc_point()
    out.update(summary(t))
    out.update({"reached_pairs": info["reached_pairs"], "max_depth": info["max_depth"], "rounds": info["rounds"],
                "call_ms": info["ms"]})
    out["per_seed_ms"] = {k: [round(float(x), 4) for x in t[k]] for k in SPANS}

    # tgo_bfs of the same roots: the call's own HIP-event timing, tracing off
    def bfs_ms():
        ms = []
        for s in roots:
            eng.bfs(int(s), n, L.SCOPE_BOTH_E, seed_is_dense=True, fetch=False)
            ms.append(eng.stats()["last_kernel_ms"])
        return ms
    for _ in range(args.warmup):
        bfs_ms()
    plain = np.median(np.asarray([bfs_ms() for _ in range(args.runs)]), axis=0)
    out["tgo_bfs_ms_per_seed"] = float(plain.mean())
    out["sweeps_over_tgo_bfs"] = float((t["sigma"] + t["delta"]).sum() / plain.sum())

    # algorithmic bytes of each sweep, from the levels of every root
    row, nb = simple_adjacency(eng.graph_csr(0), eng.graph_csr(1), n)
    perm = np.asarray(eng.graph_perm(), np.int64)
    assert 4 * len(row) + 8 * (n + 1) == out["device_bytes_lists"]
    bytes_sigma, bytes_delta = [], []
    for s in roots:
        d = eng.bfs(int(s), n, L.SCOPE_BOTH_E, seed_is_dense=True)
        lvl = np.full(n, -1, np.int64)
        lvl[perm] = np.where(d == L.DIST_ABSENT, -1, d)
        reached = lvl[row] >= 0
        entries = int(reached.sum())
        verts = int((lvl >= 0).sum())
        pred = int((reached & (lvl[nb] == lvl[row] - 1)).sum())
        succ = int((reached & (lvl[nb] == lvl[row] + 1)).sum())
        bytes_sigma.append(8 * entries + 8 * pred + 16 * verts)
        bytes_delta.append(8 * entries + 8 * succ + 16 * verts)
    out["sigma_gb_per_s"] = float(np.sum(bytes_sigma) / (t["sigma"].sum() * 1e-3) / 1e9)
    out["delta_gb_per_s"] = float(np.sum(bytes_delta) / (t["delta"].sum() * 1e-3) / 1e9)
    out["sigma_bytes_per_seed"] = float(np.mean(bytes_sigma))
    out["delta_bytes_per_seed"] = float(np.mean(bytes_delta))

    if args.sweep:
        out["sweep"] = {}
        for w in (16, 64, 256):
            eng.set_tuning(L.TUNE_BC_WAVE_ROW, w)
            tw, iw = bc_point()
            assert {k: iw[k] for k in ("sources", "reached_pairs", "max_depth")} == \
                   {k: info[k] for k in ("sources", "reached_pairs", "max_depth")}
            out["sweep"][str(w)] = summary(tw)
        eng.set_tuning(L.TUNE_BC_WAVE_ROW, -1)
    eng.close()
    shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
