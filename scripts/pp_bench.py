#!/usr/bin/env python3
"""Peer-pressure clustering on the bench's RMAT bothE graph (tgo_peer_pressure): for vote_scope OUT and
BOTH, distribute 0 and 1, the device time of the spans (peer_pressure.first / .vote = the lane tier of
round 1 / of a later round, peer_pressure.queue = the wave and the workgroup tier of a round, from the
engine's trace), the rounds to convergence, the whole call, and the bytes per second a later round
reaches against its algorithmic bytes: 4 B of adjacency + 4 B (distribute: 8 B) of vote per receive
entry + 8 (n + 1) of offsets + 12 n of own vote, new vote and change.  The same program as a generic
vertex program without a combiner (tests/pp_generic.py: tgo_gather_lists hands every message list to
the host, each superstep) is timed whole for vote_scope OUT, distribute 0 on the same graph in the same
run, with the share of tgo_gather_lists alone: the way to run the program before the native one.

    python scripts/pp_bench.py [--scale 20] [--edge-factor 16] [--warmup 1] [--runs 5] [--max-rounds 30]
                               [--sweep] [--no-generic]

--sweep    repeats the OUT / distribute 0 and OUT / distribute 1 timings at three values of each of
           TGO_TUNE_PP_WAVE_ROW, _BLOCK_ROW and _SLOTS (DESIGN.md 4.9 records it).

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
sys.path.insert(0, os.path.join(ROOT, "tests"))
TIERS = ("lane", "wave", "block")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--scale", type=int, default=20)
    p.add_argument("--edge-factor", type=int, default=16)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--max-rounds", type=int, default=30)
    p.add_argument("--sweep", action="store_true")
    p.add_argument("--no-generic", action="store_true")
    args = p.parse_args()
    if args.runs < 1:
        p.error("--runs must be >= 1")

    from titan_amd import Engine, GpuGraph, rmat_edges, trace
    from titan_amd import _lib as L
    from pp_generic import GenericPeerPressure                      # tests/pp_generic.py: the baseline program lives with the tests that pin it

    n = 1 << args.scale
    src, dst, _ = rmat_edges(args.scale, args.edge_factor, seed=0x54495441)      # the graph of bench.py
    out = {"workload": f"rmat{args.scale}-ef{args.edge_factor}-bothE-peer-pressure", "vertices": n, "edges": int(len(src)),
           "max_rounds": args.max_rounds}
    eng = Engine(device=0).load_edges(n, src, dst, L.SCOPE_BOTH_E, apply_cap=False)
    loaded = eng.stats()["device_bytes"]
    eng.sync()
    t0 = time.perf_counter()
    eng.peer_pressure(max_rounds=0, fetch=False)                    # builds and caches the ranks
    out["rank_build_ms"] = (time.perf_counter() - t0) * 1e3
    out["device_bytes_ranks"] = eng.stats()["device_bytes"] - loaded
    entries = {L.SCOPE_OUT_E: len(eng.graph_csr(1)["adj"]), L.SCOPE_BOTH_E: len(eng.graph_csr(0)["adj"]) + len(eng.graph_csr(1)["adj"])}
    names = {L.SCOPE_OUT_E: "outE", L.SCOPE_BOTH_E: "bothE"}
    tmp = tempfile.mkdtemp(prefix="pp_bench_")

    def point(scope, d):
        """Medians over --runs: per-tier ms of round 1 and of a later round (mean over the rounds), call ms."""
        first, later, call, infos = [], [], [], []
        for r in range(args.warmup + args.runs):
            path = os.path.join(tmp, f"trace_{r}.json")
            trace.clear()
            trace.enable(path)
            _, info = eng.peer_pressure(scope, bool(d), args.max_rounds, fetch=False)
            ms = eng.stats()["last_kernel_ms"]
            trace.flush(path)
            trace.disable()
            if r < args.warmup:
                continue
            f, lt = dict.fromkeys(TIERS, 0.0), dict.fromkeys(TIERS, 0.0)
            for e in trace.load_events(path):
                if e.get("cat") != "device" or not e["name"].startswith("peer_pressure."):
                    continue
                a = e.get("args", {})
                kind = e["name"].split(".")[1]
                if kind not in ("first", "vote", "queue"):
                    continue
                tier = "lane" if kind != "queue" else ("wave" if "wave_rows" in a else "block")
                (f if int(a["round"]) == 1 else lt)[tier] += e["dur"] / 1e3
            first.append([f[t] for t in TIERS])
            later.append([lt[t] / max(info["rounds"] - 1, 1) for t in TIERS])
            call.append(ms)
            infos.append(info)
        assert all(i == infos[0] for i in infos)                    # deterministic, rounds included
        first, later = np.median(np.asarray(first), axis=0), np.median(np.asarray(later), axis=0)
        per_round_bytes = entries[scope] * (4 + (8 if d else 4)) + 8 * (n + 1) + 12 * n
        res = {"rounds": infos[0]["rounds"], "converged": infos[0]["converged"], "clusters": infos[0]["clusters"],
               "largest": infos[0]["largest"], "call_ms": float(np.median(call)),
               "call_ms_spread": [float(min(call)), float(max(call))],
               "first_round_ms": {t: round(float(x), 4) for t, x in zip(TIERS, first)},
               "later_round_ms": {t: round(float(x), 4) for t, x in zip(TIERS, later)},
               "bytes_per_round": per_round_bytes}
        if infos[0]["rounds"] > 1 and later.sum() > 0:
            res["later_round_gb_per_s"] = float(per_round_bytes / (later.sum() * 1e-3) / 1e9)
        res["first_round_gb_per_s"] = float(per_round_bytes / (first.sum() * 1e-3) / 1e9)
        print(f"[pp_bench] {names[scope]}/{d}: {json.dumps(res)}", file=sys.stderr, flush=True)
        return res

    out["native"] = {}
    for scope in (L.SCOPE_OUT_E, L.SCOPE_BOTH_E):
        for d in (0, 1):
            out["native"][f"{names[scope]}/{d}"] = point(scope, d)

    if args.sweep:
        out["sweep"] = {}
        keys = (("wave_row", L.TUNE_PP_WAVE_ROW, (8, 16, 32)), ("block_row", L.TUNE_PP_BLOCK_ROW, (512, 2048, 8192)),
                ("slots", L.TUNE_PP_SLOTS, (256, 512, 1024)))
        for name, key, values in keys:
            for v in values:
                eng.set_tuning(key, v)
                for scope, d in ((L.SCOPE_OUT_E, 0), (L.SCOPE_OUT_E, 1)):
                    r = point(scope, d)
                    base = out["native"][f"{names[scope]}/{d}"]
                    assert (r["rounds"], r["clusters"], r["largest"]) == (base["rounds"], base["clusters"], base["largest"])
                    out["sweep"][f"{name}={v} {names[scope]}/{d}"] = {k: r[k] for k in ("call_ms", "call_ms_spread", "later_round_ms")}
                    print(f"[pp_bench] sweep {name}={v}", file=sys.stderr, flush=True)
            eng.set_tuning(key, -1)
    eng.close()

    if not args.no_generic:
        # vote_scope OUT, distribute 0 only: a superstep sorts every message on the host
        graph = GpuGraph(edges=(n, src, dst, None), apply_cap=False)
        geng = graph.engine_for(L.SCOPE_BOTH_E, 0, column_order=True)   # the engine the program runs on; its load is not timed
        gather = {"ms": 0.0, "calls": 0}
        plain = geng.gather_lists

        def timed(*a, **k):
            t = time.perf_counter()
            r = plain(*a, **k)
            gather["ms"] += (time.perf_counter() - t) * 1e3
            gather["calls"] += 1
            return r
        geng.gather_lists = timed
        prog = GenericPeerPressure("outE", False, args.max_rounds)
        print("[pp_bench] generic program", file=sys.stderr, flush=True)
        t0 = time.perf_counter()
        graph.compute().program(prog).submit().get()
        wall = (time.perf_counter() - t0) * 1e3
        native = out["native"]["outE/0"]
        assert prog.rounds == native["rounds"]
        out["generic"] = {"case": "outE/0", "wall_ms": wall, "rounds": prog.rounds, "gather_lists_ms": gather["ms"],
                          "gather_lists_calls": gather["calls"], "native_call_ms": native["call_ms"],
                          "speedup": wall / native["call_ms"], "speedup_over_gather_lists_alone": gather["ms"] / native["call_ms"]}
    shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
