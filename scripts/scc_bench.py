#!/usr/bin/env python3
"""Strongly connected components on the bench's RMAT bothE graph (tgo_scc), timed with the ctx's HIP
events: the median of --runs runs after --warmup, and the result's figures.

    python scripts/scc_bench.py [--scale 20] [--edge-factor 16] [--warmup 2] [--runs 12]
                                [--sweep] [--phases] [--host 1] [--generic 1]

--sweep    times TGO_TUNE_SCC_WAVE_ROW in {lane-only, 8, 32, 64} x TGO_TUNE_SCC_TAIL in {0, 256, 1024,
           4096} (DESIGN.md 4.7 records the sweep).
--phases   one more run with the trace on: the device time of every scc.* span, summed by name.
--host     Tarjan on one host thread (scripts/scc_host.cpp, compiled on first use; the algorithm does
           not parallelise) over the assembled device lists; checks the device's partition against it.
--generic  also runs the same colouring as a generic vertex program (tests/scc_generic.py: one
           tgo_gather and two host round trips per superstep) and reports its wall time without the load.

Prints one JSON line.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))         # scc_generic: the one copy of the generic program
HERE = os.path.dirname(os.path.abspath(__file__))
FIXED = ("components", "largest", "singletons")


def host_lib():
    so = os.path.join(HERE, "libscc_host.so")
    src = os.path.join(HERE, "scc_host.cpp")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.run(["g++", "-O3", "-std=c++17", "-shared", "-fPIC", src, "-o", so], check=True)
    lib = C.CDLL(so)
    lib.scc_host_tarjan.argtypes = [C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.scc_host_tarjan.restype = C.c_int64
    return lib


def timed(eng, runs):
    ms, rounds, passes, info = [], [], [], None
    for _ in range(runs):
        _, info = eng.scc(fetch=False)
        ms.append(eng.stats()["last_kernel_ms"])
        rounds.append(info["rounds"])
        passes.append(info["passes"])
    return ms, rounds, passes, info


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--scale", type=int, default=20)
    p.add_argument("--edge-factor", type=int, default=16)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--runs", type=int, default=12)
    p.add_argument("--sweep", action="store_true")
    p.add_argument("--sweep-runs", type=int, default=3)
    p.add_argument("--phases", action="store_true")
    p.add_argument("--host", type=int, default=0)
    p.add_argument("--generic", type=int, default=0)
    args = p.parse_args()
    if args.runs < 1:
        p.error("--runs must be >= 1")

    from titan_amd import Engine, GpuGraph, rmat_edges, trace
    from titan_amd import _lib as L

    n = 1 << args.scale
    src, dst, _ = rmat_edges(args.scale, args.edge_factor, seed=0x54495441)      # the graph of bench.py
    out = {"workload": f"rmat{args.scale}-ef{args.edge_factor}-bothE-scc", "vertices": n, "edges": int(len(src))}
    eng = Engine(device=0).load_edges(n, src, dst, L.SCOPE_BOTH_E, apply_cap=False)
    if not args.generic:
        del src, dst
    st = eng.stats()
    out["entries"] = int(st["out_entries"] + st["in_entries"])
    timed(eng, args.warmup)
    ms, rounds, passes, info = timed(eng, args.runs)
    med = float(np.median(ms))
    lab = eng.copy_scc()
    sizes = np.unique(lab, return_counts=True)[1]
    assert len(sizes) == info["components"] and int(sizes.max()) == info["largest"]
    assert int((sizes == 1).sum()) == info["singletons"]
    out.update({k: info[k] for k in FIXED})
    out.update({"rounds_min": int(min(rounds)), "rounds_max": int(max(rounds)), "passes_min": int(min(passes)),
                "passes_max": int(max(passes)), "ms_median": med, "ms_min": float(min(ms)), "ms_max": float(max(ms)),
                "runs": args.runs})
    # algorithmic bytes: the degrees' pass and the trim's walk of every retired vertex read both
    # lists once each (4 bytes an entry, 8 an offset); the state arrays (comp, two degrees, mark:
    # int32) are written once and read at least once
    out["algorithmic_bytes"] = int(2 * (4 * out["entries"] + 2 * 8 * n) + 2 * 4 * 4 * n)
    out["algorithmic_gb_s"] = out["algorithmic_bytes"] / (med * 1e-3) / 1e9

    if args.phases:
        path = os.path.join(tempfile.mkdtemp(), "scc_trace.json")
        trace.clear()
        trace.enable(path)
        eng.scc(fetch=False)
        trace.flush(path)
        trace.disable()
        phases = {}
        for ev in trace.load_events(path):
            if ev.get("ph") == "X" and str(ev.get("name", "")).startswith("scc."):
                ph = phases.setdefault(ev["name"], {"ms": 0.0, "spans": 0})
                ph["ms"] += ev["dur"] / 1e3
                ph["spans"] += 1
        out["phases"] = phases

    if args.sweep:
        def point(wave_row, tail):
            eng.set_tuning(L.TUNE_SCC_WAVE_ROW, wave_row).set_tuning(L.TUNE_SCC_TAIL, tail)
            t, r, ps, i = timed(eng, args.sweep_runs)
            assert {k: i[k] for k in FIXED} == {k: info[k] for k in FIXED}      # policy only, never the result
            eng.set_tuning(L.TUNE_SCC_WAVE_ROW, -1).set_tuning(L.TUNE_SCC_TAIL, -1)
            return {"ms": float(np.median(t)), "rounds": int(np.median(r)), "passes": int(np.median(ps))}
        out["sweep"] = {f"{'lane' if w > 1 << 40 else w}/{t}": point(w, t)
                        for w in (1 << 50, 8, 32, 64) for t in (0, 256, 1024, 4096)}

    if args.host:
        lib = host_lib()
        o = eng.graph_csr(0)
        comp = np.zeros(n, np.int32)
        t0 = time.perf_counter()
        k = int(lib.scc_host_tarjan(n, L.ptr(o["off"], C.c_int64), L.ptr(o["adj"], C.c_int32), L.ptr(comp, C.c_int32)))
        out["host_tarjan_ms"] = (time.perf_counter() - t0) * 1e3
        out["host_threads"] = 1
        assert k == info["components"]
        # the same partition: every host component carries one device label and the counts agree
        hc = comp[eng.graph_perm()]                     # internal ids -> row order
        pairs = np.unique(np.stack([hc.astype(np.int64), lab]), axis=1)
        assert pairs.shape[1] == k
        out["host_over_device"] = out["host_tarjan_ms"] / med
        del o
    eng.close()

    if args.generic:
        from scc_generic import GenericScc
        graph = GpuGraph(edges=(n, src, dst, None))
        graph.engine_for(L.SCOPE_BOTH_E)                # the load is not part of the time
        prog = GenericScc()
        t0 = time.perf_counter()
        res = graph.compute().program(prog).submit().get()
        out["generic_wall_ms"] = (time.perf_counter() - t0) * 1e3
        out["generic_supersteps"] = int(res.memory().getIteration())
        out["generic_passes"] = int(prog.passes)
        gids, (glab, _) = res.vertex_properties["scc"]
        assert len(np.unique(glab)) == info["components"]
        assert np.array_equal(np.asarray(glab, np.int64), lab)
        out["generic_over_device"] = out["generic_wall_ms"] / med
    print(json.dumps(out))


if __name__ == "__main__":
    main()
