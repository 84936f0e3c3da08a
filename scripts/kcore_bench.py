#!/usr/bin/env python3
"""k-core decomposition on the bench's RMAT bothE graph (tgo_kcore), timed with the ctx's HIP
events: the median of --runs runs after --warmup, the one-off list build separately (wall of the
first call minus its kernel time), and the result's figures.

    python scripts/kcore_bench.py [--scale 20] [--edge-factor 16] [--warmup 2] [--runs 10]
                                  [--sweep] [--host 1] [--threads 16] [--generic 1]

--sweep    times TGO_TUNE_CORE_TAIL, then TGO_TUNE_CORE_WAVE_ROW and TGO_TUNE_CORE_LDS_QUEUE at the
           best tail (DESIGN.md 4.6 records the sweep the defaults in api_kcore.cpp come from).
--host     rebuilds the projection on the host from the assembled device lists and peels it with
           --threads threads (scripts/kcore_host.cpp, compiled on first use); checks the device's
           core numbers against it.
--generic  also runs the H-index iteration as a generic vertex program without a combiner (every
           vertex's message list comes to the host each superstep) and reports its wall time; it
           needs a duplicate-free, loop-free edge list, which is built from the same graph.

Prints one JSON line.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))         # kcore_generic: the one copy of the generic program
HERE = os.path.dirname(os.path.abspath(__file__))
FIXED = ("degeneracy", "innermost", "simple_edges", "levels")


def host_lib():
    so = os.path.join(HERE, "libkcore_host.so")
    src = os.path.join(HERE, "kcore_host.cpp")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.run(["g++", "-O3", "-std=c++17", "-shared", "-fPIC", "-pthread", src, "-o", so], check=True)
    lib = C.CDLL(so)
    i64p, i32p = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    lib.kcore_host_projection.argtypes = [C.c_int64, i64p, i32p, i64p, i32p, i64p, i64p, i32p, C.c_int]
    lib.kcore_host_projection.restype = None
    lib.kcore_host_peel.argtypes = [C.c_int64, i64p, i32p, i32p, C.c_int]
    lib.kcore_host_peel.restype = C.c_int64
    return lib


def timed(eng, runs):
    ms, rounds, info = [], [], None
    for _ in range(runs):
        _, info = eng.kcore(fetch=False)
        ms.append(eng.stats()["last_kernel_ms"])
        rounds.append(info["rounds"])
    return ms, rounds, info


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--scale", type=int, default=20)
    p.add_argument("--edge-factor", type=int, default=16)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--runs", type=int, default=10)
    p.add_argument("--sweep", action="store_true")
    p.add_argument("--sweep-runs", type=int, default=3)
    p.add_argument("--host", type=int, default=0)
    p.add_argument("--threads", type=int, default=16)
    p.add_argument("--generic", type=int, default=0)
    args = p.parse_args()
    if args.runs < 1:
        p.error("--runs must be >= 1")

    from titan_amd import Engine, GpuGraph, rmat_edges
    from titan_amd import _lib as L

    n = 1 << args.scale
    src, dst, _ = rmat_edges(args.scale, args.edge_factor, seed=0x54495441)      # the graph of bench.py
    out = {"workload": f"rmat{args.scale}-ef{args.edge_factor}-bothE-kcore", "vertices": n, "edges": int(len(src))}
    eng = Engine(device=0).load_edges(n, src, dst, L.SCOPE_BOTH_E, apply_cap=False)
    if not args.generic:
        del src, dst
    loaded = eng.stats()["device_bytes"]
    eng.sync()
    t0 = time.perf_counter()
    _, info = eng.kcore(fetch=False)                    # builds and caches the forward and backward lists
    first_wall = (time.perf_counter() - t0) * 1e3
    first_kernel = eng.stats()["last_kernel_ms"]
    timed(eng, args.warmup)
    ms, rounds, info = timed(eng, args.runs)
    med = float(np.median(ms))
    core = eng.copy_cores()
    assert int(core.max()) == info["degeneracy"] and int((core == core.max()).sum()) == info["innermost"]
    assert len(np.unique(core)) == info["levels"]
    out.update({k: info[k] for k in FIXED})
    out.update({"rounds_min": int(min(rounds)), "rounds_max": int(max(rounds)),
                "ms_median": med, "ms_min": float(min(ms)), "ms_max": float(max(ms)), "runs": args.runs,
                "list_build_ms": first_wall - first_kernel, "first_call_ms": first_wall,
                "device_bytes_lists": eng.stats()["device_bytes"] - loaded,
                "isolated": int((core == 0).sum()), "mean_core": float(core.mean())})

    if args.sweep:
        def point(**keys):
            for k, v in keys.items():
                eng.set_tuning(getattr(L, "TUNE_CORE_" + k.upper()), v)
            t, r, i = timed(eng, args.sweep_runs)
            assert {k: i[k] for k in FIXED} == {k: info[k] for k in FIXED}      # policy only, never the result
            for k in keys:
                eng.set_tuning(getattr(L, "TUNE_CORE_" + k.upper()), -1)
            return {"ms": float(np.median(t)), "rounds": int(np.median(r))}
        sweep = {"tail": {}, "wave_row": {}, "lds_queue": {}}
        for t in (0, 256, 1024, 2048, 4096):
            sweep["tail"][str(t)] = point(tail=t)
        best_tail = int(min(sweep["tail"], key=lambda k: sweep["tail"][k]["ms"]))
        for w in (8, 16, 32, 64, 128, 256, 1 << 30):
            sweep["wave_row"][str(w)] = point(tail=best_tail, wave_row=w)
        for q in (1, 64, 256, 1024, 4096):
            sweep["lds_queue"][str(q)] = point(tail=best_tail, lds_queue=q)
        sweep["best_tail"] = best_tail
        out["sweep"] = sweep

    if args.host:
        lib = host_lib()
        o, i = eng.graph_csr(0), eng.graph_csr(1)
        ptr = L.ptr
        a = (n, ptr(o["off"], C.c_int64), ptr(o["adj"], C.c_int32), ptr(i["off"], C.c_int64), ptr(i["adj"], C.c_int32))
        t0 = time.perf_counter()
        d = np.zeros(n + 1, np.int64)
        lib.kcore_host_projection(*a, ptr(d, C.c_int64), None, None, args.threads)
        off = np.zeros(n + 1, np.int64)
        np.cumsum(d[:-1], out=off[1:])
        assert int(off[-1]) == 2 * info["simple_edges"]
        adj = np.zeros(max(1, int(off[-1])), np.int32)
        lib.kcore_host_projection(*a, None, ptr(off, C.c_int64), ptr(adj, C.c_int32), args.threads)
        out["host_projection_ms"] = (time.perf_counter() - t0) * 1e3
        del o, i
        hcore = np.zeros(n, np.int32)
        t0 = time.perf_counter()
        top = int(lib.kcore_host_peel(n, ptr(off, C.c_int64), ptr(adj, C.c_int32), ptr(hcore, C.c_int32), args.threads))
        out["host_peel_ms"] = (time.perf_counter() - t0) * 1e3
        out["host_threads"] = args.threads
        assert top == info["degeneracy"]
        assert np.array_equal(hcore[eng.graph_perm()], core)        # internal ids -> row order
        out["host_over_device"] = out["host_peel_ms"] / med
    eng.close()

    if args.generic:
        from kcore_generic import GenericKCore, simple_edges
        graph = GpuGraph(edges=(n, *simple_edges(n, src, dst), None))
        t0 = time.perf_counter()
        res = graph.compute().program(GenericKCore()).submit().get()
        out["generic_wall_ms"] = (time.perf_counter() - t0) * 1e3
        out["generic_supersteps"] = int(res.memory().getIteration())
        gids, (gcore, _) = res.vertex_properties["core"]
        assert np.array_equal(np.asarray(gcore, np.int64), core)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
