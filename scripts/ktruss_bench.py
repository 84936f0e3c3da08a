#!/usr/bin/env python3
"""k-truss decomposition on the bench's RMAT bothE graph (tgo_ktruss), timed with the ctx's HIP
events: the median of --runs runs after --warmup, split three ways —
  lists     the one-off build of the shared lists, the edge ids and the per-edge arrays (wall of
            the first call minus its kernel time)
  support   a run with k = 2: the support pass, one scan, the clamp and the finish; nothing is peeled
  peel      the full run minus the k = 2 run
— and the result's figures.

    python scripts/ktruss_bench.py [--scale 20] [--edge-factor 16] [--warmup 2] [--runs 10]
                                   [--sweep] [--sweep-runs 3] [--peel-sweep-runs 1] [--host 1] [--threads 16]

--sweep    times the support pass over wave_row x block_row (k = 2 runs), then the full run over
           peel_wave_row at the best pair, --peel-sweep-runs runs a point (DESIGN.md 4.11 records the sweep the defaults in
           api_truss.cpp come from).
--host     rebuilds the projection on the host from the assembled device lists and decomposes it
           with --threads threads (scripts/ktruss_host.cpp, PKT, compiled on first use; the
           projection by scripts/kcore_host.cpp); checks the device's edge values against it.

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
HERE = os.path.dirname(os.path.abspath(__file__))
FIXED = ("max_truss", "innermost_edges", "triangles", "simple_edges", "levels")


def host_libs():
    libs = []
    for name in ("kcore_host", "ktruss_host"):
        so = os.path.join(HERE, f"lib{name}.so")
        src = os.path.join(HERE, f"{name}.cpp")
        if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
            subprocess.run(["g++", "-O3", "-std=c++17", "-shared", "-fPIC", "-pthread", src, "-o", so], check=True)
        libs.append(C.CDLL(so))
    kc, kt = libs
    i64p, i32p = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    kc.kcore_host_projection.argtypes = [C.c_int64, i64p, i32p, i64p, i32p, i64p, i64p, i32p, C.c_int]
    kc.kcore_host_projection.restype = None
    kt.ktruss_host_edge_ids.argtypes = [C.c_int64, i64p, i32p, i32p, i32p, i32p, C.c_int]
    kt.ktruss_host_edge_ids.restype = C.c_int64
    kt.ktruss_host_support.argtypes = [C.c_int64, i64p, i32p, i32p, i32p, C.c_int]
    kt.ktruss_host_support.restype = None
    kt.ktruss_host_peel.argtypes = [C.c_int64, C.c_int64, i64p, i32p, i32p, i32p, i32p, i32p, i32p, i64p, C.c_int]
    kt.ktruss_host_peel.restype = C.c_int64
    return kc, kt


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def timed(eng, runs, **kw):
    ms, rounds, info = [], [], None
    for _ in range(runs):
        _, info = eng.ktruss(fetch=False, **kw)
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
    p.add_argument("--peel-sweep-runs", type=int, default=1)
    p.add_argument("--host", type=int, default=0)
    p.add_argument("--threads", type=int, default=16)
    args = p.parse_args()
    if args.runs < 1:
        p.error("--runs must be >= 1")

    from titan_amd import Engine, rmat_edges
    from titan_amd import _lib as L

    n = 1 << args.scale
    src, dst, _ = rmat_edges(args.scale, args.edge_factor, seed=0x54495441)      # the graph of bench.py
    out = {"workload": f"rmat{args.scale}-ef{args.edge_factor}-bothE-ktruss", "vertices": n, "edges": int(len(src))}
    eng = Engine(device=0).load_edges(n, src, dst, L.SCOPE_BOTH_E, apply_cap=False)
    del src, dst
    loaded = eng.stats()["device_bytes"]
    eng.sync()
    t0 = time.perf_counter()
    _, info = eng.ktruss(fetch=False)                   # builds and caches every list
    first_wall = (time.perf_counter() - t0) * 1e3
    first_kernel = eng.stats()["last_kernel_ms"]
    log(f"first call {first_wall:.1f} ms, of which kernels {first_kernel:.1f} ms; {info}")
    timed(eng, args.warmup)
    ms, rounds, info = timed(eng, args.runs)
    med = float(np.median(ms))
    vtruss = eng.copy_truss()
    u, v, truss, support = eng.copy_truss_edges()
    assert int(truss.max()) == info["max_truss"] and int((truss == truss.max()).sum()) == info["innermost_edges"]
    assert len(np.unique(truss)) == info["levels"] and int(support.sum()) == 3 * info["triangles"]
    assert int(vtruss.max()) == info["max_truss"]
    timed(eng, 1, k=2)
    sms, _, sinfo = timed(eng, args.runs, k=2)
    smed = float(np.median(sms))
    log(f"full run {med:.1f} ms, k = 2 run {smed:.1f} ms")
    assert sinfo["levels"] == 1 and sinfo["rounds"] == 0 and sinfo["triangles"] == info["triangles"]
    out.update({k: info[k] for k in FIXED})
    out.update({"rounds_min": int(min(rounds)), "rounds_max": int(max(rounds)),
                "ms_median": med, "ms_min": float(min(ms)), "ms_max": float(max(ms)), "runs": args.runs,
                "support_ms_median": smed, "support_ms_min": float(min(sms)), "support_ms_max": float(max(sms)),
                "peel_ms": med - smed, "triangles_per_s_support": info["triangles"] / (smed * 1e-3),
                "list_build_ms": first_wall - first_kernel, "first_call_ms": first_wall,
                "device_bytes_lists": eng.stats()["device_bytes"] - loaded,
                "device_bytes": eng.stats()["device_bytes"],
                "isolated": int((vtruss == 0).sum()), "mean_edge_truss": float(truss.mean())})

    if args.sweep:
        def point(**kw):
            t, r, i = timed(eng, args.sweep_runs if kw.get("k") == 2 else args.peel_sweep_runs, **kw)
            want = sinfo if kw.get("k") == 2 else info
            assert {k: i[k] for k in FIXED} == {k: want[k] for k in FIXED}      # policy only, never the result
            log(f"sweep {kw}: {float(np.median(t)):.1f} ms")
            return {"ms": float(np.median(t)), "rounds": int(np.median(r))}
        sweep = {"support": {}, "peel_wave_row": {}}
        for w in (2, 8, 32, 128, 1 << 20):
            for b in (2, 8, 32, 128, 1 << 20):
                sweep["support"][f"{w}x{b}"] = point(k=2, wave_row=w, block_row=b)
        best = min(sweep["support"], key=lambda k: sweep["support"][k]["ms"])
        bw, bb = (int(x) for x in best.split("x"))
        for q in (1, 8, 16, 32, 64, 128, 256, 1 << 20):
            sweep["peel_wave_row"][str(q)] = point(wave_row=bw, block_row=bb, peel_wave_row=q)
        sweep["best_support"] = best
        out["sweep"] = sweep

    if args.host:
        kc, kt = host_libs()
        o, i = eng.graph_csr(0), eng.graph_csr(1)
        ptr = L.ptr
        a = (n, ptr(o["off"], C.c_int64), ptr(o["adj"], C.c_int32), ptr(i["off"], C.c_int64), ptr(i["adj"], C.c_int32))
        t0 = time.perf_counter()
        d = np.zeros(n + 1, np.int64)
        kc.kcore_host_projection(*a, ptr(d, C.c_int64), None, None, args.threads)
        off = np.zeros(n + 1, np.int64)
        np.cumsum(d[:-1], out=off[1:])
        m = info["simple_edges"]
        assert int(off[-1]) == 2 * m
        adj = np.zeros(max(1, 2 * m), np.int32)
        kc.kcore_host_projection(*a, None, ptr(off, C.c_int64), ptr(adj, C.c_int32), args.threads)
        eid, eu, ev = np.zeros(max(1, 2 * m), np.int32), np.zeros(max(1, m), np.int32), np.zeros(max(1, m), np.int32)
        got = kt.ktruss_host_edge_ids(n, ptr(off, C.c_int64), ptr(adj, C.c_int32), ptr(eid, C.c_int32), ptr(eu, C.c_int32),
                                      ptr(ev, C.c_int32), args.threads)
        assert got == m
        out["host_lists_ms"] = (time.perf_counter() - t0) * 1e3
        del o, i
        hsup, htruss, hrounds = np.zeros(max(1, m), np.int32), np.zeros(max(1, m), np.int32), np.zeros(1, np.int64)
        t0 = time.perf_counter()
        kt.ktruss_host_support(n, ptr(off, C.c_int64), ptr(adj, C.c_int32), ptr(eid, C.c_int32), ptr(hsup, C.c_int32), args.threads)
        out["host_support_ms"] = (time.perf_counter() - t0) * 1e3
        log(f"host lists {out['host_lists_ms']:.0f} ms, support {out['host_support_ms']:.0f} ms")
        t0 = time.perf_counter()
        top = int(kt.ktruss_host_peel(n, m, ptr(off, C.c_int64), ptr(adj, C.c_int32), ptr(eid, C.c_int32), ptr(eu, C.c_int32),
                                      ptr(ev, C.c_int32), ptr(hsup, C.c_int32), ptr(htruss, C.c_int32),
                                      ptr(hrounds, C.c_int64), args.threads))
        out["host_peel_ms"] = (time.perf_counter() - t0) * 1e3
        out["host_rounds"] = int(hrounds[0])
        log(f"host peel {out['host_peel_ms']:.0f} ms, {out['host_rounds']} sub-rounds")
        out["host_threads"] = args.threads
        assert top == info["max_truss"]
        # internal ids -> Titan ids, then both edge lists in (u, v) order
        tid = np.empty(n, np.int64)
        tid[eng.graph_perm()] = eng.vertex_ids()
        hu, hv = tid[eu[:m]], tid[ev[:m]]
        hu, hv = np.minimum(hu, hv), np.maximum(hu, hv)
        ho, do = np.lexsort((hv, hu)), np.lexsort((v, u))
        assert np.array_equal(hu[ho], u[do]) and np.array_equal(hv[ho], v[do])
        assert np.array_equal(htruss[:m][ho], truss[do]) and np.array_equal(hsup[:m][ho], support[do])
        out["host_over_device"] = (out["host_support_ms"] + out["host_peel_ms"]) / med
        out["host_support_over_device"] = out["host_support_ms"] / smed
        out["host_peel_over_device"] = out["host_peel_ms"] / max(med - smed, 1e-9)
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
