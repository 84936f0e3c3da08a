#!/usr/bin/env python3
"""Triangle counting on the bench's RMAT bothE graph (tgo_triangles), timed with the ctx's HIP
events: the median of --runs runs after --warmup, the one-off forward-list build separately (wall
of the first call minus its kernel time), and the counts.

    python scripts/triangles_bench.py [--scale 20] [--edge-factor 16] [--warmup 2] [--runs 10]
                                      [--sweep] [--host 1] [--threads 16]

--sweep  times TGO_TUNE_TRI_BLOCK_ROW without wave rows (wave row = block row), then
         TGO_TUNE_TRI_WAVE_ROW below the best block row (the defaults in api_tri.cpp were chosen from this).
--host   rebuilds the forward lists on the host from the assembled device lists
         (scripts/tri_host_count.cpp, compiled on first use): the work measure
         sum min(|fwd(c)|, |fwd(b)|) over oriented entries and a --threads host count of the same
         lists as a sanity ratio.

Prints one JSON line.  Algorithmic bytes (the roofline's denominator): one pass over the forward
lists, 4 bytes per entry + 8 (n + 1) of offsets; the fraction is against 8 TB/s.  The count is not
a streaming pass — every entry (c, b) reads fwd(b) again — so the fraction says how far from a
single pass the intersection work is, not how well HBM is used.
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

PEAK_BYTES_PER_S = 8.0e12
HERE = os.path.dirname(os.path.abspath(__file__))


def host_lib():
    so = os.path.join(HERE, "libtri_host_count.so")
    src = os.path.join(HERE, "tri_host_count.cpp")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.run(["g++", "-O3", "-std=c++17", "-shared", "-fPIC", "-pthread", src, "-o", so], check=True)
    lib = C.CDLL(so)
    i64p, i32p = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    lib.tri_host_forward.argtypes = [C.c_int64, i64p, i32p, i64p, i32p, i64p, i64p, i32p, C.c_int]
    lib.tri_host_forward.restype = None
    for f in (lib.tri_host_work, lib.tri_host_count):
        f.argtypes = [C.c_int64, i64p, i32p, C.c_int]
        f.restype = C.c_int64
    return lib


def timed(eng, runs):
    ms = []
    for _ in range(runs):
        _, info = eng.triangles(fetch=False)
        ms.append(eng.stats()["last_kernel_ms"])
    return ms, info


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
    args = p.parse_args()
    if args.runs < 1:
        p.error("--runs must be >= 1")

    from titan_amd import Engine, rmat_edges
    from titan_amd import _lib as L

    n = 1 << args.scale
    src, dst, _ = rmat_edges(args.scale, args.edge_factor, seed=0x54495441)      # the graph of bench.py
    out = {"workload": f"rmat{args.scale}-ef{args.edge_factor}-bothE-triangles", "vertices": n, "edges": int(len(src))}
    eng = Engine(device=0).load_edges(n, src, dst, L.SCOPE_BOTH_E, apply_cap=False)
    del src, dst
    bytes_loaded = eng.stats()["device_bytes"]
    eng.sync()
    t0 = time.perf_counter()
    _, info = eng.triangles(fetch=False)                # builds and caches the forward lists
    first_wall = (time.perf_counter() - t0) * 1e3
    first_kernel = eng.stats()["last_kernel_ms"]
    timed(eng, args.warmup)
    ms, info = timed(eng, args.runs)
    med = float(np.median(ms))
    fnnz = info["simple_edges"]                         # one forward entry per simple edge
    bytes_ = 4 * fnnz + 8 * (n + 1)
    tri, deg, lcc = eng.copy_triangles()
    assert int(tri.sum()) == 3 * info["triangles"] and int(deg.sum()) == 2 * fnnz
    out.update({"triangles": info["triangles"], "wedges": info["wedges"], "simple_edges": fnnz,
                "max_forward": info["max_forward"], "transitivity": info["transitivity"],
                "max_degree": int(deg.max()), "mean_lcc": float(lcc.mean()),
                "ms_median": med, "ms_min": float(min(ms)), "ms_max": float(max(ms)), "runs": args.runs,
                "forward_build_ms": first_wall - first_kernel, "first_call_ms": first_wall,
                "forward_list_bytes": int(bytes_), "fraction_of_8TBps": bytes_ / (med * 1e-3) / PEAK_BYTES_PER_S,
                "device_bytes_forward_lists": eng.stats()["device_bytes"] - bytes_loaded})

    if args.sweep:
        def point(wave_row, block_row):
            eng.set_tuning(L.TUNE_TRI_WAVE_ROW, wave_row).set_tuning(L.TUNE_TRI_BLOCK_ROW, block_row)
            t, i = timed(eng, args.sweep_runs)
            assert i == info                            # policy only, never the result
            return float(np.median(t))
        off = info["max_forward"] + 1                   # no row reaches the path
        sweep = {"wave_row": {}, "block_row": {}}
        # the lane / block boundary first, no wave rows (wave_row = block_row) ...
        for b in (4, 8, 16, 32, 64, 128, 256, 1024, off):
            sweep["block_row"][str(b)] = point(b, b)
        best_b = int(min(sweep["block_row"], key=sweep["block_row"].get))
        # ... then the rows below it that go to a wave of their own
        for w in [w for w in (2, 4, 8, 16, 32, 64, 128) if w < best_b] + [best_b]:
            sweep["wave_row"][str(w)] = point(w, best_b)
        best = min(sweep["wave_row"], key=sweep["wave_row"].get)
        sweep["best_block_row"] = best_b
        if args.scale <= 22:                            # one lane per hub row: minutes at scale 24
            sweep["lane_only"] = point(off, off)
        sweep["wave_only"] = point(1, off)
        sweep["block_all"] = point(off, 2)
        sweep["best_wave_row"] = int(best)
        sweep["off"] = off
        out["sweep_ms"] = sweep
        eng.set_tuning(L.TUNE_TRI_WAVE_ROW, -1).set_tuning(L.TUNE_TRI_BLOCK_ROW, -1)

    if args.host:
        lib = host_lib()
        o, i = eng.graph_csr(0), eng.graph_csr(1)
        ptr = L.ptr
        flen = np.zeros(n + 1, np.int64)
        a = (n, ptr(o["off"], C.c_int64), ptr(o["adj"], C.c_int32), ptr(i["off"], C.c_int64), ptr(i["adj"], C.c_int32))
        lib.tri_host_forward(*a, ptr(flen, C.c_int64), None, None, args.threads)
        foff = np.zeros(n + 1, np.int64)
        np.cumsum(flen[:-1], out=foff[1:])
        assert int(foff[-1]) == fnnz and int(flen.max()) == info["max_forward"]
        fadj = np.zeros(max(1, fnnz), np.int32)
        lib.tri_host_forward(*a, None, ptr(foff, C.c_int64), ptr(fadj, C.c_int32), args.threads)
        del o, i
        out["work_min_rows"] = int(lib.tri_host_work(n, ptr(foff, C.c_int64), ptr(fadj, C.c_int32), args.threads))
        t0 = time.perf_counter()
        host_tri = int(lib.tri_host_count(n, ptr(foff, C.c_int64), ptr(fadj, C.c_int32), args.threads))
        out["host_count_ms"] = (time.perf_counter() - t0) * 1e3
        out["host_threads"] = args.threads
        assert host_tri == info["triangles"], (host_tri, info["triangles"])
        out["host_over_device"] = out["host_count_ms"] / med
        hist = np.bincount(np.minimum(np.ceil(np.log2(np.maximum(flen[:-1], 1))).astype(np.int64), 20), minlength=21)
        out["forward_rows_by_log2_length"] = hist.tolist()
        ent = np.bincount(np.minimum(np.ceil(np.log2(np.maximum(flen[:-1], 1))).astype(np.int64), 20),
                          weights=flen[:-1], minlength=21)
        out["forward_entries_by_log2_length"] = [int(x) for x in ent]
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
