#!/usr/bin/env python3
"""Closeness / harmonic centrality on the bench's RMAT bothE graph (tgo_closeness) from --seeds of the
bench's root picker, 64 a sweep.  One-off measurement (DESIGN.md 4.10 records it).  Two stages, each a
fresh child process under its own time limit; the first that fails ends the run:

  fold    device ms per batch in the sweep and in the fold kernel (the engine's trace spans
          closeness.sweep / closeness.fold, median over --runs), the fold's byte estimate
          (1 + nplanes) * 8 n for the masks and planes + 56 n for the accumulators (harmonic read,
          far / reach / ecc / harmonic read-modify-write) and the bandwidth it implies; then the same
          batches through tgo_bfs_multi without dist_out, per batch
  route   the same seeds through tgo_bfs_multi with dist_out (64 x n int64 to the host per batch) and a
          numpy reduction to far / reach / ecc / closeness / harmonic, wall clock, against the wall
          clock of tgo_closeness with both arrays fetched; checks that the two agree

    python scripts/cl_bench.py [--scale 20] [--edge-factor 16] [--seeds 1024] [--warmup 1] [--runs 3]
                               [--limit 600]

Prints one JSON line.
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
STAGES = ("fold", "route")


def setup(args):
    from titan_amd import Engine, pick_roots, rmat_edges
    from titan_amd import _lib as L
    n = 1 << args.scale
    src, dst, _ = rmat_edges(args.scale, args.edge_factor, seed=0x54495441)      # the graph of bench.py
    roots = np.asarray(pick_roots(n, src, dst, args.seeds, seed=7), np.int64)     # and its root picker
    assert len(roots) == args.seeds
    eng = Engine(device=0).load_edges(n, src, dst, L.SCOPE_BOTH_E, apply_cap=False)
    return n, len(src), roots, eng, L


def stage_fold(args):
    from titan_amd import trace
    n, m, roots, eng, L = setup(args)
    batches = (len(roots) + 63) // 64
    out = {"workload": f"rmat{args.scale}-ef{args.edge_factor}-bothE-closeness{len(roots)}", "vertices": n, "edges": m,
           "seeds": int(len(roots)), "batches": batches}
    before = eng.stats()["device_bytes"]
    eng.closeness(roots[:64], dense=True, fetch=False)      # allocates the sweep's and the fold's scratch
    out["device_bytes_scratch"] = eng.stats()["device_bytes"] - before
    tmp = tempfile.mkdtemp(prefix="cl_bench_")
    got = {"closeness.sweep": [], "closeness.fold": []}
    planes, info, call_ms = None, None, []
    for r in range(args.warmup + args.runs):
        path = os.path.join(tmp, f"trace_{r}.json")
        trace.clear()
        trace.enable(path)
        _, info = eng.closeness(roots, dense=True, fetch=False)
        trace.flush(path)
        trace.disable()
        if r < args.warmup:
            continue
        call_ms.append(eng.stats()["last_kernel_ms"])
        ev = [e for e in trace.load_events(path) if e["cat"] == "device"]
        for k in got:
            d = [e["dur"] / 1e3 for e in ev if e["name"] == k]
            assert len(d) == batches, (k, len(d), batches)
            got[k].append(d)
        planes = [int(e["args"]["planes"]) for e in ev if e["name"] == "closeness.fold"]
    shutil.rmtree(tmp, ignore_errors=True)
    sweep = np.median(np.asarray(got["closeness.sweep"]), axis=0)
    fold = np.median(np.asarray(got["closeness.fold"]), axis=0)
    bytes_batch = np.asarray([(1 + p) * 8 * n + 56 * n for p in planes], np.float64)
    out.update({"sweep_ms_per_batch": float(sweep.mean()), "fold_ms_per_batch": float(fold.mean()),
                "fold_over_sweep": float(fold.sum() / sweep.sum()), "planes": planes,
                "fold_bytes_per_batch": float(bytes_batch.mean()),
                "fold_gb_per_s": float(bytes_batch.sum() / (fold.sum() * 1e-3) / 1e9),
                "call_ms": float(np.median(call_ms)), "per_batch_sweep_ms": [round(float(x), 4) for x in sweep],
                "per_batch_fold_ms": [round(float(x), 4) for x in fold]})
    out.update({k: info[k] for k in ("reached_pairs", "max_depth")})
    # the same batches through tgo_bfs_multi (no dist_out): the call's own HIP-event timing, tracing off
    plain = []
    for _ in range(args.runs):
        ms = []
        for b0 in range(0, len(roots), 64):
            eng.bfs_multi(roots[b0:b0 + 64], n, L.SCOPE_BOTH_E, seed_is_dense=True, fetch=False)
            ms.append(eng.stats()["last_kernel_ms"])
        plain.append(ms)
    out["per_batch_bfs_multi_ms"] = [round(float(x), 4) for x in np.median(np.asarray(plain), axis=0)]
    eng.close()
    return out


def stage_route(args):
    n, m, roots, eng, L = setup(args)
    eng.closeness(roots[:64], dense=True)                   # warm both routes' scratch
    eng.bfs_multi(roots[:64], n, L.SCOPE_BOTH_E, seed_is_dense=True)
    eng.sync()
    t0 = time.perf_counter()
    res, info = eng.closeness(roots, dense=True)
    native_ms = (time.perf_counter() - t0) * 1e3
    all5 = eng.copy_closeness()                             # before tgo_bfs_multi replaces the result
    t0 = time.perf_counter()
    far, reach, ecc = (np.zeros(n, np.int64) for _ in range(3))
    harm = np.zeros(n, np.float64)
    for b0 in range(0, len(roots), 64):
        d = eng.bfs_multi(roots[b0:b0 + 64], n, L.SCOPE_BOTH_E, seed_is_dense=True)
        pos = d > 0                                         # absent distances are negative
        dd = np.where(pos, d, 0)
        far += dd.sum(0)
        reach += pos.sum(0)
        np.maximum(ecc, dd.max(0), out=ecc)
        harm += np.divide(1.0, dd, out=np.zeros(d.shape, np.float64), where=pos).sum(0)
    close = np.divide(reach, far, out=np.zeros(n, np.float64), where=far > 0)
    host_ms = (time.perf_counter() - t0) * 1e3
    assert np.array_equal(all5["far"], far) and np.array_equal(all5["reach"], reach) and np.array_equal(all5["ecc"], ecc)
    assert close.tobytes() == res["closeness"].tobytes()
    worst = float(np.max(np.abs(harm - res["harmonic"]) / np.maximum(harm, 1e-300)))
    assert worst <= len(roots) * 2.0 ** -52, worst          # another summation order: within S 2^-52
    eng.close()
    return {"closeness_wall_ms": native_ms, "bfs_multi_numpy_wall_ms": host_ms, "host_route_over_native": host_ms / native_ms,
            "harmonic_worst_relative_difference": worst, "reached_pairs_route": int(reach.sum()),
            "reached_pairs_native": info["reached_pairs"]}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--scale", type=int, default=20)
    p.add_argument("--edge-factor", type=int, default=16)
    p.add_argument("--seeds", type=int, default=1024)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--runs", type=int, default=3)
    p.add_argument("--limit", type=int, default=600, help="seconds each stage may take")
    p.add_argument("--stage", choices=STAGES)
    args = p.parse_args()
    if args.runs < 1 or args.seeds < 1:
        p.error("--runs and --seeds must be >= 1")
    if args.stage:
        print(json.dumps({"fold": stage_fold, "route": stage_route}[args.stage](args)))
        return 0
    out = {}
    for stage in STAGES:                                    # a fresh process per stage, each under its own limit
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--stage", stage,
               "--scale", str(args.scale), "--edge-factor", str(args.edge_factor), "--seeds", str(args.seeds),
               "--warmup", str(args.warmup), "--runs", str(args.runs)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            print(json.dumps({"failed_stage": stage, "exit": r.returncode, **out}))
            return 1
        out.update(json.loads(r.stdout.strip().splitlines()[-1]))
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
