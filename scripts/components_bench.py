#!/usr/bin/env python3
"""Connected components on the bench's RMAT bothE graph: the native program (tgo_components)
timed with the ctx's HIP events, and — with --generic — the baseline it replaces, the generic
min-label ConnectedComponents program (tests/generic_programs.py) through GpuGraphComputer.

    python scripts/components_bench.py [--scale 24] [--edge-factor 16] [--warmup 2] [--runs 10] [--generic]

Prints one JSON line.  Algorithmic bytes of the hook path (the roofline's denominator): one pass
over the OUT lists (4 bytes per entry), their offsets (8 (n + 1)), the parent array (4 n) and the
label array (8 n); of the propagate path: both lists and their offsets per round plus the labels.
The fraction is against 8 TB/s.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)

PEAK_BYTES_PER_S = 8.0e12


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--scale", type=int, default=24)
    p.add_argument("--edge-factor", type=int, default=16)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--runs", type=int, default=10)
    p.add_argument("--generic", action="store_true", help="also time the generic program through the computer")
    p.add_argument("--native", type=int, default=1, help="0: only the generic baseline (a tree without tgo_components)")
    args = p.parse_args()
    if args.runs < 1:
        p.error("--runs must be >= 1")

    from titan_amd import Engine, GpuGraph, rmat_edges
    from titan_amd import _lib as L

    n = 1 << args.scale
    src, dst, _ = rmat_edges(args.scale, args.edge_factor, seed=0x54495441)      # the graph of bench.py
    out = {"workload": f"rmat{args.scale}-ef{args.edge_factor}-bothE-components", "vertices": n, "edges": int(len(src))}

    if args.native:
        eng = Engine(device=0).load_edges(n, src, dst, L.SCOPE_BOTH_E, apply_cap=False)
        st = eng.stats()
        for _ in range(args.warmup):
            eng.components(fetch=False)
        ms = []
        for _ in range(args.runs):
            _, info = eng.components(fetch=False)
            ms.append(eng.stats()["last_kernel_ms"])
        labels = eng.copy_components()
        sizes = np.unique(labels, return_counts=True)[1]
        assert len(sizes) == info["components"]
        med = float(np.median(ms))
        if info["path"] == L.CC_HOOK:
            bytes_ = 4 * st["out_entries"] + 8 * (n + 1) + 4 * n + 8 * n
        else:
            bytes_ = info["rounds"] * (4 * (st["out_entries"] + st["in_entries"]) + 16 * (n + 1)) + 8 * n
        out.update({"path": "hook" if info["path"] == L.CC_HOOK else "propagate", "rounds": info["rounds"],
                    "components": info["components"], "largest_component": int(sizes.max()),
                    "native_ms_median": med, "native_ms_min": float(min(ms)), "native_ms_max": float(max(ms)),
                    "runs": args.runs, "algorithmic_bytes": int(bytes_),
                    "fraction_of_8TBps": bytes_ / (med * 1e-3) / PEAK_BYTES_PER_S,
                    "device_bytes": eng.stats()["device_bytes"]})
        eng.close()

    if args.generic:
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from generic_programs import ConnectedComponents
        graph = GpuGraph(edges=(n, src, dst, None), apply_cap=False)
        graph.engine_for(L.SCOPE_BOTH_E)                                       # the load is not part of the time
        t0 = time.perf_counter()
        res = graph.compute().program(ConnectedComponents()).submit().get()
        wall = (time.perf_counter() - t0) * 1e3
        cc = res.vertex_properties["cc"][1][0]
        out.update({"generic_ms": wall, "generic_supersteps": res.memory().getIteration(),
                    "generic_components": int(len(np.unique(cc)))})
        if args.native:
            ids = res.vertex_properties["cc"][0]
            assert np.array_equal(ids, np.arange(1, n + 1, dtype=np.int64) << 3) and np.array_equal(cc, labels)
            out["generic_over_native"] = wall / out["native_ms_median"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
