#!/usr/bin/env python3
"""A/B of a multi-source tuning key on one engine (RMAT bothE, the bench's 64 roots): the key is set
between sweeps (tgo_set_tuning), rounds of interleaved values, 5 timed sweeps each after one untimed,
best / median / max device ms per sweep; the per-source stats must not move.
usage: python scripts/ms_key_ab.py [scale] [rounds] [values, comma separated] [key: head]
(profiles/pl1_ms_head_ab.log: python scripts/ms_key_ab.py 24 3 0,4,8,16,32,64 head)"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from titan_amd import Engine, pick_roots, rmat_edges  # noqa: E402
from titan_amd import _lib as L  # noqa: E402

scale = int(sys.argv[1]) if len(sys.argv) > 1 else 24
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
heads = [float(x) for x in sys.argv[3].split(",")] if len(sys.argv) > 3 else [0, 4, 8, 16, 32, 64]
name = sys.argv[4] if len(sys.argv) > 4 else "head"
key = {"head": L.TUNE_MS_HEAD}[name]
n = 1 << scale
src, dst, _ = rmat_edges(scale, 16, seed=0x54495441)
roots = [int(r) for r in pick_roots(n, src, dst, 64, seed=7)]
eng = Engine(host_threads=16).load_edges(n, src, dst, L.SCOPE_BOTH_E, apply_cap=False)
del src, dst
eng.bfs_multi(roots, n, L.SCOPE_BOTH_E, seed_is_dense=True, stats=True, fetch=False)
r0, e0 = eng.multi_stats(64)
for rnd in range(1, rounds + 1):
    for h in heads:
        eng.set_tuning(key, h)
        ts = []
        for _ in range(6):
            eng.bfs_multi(roots, n, L.SCOPE_BOTH_E, seed_is_dense=True, fetch=False)
            ts.append(eng.stats()["last_kernel_ms"])
        ts = ts[1:]
        print(f"round {rnd} {name} {h:3g}: best {min(ts):.3f} median {np.median(ts):.3f} max {max(ts):.3f} ms/sweep "
              f"levels {eng.stats()['levels']}", flush=True)
eng.bfs_multi(roots, n, L.SCOPE_BOTH_E, seed_is_dense=True, stats=True, fetch=False)
r1, e1 = eng.multi_stats(64)
print("stats identical:", bool(np.array_equal(r0, r1) and np.array_equal(e0, e1)))
