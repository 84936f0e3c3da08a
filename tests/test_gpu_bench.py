"""GPU: bench.py's command line on a small graph (RMAT scale 12; the measured one is 24).

* a plain run times exactly --steps steps, reports ms_per_step, leaves the side measurements
  (single-source BFS, SSSP, rows, CPU baseline, self-check) out of the result line, and
  --dump-outputs writes what the last timed step computed: float64 arrays equal to what the
  fetching engine calls return on the same graph and roots;
* --full brings every side measurement back.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from titan_amd import Engine, pick_roots, rmat_edges
from titan_amd import _lib as L

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE = 12
SMALL = ["--gpus", "1", "--scale", str(SCALE), "--rows-scale", "10"]
SIDE_KEYS = ("single_source_gteps_hmean", "cpu_baseline", "sssp", "config2_rows", "validation")


def run_bench(*extra):
    """One bench.py process; the single JSON line it prints on stdout."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *SMALL, *extra], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [x for x in p.stdout.splitlines() if x.strip()]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_plain_run_is_lean_and_dumps_the_last_step(tmp_path):
    out = str(tmp_path / "dump")
    line = run_bench("--steps", "3", "--warmup", "1", "--dump-outputs", out)
    assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False
    assert line["unit"] == "GTEPS" and line["higher_is_better"] is True and line["value"] > 0
    assert line["dtype"] == "int32 (BFS levels); f64 (PageRank)" and line["metric"]
    assert line["ms_per_step"] > 0
    for k in SIDE_KEYS:
        assert line[k] is None, k
    # the dump: float64, the whole result at this size (n <= the sample), <= 64 MB in all
    assert sorted(os.listdir(out)) == ["bfs_levels.npy", "pagerank.npy", "sample_vertices.npy"]
    dump = {f[:-4]: np.load(os.path.join(out, f)) for f in os.listdir(out)}
    assert all(a.dtype == np.float64 for a in dump.values())
    assert sum(a.nbytes for a in dump.values()) <= 64 << 20
    n = 1 << SCALE
    assert np.array_equal(dump["sample_vertices"], np.arange(n))
    # the same graph, roots and programs through the fetching calls
    src, dst, _ = rmat_edges(SCALE, 16, seed=0x54495441)
    roots = pick_roots(n, src, dst, 64, seed=7)
    lv = Engine().load_edges(n, src, dst, L.SCOPE_BOTH_E, apply_cap=False).bfs_multi(
        roots, n, L.SCOPE_BOTH_E, seed_is_dense=True)
    assert dump["bfs_levels"].shape == lv.shape and np.array_equal(dump["bfs_levels"], lv.astype(np.float64))
    pr = Engine().load_edges(n, src, dst, L.SCOPE_IN_E, apply_cap=True).pagerank(0.85, n, 20)
    assert dump["pagerank"].shape == pr.shape and np.isfinite(dump["pagerank"]).all()
    assert float(np.abs(dump["pagerank"] - pr).sum()) <= 1e-12      # fp64 sums of ~1/n terms, L1 ~ 1


def test_full_run_reports_the_side_measurements():
    line = run_bench("--steps", "2", "--warmup", "1", "--full")
    assert line["steps"] == 2 and line["full"] is True and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["single_source_gteps_hmean"] > 0
    assert line["validation"]["msbfs_vs_single_source"].startswith("2/2 ")
    assert line["cpu_baseline"]["value"] > 0 and line["cpu_baseline"]["pagerank_s_per_iter"]["supersteps"] == 4
    assert line["sssp"]["roots"] >= 1 and line["sssp"]["gteps_hmean"] > 0
    assert 0 < line["config2_rows"]["rows"] <= 1 << 10 and line["config2_rows"]["gteps_hmean"] > 0
