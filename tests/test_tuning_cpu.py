"""CPU: tgo_set_tuning's table (titan_amd/csrc/tuning.hpp) against a recorded grid.

tests/golden/tuning_grid.json is what tgo_set_tuning answered, key by key and value by value, when every
key was a hand-written case of one switch: the return code, the message and the value kept for each of
41 keys x 24 values (984 calls on one context, 713 of them rejected).  tests/tuning_grid.cpp runs the same
calls through tuning_set, compiled over tuning.hpp alone (no HIP, no library), and every row must match.
"""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tuning_grid.json")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_tuning_table_answers_as_the_recorded_grid(tmp_path):
    exe = str(tmp_path / "tuning_grid")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "titan_amd", "csrc"),
                        os.path.join(ROOT, "tests", "tuning_grid.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    got = json.loads(run.stdout)
    with open(GOLDEN) as f:
        want = json.load(f)
    assert len(want) == 984 and sum(w["rc"] != 0 for w in want) == 713
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (g["key"], g["value"]) == (w["key"], w["value"])
        fields = ("rc", "err") if w["value"] == "nan" else ("rc", "err", "stored")
        assert [g[k] for k in fields] == [w[k] for k in fields], (g, w)
