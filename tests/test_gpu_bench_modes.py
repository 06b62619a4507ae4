"""bench.py's two modes: a plain run measures the timed steps and prints the line without any side measurement or check; --full
adds them after the timed region, which stays the same steps on the same inputs (what --dump-outputs writes is identical).
Each run is a child process with a kernel cache of its own, so that nothing one run compiles is found by another."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def run_bench(tmp_path, tag, *args):
    env = dict(os.environ, KC_KERNEL_CACHE_DIR=str(tmp_path / ("kcache_" + tag)))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, "bench.py %s: rc %d\n%s" % (" ".join(args), r.returncode, r.stderr[-4000:])
    lines = [x for x in r.stdout.splitlines() if x.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_and_full_runs(tmp_path):
    common = ("--steps", "5", "--warmup", "2", "--size", "1024")
    plain = run_bench(tmp_path, "plain", *common, "--dump-outputs", str(tmp_path / "plain"))
    full = run_bench(tmp_path, "full", *common, "--full", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "full"))
    for line in (plain, full):
        for k in HEADLINE_KEYS:
            assert k in line, k
        assert line["steps"] == 5 and line["warmup"] == 2 and line["value"] > 0
        assert line["roofline"]["launches_per_step"] >= 1 and line["roofline"]["algorithmic_bytes_per_step"] > 0
    assert plain["metric"] == full["metric"] and plain["unit"] == full["unit"]

    assert plain["config"]["full"] is False
    for k in ("cpu_baseline", "cpu_baseline_all_cores", "parity", "unfused", "pcie_inclusive"):
        assert k not in plain, k
    assert "cold" not in plain["roofline"] and plain["roofline"]["frac_cold"] is None
    assert "step_us_median" not in plain["roofline"]

    assert full["config"]["full"] is True
    assert full["unfused"]["launches_per_step"] > full["roofline"]["launches_per_step"] and full["pcie_inclusive"]["seconds"] > 0
    assert full["roofline"]["cold"]["steps"] > 0 and full["roofline"]["frac_cold"] > 0
    assert full["roofline"]["step_us_min"] <= full["roofline"]["step_us_median"] <= full["roofline"]["step_us_max"]

    files = plain["dump_outputs"]["files"]
    assert sorted(files) == sorted(full["dump_outputs"]["files"]) == ["result_a", "result_b", "result_g", "result_r"]
    for name in files:
        a, b = np.load(tmp_path / "plain" / (name + ".npy")), np.load(tmp_path / "full" / (name + ".npy"))
        assert a.shape == b.shape == (1024, 1024)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), name


def test_full_run_checks_parity(tmp_path):
    line = run_bench(tmp_path, "mix1", "--workload", "mix1", "--size", "512", "--steps", "3", "--warmup", "1", "--full", "--no-extras")
    assert line["parity"] == {"checked_pixels": 512 * 512 * 4, "bit_mismatches": 0}
    assert "cold" not in line["roofline"] and "step_us_median" in line["roofline"]
    plain = run_bench(tmp_path, "mix1_plain", "--workload", "mix1", "--size", "512", "--steps", "3", "--warmup", "1")
    assert "parity" not in plain
