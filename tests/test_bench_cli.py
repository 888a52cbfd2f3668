"""bench.py command line: a plain run is lean (no cpu_baseline leg), --steps
sets the number of timed steps, and --dump-outputs writes the last timed
step's results as float64 .npy, identical from run to run."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*extra):
    r = subprocess.run(
        [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
         "--rows", "1000003", "--steps", "3", "--warmup", "1", *extra],
        cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_full_and_dump_options_exist():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"),
                        "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_outputs(tmp_path):
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    out = _bench("--dump-outputs", d1)
    assert out["metric"] == "tpch_q6_sf100_rows_per_s"
    assert out["unit"] == "rows/s" and out["higher_is_better"] is True
    assert out["dtype"] == "int128"
    assert out["steps"] == 3 and out["ms_per_step"] > 0
    # value and ms_per_step describe the same 3 timed steps
    assert out["value"] == pytest.approx(
        1000003 / (out["ms_per_step"] * 1e-3), rel=1e-9)
    assert out["cpu_baseline"] is None  # only with --full

    names = sorted(os.listdir(d1))
    assert names == ["q6_count.npy", "q6_sum.npy", "q6_sum_limbs.npy"]
    arrs = {n: np.load(os.path.join(d1, n)) for n in names}
    assert all(a.dtype == np.float64 for a in arrs.values())
    cnt = int(arrs["q6_count.npy"][0])
    assert cnt == round(out["config"]["k_filter_selectivity"] * 1000003)
    limbs = [int(v) for v in arrs["q6_sum_limbs.npy"]]
    total = sum(l << (32 * i) for i, l in enumerate(limbs))
    assert 0 < total < 1 << 127
    assert arrs["q6_sum.npy"][0] == float(total)
    # every selected row contributes price*discount within the q6 window
    assert cnt * 90000 * 5 <= total <= cnt * 10495100 * 7

    # same arguments -> same inputs -> same outputs
    _bench("--dump-outputs", d2)
    for n in names:
        assert np.array_equal(arrs[n], np.load(os.path.join(d2, n)))
