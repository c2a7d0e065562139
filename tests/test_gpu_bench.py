"""bench.py end to end on the GPU: a plain run prints the headline alone and spends little time besides its steps; --full adds
what the headline does not need."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, STEPS, WARMUP = 2048, 2, 1


def _bench(*extra):
    t = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", str(STEPS), "--warmup", str(WARMUP),
                        "--particles", str(N)] + list(extra), capture_output=True, text=True, timeout=600)
    wall = time.perf_counter() - t
    assert r.returncode == 0, r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1]), wall


def test_plain_run_is_the_headline_alone(tmp_path):
    line, wall = _bench("--dump-outputs", str(tmp_path))
    assert line["unit"] == "particles/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["metric"].startswith("particles/sec aligned, 90x90 nref=10")
    assert line["value"] > 0 and np.isclose(line["value"] * line["ms_per_step"] * 1e-3, N, rtol=1e-6)
    assert not {"parity", "pcie_inclusive", "cpu_baseline", "other_workloads"} & set(line)
    assert line["roofline"]["launches"] == STEPS
    assert np.load(os.path.join(str(tmp_path), "param_alpha.npy")).shape == (N,)
    assert wall - (STEPS + WARMUP) * line["ms_per_step"] * 1e-3 < 30.0


def test_full_run_adds_parity_and_pcie():
    line, _ = _bench("--full", "--no-cpu-baseline")
    assert line["pcie_inclusive"]["h2d_seconds"] > 0
    for sig in ("sigma_0.25", "sigma_1"):
        assert line["parity"][sig]["max_rel_peak"] < line["parity"]["peak_tolerance"]
    assert "cpu_baseline" not in line and "other_workloads" not in line       # --particles: a custom geometry, no side runs
