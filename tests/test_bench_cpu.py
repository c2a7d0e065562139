"""bench.py's host-side pieces: the step count it is given, what a plain run does besides its steps, what --dump-outputs
writes, the size of the result line's side-workload entries (no GPU)."""
import json
import os

import numpy as np
import pytest

import bench


def test_steps_and_warmup_are_what_was_asked():
    a = bench.parse_args(["--steps", "3", "--warmup", "0"])
    assert a.steps == 3 and a.warmup == 0 and a.dump_outputs is None
    a = bench.parse_args(["--workload", "largebox"])
    assert (a.steps, a.warmup) == bench.WORKLOADS["largebox"][6:8]
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        with pytest.raises(SystemExit):
            bench.parse_args(bad)


def test_plain_run_is_the_headline_alone():
    parts = ("pcie", "parity", "cpu_baseline", "others")
    for argv in ([], ["--gpus", "1", "--steps", "6", "--warmup", "1"], ["--no-parity", "--no-others"], ["--workload", "reffree"]):
        a = bench.parse_args(argv)
        assert not a.full and not any(getattr(a, p) for p in parts), argv
    a = bench.parse_args(["--full"])
    assert all(getattr(a, p) for p in parts)
    a = bench.parse_args(["--full", "--no-parity", "--no-pcie"])
    assert (a.pcie, a.parity, a.cpu_baseline, a.others) == (False, False, True, True)
    a = bench.parse_args(["--full", "--no-cpu-baseline", "--no-others"])
    assert (a.pcie, a.parity, a.cpu_baseline, a.others) == (True, True, False, False)
    # the side workloads follow the default mref geometry only
    assert not bench.parse_args(["--full", "--workload", "reffree"]).others
    assert not bench.parse_args(["--full", "--particles", "2048"]).others


def _outputs(n, nref, nx):
    rng = np.random.default_rng(3)
    out = {"param_alpha": rng.random(n, dtype=np.float32), "param_ref_id": rng.integers(0, nref, n).astype(np.float64),
           "shift_state": rng.random((n, 2), dtype=np.float32),
           "references": rng.random((nref, nx, nx), dtype=np.float32), "class_sizes": np.arange(nref, dtype=np.float64)}
    return out


def _read(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_under_the_budget_is_every_array_whole(tmp_path):
    arrs = _outputs(1000, 4, 16)
    names = bench.write_outputs(str(tmp_path), arrs, 1000)
    got = _read(str(tmp_path))
    assert sorted(got) == names == sorted(arrs)
    for k, a in arrs.items():
        assert got[k].dtype in (np.float32, np.float64) and np.array_equal(got[k], a)


def test_dump_over_the_budget_is_a_fixed_sample_of_rows(tmp_path):
    n, nref, nx = 5000, 40, 32
    arrs = _outputs(n, nref, nx)
    budget = 150_000          # references (164 KB) and the particles (80 KB) do not fit together
    bench.write_outputs(str(tmp_path / "a"), arrs, n, budget)
    bench.write_outputs(str(tmp_path / "b"), arrs, n, budget)
    a, b = _read(str(tmp_path / "a")), _read(str(tmp_path / "b"))
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    assert sum(v.nbytes for v in a.values()) <= budget
    rows = a["particle_rows"].astype(np.int64)
    assert 0 < rows.size < n and np.all(np.diff(rows) > 0)
    for k in ("param_alpha", "param_ref_id", "shift_state"):
        assert np.array_equal(a[k], arrs[k][rows])
    ref_rows = a["references_rows"].astype(np.int64)
    assert 0 < ref_rows.size < nref and np.array_equal(a["references"], arrs["references"][ref_rows])
    assert np.array_equal(a["class_sizes"], arrs["class_sizes"])


def test_side_workload_entry_is_short():
    sig = {"max_rel_peak": 2.2770270788896596e-06, "exact_match_rate": 1.0, "tie_flips": 0, "max_rel_peak_gap_of_flips": 0.0,
           "alpha_outliers_gt_2e-3_deg": 0, "max_alpha_diff_deg": 6.103515625e-05}
    line = {"metric": "particles/sec aligned, 256x256 nref=100 xr=yr=5 ou=120", "value": 856240.0599963284, "unit": "particles/s",
            "steps": 6, "warmup": 2, "ms_per_step": 9.567410335876048, "dtype": "f32", "config": {"workload": "x" * 400},
            "roofline": {"bound": "mfma", "frac": 0.3070419269978484, "kernel": "ccf_generic_kernel", "whole_path": {"frac": 0.17003899885720805},
                         "traffic_source": "profiles/r05_box256_pmc_summary.json", "achieved": 48.29769511676155},
            "parity": {"particles_per_set": 256, "sigma_0.25": dict(sig, tie_flips=1), "sigma_1": sig, "search_path": "fused"}}
    s = bench.side_summary(line)
    assert s["ms_per_step"] == line["ms_per_step"] and s["value"] == line["value"] and s["kernel"] == "ccf_generic_kernel"
    assert s["parity"]["tie_flips"] == 1 and s["parity"]["exact_match_rate"] == 1.0
    assert len(json.dumps(s)) < 500
