"""The JSON line of bench.py (the driver's contract + what SURVEY.md 8d / VERDICT r3 ask of it), on a small batch so that it runs in
seconds: every object is there, the timed work was checked (goldens for the cold-start batches, the CPU restatement for the ticks)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_default_line_carries_roofline_tick_and_both_cpu_baselines():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "6", "--warmup", "2", "--batch", "1024", "--tick-batch", "512", "--tick-ticks", "60",
                        "--cpu-seconds", "1"], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert k in d, k
    assert d["steps"] == 6 and d["warmup"] == 2 and d["n_gpus"] == 1 and d["dtype"] == "f64" and d["vs_baseline"] is None and "workload" in d["config"]
    assert d["repeats"] == 5 and d["value_min"] <= d["value"] <= d["value_max"]
    assert abs(d["value"] - 2 * 1024 * 6 / (d["ms_per_step"] * 6e-3)) <= 1e-6 * d["value"]          # value IS the median region
    rf = d["roofline"]
    assert rf["bound"] == "hbm" and rf["kernel"] == "qp_plan_kernel" and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-12 and "traffic" in rf
    assert rf["algorithmic_bytes_per_launch"] == 6296 * 1024 * 6 and rf["single_launch_form"]["frac"] > 0
    s = d["solved"]
    assert s["ik"] == 1024 and s["mpc"] == 1024 and s["golden_active_set_mismatches"] == 0 and s["golden_max_abs_err"] <= 1e-9
    assert s["golden_rows_checked"] == 6 * 2 * 1024                       # 6 ways (one per step), both QPs, every row
    for name in ("fused_kinematics", "constant_jacobians"):
        t = d["tick"][name]
        assert "error" not in t, t
        assert t["value"] > 0 and t["us_per_tick"] > 0 and t["roofline"]["bound"] == "latency" and t["roofline"]["own_hbm_bytes_per_robot_tick"] > 0
        assert t["solved"]["ticks_executed"] == 60 + 24 and t["solved"]["mpc_fail"] == 0
        oc = t["oracle_check"]
        assert oc["ok"] is True and oc["ticks"] == 16 and len(oc["robots"]) >= 5 and oc["max_abs_err_u0"] <= 1e-9 and oc["max_abs_err_dq"] <= 1e-8, oc
    assert d["tick"]["fused_kinematics"]["solved"]["robots_with_ik_fail"] == 0
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] >= 1 and cb["value"] > 0 and cb["same_algorithm_qps"] > cb["value"]


def test_dump_outputs_keeps_a_fixed_sample_under_the_budget(tmp_path):
    """bench.dump_outputs (--dump-outputs): float64 files, whole arrays when they fit; over the budget the same seeded, sorted sample
    of rows in every array, its indices in rows.npy, and the files together no larger than the budget."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    rng = np.random.default_rng(5)
    arrays = {"dq": rng.standard_normal((1000, 23)), "status": rng.integers(-3, 3, 1000).astype(np.int32),
              "mask": rng.integers(0, 2 ** 32, 1000, dtype=np.uint64).astype(np.uint32)}
    full = bench.dump_outputs(str(tmp_path / "full"), arrays)
    assert sorted(os.listdir(tmp_path / "full")) == ["dq.npy", "mask.npy", "status.npy"]
    for k, a in arrays.items():
        got = np.load(tmp_path / "full" / (k + ".npy"))
        assert got.dtype == np.float64 and np.array_equal(got, a.astype(np.float64)) and np.array_equal(full[k], got)
    budget = 40000
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), arrays, budget=budget)
        assert sum(os.path.getsize(tmp_path / d / f) for f in os.listdir(tmp_path / d)) <= budget
    rows = np.load(tmp_path / "s1" / "rows.npy")
    assert rows.dtype == np.float64 and 0 < len(rows) < 1000 and np.all(np.diff(rows) > 0)
    for f in ("rows", "dq", "status", "mask"):
        a, b = np.load(tmp_path / "s1" / (f + ".npy")), np.load(tmp_path / "s2" / (f + ".npy"))
        assert np.array_equal(a, b), f
        if f != "rows":
            assert np.array_equal(a, arrays[f][rows.astype(np.int64)].astype(np.float64)), f
    # a later run that fits does not leave the earlier sample's index behind
    bench.dump_outputs(str(tmp_path / "s1"), arrays)
    assert not os.path.exists(tmp_path / "s1" / "rows.npy")


@pytest.mark.gpu
def test_dump_outputs_is_the_last_timed_step(tmp_path):
    """--dump-outputs DIR: the QpStep outputs of the last timed step, rows in instance order (the step read a rolled input set), equal to
    the golden optimum of every row, and identical from run to run with the same arguments."""
    import numpy as np
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    names = ("u0", "mpc_status", "mpc_active", "mpc_margin", "dq", "ik_status", "active_lower", "active_upper", "iters")
    dumps = []
    for d in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--batch", "1024", "--no-tick",
                            "--no-cpu-baseline", "--dump-outputs", str(tmp_path / d)], capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, r.stderr[-3000:]
        assert sorted(os.listdir(tmp_path / d)) == sorted(n + ".npy" for n in names)
        dumps.append({n: np.load(tmp_path / d / (n + ".npy")) for n in names})
    for n in names:
        assert dumps[0][n].dtype == np.float64 and len(dumps[0][n]) == 1024 and np.array_equal(dumps[0][n], dumps[1][n]), n
    o = dumps[0]
    gm = np.load(os.path.join(ROOT, "tests", "golden", "mpc_cfg2_b4096.npz"), allow_pickle=False)
    gi = np.load(os.path.join(ROOT, "tests", "golden", "ik_qpoases_v050_b4096.npz"), allow_pickle=False)
    assert np.abs(o["u0"] - gm["u0"][:1024]).max() <= 1e-9 and np.all(o["mpc_status"] == 0)
    assert np.abs(o["dq"] - gi["dq"][:1024]).max() <= 1e-9 and np.array_equal(o["ik_status"], gi["status"][:1024].astype(np.float64))
