#!/usr/bin/env python3
"""Cost of resetting robots of a sensor-fed fleet (wcqp_tick_reset_robots), at `--batch` robots x T = ticks + 51 stages and
S = `--stage` ticks enqueued, medians of `--reps` after a warm-up, the protocol of tools/plan_restart_timing.py:

  reset        the call's kernels on the stream, between events behind a busy stream, with 1 %, 10 % and 100 % of the fleet reset, on a
               sensor-fed resident handle (filters on, the reactive controller with gain scheduling: every array the call writes exists);
               the host wall clock of the call against that of wcqp_tick_upload_footsteps on that handle, today's only alternative
  restart      the yardstick, in the same session: wcqp_tick_restart_robots on a planned handle of the same geometry - the same fill, so
               the difference is what only an EXTERNAL handle keeps
  filter_tick  the sensor-fed resident tick with filters on, microseconds per tick over `--tick-ticks` ticks of a standing fleet (the
               sensor kernel's work does not depend on the gait), this tree against `--parent-root` (a checkout of the parent commit
               with its library built), alternating, `--reps` runs each, every run a process of its own; without --parent-root only this tree's

    python tools/tick_reset_timing.py [--batch 8192] [--ticks 1200] [--stage 200] [--parent-root DIR] [--out profiles/tick_reset_timing.json]

This process never opens the GPU: each step is a child process of its own under `timeout -k 10 LIMIT`; after a step that fails or is ended
no further step starts, and the result holds what was measured so far."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("WCQP_PACKAGE_ROOT") or ROOT)      # (a filter_tick child of the parent commit imports THAT tree's package)
FRACTIONS = (("1pct", 100), ("10pct", 10), ("100pct", 1))      # every k-th robot is reset
FILTERS = dict(joint_velocity=10.0, wrench=10.0, com=10.0)
CTL = dict(dcm_controller="reactive", k_dcm=1.0, zmp_gain_scheduling=True, k_com_stance=6.0, k_zmp_stance=0.9, zmp_smoothing_time=0.05)


def _ik(wca):
    S = wca.synth
    return wca.IkSolver(form=wca.IK_FORM_QPOASES, v_max=S.WALK_VMAX, joint_reg_rad=np.deg2rad(S.WALK_POSTURE_DEG))


def _footsteps(wca, B, T, standing=False):
    """tools/plan_restart_timing.py's walk (standing: nobody takes a step)"""
    S = wca.synth
    kin = wca.KinModel(S.icub_like_model())
    kb = S.synth_walk_kin_batch(B)
    poses = kin.jacobians_host(kb["base"], kb["q"], state=np.zeros((B, 87)))["state"]
    fs = S.synth_footstep_walk_batch(B, T, poses, kb, n_steps=max(1, (T - 110) // 180), yaw_step=(0.03, 0.08))
    fs["final_ds_ticks"] = 0
    if standing:
        fs["n_steps"] = np.zeros(B, np.int32)
    return fs


def _stats(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "all": [float(x) for x in v]}


def _mode(wca, B, every):
    m = np.zeros(B, np.uint8)
    m[np.arange(0, B, every)] = wca.capi.TICK_RESTART_ALWAYS
    return m


def _readings(torch, fs, B):
    """a standing robot's readings on the device: its start joints, no velocity, 150 N on each sole"""
    dev = torch.device("cuda", 0)
    w = np.zeros((B, 6)); w[:, 2] = 150.0
    t_ = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)
    return t_(fs["q0"]), t_(np.zeros((B, 23))), t_(w), t_(w)


def step(a):
    import torch  # the GPU runtime first, then libwcqp
    import walking_controllers_amd as wca
    out = {"device": torch.cuda.get_device_name(0), "source_hash": wca.capi.source_hash()}
    B, T, S0 = a.batch, a.ticks, a.stage
    stream = torch.cuda.current_stream().cuda_stream
    ev = lambda: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    kin = wca.KinModel(wca.synth.icub_like_model())
    if a.step == "filter_tick":
        n = a.tick_ticks
        fs = _footsteps(wca, B, n, standing=True)
        pipe = wca.TickPipeline(B, n, wca.MpcSolver(horizon=50), _ik(wca), kin=kin, external_feedback=True, streamed_trajectories=True,
                                resident_plan=True, neck_additional_rotation=np.eye(3), sensor_filters=FILTERS)
        rd = _readings(torch, fs, B)
        ptr = tuple(x.data_ptr() for x in rd)
        us = []
        for _ in range(2):      # (the first pass: code load, first touch)
            pipe.upload_footsteps(fs, fs)
            torch.cuda.synchronize()
            e0, e1 = ev()
            e0.record()
            for _t in range(n):
                pipe.set_desired_from_plan(stream=stream)
                pipe.set_sensor_feedback_device(*ptr, stream=stream)
                pipe.run(1, stream=stream)
            e1.record()
            torch.cuda.synchronize()
            us.append(1e3 * e0.elapsed_time(e1) / n)
        o = pipe.download()
        out.update(batch=B, ticks=n, us_per_tick=us[1], robots_with_ik_fail=int((o["ik_fail"] > 0).sum()), feedback_fail=int(o["feedback_fail"].sum()))
        print("RESULT " + json.dumps(out))
        return
    fs = _footsteps(wca, B, T)
    rows = {k: fs[k] for k in ("state0", "q0", "com0")}
    out.update(batch=B, stages=T + 51, stage=S0)
    reset = a.step == "reset"
    if reset:
        pipe = wca.TickPipeline(B, T, wca.MpcSolver(horizon=50), _ik(wca), kin=kin, external_feedback=True, streamed_trajectories=True,
                                resident_plan=True, neck_additional_rotation=np.eye(3), sensor_filters=FILTERS, **CTL)
        rd = _readings(torch, fs, B)
        ptr = tuple(x.data_ptr() for x in rd)
    else:
        pipe = wca.TickPipeline(B, T, wca.MpcSolver(horizon=50), _ik(wca), kin=kin, planned_trajectories=True, neck_additional_rotation=np.eye(3),
                                noise=0.0, **CTL)

    def walk_to_stage():
        if not reset:
            pipe.run(S0)
            return
        for _t in range(S0):
            pipe.set_desired_from_plan(stream=stream)
            pipe.set_sensor_feedback_device(*ptr, stream=stream)
            pipe.run(1, stream=stream)
    call = pipe.reset_robots if reset else pipe.restart_robots
    up = []
    for _ in range(a.reps + 1):
        t0 = time.perf_counter(); pipe.upload_footsteps(fs, fs); up.append(1e3 * (time.perf_counter() - t0))
    gx, gy = (torch.zeros(1 << 30, dtype=torch.uint8, device="cuda") for _ in range(2))
    for name, every in FRACTIONS:
        # (a fresh plan per fraction: every call at the same stage takes one more of a robot's set slots)
        pipe.upload_footsteps(fs, fs)
        walk_to_stage()
        torch.cuda.synchronize()
        m, dev, wall = _mode(wca, B, every), [], []
        for _ in range(a.reps + 1):
            e0, e1 = ev()
            for _k in range(10):      # the stream is kept busy while the host stages the call's rows
                gy.copy_(gx)
            e0.record()
            t0 = time.perf_counter()
            call(m, rows, stream=stream)
            wall.append(1e3 * (time.perf_counter() - t0))
            e1.record()
            torch.cuda.synchronize()
            dev.append(e0.elapsed_time(e1))
        res = pipe.restart_result()
        assert res["stage"] == S0 and int(res["restarted"].sum()) == int(m.sum())
        out[name] = dict(robots=int(m.sum()), kernels_ms=_stats(dev[1:]), call_wall_ms=_stats(wall[1:]))
    out.update(upload_footsteps_wall_ms=_stats(up[1:]))
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--ticks", type=int, default=1200)
    ap.add_argument("--stage", type=int, default=200)
    ap.add_argument("--tick-ticks", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds per step")
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit, built: filter_tick alternates it with this tree")
    ap.add_argument("--step", choices=("reset", "restart", "filter_tick"), default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.step:
        step(a)
        return
    out = {}
    args = [str(x) for x in ("--batch", a.batch, "--ticks", a.ticks, "--stage", a.stage, "--reps", a.reps, "--tick-ticks", a.tick_ticks)]

    def child(name, root=None):
        env = dict(os.environ)
        if root:
            env["WCQP_PACKAGE_ROOT"] = os.path.abspath(root)
        r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--step", name] + args,
                           capture_output=True, text=True, env=env)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            return {"failed": True, "exit_status": r.returncode, "stderr_tail": r.stderr[-600:]}
        return json.loads(lines[-1][7:])

    def save():
        print(json.dumps(out))
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)
    for name in ("reset", "restart"):
        out[name] = child(name)
        if out[name].get("failed"):
            return save()
    out["ratios"] = {name: {"reset_kernels_over_restart_kernels": out["reset"][name]["kernels_ms"]["median"] / out["restart"][name]["kernels_ms"]["median"],
                            "reset_call_over_upload_footsteps_wall": out["reset"][name]["call_wall_ms"]["median"] / out["reset"]["upload_footsteps_wall_ms"]["median"]}
                     for name, _ in FRACTIONS}
    runs = {"change": [], "parent": []}
    for rep in range(a.reps):
        order = ("parent", "change") if rep % 2 == 0 else ("change", "parent")
        for who in order:
            if who == "parent" and not a.parent_root:
                continue
            r = child("filter_tick", a.parent_root if who == "parent" else None)
            if r.get("failed"):
                out["filter_tick"] = r
                return save()
            runs[who].append(r["us_per_tick"])
            out.setdefault("filter_tick_runs", {})[who] = {k: r[k] for k in ("source_hash", "robots_with_ik_fail", "feedback_fail", "batch", "ticks")}
    ft = {who: _stats(v) for who, v in runs.items() if v}
    if "parent" in ft:
        ft["change_median_within_parent_spread"] = bool(ft["change"]["median"] <= ft["parent"]["max"])      # (no slower than the parent's own runs)
    out["filter_tick"] = ft
    save()


if __name__ == "__main__":
    main()
