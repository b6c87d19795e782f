#!/usr/bin/env python3
"""Cost of sending running walks on to new goals (wcqp_tick_replan_goals), for `--batch` robots with K = `--max-steps` steps of
D = `--step-ticks` samples on a planned handle of `--ticks` ticks, medians of `--reps` after one untimed call, every call on a freshly
uploaded walk (upload_goal, untimed) with the device idle:

  (a) the host wall time of one TickPipeline.replan_goals call (AUTO, SIDE_AUTO, lead 20): it enqueues and returns,
  (b) the time from that call to the completion of its event (wcqp_tick_get_goal_result with no output rows: it waits for the event only),
  (c) the whole TickPipeline.replan_goal call - the host composition of plan_window, plan_host and replan_footsteps - at the merge stage
      and side (a) takes, on the same machine in the same session.

    python tools/goal_replan_timing.py [--batch 8192] [--out profiles/goal_replan_timing.json]

The result's `gate` says whether (a) is below (c): the largest of (a)'s runs against the smallest of (c)'s.  This process never opens the
GPU: each step is a child process of its own (`--step NAME`) under `timeout -k 10 LIMIT`, which ends a step that hangs inside a device
call; after a step that fails or is ended no further step starts, and the result holds what was measured so far."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = ("replan_goals", "replan_goal")


def _stats(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def step(a):
    import walking_controllers_amd as wca
    S = wca.synth
    B, K, D, T = a.batch, a.max_steps, a.step_ticks, a.ticks
    ss, ds = D - D // 3, D // 3
    out = {"source_hash": wca.capi.source_hash(), "batch": B, "max_steps": K, "step_ticks": D, "ticks": T}
    kin = wca.KinModel(S.icub_like_model())
    kb = S.synth_walk_kin_batch(B)
    poses = kin.jacobians_host(kb["base"], kb["q"], state=np.zeros((B, 87)))["state"]
    fs = S.synth_footstep_walk_batch(B, T, poses, kb)
    g = S.synth_goal_batch(B, state0=fs["state0"], cases=False, radius=0.3)
    g2 = S.synth_goal_batch(B, seed=6022, state0=fs["state0"], cases=False, radius=0.3)
    pl = wca.UnicyclePlanner(nominal_width=0.118, min_width=0.10, step_ticks=D, max_steps=K, max_linear_velocity=0.03, max_angular_velocity=0.15,
                             min_step_length=0.005, min_angle_variation=0.01)
    ik = wca.IkSolver(form=wca.IK_FORM_QPOASES, v_max=S.WALK_VMAX, joint_reg_rad=np.deg2rad(S.WALK_POSTURE_DEG))
    pipe = wca.TickPipeline(B, T, wca.MpcSolver(horizon=50), ik, kin=kin, planned_trajectories=True, neck_additional_rotation=np.eye(3))
    M = ds + ss                      # the first merge point of a walk of two steps or more: where its first inner double support starts
    call_ms, done_ms = [], []
    for _ in range(a.reps + 1):
        pipe.upload_goal(fs, g["goals"], pl, 1, ds, ss, ds)         # (synchronises: the device is idle)
        if a.step == "replan_goals":
            none = wca.capi.TickGoalResult()
            t0 = time.perf_counter()
            pipe.replan_goals(g2["goals"], pl, ds, min_lead_ticks=20)
            t1 = time.perf_counter()
            wca.capi.check(wca.capi.lib().wcqp_tick_get_goal_result(pipe._h, C.byref(none)))
            t2 = time.perf_counter()
            call_ms.append(1e3 * (t1 - t0)); done_ms.append(1e3 * (t2 - t0))
        else:
            t0 = time.perf_counter()
            res = pipe.replan_goal(np.full(B, M, np.int32), g2["goals"], pl, 0, ds)
            call_ms.append(1e3 * (time.perf_counter() - t0))
    if a.step == "replan_goals":
        res = pipe.goal_result()
        out.update(call_ms=_stats(call_ms[1:]), to_event_ms=_stats(done_ms[1:]), first_call_ms=call_ms[0],
                   at_stage_M=int((res["merge_stage"] == M).sum()), left_first=int((res["first_side"] == 0).sum()))
    else:
        out.update(call_ms=_stats(call_ms[1:]), first_call_ms=call_ms[0])
    out.update(merge_stage=M, status_counts=np.bincount(res["status"][res["status"] >= 0], minlength=4).tolist(), mean_steps=float(res["n_steps"].mean()))
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--max-steps", type=int, default=20)
    ap.add_argument("--step-ticks", type=int, default=100)
    ap.add_argument("--ticks", type=int, default=1200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=170, help="seconds per step")
    ap.add_argument("--step", choices=STEPS, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.step:
        step(a)
        return
    out = {}
    args = ["--batch", a.batch, "--max-steps", a.max_steps, "--step-ticks", a.step_ticks, "--ticks", a.ticks, "--reps", a.reps]
    for name in STEPS:
        r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--step", name] + [str(x) for x in args],
                           capture_output=True, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            out[name] = {"failed": True, "exit_status": r.returncode, "stderr_tail": r.stderr[-600:]}
            break
        out[name] = json.loads(lines[-1][7:])
    if all(k in out and "call_ms" in out[k] for k in STEPS):
        a_ms, c_ms = out["replan_goals"]["call_ms"], out["replan_goal"]["call_ms"]
        out["gate"] = {"rule": "the largest replan_goals call of the runs is below the smallest replan_goal call", "a_max_ms": a_ms["max"], "c_min_ms": c_ms["min"],
                       "passed": bool(a_ms["max"] < c_ms["min"])}
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    if "gate" not in out or not out["gate"]["passed"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
