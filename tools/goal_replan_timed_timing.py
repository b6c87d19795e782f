#!/usr/bin/env python3
"""Cost of sending running TIMED walks on to new goals (wcqp_tick_replan_goals_timed), for `--batch` robots with K =
`--max-steps` steps of `--min-ticks` / `--nominal-ticks` / `--max-ticks` samples (the reference's weights and ratio) on a planned handle
of `--ticks` ticks, medians of `--reps` after one untimed call, every call on a freshly uploaded walk (upload_goal, untimed by the clock)
with the device idle:

  (a) the host wall time of one TickPipeline.replan_goals(timing=) call (AUTO, SIDE_AUTO, lead 20): it enqueues and returns,
  (b) the time from that call to the completion of its event (wcqp_tick_get_goal_timing with no output rows: it waits for the event only),
  (c) the whole TickPipeline.replan_goal(timing=) call - the host composition of plan_window, plan_host and replan_footsteps - on a twin,
      at the merge stages and side (a) takes, on the same machine in the same session,
  (d) beside (a) and (b), in the same child process: the untimed wcqp_tick_replan_goals on an untimed handle of the same size, whose
      steps last nominal-ticks samples - its call and its time to the event.

    python tools/goal_replan_timed_timing.py [--batch 8192] [--out profiles/goal_replan_timed_timing.json]

The result's `gate` says whether (a) is below (c): the largest of (a)'s runs against the smallest of (c)'s.  This process never opens the
GPU: each step is a child process of its own (`--step NAME`) under `timeout -k 10 LIMIT`, which ends a step that hangs inside a device
call; after a step that fails or is ended no further step starts, and the result holds what was measured so far."""
import argparse
import ctypes as C
import json
import math
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = ("replan_goals_timed", "replan_goal_timed")
LEAD = 20


def _stats(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def step(a):
    import walking_controllers_amd as wca
    S = wca.synth
    B, K, T = a.batch, a.max_steps, a.ticks
    timing = dict(wca.UnicyclePlanner.TIMING_DEFAULTS, min_step_ticks=a.min_ticks, nominal_step_ticks=a.nominal_ticks, max_step_ticks=a.max_ticks)
    rho = timing["switch_over_swing_ratio"] / (1.0 + timing["switch_over_swing_ratio"])
    ds = min(max(int(math.floor(a.nominal_ticks * rho + 0.5)), 1), a.nominal_ticks - 1)        # the nominal step's split
    ss = a.nominal_ticks - ds
    out = {"source_hash": wca.capi.source_hash(), "batch": B, "max_steps": K, "timing": timing, "ticks": T, "first_ds_ticks": ds}
    kin = wca.KinModel(S.icub_like_model())
    kb = S.synth_walk_kin_batch(B)
    poses = kin.jacobians_host(kb["base"], kb["q"], state=np.zeros((B, 87)))["state"]
    fs = S.synth_footstep_walk_batch(B, T, poses, kb)
    g = S.synth_goal_batch(B, state0=fs["state0"], cases=False, radius=0.3)
    g2 = S.synth_goal_batch(B, seed=6022, state0=fs["state0"], cases=False, radius=0.3)
    pl = wca.UnicyclePlanner(nominal_width=0.118, min_width=0.10, step_ticks=a.nominal_ticks, max_steps=K, max_linear_velocity=0.03,
                             max_angular_velocity=0.15, min_step_length=0.005, min_angle_variation=0.01)

    def pipe():
        ik = wca.IkSolver(form=wca.IK_FORM_QPOASES, v_max=S.WALK_VMAX, joint_reg_rad=np.deg2rad(S.WALK_POSTURE_DEG))
        return wca.TickPipeline(B, T, wca.MpcSolver(horizon=50), ik, kin=kin, planned_trajectories=True, neck_additional_rotation=np.eye(3))
    timed = pipe()
    call_ms, done_ms = [], []
    for _ in range(a.reps + 1):
        up = timed.upload_goal(fs, g["goals"], pl, 1, ds, timing=timing)         # (synchronises: the device is idle)
        if a.step == "replan_goals_timed":
            t0 = time.perf_counter()
            timed.replan_goals(g2["goals"], pl, ds, min_lead_ticks=LEAD, timing=timing)
            t1 = time.perf_counter()
            wca.capi.check(wca.capi.lib().wcqp_tick_get_goal_timing(timed._h, None, None))
            t2 = time.perf_counter()
            call_ms.append(1e3 * (t1 - t0)); done_ms.append(1e3 * (t2 - t0))
        else:
            # the stages AUTO takes with t0 = 0: the first merge point at or above the lead - where the first step's single support ends -,
            # or the lead itself for a robot that stands; the left foot swings first behind a first step of the right one
            M = np.where(up["n_steps"] >= 1, ds + up["ss_ticks"][:, 0], LEAD).astype(np.int32)
            assert (M >= LEAD).all()
            t0 = time.perf_counter()
            res = timed.replan_goal(M, g2["goals"], pl, 0, ds, timing=timing)
            call_ms.append(1e3 * (time.perf_counter() - t0))
    if a.step == "replan_goals_timed":
        res = timed.goal_result()
        M = np.where(up["n_steps"] >= 1, ds + up["ss_ticks"][:, 0], LEAD)
        out.update(call_ms=_stats(call_ms[1:]), to_event_ms=_stats(done_ms[1:]), first_call_ms=call_ms[0],
                   at_the_composition_s_stage=int((res["merge_stage"] == M).sum()), left_first=int((res["first_side"] == 0).sum()))
        # (d) the untimed call on an untimed handle of the same size, in this child
        untimed = pipe()
        none = wca.capi.TickGoalResult()
        u_call, u_done = [], []
        for _ in range(a.reps + 1):
            untimed.upload_goal(fs, g["goals"], pl, 1, ds, ss, ds)
            t0 = time.perf_counter()
            untimed.replan_goals(g2["goals"], pl, ds, min_lead_ticks=LEAD)
            t1 = time.perf_counter()
            wca.capi.check(wca.capi.lib().wcqp_tick_get_goal_result(untimed._h, C.byref(none)))
            t2 = time.perf_counter()
            u_call.append(1e3 * (t1 - t0)); u_done.append(1e3 * (t2 - t0))
        ures = untimed.goal_result()
        out["untimed"] = dict(call_ms=_stats(u_call[1:]), to_event_ms=_stats(u_done[1:]), first_call_ms=u_call[0], step_ticks=a.nominal_ticks,
                              mean_steps=float(ures["n_steps"].mean()), set_slots_per_robot=1 + 2 * ((T + 1) // (ss + 1) + 1))
        out["set_slots_per_robot"] = 1 + 2 * ((T + 1) // 2 + 1)
    else:
        out.update(call_ms=_stats(call_ms[1:]), first_call_ms=call_ms[0], distinct_merge_stages=int(len(np.unique(M))))
    taken = np.arange(K)[None, :] < res["n_steps"][:, None]
    m = (res["ss_ticks"] + res["ds_ticks"])[taken]
    out.update(status_counts=np.bincount(res["status"][res["status"] >= 0], minlength=4).tolist(), mean_steps=float(res["n_steps"].mean()),
               step_ticks_chosen={"min": int(m.min()), "max": int(m.max()), "mean": float(m.mean())} if m.size else None)
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--max-steps", type=int, default=20)
    ap.add_argument("--min-ticks", type=int, default=80)
    ap.add_argument("--nominal-ticks", type=int, default=90)
    ap.add_argument("--max-ticks", type=int, default=100)
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
    args = ["--batch", a.batch, "--max-steps", a.max_steps, "--min-ticks", a.min_ticks, "--nominal-ticks", a.nominal_ticks, "--max-ticks", a.max_ticks,
            "--ticks", a.ticks, "--reps", a.reps]
    for name in STEPS:
        r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--step", name] + [str(x) for x in args],
                           capture_output=True, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            out[name] = {"failed": True, "exit_status": r.returncode, "stderr_tail": r.stderr[-600:]}
            break
        out[name] = json.loads(lines[-1][7:])
    if all(k in out and "call_ms" in out[k] for k in STEPS):
        a_ms, c_ms = out[STEPS[0]]["call_ms"], out[STEPS[1]]["call_ms"]
        out["gate"] = {"rule": "the largest timed replan_goals call of the runs is below the smallest replan_goal(timing=) call", "a_max_ms": a_ms["max"],
                       "c_min_ms": c_ms["min"], "passed": bool(a_ms["max"] < c_ms["min"])}
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    if "gate" not in out or not out["gate"]["passed"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
