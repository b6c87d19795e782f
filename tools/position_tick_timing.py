#!/usr/bin/env python3
"""Cost of the POSITION mode of the closed-loop tick (wcqp_tick_params.ik_mode): `--batch` robots prepared at a CoM height of
0.42 m walk `--ticks` ticks of a generated plan (steps of 60 + 40 stages behind a double support of 40) in ONE launch, medians of
`--reps` runs timed between events:

  position        the POSITION handle at the default tolerances (1e-12 / 1e-10), 30 iterations per tick at most
  position_loose  the POSITION handle at 1e-4 / 1e-4 (the reference's tolerances)
  velocity        the planned VELOCITY handle on the same plan: the yardstick

each with the time per tick, and for the POSITION handles the mean Gauss-Newton iterations per robot and tick (ik_iters) and the robots
stopped.  `--controller reactive` (the default: the reactive law with gain scheduling) or `mpc` (N = 50).  With the MPC the closed loop of
this walk at this CoM height drifts: from about tick 175 on p_star has left the feet's reach, the IK of either mode stops the robots, and a
stopped robot costs no iterations - tests/helpers/position_tick.py's restatement shows the same on the CPU.  The reactive loop keeps every
robot walking for the 200 ticks, so it is the one that measures 200 ticks of IK.

    python tools/position_tick_timing.py [--batch 8192] [--ticks 200] [--out profiles/position_tick_timing.json]

This process never opens the GPU: each step is a child process of its own (`--step NAME`) under `timeout -k 10 LIMIT`, which ends a step that
hangs inside a device call; after a step that fails or is ended no further step starts, and the result holds what was measured so far."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
STEPS = ("position", "position_loose", "velocity")
H, N, STEP_TICKS, DS_TICKS = 0.42, 50, 100, 40


def step(a):
    import torch  # the GPU runtime first, then libwcqp
    import walking_controllers_amd as wca
    import robots
    from helpers import zmp_gains as zg
    S = wca.synth
    B, T = a.batch, a.ticks
    out = {"device": torch.cuda.get_device_name(0), "source_hash": wca.capi.source_hash(), "batch": B, "ticks": T}
    model = S.icub_like_model()
    q_reg = np.deg2rad(S.WALK_POSTURE_DEG)
    d = S.synth_prepare_batch(B, com_height=(H, H))
    o = wca.PrepareSolver(wca.KinModel(model), q_reg).solve_host(d["left_d"], d["right_d"], d["com_d"], d["q_guess"], d["Rd_neck"])
    assert (o["status"] == 0).all()
    fs = S.synth_footstep_walk_batch(B, T, o["state"], dict(q=o["q"]), step_ticks=STEP_TICKS, ds_ticks=DS_TICKS, n_steps=max(1, -(-(T - DS_TICKS) // STEP_TICKS)),
                                     com_height=H)
    fs["state0"] = o["state"]
    R = robots.ROBOTS["iCubGazeboV2_5"]
    ik = wca.IkSolver(form=wca.IK_FORM_QPOASES, neck_weight=R["neck_weight"] * np.eye(3), joint_reg_weights=np.array(R["reg_w"], float),
                      joint_reg_gains=np.array(R["reg_k"], float), joint_reg_rad=q_reg, v_max=S.WALK_VMAX.copy(), k_pos_com=R["k_pos_com"],
                      k_pos_foot=R["k_pos_foot"], k_att_foot=R["k_att_foot"], k_neck=R["k_neck"])
    mode = dict(dcm_controller="reactive", k_dcm=1.0, zmp_gain_scheduling=True, **zg.ZMP_SCHEDULE["iCubGazeboV2_5"]) if a.controller == "reactive" else {}
    out["controller"] = a.controller
    if a.step != "velocity":
        tol = dict(tol_step=1e-4, tol_constraint=1e-4) if a.step == "position_loose" else {}
        mode.update(ik_mode="position", position_ik=dict(q_reg=q_reg, max_iter=30, **tol))
    pipe = wca.TickPipeline(B, T, wca.MpcSolver(horizon=N, com_height=H), ik, k_com=R["k_com"], k_zmp=R["k_zmp"], kin=wca.KinModel(model),
                            planned_trajectories=True, neck_additional_rotation=np.eye(3), **mode)
    info = pipe.info()
    ms = []
    for _ in range(a.reps + 1):
        pipe.upload_footsteps(fs, fs)            # (rewinds to tick 0; synchronises)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); pipe.run(T); e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms = ms[1:]                                  # (the first: code load, first touch of the pages)
    res = pipe.download()
    out.update(ik_mode=info["ik_mode"], ticks_per_launch=info["ticks_per_launch"], run_ms={"median": float(np.median(ms)), "min": min(ms), "max": max(ms)},
               ms_per_tick=float(np.median(ms)) / T, ticks_done=int(res["tick"]), robots_stopped=int((res["ik_fail"] > 0).sum()),
               mpc_fail_ticks=int(res["mpc_fail"].sum()))
    if "ik_iters" in res:
        out.update(mean_iterations_per_tick=float(res["ik_iters"].mean()) / T, max_iterations_per_tick=float(res["ik_iters"].max()) / T)
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=150, help="seconds per step")
    ap.add_argument("--controller", choices=("reactive", "mpc"), default="reactive")
    ap.add_argument("--step", choices=STEPS, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.step:
        step(a)
        return
    out = {}
    for name in STEPS:
        r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--step", name, "--batch", str(a.batch),
                            "--ticks", str(a.ticks), "--reps", str(a.reps), "--controller", a.controller], capture_output=True, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            out[name] = {"failed": True, "exit_status": r.returncode, "stderr_tail": r.stderr[-600:]}
            break
        out[name] = json.loads(lines[-1][7:])
    if all(k in out and not out[k].get("failed") for k in ("position", "velocity")):
        out["position_over_velocity"] = out["position"]["ms_per_tick"] / out["velocity"]["ms_per_tick"]
        out["ms_per_iteration"] = out["position"]["ms_per_tick"] / out["position"]["mean_iterations_per_tick"]
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
