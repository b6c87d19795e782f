#!/usr/bin/env python3
"""Cost of the POSITION tick on the measured robot (WCQP_TICK_OPT_POSITION_STREAMED) at `--batch` robots, one run call per
tick, on ONE generated walk - tools/position_tick_timing.py's: robots prepared at a CoM height of 0.42 m, steps of 60 + 40 stages behind a
double support of 40, the reactive law with gain scheduling (the loop that keeps every robot walking for 200 ticks), fused kinematics:

  (a) the sensor-fed resident-plan POSITION tick: tick_stage_from_plan_kernel + tick_sensor_kernel<PL> + position_tick_external_kernel
  (b) the sensor-fed resident-plan VELOCITY tick on the same plan and recording: the same two kernels + prime + tick kernel
  (c) the internal POSITION tick of a planned handle on the same walk, one tick per run call (and, beside it, the 200 ticks in one launch)

    python tools/position_external_timing.py [--batch 8192] [--ticks 200] [--reps 5] [--out profiles/position_external_timing.json] [--timeout 900]

The expectation, stated beforehand: (a) = (c) + the staging kernel (3.6 us, §8.18) + the sensor kernel (the difference between §8.18's
sensor-fed tick and §8.11's plain-fed one, about 10 us) - the IK dominates, so (a) should be (c) within a few per cent, and dozens of times (b).

The protocol is tools/resident_plan_timing.py's: an untimed recording pass on the POSITION handle feeds every tick the joints the tick
before commanded, zero joint velocities and wrenches that follow the contact pair, and keeps them on the device; the timed passes replay it
on both sensor-fed handles.  Per repetition: re-upload, `--ticks` timed ticks between device events, the forms alternating; medians over the
repetitions, with their spreads.  The process that is started measures nothing itself: the GPU work runs in a child process under a time limit
of its own."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, N, STEP_TICKS, DS_TICKS = 0.42, 50, 100, 40


def measure(a):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch  # (the GPU runtime first, then libwcqp)
    import walking_controllers_amd as wca
    import robots
    from helpers import zmp_gains as zg

    B, T = a.batch, a.ticks
    dev = torch.device("cuda", 0)
    S = wca.synth
    model = S.icub_like_model()
    q_reg = np.deg2rad(S.WALK_POSTURE_DEG)
    d = S.synth_prepare_batch(B, com_height=(H, H))
    o = wca.PrepareSolver(wca.KinModel(model), q_reg).solve_host(d["left_d"], d["right_d"], d["com_d"], d["q_guess"], d["Rd_neck"])
    assert (o["status"] == 0).all()
    fs = S.synth_footstep_walk_batch(B, T, o["state"], dict(q=o["q"]), step_ticks=STEP_TICKS, ds_ticks=DS_TICKS,
                                     n_steps=max(1, -(-(T - DS_TICKS) // STEP_TICKS)), com_height=H)
    fs["state0"] = o["state"]
    R = robots.ROBOTS["iCubGazeboV2_5"]
    ik = lambda: wca.IkSolver(form=wca.IK_FORM_QPOASES, neck_weight=R["neck_weight"] * np.eye(3), joint_reg_weights=np.array(R["reg_w"], float),
                              joint_reg_gains=np.array(R["reg_k"], float), joint_reg_rad=q_reg, v_max=S.WALK_VMAX.copy(), k_pos_com=R["k_pos_com"],
                              k_pos_foot=R["k_pos_foot"], k_att_foot=R["k_att_foot"], k_neck=R["k_neck"])
    ctl = dict(dcm_controller="reactive", k_dcm=1.0, zmp_gain_scheduling=True, **zg.ZMP_SCHEDULE["iCubGazeboV2_5"])
    pos = dict(ik_mode="position", position_ik=dict(q_reg=q_reg, max_iter=30))
    common = dict(k_com=R["k_com"], k_zmp=R["k_zmp"], kin=wca.KinModel(model), neck_additional_rotation=np.eye(3), **ctl)
    ext = dict(external_feedback=True, streamed_trajectories=True, resident_plan=True)
    mk = lambda **kw: wca.TickPipeline(B, T, wca.MpcSolver(horizon=N, com_height=H), ik(), **common, **kw)
    pe, ve, pi = mk(**ext, **pos), mk(**ext), mk(planned_trajectories=True, **pos)
    assert pe.option(wca.capi.TICK_OPT_POSITION_STREAMED) == 1 and ve.option(wca.capi.TICK_OPT_POSITION_STREAMED) == 0
    t_ = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)
    s = torch.cuda.current_stream().cuda_stream
    pe.upload_footsteps(fs, fs)
    code = np.swapaxes(pe.plan_window(m=T, keys=("contact",))["contact"].astype(int) & 3, 0, 1) - 1          # [T][B]
    wl = np.zeros((T, B, 6)); wr = np.zeros((T, B, 6))
    for x, off in ((wl, 1), (wr, 0)):
        x[:, :, 2] = np.where(code == off, 0.0, np.where(code == 2, 150.0, 300.0)); x[:, :, 3] = 0.3; x[:, :, 4] = -0.6
    WL, WR = t_(wl), t_(wr)
    Q = torch.zeros(T, B, 23, dtype=torch.float64, device=dev); DQ = torch.zeros(T, B, 23, dtype=torch.float64, device=dev)
    # the recording pass, on the POSITION handle: the encoders report the joints the tick before commanded
    q = fs["q0"]
    for t in range(T):
        Q[t] = t_(q)
        pe.set_desired_from_plan(stream=s)
        pe.set_sensor_feedback_device(Q[t], DQ[t], WL[t], WR[t], stream=s)
        pe.run(1, stream=s)
        q = pe.download()["q_des"]
    rec = pe.download()
    rp = [tuple(x[t].data_ptr() for x in (Q, DQ, WL, WR)) for t in range(T)]

    def sensor_tick(h):
        def tick(t):
            h.set_desired_from_plan(stream=s)
            h.set_sensor_feedback_device(*rp[t], stream=s)
            h.run(1, stream=s)
        return tick

    def timed(fn, n=T):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for t in range(n):
            fn(t)
        e1.record()
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / T
    forms = (("position_external", pe, sensor_tick(pe)), ("velocity_external", ve, sensor_tick(ve)), ("position_internal", pi, lambda t: pi.run(1, stream=s)))
    rows = {name: [] for name, _, _ in forms}
    rows["position_internal_one_launch"] = []
    done = {}
    for rep in range(a.reps + 1):                # (the first: code load, first touch of the pages)
        order = forms if rep % 2 == 0 else forms[::-1]
        for name, h, tick in order:
            h.upload_footsteps(fs, fs)           # (rewinds to tick 0; synchronises)
            us = timed(tick)
            if rep > 0:
                rows[name].append(us)
            done[name] = h.download()
        pi.upload_footsteps(fs, fs)
        us = timed(lambda t: pi.run(T, stream=s), n=1)
        if rep > 0:
            rows["position_internal_one_launch"].append(us)
    stat = lambda v: dict(median_us=float(np.median(v)), min_us=float(np.min(v)), max_us=float(np.max(v)), all_us=[float(x) for x in v])
    med = {k: float(np.median(v)) for k, v in rows.items()}
    out = {"batch": B, "ticks": T, "reps": a.reps, "controller": "reactive, gain scheduling", "com_height": H, "device": torch.cuda.get_device_name(0),
           "a_position_sensor_fed_resident_plan_tick": stat(rows["position_external"]),
           "b_velocity_sensor_fed_resident_plan_tick": stat(rows["velocity_external"]),
           "c_position_internal_tick_one_run_call_per_tick": stat(rows["position_internal"]),
           "position_internal_tick_one_launch": stat(rows["position_internal_one_launch"]),
           "a_minus_c_us": med["position_external"] - med["position_internal"],
           "ratio_a_over_c": med["position_external"] / med["position_internal"], "ratio_a_over_b": med["position_external"] / med["velocity_external"],
           "mean_iterations_per_tick": {k: float(done[k]["ik_iters"].mean()) / T for k in ("position_external", "position_internal")},
           "robots_with_ik_fail": dict(recording=int((rec["ik_fail"] > 0).sum()), **{k: int((v["ik_fail"] > 0).sum()) for k, v in done.items()}),
           "feedback_fail": {k: int(done[k]["feedback_fail"].sum()) for k in ("position_external", "velocity_external")},
           "max_abs_q_des_difference_a_vs_recording": float(np.abs(done["position_external"]["q_des"] - rec["q_des"]).max()),
           "source_hash": wca.capi.source_hash()}
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=900, help="seconds the measuring child process may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return measure(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--batch", str(a.batch), "--ticks", str(a.ticks), "--reps", str(a.reps)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not lines:
        sys.stderr.write(r.stdout[-4000:] + r.stderr[-4000:])
        return 1
    out = json.loads(lines[-1][len("RESULT "):])
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
