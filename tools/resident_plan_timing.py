#!/usr/bin/env python3
"""Cost of a resident plan (wcqp_tick_params_ext.resident_plan) at `--batch` robots, fused kinematics, horizon 50, one run call per tick, on ONE
generated walk (wcqp_tick_upload_footsteps on the resident-plan handle; the streamed handle is handed that handle's plan_window()):

  (a) the streamed sensor-fed tick with every stage handed over by wcqp_tick_set_desired_device from device arrays
      (tick_desired_kernel + tick_sensor_kernel<PL> + prime + tick kernel) - the yardstick, measured in the same run,
  (b) the resident-plan tick (tick_stage_from_plan_kernel in tick_desired_kernel's place),
  (c) tick_stage_from_plan_kernel alone between events, back-to-back launches - and tick_desired_kernel the same way beside it.

    python tools/resident_plan_timing.py [--batch 8192] [--ticks 200] [--reps 5] [--out profiles/resident_plan_timing.json] [--timeout 900]

The protocol is tools/streamed_tick_timing.py's: an untimed recording pass feeds every tick the robot's own desired joints and previous
joint velocities with wrenches that follow the contact pair and keeps them on the device; the timed passes replay it.  Per repetition:
re-upload, `--ticks` timed ticks between device events, the forms alternating; medians over the repetitions, with their spreads.  The
process that is started measures nothing itself: the GPU work runs in a child process under a time limit of its own."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def measure(a):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch  # (the GPU runtime first, then libwcqp)
    import walking_controllers_amd as wca

    B, T = a.batch, a.ticks
    dev = torch.device("cuda", 0)
    S = wca.synth
    kin = wca.KinModel(S.icub_like_model())
    kb = S.synth_walk_kin_batch(B)
    poses = kin.jacobians_host(kb["base"], kb["q"], state=np.zeros((B, 87)))["state"]
    fs = S.synth_footstep_walk_batch(B, T, poses, kb, yaw_step=(0.03, 0.08))
    ik = lambda: wca.IkSolver(form=wca.IK_FORM_QPOASES, v_max=S.WALK_VMAX, joint_reg_rad=np.deg2rad(S.WALK_POSTURE_DEG))
    common = dict(kin=kin, external_feedback=True, streamed_trajectories=True, neck_additional_rotation=np.eye(3))
    res = wca.TickPipeline(B, T, wca.MpcSolver(horizon=50), ik(), resident_plan=True, **common)
    strm = wca.TickPipeline(B, T, wca.MpcSolver(horizon=50), ik(), **common)
    res.upload_footsteps(fs, fs)
    ref = res.plan_window(keys=("ref_traj",))["ref_traj"]
    u_init = res.plan_window(m=1, keys=("u_init",))["u_init"]
    w = res.plan_window(m=T, keys=("left_traj", "right_traj", "left_twist", "right_twist", "contact", "com_height", "com_height_vel"))
    data = dict(state0=fs["state0"], q0=fs["q0"], com0=fs["com0"], ref_traj=ref, dcm0=ref[:, 0].copy(), u_init=u_init)
    t_ = lambda x, dt=np.float64: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(dev)
    keys = ("left_traj", "right_traj", "left_twist", "right_twist", "contact", "com_height", "com_height_vel")
    st = {k: t_(np.swapaxes(w[k], 0, 1), np.uint8 if k == "contact" else np.float64) for k in keys}       # the stages on the device, [T][B][..]
    s = torch.cuda.current_stream().cuda_stream
    # raw addresses, formed once: the binding's tensor checks and torch's slicing cost more host time per call than the kernel runs
    sp = [tuple(st[k][t].data_ptr() for k in keys) for t in range(T)]
    stage = lambda t: strm.set_desired_device(*sp[t], stream=s)
    code = np.swapaxes(w["contact"].astype(int) & 3, 0, 1) - 1          # [T][B]
    wl = np.zeros((T, B, 6)); wr = np.zeros((T, B, 6))
    for x, off in ((wl, 1), (wr, 0)):
        x[:, :, 2] = np.where(code == off, 0.0, np.where(code == 2, 150.0, 300.0)); x[:, :, 3] = 0.3; x[:, :, 4] = -0.6
    WL, WR = t_(wl), t_(wr)
    Q = torch.zeros(T, B, 23, dtype=torch.float64, device=dev); DQ = torch.zeros(T, B, 23, dtype=torch.float64, device=dev)
    # the recording pass, on the streamed handle
    strm.upload(data)
    q, dq = fs["q0"], np.zeros((B, 23))
    for t in range(T):
        Q[t] = t_(q); DQ[t] = t_(dq)
        stage(t)
        strm.set_sensor_feedback_device(Q[t], DQ[t], WL[t], WR[t], stream=s)
        strm.run(1, stream=s)
        q_new = strm.download()["q_des"]
        dq = 2.0 * (q_new - q) / 0.01 - dq              # the trapezoid of the post step, inverted: this tick's joint velocity
        q = q_new
    rec = strm.download()
    rp = [tuple(x[t].data_ptr() for x in (Q, DQ, WL, WR)) for t in range(T)]

    def tick_a(t):
        stage(t)
        strm.set_sensor_feedback_device(*rp[t], stream=s)
        strm.run(1, stream=s)

    def tick_b(t):
        res.set_desired_from_plan(stream=s)
        res.set_sensor_feedback_device(*rp[t], stream=s)
        res.run(1, stream=s)

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for t in range(T):
            fn(t)
        e1.record()
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / T
    out_rows = {"handed_over": [], "resident_plan": [], "stage_from_plan_kernel": [], "desired_kernel": []}
    for rep in range(a.reps):
        order = (("handed_over", tick_a), ("resident_plan", tick_b)) if rep % 2 == 0 else (("resident_plan", tick_b), ("handed_over", tick_a))
        for name, tick in order:
            if name == "handed_over":
                strm.upload(data)
            else:
                res.upload_footsteps(fs, fs)
            out_rows[name].append(timed(tick))
        res.upload_footsteps(fs, fs)
        out_rows["stage_from_plan_kernel"].append(timed(lambda t: res.set_desired_from_plan(stream=s)))
        strm.upload(data)
        out_rows["desired_kernel"].append(timed(stage))
    strm.upload(data)
    res.upload_footsteps(fs, fs)
    for t in range(T):
        tick_a(t); tick_b(t)
    oa, ob = strm.download(), res.download()
    stat = lambda v: dict(median_us=float(np.median(v)), min_us=float(np.min(v)), max_us=float(np.max(v)), all_us=[float(x) for x in v])
    out = {"batch": B, "ticks": T, "reps": a.reps, "horizon": 50, "device": torch.cuda.get_device_name(0),
           "a_streamed_sensor_tick_handed_over": stat(out_rows["handed_over"]),
           "b_resident_plan_sensor_tick": stat(out_rows["resident_plan"]),
           "c_stage_from_plan_kernel_back_to_back": stat(out_rows["stage_from_plan_kernel"]),
           "tick_desired_kernel_back_to_back": stat(out_rows["desired_kernel"]),
           "ratio_b_over_a": float(np.median(out_rows["resident_plan"]) / np.median(out_rows["handed_over"])),
           "robots_with_ik_fail": {"recording": int((rec["ik_fail"] > 0).sum()), "handed_over": int((oa["ik_fail"] > 0).sum()),
                                   "resident_plan": int((ob["ik_fail"] > 0).sum())},
           "feedback_fail": {"handed_over": int(oa["feedback_fail"].sum()), "resident_plan": int(ob["feedback_fail"].sum())},
           "max_abs_q_des_difference_b_vs_a": float(np.abs(ob["q_des"] - oa["q_des"]).max()),
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
