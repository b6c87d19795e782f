#!/usr/bin/env python3
"""Cost of streamed trajectories (wcqp_tick_set_desired_device) at `--batch` robots, fused kinematics, horizon 50, one run call per tick:

  (a) the sensor-fed EXTERNAL tick on the synthetic gait (tick_sensor_kernel + prime + tick kernel),
  (b) the streamed sensor-fed tick (tick_desired_kernel + tick_sensor_kernel<PL> + prime + tick kernel) on the same gait written as stages
      (tests/helpers/planned_tick.py::synthetic_as_planned, the stage source oracle/tick_spec.py::run_ticks(stages=...) restates), so that
      both sides do the same work,
  (c) tick_desired_kernel alone, back-to-back launches.

    python tools/streamed_tick_timing.py [--batch 8192] [--ticks 200] [--reps 5] [--out profiles/streamed_tick_timing.json]

The readings follow the walk: an untimed recording pass of handle (b) feeds every tick the robot's own desired joints and previous joint
velocities (downloaded) with wrenches that follow the contact pair, and keeps them on the device; the timed passes replay the recording, so
they repeat that run.  Per repetition: re-upload, `--ticks` timed ticks between device events, the forms alternating; the median over the
repetitions is reported, with the robots that ended stopped.  Kernel statistics: run this under `rocprofv3 --kernel-trace --stats` in a run
of its own."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402  (the GPU runtime first, then libwcqp)
import walking_controllers_amd as wca  # noqa: E402
from helpers import planned_tick as pt  # noqa: E402
from oracle import tick_spec as ts  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, T = a.batch, a.ticks
    dev = torch.device("cuda", 0)
    S = wca.synth
    kin = wca.KinModel(S.icub_like_model())
    kb = S.synth_walk_kin_batch(B)
    poses = kin.jacobians_host(kb["base"], kb["q"], state=np.zeros((B, 87)))["state"]
    p = ts.TickParams()
    plan, data = pt.synthetic_as_planned(p, S.synth_walk_batch(B, T, poses, kb), T, np.eye(3))
    ik = lambda: wca.IkSolver(form=wca.IK_FORM_QPOASES, v_max=S.WALK_VMAX, joint_reg_rad=np.deg2rad(S.WALK_POSTURE_DEG))
    synth = wca.TickPipeline(B, T, wca.MpcSolver(horizon=50), ik(), kin=kin, external_feedback=True)
    strm = wca.TickPipeline(B, T, wca.MpcSolver(horizon=50), ik(), kin=kin, external_feedback=True, streamed_trajectories=True,
                            neck_additional_rotation=np.eye(3))
    t_ = lambda x, dt=np.float64: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(dev)
    # the stages on the device, [T][B][..]
    st = {k: t_(np.swapaxes(plan[src], 0, 1)) for src, k in (("left_traj", "lp"), ("right_traj", "rp"), ("left_twist", "lt"), ("right_twist", "rt"))}
    st["c"] = t_(np.swapaxes(plan["contact"], 0, 1), np.uint8)
    s = torch.cuda.current_stream().cuda_stream
    # raw addresses, formed once: the binding's tensor checks and torch's slicing cost more host time per call than the kernel runs
    sp = [tuple(st[k][t].data_ptr() for k in ("lp", "rp", "lt", "rt", "c")) for t in range(T)]
    stage = lambda t: strm.set_desired_device(*sp[t], stream=s)
    # the recording pass: the robot's own joints and velocities as readings, wrenches by the contact pair
    code = np.swapaxes(plan["contact"].astype(int) & 3, 0, 1) - 1          # [T][B]
    wl = np.zeros((T, B, 6)); wr = np.zeros((T, B, 6))
    for w, off in ((wl, 1), (wr, 0)):
        w[:, :, 2] = np.where(code == off, 0.0, np.where(code == 2, 150.0, 300.0)); w[:, :, 3] = 0.3; w[:, :, 4] = -0.6
    WL, WR = t_(wl), t_(wr)
    Q = torch.zeros(T, B, 23, dtype=torch.float64, device=dev); DQ = torch.zeros(T, B, 23, dtype=torch.float64, device=dev)
    strm.upload(data)
    q, dq = data["q0"], np.zeros((B, 23))
    for t in range(T):
        Q[t] = t_(q); DQ[t] = t_(dq)
        stage(t)
        strm.set_sensor_feedback_device(Q[t], DQ[t], WL[t], WR[t], stream=s)
        strm.run(1, stream=s)
        q_new = strm.download()["q_des"]
        dq = 2.0 * (q_new - q) / p.dT - dq              # the trapezoid of the post step, inverted: this tick's joint velocity
        q = q_new
    rec = strm.download()

    rp = [tuple(x[t].data_ptr() for x in (Q, DQ, WL, WR)) for t in range(T)]

    def tick_a(t):
        synth.set_sensor_feedback_device(*rp[t], stream=s)
        synth.run(1, stream=s)

    def tick_b(t):
        stage(t)
        strm.set_sensor_feedback_device(*rp[t], stream=s)
        strm.run(1, stream=s)
    res = {"synthetic_sensor": [], "streamed_sensor": [], "desired_kernel": []}
    for rep in range(a.reps):
        for name, pipe, tick in (("synthetic_sensor", synth, tick_a), ("streamed_sensor", strm, tick_b)):
            pipe.upload(data)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for t in range(T):
                tick(t)
            e1.record()
            torch.cuda.synchronize()
            res[name].append(1e3 * e0.elapsed_time(e1) / T)
        strm.upload(data)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for t in range(T):
            stage(t)
        e1.record()
        torch.cuda.synchronize()
        res["desired_kernel"].append(1e3 * e0.elapsed_time(e1) / T)
    strm.upload(data)
    for t in range(T):
        tick_b(t)
    tick_b_out = strm.download()
    oa = synth.download()
    med = {k: float(np.median(v)) for k, v in res.items()}
    out = {"batch": B, "ticks": T, "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "us_per_tick_synthetic_sensor_external": med["synthetic_sensor"], "us_per_tick_streamed_sensor_external": med["streamed_sensor"],
           "us_desired_kernel_back_to_back": med["desired_kernel"],
           "ratio_streamed_over_synthetic": med["streamed_sensor"] / med["synthetic_sensor"],
           "spread_synthetic_us": float(np.max(res["synthetic_sensor"]) - np.min(res["synthetic_sensor"])),
           "all_reps_us": res,
           "robots_with_ik_fail": {"recording": int((rec["ik_fail"] > 0).sum()), "synthetic": int((oa["ik_fail"] > 0).sum()),
                                   "streamed": int((tick_b_out["ik_fail"] > 0).sum())},
           "feedback_fail": {"synthetic": int(oa["feedback_fail"].sum()), "streamed": int(tick_b_out["feedback_fail"].sum())},
           "max_abs_q_des_difference_streamed_vs_synthetic": float(np.abs(tick_b_out["q_des"] - oa["q_des"]).max()),
           "source_hash": wca.capi.source_hash()}
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
