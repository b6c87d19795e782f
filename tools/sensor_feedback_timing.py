#!/usr/bin/env python3
"""Cost of sensor feedback (wcqp_tick_set_sensor_feedback_device): the sensor kernel alone, and a sensor-fed EXTERNAL tick against a plain
EXTERNAL tick (wcqp_tick_set_feedback_device), at `--batch` robots with fused kinematics (horizon 50, the walk scenario of bench.py).

    python tools/sensor_feedback_timing.py [--batch 8192] [--ticks 200] [--reps 5] [--out profiles/r08_sensor_feedback_timing.json]

Per repetition: both handles re-upload, run `--warmup` ticks, then `--ticks` timed ticks, one wcqp_tick_run(1) per tick behind its
feedback call (device events around the loop), the two forms alternating.  The sensors are held (the initial joints, zero velocity, both
feet loaded), the plain form is fed what the sensor kernel evaluates from them: both handles run the same ticks.  The kernel alone:
`--ticks` back-to-back sensor launches between events.  The median over the repetitions is reported.  Kernel statistics: run this under
`rocprofv3 --kernel-trace --stats` in a run of its own."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (the GPU runtime first, then libwcqp)
import walking_controllers_amd as wca  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, T, W = a.batch, a.ticks, a.warmup
    dev = torch.device("cuda", 0)
    S = wca.synth
    kin = wca.KinModel(S.icub_like_model())
    kb = S.synth_walk_kin_batch(B)
    poses = kin.jacobians_host(kb["base"], kb["q"], state=np.zeros((B, 87)))["state"]
    data = S.synth_walk_batch(B, T + W, poses, kb)
    mk = lambda: wca.TickPipeline(B, T + W, wca.MpcSolver(horizon=50), wca.IkSolver(form=wca.IK_FORM_QPOASES, v_max=S.WALK_VMAX,
                                  joint_reg_rad=np.deg2rad(S.WALK_POSTURE_DEG)), kin=kin, external_feedback=True)
    plain, sens = mk(), mk()
    t_ = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)
    w = np.zeros((B, 6)); w[:, 2] = 150.0; w[:, 3] = 0.3; w[:, 4] = -0.6
    sf = [t_(data["q0"]), t_(np.zeros((B, 23))), t_(w), t_(w)]
    s = torch.cuda.current_stream().cuda_stream
    # the plain form is fed what the sensor kernel evaluates from these readings: both handles then run the same ticks
    sens.upload(data)
    sens.set_sensor_feedback_device(*sf, stream=s)
    sens.run(1, stream=s)
    m = sens.download()["measured"]
    fb = [t_(m[:, 0:2]), t_(m[:, 2:4]), t_(m[:, 4:6]), t_(data["q0"])]

    def run(pipe, feed, n):
        for _ in range(n):
            feed()
            pipe.run(1, stream=s)
    feed_plain = lambda: plain.set_feedback_device(*(x.data_ptr() for x in fb), stream=s)
    feed_sens = lambda: sens.set_sensor_feedback_device(*sf, stream=s)
    res = {"plain": [], "sensor": [], "kernel": []}
    for rep in range(a.reps):
        for name, pipe, feed in (("plain", plain, feed_plain), ("sensor", sens, feed_sens)):
            pipe.upload(data)
            run(pipe, feed, W)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); run(pipe, feed, T); e1.record()
            torch.cuda.synchronize()
            res[name].append(1e3 * e0.elapsed_time(e1) / T)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(T):
            feed_sens()
        e1.record()
        torch.cuda.synchronize()
        res["kernel"].append(1e3 * e0.elapsed_time(e1) / T)
    o, op = sens.download(), plain.download()
    med = {k: float(np.median(v)) for k, v in res.items()}
    out = {"batch": B, "ticks": T, "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "us_per_tick_plain_external": med["plain"], "us_per_tick_sensor_external": med["sensor"],
           "ratio_sensor_over_plain": med["sensor"] / med["plain"], "us_sensor_kernel_back_to_back": med["kernel"],
           "goal_kernel_under_10us": med["kernel"] < 10.0, "goal_ratio_at_most_1.15": med["sensor"] / med["plain"] <= 1.15,
           "all_reps_us": res, "sensor_run_feedback_fail": int(o["feedback_fail"].sum()), "sensor_run_robots_stopped": int((o["ik_fail"] > 0).sum()),
           "plain_run_robots_stopped": int((op["ik_fail"] > 0).sum()), "same_q_des_in_both_runs": bool(np.array_equal(o["q_des"], op["q_des"])),
           "source_hash": wca.capi.source_hash()}
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
