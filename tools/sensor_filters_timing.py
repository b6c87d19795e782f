#!/usr/bin/env python3
"""Cost of the sensor form's low-pass filters (wcqp_tick_params.*_cut_frequency): tick_sensor_kernel<., true> with all three
filters on against tick_sensor_kernel<., false>, and a whole sensor-fed EXTERNAL tick filtered against unfiltered, at `--batch` robots
with fused kinematics (horizon 50, the walk scenario of bench.py), the two forms alternating within one session.

    python tools/sensor_filters_timing.py [--batch 8192] [--ticks 200] [--reps 5] [--out profiles/sensor_filters_timing.json]

Per repetition and form: re-upload, `--warmup` ticks, then `--ticks` timed ticks, one wcqp_tick_run(1) per tick behind its sensor call
(device events around the loop); then `--ticks` back-to-back sensor launches between events (replaced calls: every one reads the same
state slot and writes the other, the traffic of a real tick).  Held readings (the initial joints, zero velocity, both feet loaded).  The
median over the repetitions is reported.

The bar: the filtered kernel moves 66 doubles of state in and 66 out per robot, 1056 B; at 8192 robots 8.65 MB per tick.  Over half the
8 TB/s HBM peak (the project's roofline) that is the time the filters may add if none of it hides under the kinematics chain.  The
filtered kernel should cost no more than the unfiltered one re-measured here + that + the spread (max - min) of the unfiltered
repetitions.  Kernel statistics: run this under `rocprofv3 --kernel-trace --stats` in a run of its own."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (the GPU runtime first, then libwcqp)
import walking_controllers_amd as wca  # noqa: E402

STATE_BYTES_PER_ROBOT = 2 * 66 * 8
ROOFLINE_BYTES_PER_S = 0.5 * 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cut", type=float, default=10.0, help="cut frequency of all three filters [Hz]")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, T, W = a.batch, a.ticks, a.warmup
    dev = torch.device("cuda", 0)
    S = wca.synth
    kin = wca.KinModel(S.icub_like_model())
    kb = S.synth_walk_kin_batch(B)
    poses = kin.jacobians_host(kb["base"], kb["q"], state=np.zeros((B, 87)))["state"]
    data = S.synth_walk_batch(B, T + W, poses, kb)
    mk = lambda f: wca.TickPipeline(B, T + W, wca.MpcSolver(horizon=50), wca.IkSolver(form=wca.IK_FORM_QPOASES, v_max=S.WALK_VMAX,
                                    joint_reg_rad=np.deg2rad(S.WALK_POSTURE_DEG)), kin=kin, external_feedback=True, sensor_filters=f)
    pipes = {"unfiltered": mk(None), "filtered": mk(dict(joint_velocity=a.cut, wrench=a.cut, com=a.cut))}
    assert pipes["unfiltered"].info()["sensor_filters"] == 0 and pipes["filtered"].info()["sensor_filters"] == 7
    t_ = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)
    w = np.zeros((B, 6)); w[:, 2] = 150.0; w[:, 3] = 0.3; w[:, 4] = -0.6
    sf = [t_(data["q0"]), t_(np.zeros((B, 23))), t_(w), t_(w)]
    s = torch.cuda.current_stream().cuda_stream

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / n
    res = {f"{k}_{name}": [] for k in ("tick", "kernel") for name in pipes}
    for rep in range(a.reps):
        for name, pipe in pipes.items():
            feed = lambda: pipe.set_sensor_feedback_device(*sf, stream=s)

            def tick():
                feed()
                pipe.run(1, stream=s)
            pipe.upload(data)
            for _ in range(W):
                tick()
            res["tick_" + name].append(timed(tick, T))
            res["kernel_" + name].append(timed(feed, T))
    outs = {name: p.download() for name, p in pipes.items()}
    med = {k: float(np.median(v)) for k, v in res.items()}
    allowance = 1e6 * B * STATE_BYTES_PER_ROBOT / ROOFLINE_BYTES_PER_S
    spread = float(max(res["kernel_unfiltered"]) - min(res["kernel_unfiltered"]))
    bar = med["kernel_unfiltered"] + allowance + spread
    out = {"batch": B, "ticks": T, "reps": a.reps, "cut_hz": a.cut, "device": torch.cuda.get_device_name(0),
           "us_sensor_kernel_unfiltered": med["kernel_unfiltered"], "us_sensor_kernel_filtered": med["kernel_filtered"],
           "us_per_tick_unfiltered": med["tick_unfiltered"], "us_per_tick_filtered": med["tick_filtered"],
           "state_bytes_per_tick": B * STATE_BYTES_PER_ROBOT, "us_state_traffic_at_half_hbm_peak": allowance,
           "us_spread_unfiltered_kernel_reps": spread, "us_bar_filtered_kernel": bar, "bar_met": bool(med["kernel_filtered"] <= bar),
           "all_reps_us": res, "feedback_fail": {k: int(o["feedback_fail"].sum()) for k, o in outs.items()},
           "robots_stopped": {k: int((o["ik_fail"] > 0).sum()) for k, o in outs.items()}, "source_hash": wca.capi.source_hash()}
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
