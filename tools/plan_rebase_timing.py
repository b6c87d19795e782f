#!/usr/bin/env python3
"""Cost of rebasing a running generated plan (wcqp_tick_rebase_plan), at `--batch` robots x T = ticks + 51 stages with a shift
of `--shift` stages, medians of `--reps`, all in one session:

  (a) the rebase kernels on the stream, between events,
  (b) a plain, non-overlapping hipMemcpyAsync device-to-device copy of the same bytes (records, ref_traj and dcm_vel: batch x T x 352 B)
      between events - the yardstick for (a),
  (c) the host wall clock of the whole rebase call (it is enqueue-only),
  (d) the whole wcqp_tick_upload_footsteps call at that size (host wall clock: the call synchronises) - the only other way to go on past
      max_ticks, and it loses the robots' state,

and the ratios (a) / (b), (c) / (d), with what a rebase every `--shift` ticks costs per tick.

    python tools/plan_rebase_timing.py [--batch 8192] [--ticks 1200] [--shift 1000] [--out profiles/plan_rebase_timing.json]

At `--shift 1000` of 1251 stages the rebase writes every byte but reads only the stages it keeps; `--shift 2` (kept as
profiles/plan_rebase_timing_shift2.json) reads and writes every byte, as the copy does.

This process never opens the GPU: each step is a child process of its own (`--step NAME`) under `timeout -k 10 LIMIT`, which ends a step that
hangs inside a device call; after a step that fails or is ended no further step starts, and the result holds what was measured so far."""
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
STEPS = ("copy", "rebase")


def _pipe(wca, B, T):
    """the reactive controller with gain scheduling: the handle keeps every array a rebase moves (dcm_vel among them), and its ticks are
    the cheapest way to the tick count a shift needs; the internal plant undisturbed, as a rebase asks"""
    S = wca.synth
    ik = wca.IkSolver(form=wca.IK_FORM_QPOASES, v_max=S.WALK_VMAX, joint_reg_rad=np.deg2rad(S.WALK_POSTURE_DEG))
    return wca.TickPipeline(B, T, wca.MpcSolver(horizon=50), ik, kin=wca.KinModel(S.icub_like_model()), planned_trajectories=True,
                            neck_additional_rotation=np.eye(3), noise=0.0, dcm_controller="reactive", k_dcm=1.0, zmp_gain_scheduling=True,
                            k_com_stance=6.0, k_zmp_stance=0.9, zmp_smoothing_time=0.05)


def _footsteps(wca, B, T):
    """tools/footstep_plan_timing.py's walk, with a last double support that ends: the plan stands within max_ticks"""
    S = wca.synth
    kin = wca.KinModel(S.icub_like_model())
    kb = S.synth_walk_kin_batch(B)
    poses = kin.jacobians_host(kb["base"], kb["q"], state=np.zeros((B, 87)))["state"]
    n = max(1, (T - 110) // 180)
    fs = S.synth_footstep_walk_batch(B, T, poses, kb, n_steps=n, yaw_step=(0.03, 0.08))
    fs["final_ds_ticks"] = 0
    assert fs["first_ds_ticks"] + n * (fs["ss_ticks"] + fs["ds_ticks"]) <= T, "the plan must stand within max_ticks"
    return fs


def _stats(v, nbytes=None):
    out = {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}
    if nbytes:
        out["GBps"] = nbytes / out["median"] / 1e6
    return out


def step(a):
    import torch  # the GPU runtime first, then libwcqp
    import walking_controllers_amd as wca
    out = {"device": torch.cuda.get_device_name(0), "source_hash": wca.capi.source_hash()}
    B, T, R = a.batch, a.ticks, a.shift
    nbytes = B * (T + 51) * 352
    stream = torch.cuda.current_stream().cuda_stream
    ev = lambda: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    if a.step == "copy":
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        src, dst = (torch.zeros(nbytes, dtype=torch.uint8, device="cuda") for _ in range(2))
        ms = []
        for _ in range(a.reps + 1):
            e0, e1 = ev()
            e0.record()
            assert hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, 3, stream) == 0       # (3: hipMemcpyDeviceToDevice)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        out.update(batch=B, stages=T + 51, bytes=nbytes, copy_ms=_stats(ms[1:], nbytes))
    else:
        fs = _footsteps(wca, B, T)
        pipe = _pipe(wca, B, T)
        up = []
        for _ in range(a.reps + 1):
            t0 = time.perf_counter(); pipe.upload_footsteps(fs, fs); up.append(1e3 * (time.perf_counter() - t0))
        dev, wall = [], []
        for _ in range(a.reps + 1):
            pipe.run(R)
            torch.cuda.synchronize()
            e0, e1 = ev()
            e0.record()
            t0 = time.perf_counter()
            took = pipe.rebase_plan(R, stream=stream)
            wall.append(1e3 * (time.perf_counter() - t0))
            e1.record()
            torch.cuda.synchronize()
            assert took == R
            dev.append(e0.elapsed_time(e1))
        # (the first of each: first touch of the pages, code load)
        out.update(batch=B, stages=T + 51, shift=R, bytes=nbytes, rebase_kernels_ms=_stats(dev[1:], nbytes), rebase_call_wall_ms=_stats(wall[1:]),
                   upload_footsteps_wall_ms=_stats(up[1:]), plan_shift=pipe.option(wca.capi.TICK_OPT_PLAN_SHIFT))
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--ticks", type=int, default=1200)
    ap.add_argument("--shift", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds per step")
    ap.add_argument("--step", choices=STEPS, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.step:
        step(a)
        return
    out = {}
    args = ["--batch", a.batch, "--ticks", a.ticks, "--shift", a.shift, "--reps", a.reps]
    for name in STEPS:
        r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--step", name] + [str(x) for x in args],
                           capture_output=True, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            out[name] = {"failed": True, "exit_status": r.returncode, "stderr_tail": r.stderr[-600:]}
            break
        out[name] = json.loads(lines[-1][7:])
    if "rebase" in out and not out["rebase"].get("failed"):
        c, r = out["copy"], out["rebase"]
        out["ratios"] = {"rebase_kernels_over_copy": r["rebase_kernels_ms"]["median"] / c["copy_ms"]["median"],
                         "rebase_call_over_upload_footsteps": r["rebase_call_wall_ms"]["median"] / r["upload_footsteps_wall_ms"]["median"],
                         "rebase_kernels_us_per_tick": 1e3 * r["rebase_kernels_ms"]["median"] / a.shift}
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
