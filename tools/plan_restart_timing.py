#!/usr/bin/env python3
"""Cost of restarting robots of a running fleet (wcqp_tick_restart_robots), at `--batch` robots x T = ticks + 51 stages and
S = `--stage` ticks enqueued, medians of `--reps` after a warm-up, all in one session:

  (a) the call's kernels on the stream, between events (behind a busy stream, so that the host's staging is not in the interval), with
      1 %, 10 % and 100 % of the robots restarting (every 100th, every 10th, all), each against a plain hipMemcpyAsync device-to-device
      copy of the bytes its fill writes (robots x (T - S) x 352 B: records, ref_traj and dcm_vel) and against
      wcqp_tick_info.plan_record_ms of a full wcqp_tick_upload_footsteps, today's only alternative (`--reps` uploads after a warm-up),
  (b) the host wall clock of the call (it is enqueue-only) against that of the upload (which synchronises),
  (c) a wcqp_tick_run of 100 ticks before and after a 1 % restart, between events: the ticks that follow cost what they did.

    python tools/plan_restart_timing.py [--batch 8192] [--ticks 1200] [--stage 200] [--out profiles/plan_restart_timing.json]

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
STEPS = ("copy", "restart", "ticks")
FRACTIONS = (("1pct", 100), ("10pct", 10), ("100pct", 1))      # every k-th robot restarts


def _pipe(wca, B, T):
    """the reactive controller with gain scheduling: the handle keeps every array a restart writes (dcm_vel and the gain smoother among
    them); the internal plant undisturbed"""
    S = wca.synth
    ik = wca.IkSolver(form=wca.IK_FORM_QPOASES, v_max=S.WALK_VMAX, joint_reg_rad=np.deg2rad(S.WALK_POSTURE_DEG))
    return wca.TickPipeline(B, T, wca.MpcSolver(horizon=50), ik, kin=wca.KinModel(S.icub_like_model()), planned_trajectories=True,
                            neck_additional_rotation=np.eye(3), noise=0.0, dcm_controller="reactive", k_dcm=1.0, zmp_gain_scheduling=True,
                            k_com_stance=6.0, k_zmp_stance=0.9, zmp_smoothing_time=0.05)


def _footsteps(wca, B, T):
    """tools/footstep_plan_timing.py's walk"""
    S = wca.synth
    kin = wca.KinModel(S.icub_like_model())
    kb = S.synth_walk_kin_batch(B)
    poses = kin.jacobians_host(kb["base"], kb["q"], state=np.zeros((B, 87)))["state"]
    fs = S.synth_footstep_walk_batch(B, T, poses, kb, n_steps=max(1, (T - 110) // 180), yaw_step=(0.03, 0.08))
    fs["final_ds_ticks"] = 0
    return fs


def _stats(v, nbytes=None):
    out = {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}
    if nbytes:
        out["GBps"] = nbytes / out["median"] / 1e6
    return out


def _listed(B, every):
    return np.arange(0, B, every)


def step(a):
    import torch  # the GPU runtime first, then libwcqp
    import walking_controllers_amd as wca
    out = {"device": torch.cuda.get_device_name(0), "source_hash": wca.capi.source_hash()}
    B, T, S0 = a.batch, a.ticks, a.stage
    stages = T + 51
    stream = torch.cuda.current_stream().cuda_stream
    ev = lambda: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    out.update(batch=B, stages=stages, stage=S0)
    if a.step == "copy":
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        full = B * (stages - S0) * 352
        src, dst = (torch.zeros(full, dtype=torch.uint8, device="cuda") for _ in range(2))
        for name, every in FRACTIONS:
            nbytes = len(_listed(B, every)) * (stages - S0) * 352
            ms = []
            for _ in range(a.reps + 1):
                e0, e1 = ev()
                e0.record()
                assert hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, 3, stream) == 0       # (3: hipMemcpyDeviceToDevice)
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1))
            out[name] = dict(bytes=nbytes, copy_ms=_stats(ms[1:], nbytes))
    else:
        fs = _footsteps(wca, B, T)
        rows = {k: fs[k] for k in ("state0", "q0", "com0")}
        pipe = _pipe(wca, B, T)

        def mode(every):
            m = np.zeros(B, np.uint8)
            m[_listed(B, every)] = wca.capi.TICK_RESTART_ALWAYS
            return m
        if a.step == "restart":
            up, rec = [], []
            for _ in range(a.reps + 1):      # the alternative: the whole upload, its record pass timed by the library
                t0 = time.perf_counter(); pipe.upload_footsteps(fs, fs); up.append(1e3 * (time.perf_counter() - t0))
                rec.append(pipe.info()["plan_record_ms"])
            for name, every in FRACTIONS:
                # (a fresh plan per fraction: every restart at the same stage takes one more of a robot's set slots)
                pipe.upload_footsteps(fs, fs)
                pipe.run(S0)
                torch.cuda.synchronize()
                m, dev, wall = mode(every), [], []
                gx, gy = (torch.zeros(1 << 30, dtype=torch.uint8, device="cuda") for _ in range(2))
                nbytes = len(_listed(B, every)) * (stages - S0) * 352
                for _ in range(a.reps + 1):
                    e0, e1 = ev()
                    # the call stages its rows on the host before it enqueues: the stream is kept busy meanwhile (ten 1 GiB copies, several
                    # milliseconds), so that the first event is reached with the call's kernels already queued behind it
                    for _ in range(10):
                        gy.copy_(gx)
                    e0.record()
                    t0 = time.perf_counter()
                    pipe.restart_robots(m, rows, stream=stream)
                    wall.append(1e3 * (time.perf_counter() - t0))
                    e1.record()
                    torch.cuda.synchronize()
                    dev.append(e0.elapsed_time(e1))
                res = pipe.restart_result()
                assert res["stage"] == S0 and int(res["restarted"].sum()) == len(_listed(B, every))
                # (the first of each: first touch of the pages, code load, the block's growth)
                out[name] = dict(robots=len(_listed(B, every)), bytes=nbytes, restart_kernels_ms=_stats(dev[1:], nbytes), restart_call_wall_ms=_stats(wall[1:]))
            out.update(upload_footsteps_wall_ms=_stats(up[1:]), plan_record_ms=_stats(rec[1:]))
        else:
            pipe.upload_footsteps(fs, fs)
            pipe.run(S0 - 100)
            torch.cuda.synchronize()
            ms = []
            for k in range(2):
                e0, e1 = ev()
                e0.record()
                pipe.run(100, stream=stream)
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1))
                if k == 0:
                    pipe.restart_robots(mode(100), rows, stream=stream)
                    torch.cuda.synchronize()
            out.update(run_100_ticks_before_ms=ms[0], run_100_ticks_after_ms=ms[1], ik_fail_robots=int((pipe.download()["ik_fail"] > 0).sum()))
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--ticks", type=int, default=1200)
    ap.add_argument("--stage", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds per step")
    ap.add_argument("--step", choices=STEPS, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.step:
        step(a)
        return
    out = {}
    args = ["--batch", a.batch, "--ticks", a.ticks, "--stage", a.stage, "--reps", a.reps]
    for name in STEPS:
        r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--step", name] + [str(x) for x in args],
                           capture_output=True, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            out[name] = {"failed": True, "exit_status": r.returncode, "stderr_tail": r.stderr[-600:]}
            break
        out[name] = json.loads(lines[-1][7:])
    if all(k in out and not out[k].get("failed") for k in STEPS):
        c, r, t = out["copy"], out["restart"], out["ticks"]
        out["ratios"] = {}
        for name, _ in FRACTIONS:
            out["ratios"][name] = {"restart_kernels_over_copy": r[name]["restart_kernels_ms"]["median"] / c[name]["copy_ms"]["median"],
                                   "restart_kernels_over_upload_record_pass": r[name]["restart_kernels_ms"]["median"] / r["plan_record_ms"]["median"],
                                   "restart_call_over_upload_footsteps_wall": r[name]["restart_call_wall_ms"]["median"] / r["upload_footsteps_wall_ms"]["median"]}
        out["ratios"]["run_100_ticks_after_over_before"] = t["run_100_ticks_after_ms"] / t["run_100_ticks_before_ms"]
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
