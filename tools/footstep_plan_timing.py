#!/usr/bin/env python3
"""Cost of generating planned walks on the device (wcqp_tick_upload_footsteps):

  (a) the record pass (plan_record_kernel, timed by the library with events around it: wcqp_tick_info.plan_record_ms) at `--batch` robots x
      T stages against a hipMemsetAsync of the same bytes (batch x T x 320 B) between events on the same device, and their ratio,
  (b) the whole upload_footsteps call at that size (host wall clock: the call synchronises), in the same child as (a),
  (c) both upload paths for the same plan at `--small-batch` robots x `--small-ticks` ticks, alternating, median of `--reps`: upload_footsteps
      against wcqp_tick_upload fed that plan from plan_window() (the classic path: three host passes over every stage, then the copy).

    python tools/footstep_plan_timing.py [--batch 8192] [--ticks 1200] [--out profiles/footstep_plan_timing.json]

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
STEPS = ("record_pass", "both_paths")


def _pipe(wca, B, T):
    S = wca.synth
    ik = wca.IkSolver(form=wca.IK_FORM_QPOASES, v_max=S.WALK_VMAX, joint_reg_rad=np.deg2rad(S.WALK_POSTURE_DEG))
    return wca.TickPipeline(B, T, wca.MpcSolver(horizon=50), ik, kin=wca.KinModel(S.icub_like_model()), planned_trajectories=True,
                            neck_additional_rotation=np.eye(3))


def _footsteps(wca, B, T):
    S = wca.synth
    kin = wca.KinModel(S.icub_like_model())
    kb = S.synth_walk_kin_batch(B)
    poses = kin.jacobians_host(kb["base"], kb["q"], state=np.zeros((B, 87)))["state"]
    return S.synth_footstep_walk_batch(B, T, poses, kb, n_steps=max(1, (T - 110) // 180), yaw_step=(0.03, 0.08))


def step(a):
    import torch  # the GPU runtime first, then libwcqp
    import walking_controllers_amd as wca
    out = {"device": torch.cuda.get_device_name(0), "source_hash": wca.capi.source_hash()}
    B, T = a.batch, a.ticks
    if a.step == "record_pass":
        nbytes = B * (T + 51) * 320
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
        buf = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        fill = []
        for _ in range(a.reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            assert hip.hipMemsetAsync(buf.data_ptr(), 0, nbytes, stream) == 0
            e1.record()
            torch.cuda.synchronize()
            fill.append(e0.elapsed_time(e1))
        del buf
        torch.cuda.empty_cache()
        fs = _footsteps(wca, B, T)
        pipe = _pipe(wca, B, T)
        rec, wall = [], []
        for _ in range(a.reps + 1):
            t0 = time.perf_counter(); pipe.upload_footsteps(fs, fs); wall.append(1e3 * (time.perf_counter() - t0))
            rec.append(pipe.info()["plan_record_ms"])
        fill, rec = fill[1:], rec[1:]          # (the first of each: first touch of the pages, code load)
        out.update(batch=B, stages=T + 51, record_bytes=nbytes,
                   memset_ms={"median": float(np.median(fill)), "min": min(fill), "max": max(fill), "GBps": nbytes / np.median(fill) / 1e6},
                   record_pass_ms={"median": float(np.median(rec)), "min": min(rec), "max": max(rec), "GBps": nbytes / np.median(rec) / 1e6},
                   record_pass_over_memset=float(np.median(rec) / np.median(fill)),
                   upload_footsteps_wall_ms={"first": wall[0], "median_of_rest": float(np.median(wall[1:])), "min": min(wall[1:]), "max": max(wall[1:])})
    else:
        Bs, Ts = a.small_batch, a.small_ticks
        fs = _footsteps(wca, Bs, Ts)
        gen, cla = _pipe(wca, Bs, Ts), _pipe(wca, Bs, Ts)
        gen.upload_footsteps(fs, fs)
        w = gen.plan_window()
        d = dict(fs, ref_traj=w["ref_traj"], dcm0=w["ref_traj"][:, 0].copy(), u_init=w["u_init"])
        kw = dict(left_traj=w["left_traj"], right_traj=w["right_traj"], left_twist=w["left_twist"], right_twist=w["right_twist"],
                  contact=w["contact"], com_height_traj=w["com_height"], com_height_vel=w["com_height_vel"])
        res = {"footsteps": [], "classic": []}
        for _ in range(a.reps):
            t0 = time.perf_counter(); gen.upload_footsteps(fs, fs); res["footsteps"].append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter(); cla.upload(d, **kw); res["classic"].append(1e3 * (time.perf_counter() - t0))
        ratio = [c / f for c, f in zip(res["classic"], res["footsteps"])]
        out.update(batch=Bs, ticks=Ts, ms=res, median_ms={k: float(np.median(v)) for k, v in res.items()},
                   classic_over_footsteps={"median": float(np.median(ratio)), "min": float(min(ratio)), "max": float(max(ratio))})
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--ticks", type=int, default=1200)
    ap.add_argument("--small-batch", type=int, default=1024)
    ap.add_argument("--small-ticks", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=170, help="seconds per step")
    ap.add_argument("--step", choices=STEPS, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.step:
        step(a)
        return
    out = {}
    args = ["--batch", a.batch, "--ticks", a.ticks, "--small-batch", a.small_batch, "--small-ticks", a.small_ticks, "--reps", a.reps]
    for name in STEPS:
        r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--step", name] + [str(x) for x in args],
                           capture_output=True, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            out[name] = {"failed": True, "exit_status": r.returncode, "stderr_tail": r.stderr[-600:]}
            break
        out[name] = json.loads(lines[-1][7:])
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
