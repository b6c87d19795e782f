#!/usr/bin/env python3
"""Cost of planning footsteps on the device from per-robot goals (wcqp_unicycle_*):

  (a) wcqp_unicycle_plan_device for `--batch` robots with K = `--max-steps` steps of D = `--step-ticks` samples, between events on the
      null stream, median of `--reps` after one untimed call - goals from the disc of 1 m, so most robots walk all K x D samples,
  (b) the whole TickPipeline.upload_goal call at that size on a handle of `--ticks` ticks (host wall clock: the call synchronises) next to
      upload_footsteps alone fed the same footsteps, alternating, median of `--reps`.

    python tools/unicycle_plan_timing.py [--batch 8192] [--out profiles/unicycle_plan_timing.json]

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
STEPS = ("plan_device", "upload_goal")
OUT = ("n_steps", "side", "target", "status", "desired_point", "unicycle_end")


def _stats(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def step(a):
    import walking_controllers_amd as wca
    S = wca.synth
    B, K, D = a.batch, a.max_steps, a.step_ticks
    out = {"source_hash": wca.capi.source_hash(), "batch": B, "max_steps": K, "step_ticks": D}
    par = dict(step_ticks=D, max_steps=K, max_linear_velocity=0.03, max_angular_velocity=0.15, min_step_length=0.005, min_angle_variation=0.01)
    if a.step == "plan_device":
        # device arrays and events from the HIP runtime libwcqp is linked against, through the library's own handle
        L = wca.capi.lib()
        L.hipMalloc.argtypes, L.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p]
        L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        L.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
        L.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        L.hipEventSynchronize.argtypes = [C.c_void_p]
        L.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        g = S.synth_goal_batch(B, cases=False)
        pl = wca.UnicyclePlanner(**par)
        host = {k: np.ascontiguousarray(g[k]) for k in ("left0", "right0", "goals", "first_side")}
        host.update(n_steps=np.zeros(B, np.int32), side=np.zeros((B, K), np.uint8), target=np.zeros((B, K, 3)), status=np.zeros(B, np.int32),
                    desired_point=np.zeros((B, 2)), unicycle_end=np.zeros((B, 3)))
        ptr = {}
        for k, v in host.items():
            ptr[k] = C.c_void_p()
            assert L.hipMalloc(C.byref(ptr[k]), max(v.nbytes, 8)) == 0 and L.hipMemcpy(ptr[k], v.ctypes.data, v.nbytes, 1) == 0
        e0, e1 = C.c_void_p(), C.c_void_p()
        assert L.hipEventCreate(C.byref(e0)) == 0 and L.hipEventCreate(C.byref(e1)) == 0
        ms = []
        for _ in range(a.reps + 1):
            assert L.hipEventRecord(e0, None) == 0
            pl.plan_device(B, ptr["left0"].value, ptr["right0"].value, ptr["goals"].value, ptr["first_side"].value, ptr["n_steps"].value,
                           ptr["side"].value, ptr["target"].value, ptr["status"].value, ptr["desired_point"].value, ptr["unicycle_end"].value)
            assert L.hipEventRecord(e1, None) == 0 and L.hipEventSynchronize(e1) == 0
            t = C.c_float()
            assert L.hipEventElapsedTime(C.byref(t), e0, e1) == 0
            ms.append(t.value)
        for k in ("n_steps", "status"):
            assert L.hipMemcpy(host[k].ctypes.data, ptr[k], host[k].nbytes, 2) == 0
        for v in ptr.values():
            L.hipFree(v)
        out.update(plan_device_ms=_stats(ms[1:]), first_call_ms=ms[0], samples_walked=int(host["n_steps"].sum()) * D,
                   status_counts=np.bincount(host["status"], minlength=4).tolist(), mean_steps=float(host["n_steps"].mean()))
    else:
        T = a.ticks
        kin = wca.KinModel(S.icub_like_model())
        kb = S.synth_walk_kin_batch(B)
        poses = kin.jacobians_host(kb["base"], kb["q"], state=np.zeros((B, 87)))["state"]
        fs = S.synth_footstep_walk_batch(B, T, poses, kb)
        g = S.synth_goal_batch(B, state0=fs["state0"], cases=False, radius=0.3)
        ss, ds = D - D // 3, D // 3
        pl = wca.UnicyclePlanner(nominal_width=0.118, min_width=0.10, **par)
        ik = wca.IkSolver(form=wca.IK_FORM_QPOASES, v_max=S.WALK_VMAX, joint_reg_rad=np.deg2rad(S.WALK_POSTURE_DEG))
        pipe = wca.TickPipeline(B, T, wca.MpcSolver(horizon=50), ik, kin=kin, planned_trajectories=True, neck_additional_rotation=np.eye(3))
        res = {"upload_goal": [], "plan_host": [], "upload_footsteps": []}
        for _ in range(a.reps + 1):
            t0 = time.perf_counter(); plan = pipe.upload_goal(fs, g["goals"], pl, g["first_side"], ds, ss, ds); res["upload_goal"].append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter(); pl.plan_host(g["left0"], g["right0"], g["goals"], g["first_side"]); res["plan_host"].append(1e3 * (time.perf_counter() - t0))
            steps = dict(fs, n_steps=plan["n_steps"], side=plan["side"], target=plan["target"], first_ds_ticks=ds, ss_ticks=ss, ds_ticks=ds, final_ds_ticks=0)
            t0 = time.perf_counter(); pipe.upload_footsteps(fs, steps); res["upload_footsteps"].append(1e3 * (time.perf_counter() - t0))
        out.update(ticks=T, first_call_ms={k: v[0] for k, v in res.items()}, wall_ms={k: _stats(v[1:]) for k, v in res.items()},
                   status_counts=np.bincount(plan["status"], minlength=4).tolist(), mean_steps=float(plan["n_steps"].mean()))
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--max-steps", type=int, default=20)
    ap.add_argument("--step-ticks", type=int, default=100)
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
    args = ["--batch", a.batch, "--max-steps", a.max_steps, "--step-ticks", a.step_ticks, "--ticks", a.ticks, "--reps", a.reps]
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
