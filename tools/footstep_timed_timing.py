#!/usr/bin/env python3
"""Cost of per-step timings, next to the untimed forms at the same size and in the same child process:

  (a) upload_footsteps at `--batch` robots x `--ticks` ticks, untimed and timed (synth_timed_footstep_walk_batch: the same footsteps,
      durations that differ per robot and per step), one form after the other: the record pass (events around it: wcqp_tick_info.plan_record_ms) and the
      whole call (host wall clock: it synchronises), medians of `--reps` after one untimed call of each,
  (b) wcqp_unicycle_plan_device with D = `--step-ticks` samples per step and wcqp_unicycle_plan_timed_device with min / nominal / max =
      0.8 D / 0.9 D / D, for `--batch` robots and K = `--max-steps` steps, between events on the null stream, medians likewise.

    python tools/footstep_timed_timing.py [--batch 8192] [--out profiles/footstep_timed_timing.json]

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
STEPS = ("upload", "planner")


def _stats(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def step(a):
    import walking_controllers_amd as wca
    S = wca.synth
    B = a.batch
    out = {"source_hash": wca.capi.source_hash(), "batch": B}
    if a.step == "upload":
        T = a.ticks
        kin = wca.KinModel(S.icub_like_model())
        kb = S.synth_walk_kin_batch(B)
        poses = kin.jacobians_host(kb["base"], kb["q"], state=np.zeros((B, 87)))["state"]
        kw = dict(n_steps=max(1, (T - 110) // 180), yaw_step=(0.03, 0.08))
        fs = {"untimed": S.synth_footstep_walk_batch(B, T, poses, kb, **kw), "timed": S.synth_timed_footstep_walk_batch(B, T, poses, kb, **kw)}
        ik = wca.IkSolver(form=wca.IK_FORM_QPOASES, v_max=S.WALK_VMAX, joint_reg_rad=np.deg2rad(S.WALK_POSTURE_DEG))
        pipe = wca.TickPipeline(B, T, wca.MpcSolver(horizon=50), ik, kin=kin, planned_trajectories=True, neck_additional_rotation=np.eye(3))
        rec, wall = {k: [] for k in fs}, {k: [] for k in fs}
        for k, f in fs.items():        # (one form after the other: an upload frees and allocates the set tables, whose size differs)
            for _ in range(a.reps + 1):
                t0 = time.perf_counter(); pipe.upload_footsteps(f, f); wall[k].append(1e3 * (time.perf_counter() - t0))
                rec[k].append(pipe.info()["plan_record_ms"])
                assert pipe.info()["plan_timed"] is (k == "timed")
        info = pipe.info()
        out.update(ticks=T, stages=T + 51, steps=int(kw["n_steps"]), set_slots_per_robot={"untimed": 1 + 2 * ((T + 1) // (int(fs["untimed"]["ss_ticks"]) + 1) + 1),
                                                                                         "timed": 1 + 2 * ((T + 1) // 2 + 1)}, plan_timed=info["plan_timed"], record_pass_ms={k: _stats(v[1:]) for k, v in rec.items()},
                   upload_wall_ms={k: _stats(v[1:]) for k, v in wall.items()}, first_call_wall_ms={k: v[0] for k, v in wall.items()},
                   timed_over_untimed_record_pass=float(np.median(rec["timed"][1:]) / np.median(rec["untimed"][1:])))
    else:
        K, D = a.max_steps, a.step_ticks
        L = wca.capi.lib()
        L.hipMalloc.argtypes, L.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p]
        L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        L.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
        L.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        L.hipEventSynchronize.argtypes = [C.c_void_p]
        L.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        g = S.synth_goal_batch(B, cases=False)
        pl = wca.UnicyclePlanner(step_ticks=D, max_steps=K, max_linear_velocity=0.03, max_angular_velocity=0.15, min_step_length=0.005, min_angle_variation=0.01)
        timing = dict(min_step_ticks=max(2, (8 * D) // 10), nominal_step_ticks=max(2, (9 * D) // 10), max_step_ticks=D)
        host = {k: np.ascontiguousarray(g[k]) for k in ("left0", "right0", "goals", "first_side")}
        host.update(n_steps=np.zeros(B, np.int32), side=np.zeros((B, K), np.uint8), target=np.zeros((B, K, 3)), status=np.zeros(B, np.int32),
                    desired_point=np.zeros((B, 2)), unicycle_end=np.zeros((B, 3)), ss_ticks=np.zeros((B, K), np.int32), ds_ticks=np.zeros((B, K), np.int32))
        ptr = {}
        for k, v in host.items():
            ptr[k] = C.c_void_p()
            assert L.hipMalloc(C.byref(ptr[k]), max(v.nbytes, 8)) == 0 and L.hipMemcpy(ptr[k], v.ctypes.data, v.nbytes, 1) == 0
        e0, e1 = C.c_void_p(), C.c_void_p()
        assert L.hipEventCreate(C.byref(e0)) == 0 and L.hipEventCreate(C.byref(e1)) == 0
        ms, res = {"untimed": [], "timed": []}, {}
        args = [ptr[k].value for k in ("left0", "right0", "goals", "first_side", "n_steps", "side", "target", "status", "desired_point", "unicycle_end")]
        for _ in range(a.reps + 1):
            for form in ms:
                extra = {} if form == "untimed" else dict(timing=timing, ss_ticks=ptr["ss_ticks"].value, ds_ticks=ptr["ds_ticks"].value)
                assert L.hipEventRecord(e0, None) == 0
                pl.plan_device(B, *args, **extra)
                assert L.hipEventRecord(e1, None) == 0 and L.hipEventSynchronize(e1) == 0
                t = C.c_float()
                assert L.hipEventElapsedTime(C.byref(t), e0, e1) == 0
                ms[form].append(t.value)
                for k in ("n_steps", "status", "ss_ticks", "ds_ticks"):
                    assert L.hipMemcpy(host[k].ctypes.data, ptr[k], host[k].nbytes, 2) == 0
                res[form] = dict(status_counts=np.bincount(host["status"], minlength=4).tolist(), mean_steps=float(host["n_steps"].mean()))
                if form == "timed":
                    m = (host["ss_ticks"] + host["ds_ticks"])
                    res[form]["step_ticks_counts"] = {str(int(v)): int(c) for v, c in zip(*np.unique(m[m > 0], return_counts=True))}
        for v in ptr.values():
            L.hipFree(v)
        out.update(max_steps=K, step_ticks=D, timing=pl.timing_values(timing), plan_device_ms={k: _stats(v[1:]) for k, v in ms.items()},
                   first_call_ms={k: v[0] for k, v in ms.items()}, plans=res,
                   timed_over_untimed=float(np.median(ms["timed"][1:]) / np.median(ms["untimed"][1:])))
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--ticks", type=int, default=1200)
    ap.add_argument("--max-steps", type=int, default=20)
    ap.add_argument("--step-ticks", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=170, help="seconds per step")
    ap.add_argument("--step", choices=STEPS, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.step:
        step(a)
        return
    out = {}
    args = ["--batch", a.batch, "--ticks", a.ticks, "--max-steps", a.max_steps, "--step-ticks", a.step_ticks, "--reps", a.reps]
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
