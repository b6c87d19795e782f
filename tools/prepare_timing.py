#!/usr/bin/env python3
"""Cost of the batched non-linear IK (wcqp_prepare_solve_device) at `--batch` robots with the targets of
synth.synth_prepare_batch, medians of `--reps`:

  (a) one solve_device call between events (all Gauss-Newton iterations in one launch), and the mean iterations per robot,
  (b) one stand-alone wcqp_kin_jacobians_device call at the same batch between events, multiplied by the mean iteration count of (a):
      the floor a loop of kinematics alone would take; and the ratio (a) / (b).

    python tools/prepare_timing.py [--batch 8192] [--out profiles/prepare_timing.json]

This process never opens the GPU: each step is a child process of its own (`--step NAME`) under `timeout -k 10 LIMIT`, which ends a step that
hangs inside a device call; after a step that fails or is ended no further step starts, and the result holds what was measured so far."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = ("solve", "kinematics")


def _timed(torch, fn, reps):
    ms = []
    for _ in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms = ms[1:]                                 # (the first: code load, first touch of the pages)
    return {"median": float(np.median(ms)), "min": min(ms), "max": max(ms)}


def step(a):
    import torch  # the GPU runtime first, then libwcqp
    import walking_controllers_amd as wca
    S = wca.synth
    out = {"device": torch.cuda.get_device_name(0), "source_hash": wca.capi.source_hash(), "batch": a.batch}
    B = a.batch
    kin = wca.KinModel(S.icub_like_model())
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    z = lambda *shape, dt=torch.float64: torch.zeros(*shape, dtype=dt, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    if a.step == "solve":
        d = S.synth_prepare_batch(B)
        sol = wca.PrepareSolver(kin, np.deg2rad(S.WALK_POSTURE_DEG))
        ins = {k: t(d[k]) for k in ("left_d", "right_d", "com_d", "Rd_neck", "q_guess")}
        q, base, state, res = z(B, 23), z(B, 12), z(B, 87), z(B, 2)
        status, iters = z(B, dt=torch.int32), z(B, dt=torch.int32)
        run = lambda: sol.solve_device(B, ins["left_d"].data_ptr(), ins["right_d"].data_ptr(), ins["com_d"].data_ptr(), ins["q_guess"].data_ptr(),
                                       q.data_ptr(), status.data_ptr(), Rd_neck=ins["Rd_neck"].data_ptr(), base=base.data_ptr(), state=state.data_ptr(),
                                       iters=iters.data_ptr(), residual=res.data_ptr(), stream=stream)
        out["solve_ms"] = _timed(torch, run, a.reps)
        it = iters.cpu().numpy()
        out.update(solved=int((status == 0).sum()), mean_iterations=float(it.mean()), max_iterations=int(it.max()),
                   us_per_robot=1e3 * out["solve_ms"]["median"] / B)
    else:
        kb = S.synth_walk_kin_batch(B)
        base, q = t(kb["base"]), t(kb["q"])
        JL, JR, JN, JC, st = z(B, 6, 29), z(B, 6, 29), z(B, 3, 29), z(B, 3, 29), z(B, 87)
        run = lambda: kin.jacobians_device(B, base.data_ptr(), q.data_ptr(), JL.data_ptr(), JR.data_ptr(), JN.data_ptr(), JC.data_ptr(), st.data_ptr(), stream)
        out["kin_jacobians_ms"] = _timed(torch, run, a.reps)
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=120, help="seconds per step")
    ap.add_argument("--step", choices=STEPS, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.step:
        step(a)
        return
    out = {}
    for name in STEPS:
        r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--step", name, "--batch", str(a.batch),
                            "--reps", str(a.reps)], capture_output=True, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            out[name] = {"failed": True, "exit_status": r.returncode, "stderr_tail": r.stderr[-600:]}
            break
        out[name] = json.loads(lines[-1][7:])
    if "solve" in out and "kinematics" in out and not out["kinematics"].get("failed"):
        floor = out["kinematics"]["kin_jacobians_ms"]["median"] * out["solve"]["mean_iterations"]
        out["kinematics_only_floor_ms"] = floor
        out["solve_over_floor"] = out["solve"]["solve_ms"]["median"] / floor
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
