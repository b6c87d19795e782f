#!/usr/bin/env python3
"""What a swing profile costs the plan generator (wcqp_tick_set_swing_profile): at `--batch` robots x T stages, in one session
and alternating, `--reps` uploads each (the first of each left out: first touch, code load) of

  the zero profile      - plan_record_kernel, the kernel every upload ran before there were profiles -, and
  a profile whose four fields are all non-zero - plan_record_shaped_kernel -:

the record pass between its events (wcqp_tick_info.plan_record_ms) and the whole upload_footsteps call (host wall clock: the call
synchronises), their medians and the shaped / zero ratios.  Both passes write the same batch x T x 320 bytes.

    python tools/swing_profile_timing.py [--batch 8192] [--ticks 1200] [--out profiles/swing_profile_timing.json]

This process never opens the GPU: the measurement is a child process (`--child`) under `timeout -k 10 LIMIT`, which ends it if it hangs
inside a device call; the result then says so."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ALL_FIELDS = dict(apex_ratio=0.8, landing_velocity=-0.05, pitch_delta=0.03, com_height_delta=0.01)


def child(a):
    import torch  # the GPU runtime first, then libwcqp
    import walking_controllers_amd as wca
    import footstep_plan_timing as fpt
    B, T = a.batch, a.ticks
    fs = fpt._footsteps(wca, B, T)
    pipes = {"zero": fpt._pipe(wca, B, T), "shaped": fpt._pipe(wca, B, T)}
    pipes["shaped"].set_swing_profile(**ALL_FIELDS)
    rec, wall = {k: [] for k in pipes}, {k: [] for k in pipes}
    for _ in range(a.reps + 1):
        for k, p in pipes.items():
            t0 = time.perf_counter(); p.upload_footsteps(fs, fs); wall[k].append(1e3 * (time.perf_counter() - t0))
            rec[k].append(p.info()["plan_record_ms"])
    assert pipes["zero"].option(wca.capi.TICK_OPT_SWING_PROFILE) == 0 and pipes["shaped"].option(wca.capi.TICK_OPT_SWING_PROFILE) == 1
    stat = lambda v: {"median": float(np.median(v[1:])), "min": min(v[1:]), "max": max(v[1:]), "first": v[0]}
    nbytes = B * (T + 51) * 320
    out = {"device": torch.cuda.get_device_name(0), "source_hash": wca.capi.source_hash(), "batch": B, "stages": T + 51, "record_bytes": nbytes,
           "reps": a.reps, "profile": ALL_FIELDS,
           "record_pass_ms": {k: dict(stat(v), GBps=nbytes / np.median(v[1:]) / 1e6) for k, v in rec.items()},
           "upload_footsteps_wall_ms": {k: stat(v) for k, v in wall.items()}}
    out["record_pass_shaped_over_zero"] = out["record_pass_ms"]["shaped"]["median"] / out["record_pass_ms"]["zero"]["median"]
    out["upload_shaped_over_zero"] = out["upload_footsteps_wall_ms"]["shaped"]["median"] / out["upload_footsteps_wall_ms"]["zero"]["median"]
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--ticks", type=int, default=1200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds for the child")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", "--batch", str(a.batch),
                        "--ticks", str(a.ticks), "--reps", str(a.reps)], capture_output=True, text=True)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    out = json.loads(lines[-1][7:]) if r.returncode == 0 and lines else {"failed": True, "exit_status": r.returncode, "stderr_tail": r.stderr[-600:]}
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    sys.exit(1 if out.get("failed") else 0)


if __name__ == "__main__":
    main()
