#!/usr/bin/env python3
"""Cost of replanning a generated walk (wcqp_tick_replan_footsteps) at `--batch` robots x T stages, one handle, one session:

  (a) a replan of every robot at stage `--merge`,
  (b) a replan of one robot in sixteen at that stage,
  (c) wcqp_tick_upload_footsteps of the same handle,
the three forms alternating, medians of `--reps`.  Host wall clock around each call and the device synchronisation behind it (the replan
only enqueues; the upload synchronises itself).  (a) is to be held against (c) times the share of stages regenerated plus the spread of (c);
(b) against (a) / 16.

    python tools/footstep_replan_timing.py [--batch 8192] [--ticks 1200] [--merge 600] [--out profiles/footstep_replan_timing.json]

This process never opens the GPU: the step is a child process (`--step replan`) under `timeout -k 10 LIMIT`, which ends a step that hangs
inside a device call; the result then says that it failed."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def step(a):
    import torch  # the GPU runtime first, then libwcqp
    import walking_controllers_amd as wca
    import footstep_plan_timing as fpt
    B, T = a.batch, a.ticks
    fs = fpt._footsteps(wca, B, T)
    per = int(fs["ss_ticks"]) + int(fs["ds_ticks"])
    k = (a.merge - int(fs["first_ds_ticks"]) - int(fs["ss_ticks"])) // per + 1       # the double support the merge stage lies in
    rp = wca.synth.synth_footstep_replan_batch(fs, after_step=k, ds_offset=0)
    off = a.merge - int(rp["merge_stage"][0])
    assert 0 <= off < int(fs["ds_ticks"]) - 1, "--merge does not lie in a double support of the walk"
    rp = wca.synth.synth_footstep_replan_batch(fs, after_step=k, ds_offset=off)
    every = rp["merge_stage"].copy()
    some = np.where(np.arange(B) % 16 == 0, every, -1).astype(np.int32)
    pipe = fpt._pipe(wca, B, T)
    res = {"replan_all": [], "replan_one_in_16": [], "upload_footsteps": []}
    for rep in range(a.reps + 1):
        for name, M in (("upload_footsteps", None), ("replan_all", every), ("upload_footsteps", None), ("replan_one_in_16", some)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if M is None:
                pipe.upload_footsteps(fs, fs)
            else:
                pipe.replan_footsteps(M, rp, rp["first_ds_ticks"])
            torch.cuda.synchronize()
            if rep > 0:                 # (the first round: first touch of the pages, code load, the handle's block)
                res[name].append(1e3 * (time.perf_counter() - t0))
    stat = {k_: {"median": float(np.median(v)), "min": min(v), "max": max(v)} for k_, v in res.items()}
    share = (T + 51 - a.merge) / float(T + 51)
    out = dict(device=torch.cuda.get_device_name(0), source_hash=wca.capi.source_hash(), batch=B, stages=T + 51, merge_stage=a.merge,
               share_of_stages=share, ms=stat, expected_replan_all_ms=stat["upload_footsteps"]["median"] * share,
               upload_spread_ms=stat["upload_footsteps"]["max"] - stat["upload_footsteps"]["min"],
               one_in_16_over_all=stat["replan_one_in_16"]["median"] / stat["replan_all"]["median"])
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--ticks", type=int, default=1200)
    ap.add_argument("--merge", type=int, default=600)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds for the step")
    ap.add_argument("--step", choices=("replan",), default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.step:
        step(a)
        return
    args = ["--batch", a.batch, "--ticks", a.ticks, "--merge", a.merge, "--reps", a.reps]
    r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--step", "replan"] + [str(x) for x in args],
                       capture_output=True, text=True)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not lines:
        out = {"replan": {"failed": True, "exit_status": r.returncode, "stderr_tail": r.stderr[-600:]}}
    else:
        out = {"replan": json.loads(lines[-1][7:])}
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
