#!/usr/bin/env python3
"""Cost of standing stopped robots up on the device (wcqp_tick_recover_robots) against the host composition it replaces, at
`--batch` robots x T = ticks + 51 stages and S = `--stage` ticks enqueued, medians of `--reps` after a warm-up, all in one session on one
handle.  A fraction of the fleet (every 100th robot, or all of them) is sent a first step 0.6 m ahead, so that its IK has given up by
stage S; every call lists EVERY robot as IF_STOPPED, the caller's targets are the start soles and the start CoM.  Per fraction:

  (a) the recover call: its kernels on the stream between events (behind a busy stream, so that the host's staging is not in the
      interval) and the host wall clock of the call, which is enqueue-only;
  (b) the host composition: download() + PrepareSolver.solve_host for the whole fleet (only the device knows who stopped) +
      restart_robots(ALWAYS where stopped) + a device synchronise, host wall clock from the first call to the end of the last;
  (c) wcqp_prepare_solve_device on as many rows as robots were stopped, from the same joints towards the same targets, between events:
      (a) minus (c) is what the call adds around the IK - decision and packing, the gate, the restart, the row sets, the result rows.

Each repetition starts from a fresh upload_footsteps + run(S): a recovered robot is no longer stopped.

    python tools/plan_recover_timing.py [--batch 8192] [--ticks 1200] [--stage 200] [--out profiles/recover_timing.json]

This process never opens the GPU: the measurement is a child process (`--step`) under `timeout -k 10 LIMIT`, which ends a step that hangs
inside a device call; the result then says so and holds nothing else."""
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
FRACTIONS = (("1pct", 100), ("100pct", 1))      # every k-th robot's first step is out of reach
OUT_OF_REACH = 0.6


def _stats(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def step(a):
    import torch  # the GPU runtime first, then libwcqp
    import walking_controllers_amd as wca
    import plan_restart_timing as prt
    capi = wca.capi
    out = {"device": torch.cuda.get_device_name(0), "source_hash": capi.source_hash()}
    B, T, S0 = a.batch, a.ticks, a.stage
    stream = torch.cuda.current_stream().cuda_stream
    ev = lambda: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    out.update(batch=B, stages=T + 51, stage=S0)
    base = prt._footsteps(wca, B, T)
    pipe = prt._pipe(wca, B, T)
    prep = wca.PrepareSolver(wca.KinModel(wca.synth.icub_like_model()), np.deg2rad(wca.synth.WALK_POSTURE_DEG))
    mode = np.full(B, capi.TICK_RESTART_IF_STOPPED, np.uint8)
    tg = dict(left_d=np.ascontiguousarray(base["state0"][:, 24:36]), right_d=np.ascontiguousarray(base["state0"][:, 36:48]),
              com_d=np.column_stack([base["com0"], base["state0"][:, 68]]))
    gx, gy = (torch.zeros(1 << 30, dtype=torch.uint8, device="cuda") for _ in range(2))
    for name, every in FRACTIONS:
        fs = dict(base, target=base["target"].copy())
        for i in range(0, B, every):
            sw = int(fs["side"][i, 0])
            fs["target"][i, 0, :2] = fs["state0"][i, 24 + 12 * sw:26 + 12 * sw] + np.array([OUT_OF_REACH, 0.0])

        def fresh():
            pipe.upload_footsteps(fs, fs)
            pipe.run(S0)
            torch.cuda.synchronize()
        dev, wall, comp, parts = [], [], [], []
        for _ in range(a.reps + 1):
            fresh()
            e0, e1 = ev()
            for _ in range(10):       # (several milliseconds of copies: the call's kernels are queued before the first event is reached)
                gy.copy_(gx)
            e0.record()
            t0 = time.perf_counter()
            pipe.recover_robots(mode, prep, stream=stream, **tg)
            wall.append(1e3 * (time.perf_counter() - t0))
            e1.record()
            torch.cuda.synchronize()
            dev.append(e0.elapsed_time(e1))
        res = pipe.recover_result()
        n_stopped = int((res["status"] != capi.RECOVER_NOT_STOPPED).sum())
        for _ in range(a.reps + 1):
            fresh()
            t0 = time.perf_counter()
            o = pipe.download()
            t1 = time.perf_counter()
            p = prep.solve_host(tg["left_d"], tg["right_d"], tg["com_d"], o["q_des"])
            t2 = time.perf_counter()
            go = (o["ik_fail"] > 0) & (p["status"] == 0)
            pipe.restart_robots(np.where(go, capi.TICK_RESTART_ALWAYS, capi.TICK_RESTART_KEEP).astype(np.uint8),
                                dict(state0=p["state"], q0=p["q"], com0=np.ascontiguousarray(p["state"][:, 66:68])), stream=stream)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            comp.append(1e3 * (t3 - t0)); parts.append([1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t3 - t2)])
        assert int(go.sum()) == int(res["restarted"].sum()), (int(go.sum()), int(res["restarted"].sum()), n_stopped)
        # (c) the IK alone on the stopped robots' rows, device pointers
        rows = np.nonzero(o["ik_fail"] > 0)[0]
        n = len(rows)
        dv = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
        d_in = [dv(tg[k][rows]) for k in ("left_d", "right_d", "com_d")] + [dv(o["q_des"][rows])]
        d_q, d_state, d_res = (torch.zeros(n, w, dtype=torch.float64, device="cuda") for w in (23, 87, 2))
        d_status, d_iters = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2))
        ik = []
        for _ in range(a.reps + 1):
            e0, e1 = ev()
            e0.record()
            prep.solve_device(n, d_in[0].data_ptr(), d_in[1].data_ptr(), d_in[2].data_ptr(), d_in[3].data_ptr(), d_q.data_ptr(), d_status.data_ptr(),
                              state=d_state.data_ptr(), iters=d_iters.data_ptr(), residual=d_res.data_ptr(), stream=stream)
            e1.record()
            torch.cuda.synchronize()
            ik.append(e0.elapsed_time(e1))
        assert np.array_equal(d_iters.cpu().numpy(), res["iters"][rows]) and np.array_equal(d_status.cpu().numpy(), res["status"][rows])
        pm = np.median(np.array(parts[1:]), axis=0)
        out[name] = dict(robots_listed=B, robots_stopped=n_stopped, robots_restarted=int(res["restarted"].sum()), ik_iters_max=int(res["iters"].max()), ik_iters_mean_of_stopped=float(res["iters"][rows].mean()),
                         recover_kernels_ms=_stats(dev[1:]), recover_call_wall_ms=_stats(wall[1:]), composition_wall_ms=_stats(comp[1:]),
                         composition_parts_ms=dict(download=float(pm[0]), solve_host=float(pm[1]), restart_robots_and_synchronise=float(pm[2])),
                         prepare_solve_device_ms=_stats(ik[1:]),
                         overhead_ms=float(np.median(dev[1:]) - np.median(ik[1:])),
                         recover_kernels_over_composition=float(np.median(dev[1:]) / np.median(comp[1:])))
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--ticks", type=int, default=1200)
    ap.add_argument("--stage", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=300, help="seconds for the measuring step")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.step:
        step(a)
        return
    args = ["--batch", a.batch, "--ticks", a.ticks, "--stage", a.stage, "--reps", a.reps]
    r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--step"] + [str(x) for x in args],
                       capture_output=True, text=True)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not lines:
        out = {"failed": True, "exit_status": r.returncode, "stderr_tail": r.stderr[-1200:]}
    else:
        out = json.loads(lines[-1][7:])
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    sys.exit(1 if out.get("failed") else 0)


if __name__ == "__main__":
    main()
