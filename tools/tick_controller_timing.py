#!/usr/bin/env python3
"""Time per tick of the closed-loop tick with either DCM controller (wcqp_tick_params.dcm_controller): the DCM-MPC and the reactive
controller side by side, for constant Jacobians and fused kinematics at horizon 50, and the fused reactive tick at horizon 200.

    python tools/tick_controller_timing.py [--batch 8192] [--ticks 1000] [--reps 5] [--out profiles/r05_tick_reactive_timing.json]
    python tools/tick_controller_timing.py --zmp-gain-scheduling [...]     (both controllers, constant Jacobians and fused kinematics at
        N = 50, each with ZMP gain scheduling - iCubGazeboV2_5's zmpControllerParams.ini - and without, side by side)

Per case: one pipeline of `batch` robots; every repetition re-uploads the inputs, runs `--warmup` ticks, then `--ticks` timed ticks in
ONE wcqp_tick_run call (device events around it); the median over the repetitions is reported.  The first repetition logs its first
16 ticks, and a sample of robots is replayed through the CPU restatement (oracle/tick_spec.py::run_ticks with the case's controller
and gain schedule).  Kernel statistics: run this under
`rocprofv3 --kernel-trace --stats` in a run of its own (--no-check keeps the CPU replay out of it).
    python tools/tick_controller_timing.py --planned [...]     (fused kinematics at N = 50, both controllers: planned trajectories -
        the synthetic gait written out as the planner's stages, the same work - against the synthetic gait, the two forms alternating
        within every repetition; the first 16 ticks of both forms must agree to 1e-12)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402  (the GPU runtime first, then libwcqp)
import walking_controllers_amd as wca  # noqa: E402
from helpers import planned_tick as pt  # noqa: E402
from helpers import zmp_gains as zg  # noqa: E402

GS = zg.ZMP_SCHEDULE["iCubGazeboV2_5"]       # smoothingTime 0.05, kCoM / kZMP stance 6.0 / 0.9 (walking: 9.0 / 3.0, the TickParams defaults)

K_DCM = 1.2          # iCubGazeboV2_5, app/robots/iCubGazeboV2_5/dcmReactiveControllerParams.ini:1
CHECK_TICKS = 16
CASES = [("constant_jacobians", "mpc", 50), ("constant_jacobians", "reactive", 50),
         ("fused_kinematics", "mpc", 50), ("fused_kinematics", "reactive", 50), ("fused_kinematics", "reactive", 200)]


def make_data(kin_mode, cnt, n, horizon, first, kin):
    S = wca.synth
    if kin_mode:
        kb = S.synth_walk_kin_batch(cnt, first=first)
        poses = kin.jacobians_host(kb["base"], kb["q"], state=np.zeros((cnt, 87)))["state"]
        return S.synth_walk_batch(cnt, n, poses, kb, first=first, horizon=horizon)
    return S.synth_tick_batch(cnt, n, first=first, horizon=horizon)


def check_sample(kin_mode, ctrl, horizon, B, n, logged, kin, gs=False):
    """the first CHECK_TICKS ticks of robots 0..3 and B-4..B-1 against the CPU restatement"""
    from oracle import qp_spec as qs, tick_spec as ts
    S = wca.synth
    p = ts.TickParams(horizon=horizon)
    if kin_mode:
        ipar = qs.IKParams(v_max=S.WALK_VMAX.copy(), joint_reg_deg=S.WALK_POSTURE_DEG.copy())
        kw = dict(kin_model=S.icub_like_model(), foot_rect=S.FOOT_RECT)
    else:
        ipar, kw = qs.IKParams(v_max=0.5 * np.ones(23)), {}
    eu = ed = 0.0
    fails = 0
    for f in (0, B - 4):
        one = make_data(kin_mode, 4, n, horizon, f, kin)
        ref = ts.run_ticks(p, one, CHECK_TICKS, ipar, dcm_controller=ctrl, k_dcm=K_DCM, zmp_gain_schedule=GS if gs else None, **kw)
        eu = max(eu, float(np.abs(logged["u0_log"][:, f:f + 4] - ref["u0_log"]).max()))
        ed = max(ed, float(np.abs(logged["dq_log"][:, f:f + 4] - ref["dq_log"]).max()))
        fails += int(ref["ik_fail"].sum())
    return {"ticks": CHECK_TICKS, "robots": [0, 1, 2, 3, B - 4, B - 3, B - 2, B - 1], "max_abs_err_u0": eu, "max_abs_err_dq": ed,
            "oracle_ik_fail": fails, "ok": bool(eu <= 1e-9 and ed <= 1e-8)}


def measure(kin_mode, ctrl, horizon, B, T, W, reps, check, gs=False):
    S = wca.synth
    dev = torch.device("cuda", 0)
    kin = wca.KinModel(S.icub_like_model()) if kin_mode else None
    n = T + W
    data = make_data(kin_mode, B, n, horizon, 0, kin)
    if kin_mode:
        ik = wca.IkSolver(form=wca.IK_FORM_QPOASES, v_max=S.WALK_VMAX, joint_reg_rad=np.deg2rad(S.WALK_POSTURE_DEG))
    else:
        ik = wca.IkSolver(form=wca.IK_FORM_QPOASES, v_max=0.5)
    kw = dict(dcm_controller="reactive", k_dcm=K_DCM) if ctrl == "reactive" else {}
    if gs:
        kw.update(zmp_gain_scheduling=True, **GS)
    pipe = wca.TickPipeline(B, n, wca.MpcSolver(horizon=horizon), ik, kin=kin, log_ticks=CHECK_TICKS, **kw)
    info = pipe.info()
    stream = torch.cuda.current_stream(dev)
    times, out0 = [], None
    for r in range(reps):
        pipe.upload(data)
        pipe.run(W, stream=stream.cuda_stream)
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        pipe.run(T, stream=stream.cuda_stream)
        e1.record(stream)
        torch.cuda.synchronize(dev)
        times.append(e0.elapsed_time(e1) * 1e3 / T)
        if r == 0:
            out0 = pipe.download()
    res = {"form": "fused_kinematics" if kin_mode else "constant_jacobians", "dcm_controller": ctrl, "horizon": horizon, "batch": B,
           "zmp_gain_scheduling": bool(gs), "timed_ticks": T, "warmup_ticks": W, "reps": reps, "us_per_tick_median": float(np.median(times)),
           "us_per_tick_all": [round(x, 3) for x in times], "info": info,
           "ik_fail_robots": int((out0["ik_fail"] > 0).sum()), "mpc_fail": int(out0["mpc_fail"].sum())}
    if check:
        res["oracle_check"] = check_sample(kin_mode, ctrl, horizon, B, n, out0, kin, gs)
    pipe.close()
    return res


ADD_ROT = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])      # iCubGazeboV2_5's additional_rotation (qpInverseKinematics.ini)


def measure_planned(ctrl, B, T, W, reps):
    """fused kinematics, N = 50: the synthetic gait and the same gait as planned trajectories, alternating within every repetition"""
    S = wca.synth
    dev = torch.device("cuda", 0)
    kin = wca.KinModel(S.icub_like_model())
    n = T + W
    from oracle import tick_spec as ts
    plan, data = pt.synthetic_as_planned(ts.TickParams(horizon=50), make_data(True, B, n, 50, 0, kin), n + 51, ADD_ROT)
    kw = dict(dcm_controller="reactive", k_dcm=K_DCM) if ctrl == "reactive" else {}
    pipes = {}
    for form in ("synthetic", "planned"):
        ik = wca.IkSolver(form=wca.IK_FORM_QPOASES, v_max=S.WALK_VMAX, joint_reg_rad=np.deg2rad(S.WALK_POSTURE_DEG))
        pk = dict(planned_trajectories=True, neck_additional_rotation=ADD_ROT) if form == "planned" else {}
        pipes[form] = wca.TickPipeline(B, n, wca.MpcSolver(horizon=50), ik, kin=kin, log_ticks=CHECK_TICKS, **kw, **pk)
    stream = torch.cuda.current_stream(dev)
    times = {f: [] for f in pipes}
    outs = {}
    for r in range(reps):
        for form, pipe in pipes.items():
            if form == "planned":
                pipe.upload(data, **plan)
            else:
                pipe.upload(data)
            pipe.run(W, stream=stream.cuda_stream)
            torch.cuda.synchronize(dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            pipe.run(T, stream=stream.cuda_stream)
            e1.record(stream)
            torch.cuda.synchronize(dev)
            times[form].append(e0.elapsed_time(e1) * 1e3 / T)
            if r == 0:
                outs[form] = pipe.download()
    rows = []
    for form in pipes:
        rows.append({"form": "fused_kinematics", "trajectories": form, "dcm_controller": ctrl, "horizon": 50, "batch": B, "timed_ticks": T,
                     "warmup_ticks": W, "reps": reps, "us_per_tick_median": float(np.median(times[form])),
                     "us_per_tick_all": [round(x, 3) for x in times[form]], "info": pipes[form].info(),
                     "ik_fail_robots": int((outs[form]["ik_fail"] > 0).sum()), "mpc_fail": int(outs[form]["mpc_fail"].sum())})
    rows[1]["planned_over_synthetic"] = rows[1]["us_per_tick_median"] / rows[0]["us_per_tick_median"]
    rows[1]["logged_ticks_max_abs_diff"] = {k: float(np.abs(outs["planned"][k] - outs["synthetic"][k]).max()) for k in ("u0_log", "dq_log")}
    for p_ in pipes.values():
        p_.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--ticks", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=CHECK_TICKS)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--zmp-gain-scheduling", action="store_true", help="the scheduled cases and their non-scheduled twins")
    ap.add_argument("--planned", action="store_true", help="planned trajectories against the synthetic gait (fused kinematics, N = 50)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    rows = []
    if a.planned:
        for ctrl in ("mpc", "reactive"):
            for r in measure_planned(ctrl, a.batch, a.ticks, max(a.warmup, CHECK_TICKS), a.reps):
                print(json.dumps(r), flush=True)
                rows.append(r)
        res = {"device": torch.cuda.get_device_name(0), "source_hash": wca.capi.source_hash(), "k_dcm": K_DCM, "cases": rows}
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
        return
    cases = [(f, c, h, False) for f, c, h in CASES]
    if a.zmp_gain_scheduling:
        cases = [(f, c, 50, gs) for f in ("constant_jacobians", "fused_kinematics") for c in ("mpc", "reactive") for gs in (False, True)]
    for form, ctrl, horizon, gs in cases:
        t0 = time.time()
        r = measure(form == "fused_kinematics", ctrl, horizon, a.batch, a.ticks, max(a.warmup, CHECK_TICKS), a.reps, not a.no_check, gs)
        r["wall_s"] = round(time.time() - t0, 1)
        print(json.dumps(r), flush=True)
        rows.append(r)
    res = {"device": torch.cuda.get_device_name(0), "source_hash": wca.capi.source_hash(), "k_dcm": K_DCM, "cases": rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
