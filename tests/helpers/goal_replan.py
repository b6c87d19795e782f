"""The scenarios of tests/test_goal_replan*.py, restated on the host: walks sent to goals (helpers/unicycle_plan.py, footstep_plan.py),
then sent on by replan_goals calls - the merge stage by helpers/goal_merge.py, the first side from the fixed-frame bit of the restated
plan's stage M - 1, the footsteps by the planner's restatement from the restated soles of stage M, the plan by footstep_replan.py."""
import numpy as np

import robots
from helpers import footstep_plan as fp
from helpers import footstep_replan as fr
from helpers import goal_merge as gm
from helpers import planned_tick as pt
from helpers import streamed_tick as stt
from helpers import unicycle_plan as up
from helpers import zmp_gains as zg

KEEP, AUTO, SIDE_AUTO, KEPT, TOO_LATE = -1, -2, 255, -1, -2
MARGIN = 1e-9           # a robot the restatement decided by less may be decided otherwise by the device: it is left out of a comparison
# the walk of tests/test_unicycle_planner.py: steps of 30 + 20 stages behind 20, K = 6, 400 ticks
FIRST_DS, SS, DS, K_WALK, MAXT = 20, 30, 20, 6, 400
T = MAXT + 51
WALK = dict(step_ticks=SS + DS, max_steps=K_WALK, nominal_width=0.118, min_width=0.10, max_linear_velocity=0.03, max_angular_velocity=0.15,
            min_step_length=0.005, min_angle_variation=0.01)
GOALS0 = np.array([[0.04, 0.0], [0.03, 0.03], [0.05, -0.01]])      # straight, a turn, and the robot that is replanned
GOAL1, FD = (0.02, 0.02), 15
K_DCM = 1.0
KEYS = ("u0_log", "dq_log", "q_des", "dcm", "com")
OUT = ("n_steps", "side", "target", "status", "desired_point", "unicycle_end")
ROBOT = "iCubGazeboV2_5"


def start(wca, B):
    """B robots of the walk tests sent to GOALS0 (cycled) from standing, the right foot first: footsteps, plan and the plan in force"""
    model = wca.synth.icub_like_model()
    kb = wca.synth.synth_walk_kin_batch(B)
    fs = wca.synth.synth_footstep_walk_batch(B, MAXT, pt.poses_host(model, kb), kb)
    st = fs["state0"]
    p = dict(wca.UnicyclePlanner.DEFAULTS, **WALK)
    goals0 = GOALS0[np.arange(B) % 3]
    r0 = up.unicycle_plan(p, st[:, 24:36], st[:, 36:48], goals0, 1)
    fs.update(n_steps=r0["n_steps"], side=r0["side"], target=r0["target"], first_ds_ticks=FIRST_DS, ss_ticks=SS, ds_ticks=DS, final_ds_ticks=0, lift=0.02)
    plan0 = fp.footstep_plan(fs, st, T, MAXT)
    force = dict(origin=np.zeros(B, np.int32), first_ds=np.full(B, FIRST_DS, np.int32), n_steps=r0["n_steps"].copy())
    return dict(B=B, fs=fs, p=p, goals0=goals0, r0=r0, plan0=plan0, force0=force, model=model)


def restate_call(sc, plan, force, goals, merge, side, lead, t0, fd=FD):
    """One replan_goals call on the plan in force: M [B] the merge stage taken (-1: none), decided [B] (KEPT / TOO_LATE / 0), fside [B] the
    first side taken, r the planner's rows over the batch (zero for robots without a lane, status as goal_result gives it, margin inf),
    rp / plan the footsteps and the stitched plan, force the plans in force behind the call."""
    B, p, K = sc["B"], sc["p"], sc["p"]["max_steps"]
    merge = np.full(B, AUTO) if merge is None else np.asarray(merge)
    side = np.full(B, SIDE_AUTO) if side is None else np.broadcast_to(np.asarray(side), (B,))
    M, decided, fside = np.full(B, -1, np.int32), np.zeros(B, np.int32), np.zeros(B, np.uint8)
    for i in range(B):
        if merge[i] == KEEP:
            decided[i] = KEPT
        elif merge[i] == AUTO:
            m = gm.merge_auto(int(force["origin"][i]), int(force["first_ds"][i]), int(force["n_steps"][i]), SS, DS, t0, lead, T)
            if m == gm.TOO_LATE:
                decided[i] = TOO_LATE
            else:
                M[i] = m
        else:
            assert gm.merge_allowed(int(force["origin"][i]), int(force["first_ds"][i]), int(force["n_steps"][i]), SS, DS, int(merge[i]), t0, T)
            M[i] = merge[i]
    sel = np.nonzero(M >= 1)[0]
    for i in sel:
        fside[i] = side[i] if side[i] != SIDE_AUTO else (0 if plan["contact"][i, M[i] - 1] & 4 else 1)
    r = dict(n_steps=np.zeros(B, np.int32), side=np.zeros((B, K), np.uint8), target=np.zeros((B, K, 3)), status=decided.copy(),
             desired_point=np.zeros((B, 2)), unicycle_end=np.zeros((B, 3)), margin=np.full(B, np.inf))
    if sel.size:
        got = up.unicycle_plan(p, plan["left_traj"][sel, M[sel]], plan["right_traj"][sel, M[sel]], np.asarray(goals, float)[sel], fside[sel])
        for k in r:
            r[k][sel] = got[k]
    rp = dict(n_steps=r["n_steps"], side=r["side"], target=r["target"], first_ds_ticks=fd)
    new = fr.footstep_replan(plan, sc["fs"], M, rp, T, MAXT) if sel.size else plan
    nf = {k: v.copy() for k, v in force.items()}
    nf["origin"][sel] = M[sel]; nf["first_ds"][sel] = fd; nf["n_steps"][sel] = r["n_steps"][sel]
    return dict(M=M, decided=decided, fside=fside, r=r, rp=rp, plan=new, force=nf, sel=sel)


def walk_scenario(wca):
    """three robots; after 90 ticks robot 2 is sent on to GOAL1 with AUTO, SIDE_AUTO and a lead of 10, the others keep their plans (a NaN
    goal in a KEEP row)"""
    sc = start(wca, 3)
    goals = np.array([[9.0, 9.0], [np.nan, 0.0], GOAL1])
    sc.update(t1=90, goals1=goals, merge1=np.array([KEEP, KEEP, AUTO], np.int32), lead1=10)
    sc["c1"] = restate_call(sc, sc["plan0"], sc["force0"], goals, sc["merge1"], None, 10, 90)
    return sc


B_BATCH, T1, T2, LEAD1, LEAD2, M_EXPLICIT = 70, 90, 150, 10, 20, 105


def batch_scenario(wca, B=B_BATCH):
    """B robots (70: a full wave and a tail).  After 90 ticks: robot i keeps its plan (i % 5 == 0), takes AUTO (1, 3, 4) or the explicit stage
    105 (2 - five stages into the double support behind step 2), with sides AUTO (i % 3 == 0), 0 or 1, towards the named goals of
    synth.GOAL_CASES (cycled) but "behind": a goal straight behind the robot sits on the unstable equilibrium of the unicycle's heading loop,
    where rounding decides which way it turns - the restated footsteps of such a robot move by 6e-9 when its soles move by 1e-13
    (sensitivity() below measures it), so no comparison to 1e-9 can hold for it, on whichever side.  After 150 ticks, a second call: every third robot from 1 keeps, the others AUTO / SIDE_AUTO with a lead of 20
    towards the walk goals - origins 0, 100 and 105 by then, and step counts only the first call's read-back knows."""
    sc = start(wca, B)
    i = np.arange(B)
    cases = np.array([g for name, g, _ in wca.synth.GOAL_CASES if name != "behind"])
    sc["goals1"] = cases[i % len(cases)].copy()
    sc["merge1"] = np.where(i % 5 == 0, KEEP, np.where(i % 5 == 2, M_EXPLICIT, AUTO)).astype(np.int32)
    sc["side1"] = np.where(i % 3 == 0, SIDE_AUTO, i % 2).astype(np.uint8)
    sc["goals1"][sc["merge1"] == KEEP] = np.nan
    sc["c1"] = restate_call(sc, sc["plan0"], sc["force0"], sc["goals1"], sc["merge1"], sc["side1"], LEAD1, T1)
    sc["goals2"] = np.concatenate([GOALS0, [GOAL1]])[(i + 1) % 4].copy()
    sc["merge2"] = np.where(i % 3 == 1, KEEP, AUTO).astype(np.int32)
    sc["c2"] = restate_call(sc, sc["c1"]["plan"], sc["c1"]["force"], sc["goals2"], sc["merge2"], None, LEAD2, T2)
    return sc


def sensitivity(sc, call, plan, eps=1e-13):
    """per robot of a restated call, how far its footsteps move when the soles it plans from move by eps: the restatement's own
    conditioning (inf where the step count changes)"""
    c = sc[call]
    sel, M = c["sel"], c["M"]
    goals = np.asarray(sc["goals" + call[1:]], float)[sel]
    l, r = plan["left_traj"][sel, M[sel]], plan["right_traj"][sel, M[sel]]
    a = up.unicycle_plan(sc["p"], l, r, goals, c["fside"][sel])
    b = up.unicycle_plan(sc["p"], l + eps, r - eps, goals, c["fside"][sel])
    d = np.abs(a["target"] - b["target"]).reshape(len(sel), -1).max(axis=1) if len(sel) else np.zeros(0)
    return np.where(a["n_steps"] == b["n_steps"], d, np.inf)


def left_out(sc, calls=("c1", "c2")):
    """robots the restatement decided by less than MARGIN in the first upload or in a call: they may be left out of a comparison"""
    out = sc["r0"]["margin"] < MARGIN
    for c in calls:
        if c in sc:
            out = out | (sc[c]["r"]["margin"] < MARGIN)
    return out


def rows_of(d, rows, B):
    """the rows of every per-robot array of a dict (a footstep batch, a plan)"""
    return {k: (v[rows] if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == B else v) for k, v in d.items()}


def oracle_run(wca, qs, sc, plan, rows=None):
    """oracle/tick_spec.py over `plan` (of robots `rows`, the first robots of the batch: robot i of the run is robot i of the scenario):
    reactive controller, gain scheduling, as the handles of pipe()"""
    from oracle import tick_spec as ts
    R = robots.ROBOTS[ROBOT]
    B = sc["B"]
    rows = np.arange(B) if rows is None else np.asarray(rows)
    assert np.array_equal(rows, np.arange(len(rows)))
    fs, pl, pl0 = rows_of(sc["fs"], rows, B), rows_of(plan, rows, B), rows_of(sc["plan0"], rows, B)
    ipar = robots.ik_params(qs, ROBOT, v_max=wca.synth.WALK_VMAX.copy())
    ipar.joint_reg_deg = wca.synth.WALK_POSTURE_DEG.copy()
    d = dict(fs, ref_traj=pl["ref_traj"], dcm_vel_traj=pl["dcm_vel_traj"], dcm0=pl["ref_traj"][:, 0].copy(), u_init=pl0["zmp_ref"][:, 0].copy())
    return ts.run_ticks(ts.TickParams(horizon=50, k_com=R["k_com"], k_zmp=R["k_zmp"]), d, MAXT, ipar, kin_model=sc["model"], foot_rect=wca.synth.FOOT_RECT,
                        stages=stt.stages_of(pl, MAXT), neck_additional_rotation=R["additional_rotation"], dcm_controller="reactive",
                        k_dcm=K_DCM, dcm_vel=pl["dcm_vel_traj"], zmp_gain_schedule=zg.ZMP_SCHEDULE[ROBOT])


def pipe(wca, B, **kw):
    """a reactive handle with gain scheduling that holds planned trajectories, as test_unicycle_planner.py's"""
    R = robots.ROBOTS[ROBOT]
    ik = wca.IkSolver(form=wca.IK_FORM_QPOASES, neck_weight=R["neck_weight"] * np.eye(3), joint_reg_weights=np.array(R["reg_w"], float),
                      joint_reg_gains=np.array(R["reg_k"], float), joint_reg_rad=np.deg2rad(wca.synth.WALK_POSTURE_DEG),
                      v_max=wca.synth.WALK_VMAX.copy(), k_pos_com=R["k_pos_com"], k_pos_foot=R["k_pos_foot"], k_att_foot=R["k_att_foot"],
                      k_neck=R["k_neck"])
    return wca.TickPipeline(B, MAXT, wca.MpcSolver(horizon=50), ik, log_ticks=MAXT, k_com=R["k_com"], k_zmp=R["k_zmp"],
                            kin=wca.KinModel(wca.synth.icub_like_model()), dcm_controller="reactive", k_dcm=K_DCM, zmp_gain_scheduling=True,
                            **zg.ZMP_SCHEDULE[ROBOT], planned_trajectories=True, neck_additional_rotation=np.array(R["additional_rotation"]), **kw)


def upload(wca, pipe_, sc, planner):
    fs = sc["fs"]
    return pipe_.upload_goal(fs, sc["goals0"], planner, 1, FIRST_DS, SS, DS, lift=fs["lift"], zmp_delta_left=fs["zmp_delta_left"], zmp_delta_right=fs["zmp_delta_right"])
