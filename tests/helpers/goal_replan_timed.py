"""The scenarios of tests/test_goal_replan_timed*.py, restated on the host once per process (the tests share them and leave them
unchanged): timed walks (helpers/unicycle_plan_timed.py,
footstep_plan_timed.py) sent on by replan_goals(timing=) calls - the merge stage by helpers/goal_merge_timed.py on every robot's own
timeline, the first side from the fixed-frame bit of the restated plan's stage M - 1, the footsteps AND their durations by the timed
planner's restatement from the restated soles of stage M, the plan by footstep_replan_timed.  Handles, the oracle's run and the
bookkeeping of who is left out are helpers/goal_replan.py's."""
import functools

import numpy as np

from helpers import footstep_plan_timed as ft
from helpers import goal_merge_timed as gmt
from helpers import goal_replan as gr
from helpers import planned_tick as pt
from helpers import unicycle_plan_timed as ut

KEEP, AUTO, SIDE_AUTO, KEPT, TOO_LATE, MARGIN = gr.KEEP, gr.AUTO, gr.SIDE_AUTO, gr.KEPT, gr.TOO_LATE, gr.MARGIN
FIRST_DS, K_WALK, MAXT, T, FD = gr.FIRST_DS, gr.K_WALK, gr.MAXT, gr.T, gr.FD
GOALS0, GOAL1 = gr.GOALS0, gr.GOAL1
# the small robot of the timed planner's walk tests: the reference's timing scaled to it - 0.8 / 0.9 / 1.0 s there, 40 / 50 / 60 ticks here -,
# its weights and its ratio; a step may turn a foot by 0.07 rad at most, so a turning robot's steps are shorter than nominal.  The handle's
# step_ticks is not read by the timed planner
WALK = dict(step_ticks=1, max_steps=K_WALK, nominal_width=0.118, min_width=0.10, max_linear_velocity=0.03, max_angular_velocity=0.15,
            min_step_length=0.005, min_angle_variation=0.01, max_angle_variation=0.07)
WALK_TIMING = dict(min_step_ticks=40, max_step_ticks=60, nominal_step_ticks=50, time_weight=2.5, position_weight=1.0, switch_over_swing_ratio=0.7)
# the batch: a position weight at which the two terms of a candidate's score are of one size for this robot (|r - r_nom|^2 ~ 0.015^2, the
# time term ~ 0.5), so the durations chosen differ per robot and per step
BATCH_TIMING = dict(WALK_TIMING, position_weight=2000.0)
OUT = gr.OUT + ("ss_ticks", "ds_ticks")


def start(wca, B, timing):
    """B robots of the walk tests sent to GOALS0 (cycled) from standing by the timed planner, the right foot first: footsteps with their
    durations, the timed plan and the plan in force (origin, first_ds, n_steps, ss_ticks / ds_ticks [B][K])"""
    model = wca.synth.icub_like_model()
    kb = wca.synth.synth_walk_kin_batch(B)
    fs = wca.synth.synth_footstep_walk_batch(B, MAXT, pt.poses_host(model, kb), kb)
    st = fs["state0"]
    p = dict(wca.UnicyclePlanner.DEFAULTS, **WALK)
    goals0 = GOALS0[np.arange(B) % 3]
    r0 = ut.unicycle_plan_timed(p, timing, st[:, 24:36], st[:, 36:48], goals0, 1)
    fs.update(n_steps=r0["n_steps"], side=r0["side"], target=r0["target"], first_ds_ticks=FIRST_DS, ss_ticks=r0["ss_ticks"], ds_ticks=r0["ds_ticks"],
              final_ds_ticks=0, lift=0.02)
    plan0 = ft.footstep_plan_timed(fs, st, T, MAXT)
    force = dict(origin=np.zeros(B, np.int32), first_ds=np.full(B, FIRST_DS, np.int32), n_steps=r0["n_steps"].copy(),
                 ss_ticks=r0["ss_ticks"].copy(), ds_ticks=r0["ds_ticks"].copy())
    return dict(B=B, fs=fs, p=p, timing=timing, goals0=goals0, r0=r0, plan0=plan0, force0=force, model=model)


def timeline(force, i):
    """(O, fo, ss, ds) of robot i's plan in force, as helpers/goal_merge_timed.py takes it"""
    n = int(force["n_steps"][i])
    return int(force["origin"][i]), int(force["first_ds"][i]), force["ss_ticks"][i, :n].tolist(), force["ds_ticks"][i, :n].tolist()


def restate_call_timed(sc, plan, force, goals, merge, side, lead, t0, fd=FD):
    """One replan_goals(timing=) call on the plan in force: M [B] the merge stage taken (-1: none), decided [B] (KEPT / TOO_LATE / 0), fside
    [B] the first side taken, r the timed planner's rows over the batch (zero for robots without a lane, ss_ticks / ds_ticks among them,
    status as goal_result gives it, margin inf), rp / plan the footsteps and the stitched plan, force the plans in force behind the call."""
    B, p, K = sc["B"], sc["p"], sc["p"]["max_steps"]
    merge = np.full(B, AUTO) if merge is None else np.asarray(merge)
    side = np.full(B, SIDE_AUTO) if side is None else np.broadcast_to(np.asarray(side), (B,))
    M, decided, fside = np.full(B, -1, np.int32), np.zeros(B, np.int32), np.zeros(B, np.uint8)
    for i in range(B):
        if merge[i] == KEEP:
            decided[i] = KEPT
        elif merge[i] == AUTO:
            m = gmt.merge_auto(*timeline(force, i), t0, lead, T)
            if m == gmt.TOO_LATE:
                decided[i] = TOO_LATE
            else:
                M[i] = m
        else:
            assert gmt.merge_allowed(*timeline(force, i), int(merge[i]), t0, T), (i, int(merge[i]))
            M[i] = merge[i]
    sel = np.nonzero(M >= 1)[0]
    for i in sel:
        fside[i] = side[i] if side[i] != SIDE_AUTO else (0 if plan["contact"][i, M[i] - 1] & 4 else 1)
    r = dict(n_steps=np.zeros(B, np.int32), side=np.zeros((B, K), np.uint8), target=np.zeros((B, K, 3)), status=decided.copy(),
             desired_point=np.zeros((B, 2)), unicycle_end=np.zeros((B, 3)), ss_ticks=np.zeros((B, K), np.int32), ds_ticks=np.zeros((B, K), np.int32),
             margin=np.full(B, np.inf))
    if sel.size:
        got = ut.unicycle_plan_timed(p, sc["timing"], plan["left_traj"][sel, M[sel]], plan["right_traj"][sel, M[sel]], np.asarray(goals, float)[sel], fside[sel])
        for k in r:
            r[k][sel] = got[k]
    rp = dict(n_steps=r["n_steps"], side=r["side"], target=r["target"], ss_ticks=r["ss_ticks"], ds_ticks=r["ds_ticks"], first_ds_ticks=fd)
    new = ft.footstep_replan_timed(plan, sc["fs"], M, rp, T, MAXT) if sel.size else plan
    nf = {k: v.copy() for k, v in force.items()}
    nf["origin"][sel] = M[sel]; nf["first_ds"][sel] = fd
    for k in ("n_steps", "ss_ticks", "ds_ticks"):
        nf[k][sel] = r[k][sel]
    return dict(M=M, decided=decided, fside=fside, r=r, rp=rp, plan=new, force=nf, sel=sel)


@functools.lru_cache(maxsize=None)
def walk_scenario(wca):
    """three robots on WALK_TIMING; after 90 ticks robot 2 is sent on to GOAL1 with AUTO, SIDE_AUTO and a lead of 10, the others keep their
    plans (a NaN goal in a KEEP row)"""
    sc = start(wca, 3, WALK_TIMING)
    goals = np.array([[9.0, 9.0], [np.nan, 0.0], GOAL1])
    sc.update(t1=90, goals1=goals, merge1=np.array([KEEP, KEEP, AUTO], np.int32), lead1=10)
    sc["c1"] = restate_call_timed(sc, sc["plan0"], sc["force0"], goals, sc["merge1"], None, 10, 90)
    return sc


B_BATCH, T1, T2, LEAD1, LEAD2 = 70, 90, 160, 10, 20
GOAL_SEED = 5


@functools.lru_cache(maxsize=None)
def batch_scenario(wca, B=B_BATCH):
    """B robots (70: a full wave and a tail) on BATCH_TIMING, whose plans in force have durations that differ per robot and per step.  After
    90 ticks: robot i keeps its plan (i % 5 == 0), takes AUTO (1, 3, 4) or an explicit stage (2: five stages into the double support behind
    its OWN second step), with sides AUTO (i % 3 == 0), 0 or 1, towards goals drawn (seed GOAL_SEED) from a box ahead of the robot.  After
    160 ticks, a second call: every third robot from 1 keeps, the others AUTO / SIDE_AUTO with a lead of 20 towards the walk goals - by
    then origins, step counts and durations that only the first call's read-back knows."""
    sc = start(wca, B, BATCH_TIMING)
    i = np.arange(B)
    u = np.random.default_rng(GOAL_SEED).uniform(size=(B, 2))          # (row i is robot i's, whatever B)
    sc["goals1"] = np.stack([0.01 + 0.05 * u[:, 0], -0.03 + 0.06 * u[:, 1]], axis=1)
    f0 = sc["force0"]
    explicit = np.array([FIRST_DS + int(f0["ss_ticks"][j, 0] + f0["ds_ticks"][j, 0] + f0["ss_ticks"][j, 1]) + 5 if f0["n_steps"][j] >= 2 else 100 for j in i])
    sc["merge1"] = np.where(i % 5 == 0, KEEP, np.where(i % 5 == 2, explicit, AUTO)).astype(np.int32)
    sc["side1"] = np.where(i % 3 == 0, SIDE_AUTO, i % 2).astype(np.uint8)
    sc["goals1"][sc["merge1"] == KEEP] = np.nan
    sc["c1"] = restate_call_timed(sc, sc["plan0"], sc["force0"], sc["goals1"], sc["merge1"], sc["side1"], LEAD1, T1)
    sc["goals2"] = np.concatenate([GOALS0, [GOAL1]])[(i + 1) % 4].copy()
    sc["merge2"] = np.where(i % 3 == 1, KEEP, AUTO).astype(np.int32)
    sc["c2"] = restate_call_timed(sc, sc["c1"]["plan"], sc["c1"]["force"], sc["goals2"], sc["merge2"], None, LEAD2, T2)
    return sc


ORACLE_ROWS = np.arange(4)        # of the batch - KEEP then AUTO; AUTO then KEEP; the explicit stage then AUTO; AUTO twice


@functools.lru_cache(maxsize=None)
def oracle_runs(wca, qs):
    """oracle/tick_spec.py over the restated stitched plans, computed once per process and handed out unchanged: (the walk scenario's three
    robots, robots 0 to 3 of the batch scenario - the restatement's 400 ticks take a second per robot)"""
    w, b = walk_scenario(wca), batch_scenario(wca)
    return gr.oracle_run(wca, qs, w, w["c1"]["plan"]), gr.oracle_run(wca, qs, b, b["c2"]["plan"], ORACLE_ROWS)


def single_support_probe(force, i, nominal, ratio, t_min):
    """For the plan in force of robot i: (x, y) with x >= t_min a stage inside a single support of its own timeline that the timeline of
    `nominal`-tick steps (split by `ratio`) has in a double support, and y the first stage of the double support that follows x."""
    O, fo, ss, ds = timeline(force, i)
    s = gmt.step_starts(O, fo, ss, ds)
    nss, nds = ut.durations(nominal, ratio)
    for k in range(len(ss)):
        for x in range(max(s[k], t_min), s[k] + ss[k]):
            if not gmt.in_single_support(O, fo, [nss] * len(ss), [nds] * len(ss), x):
                return x, s[k] + ss[k]
    raise AssertionError("the two timelines agree on every single support of robot %d" % i)
