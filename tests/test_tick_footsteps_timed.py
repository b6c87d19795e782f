"""Per-step timings: footsteps that carry their own durations (wcqp_tick_upload_footsteps_timed / wcqp_tick_replan_footsteps_timed,
DESIGN §8.21).  CPU: the numpy restatement (helpers/footstep_plan_timed.py) with uniform durations against the untimed restatements, the
NULL refusals.  GPU: uniform timed calls against the untimed ones bit for bit, the timed plan and replan against the restatement, the
refusals that leave the handle unchanged, and both uploads at a batch whose record pass takes a second launch."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
from walking_controllers_amd.capi import E_INVALID as WCQP_E_INVALID, E_UNSUPPORTED as WCQP_E_UNSUPPORTED

import robots
from helpers import footstep_plan as fp
from helpers import footstep_plan_timed as ft
from helpers import footstep_replan as fr
from helpers import planned_tick as pt
from helpers import zmp_gains as zg

WINDOW = (("left_traj", "left_traj"), ("right_traj", "right_traj"), ("left_twist", "left_twist"), ("right_twist", "right_twist"),
          ("com_height", "com_height_traj"), ("com_height_vel", "com_height_vel"), ("ref_traj", "ref_traj"), ("dcm_vel_traj", "dcm_vel_traj"))
TOL = 1e-9              # the bar of DESIGN §8.13 / §8.16 / §8.17 for chained device arithmetic
# 35 robots (two blocks of the DCM pass, the second with dead lanes), K = 8, T = 135 + 50 + 1 = 186 stages (no multiple of the 64-stage
# tile of the record pass nor of the 32-stage tile of the DCM pass); the uniform walk: steps of 30 + 20 stages behind 20
B35, MAXT, N_MPC, K, FIRST_DS, SS, DS = 35, 135, 50, 8, 20, 30, 20
T = MAXT + N_MPC + 1
ALL_ONES, STRADDLES, CUT_BY_T, LAST_DS = 3, 4, 5, 6        # the robots of the cases named below


def _pipe(wca, B=B35, robot="iCubGazeboV2_5", **kw):
    R = robots.ROBOTS[robot]
    ik = wca.IkSolver(form=wca.IK_FORM_QPOASES, neck_weight=R["neck_weight"] * np.eye(3), joint_reg_weights=np.array(R["reg_w"], float),
                      joint_reg_gains=np.array(R["reg_k"], float), joint_reg_rad=np.deg2rad(wca.synth.WALK_POSTURE_DEG),
                      v_max=wca.synth.WALK_VMAX.copy(), k_pos_com=R["k_pos_com"], k_pos_foot=R["k_pos_foot"], k_att_foot=R["k_att_foot"],
                      k_neck=R["k_neck"])
    kw = dict(dict(planned_trajectories=True, neck_additional_rotation=np.array(R["additional_rotation"])), **kw)
    return wca.TickPipeline(B, MAXT, wca.MpcSolver(horizon=N_MPC), ik, log_ticks=MAXT, k_com=R["k_com"], k_zmp=R["k_zmp"],
                            kin=wca.KinModel(wca.synth.icub_like_model()), dcm_controller="reactive", k_dcm=1.0, zmp_gain_scheduling=True,
                            **zg.ZMP_SCHEDULE[robot], **kw)


def _footsteps(wca, B, seed, n_of=None):
    """B robots of the walk tests with 0 .. K short steps each (robot i takes i mod (K + 1), or n_of[i]), sides alternating or a foot twice
    in a row, yaw increments of both signs; rows of steps not taken hold 1e3 (they are not read)"""
    kb = wca.synth.synth_walk_kin_batch(B)
    fs = wca.synth.synth_footstep_walk_batch(B, MAXT, pt.poses_host(wca.synth.icub_like_model(), kb), kb)
    rng = np.random.default_rng(seed)
    n_steps = (np.arange(B) % (K + 1)).astype(np.int32)
    for i, n in (n_of or {}).items():
        n_steps[i] = n
    side = ((np.arange(K)[None, :] + np.arange(B)[:, None]) % 2).astype(np.uint8)
    side[2] = (1, 1, 0, 0, 1, 1, 0, 0)
    target = np.zeros((B, K, 3))
    st = fs["state0"]
    for i in range(B):
        p = [st[i, 24:26].copy(), st[i, 36:38].copy()]
        yaw = [np.arctan2(st[i, 33], st[i, 27]), np.arctan2(st[i, 45], st[i, 39])]
        for k in range(K):
            sw = side[i, k]
            inc = rng.uniform(0.02, 0.06) * (1.0 if (i + k) % 3 else -1.0)
            yaw[sw] += inc
            p[sw] = p[sw] + rng.uniform(0.015, 0.03) * np.array([np.cos(yaw[sw]), np.sin(yaw[sw])])
            target[i, k] = (p[sw][0], p[sw][1], inc)
    target[n_steps[:, None] <= np.arange(K)[None, :]] = 1e3
    fs.update(n_steps=n_steps, side=side, target=target, first_ds_ticks=FIRST_DS, ss_ticks=SS, ds_ticks=DS, final_ds_ticks=0, lift=0.02)
    return fs


@pytest.fixture(scope="module")
def scen(wca):
    """The 35 robots: `fs` the uniform walk (the untimed calls' arguments), `tfs` the same footsteps with durations that differ per robot
    and per step - among them a robot whose every step is 1 + 1 stages, one whose single supports straddle both 64-stage tile boundaries,
    one cut off by T mid-walk, one whose last double support is longer than any other of its own - and the restated timed plan, with
    final_ds_ticks = 0 (every robot's own last ds) and 7."""
    fs = _footsteps(wca, B35, 5, {ALL_ONES: 8, STRADDLES: 3, CUT_BY_T: 8, LAST_DS: 2})
    rng = np.random.default_rng(11)
    ss = rng.integers(1, 31, size=(B35, K)).astype(np.int32)
    ds = rng.integers(1, 21, size=(B35, K)).astype(np.int32)
    n = fs["n_steps"]
    ss[ALL_ONES], ds[ALL_ONES] = 1, 1
    ss[STRADDLES, :3], ds[STRADDLES, :3] = (30, 10, 30), (10, 40, 10)      # single supports [20, 50) [60, 70) [110, 140)
    ss[CUT_BY_T], ds[CUT_BY_T] = 30, 20                                      # 20 + 8 x 50 stages > T = 186
    ss[LAST_DS, :2], ds[LAST_DS, :2] = (12, 9), (3, 19)
    ss[n[:, None] <= np.arange(K)[None, :]] = 0; ds[n[:, None] <= np.arange(K)[None, :]] = 0        # (not read: the planner's zeros)
    tfs = dict(fs, ss_ticks=ss, ds_ticks=ds)
    return fs, tfs, {f: ft.footstep_plan_timed(dict(tfs, final_ds_ticks=f), fs["state0"], T, MAXT) for f in (0, 7)}


def _merge_stages(starts, ssk, n_steps):
    """per robot a merge stage of the timed timeline and what it lies in: robot i mod 5 = 0 keeps its plan (-1), 1: the first stage of a
    double support, 2: inside one (a short one where the robot has one), 3: the last double support, 4: standing"""
    M = np.full(B35, -1, np.int32)
    kind = [""] * B35
    for i in range(B35):
        n, s = int(n_steps[i]), starts[i]
        if i % 5 == 0 or n == 0 and i % 5 != 4:
            continue
        if i % 5 == 4:
            M[i], kind[i] = s[n] + 3, "standing"
        elif i % 5 == 3:
            M[i], kind[i] = s[n - 1] + int(ssk[i, n - 1]), "last"
        else:
            k = (i // 5) % max(n - 1, 1) if n > 1 else 0
            lo, hi = s[k] + int(ssk[i, k]), s[k + 1]                 # the double support behind step k: [lo, hi)
            M[i], kind[i] = (lo, "first") if i % 5 == 1 else (lo + (hi - lo) // 2, "inside")
        if not 1 <= M[i] < T - 1:
            M[i], kind[i] = -1, ""
    return M, kind


@pytest.fixture(scope="module")
def replans(wca, scen):
    """the timed replan of the scenario's timed plan (final_ds_ticks = 0): merge stages, the new steps with their durations, the stitched plan"""
    fs, tfs, plans = scen
    plan0 = plans[0]
    M, kind = _merge_stages(plan0["starts"], tfs["ss_ticks"], tfs["n_steps"])
    n_new = np.array([(i * 3) % 5 for i in range(B35)], np.int32)
    sides = ((np.arange(4)[None, :] + np.arange(B35)[:, None] // 2) % 2).astype(np.uint8)
    rp = fr.new_steps(plan0, M, n_new, sides, 9, 23)
    rng = np.random.default_rng(12)
    rp.update(ss_ticks=rng.integers(1, 25, size=(B35, 4)).astype(np.int32), ds_ticks=rng.integers(1, 15, size=(B35, 4)).astype(np.int32))
    return M, kind, rp, ft.footstep_replan_timed(plan0, tfs, M, rp, T, MAXT)


# ---------------------------------------------------------------------------------------------------------------- CPU

def test_uniform_durations_restate_the_untimed_plan(wca, scen):
    """every ss_k = ss, ds_k = ds: footstep_plan exactly - also with a final_ds_ticks of its own - and, stitched, footstep_replan exactly"""
    fs = scen[0]
    for final in (0, 7):
        f = dict(fs, final_ds_ticks=final)
        a, b = fp.footstep_plan(f, fs["state0"], T, MAXT), ft.footstep_plan_timed(ft.uniform(f), fs["state0"], T, MAXT)
        for k in a:
            assert np.array_equal(a[k], b[k]), (k, final)
    small = fr.small_footsteps(wca, pt)
    plan0, (M1, rp1, plan1), (M2, rp2, plan2) = fr.small_replans(small)
    Ts = fr.MAXT + 51
    before = plan0
    for M, rp, plan in ((M1, rp1, plan1), (M2, rp2, plan2)):
        got = ft.footstep_replan_timed(before, small, M, ft.uniform(dict(rp, ss_ticks=fr.SS, ds_ticks=fr.DS)), Ts, fr.MAXT)
        for k in fr.PLAN_KEYS + ("change", "a"):
            assert np.array_equal(got[k], plan[k], equal_nan=True), k
        before = got


def test_scenario_covers_what_it_claims(scen, replans):
    fs, tfs, plans = scen
    ss, ds, n, s = tfs["ss_ticks"], tfs["ds_ticks"], tfs["n_steps"], plans[0]["starts"]
    assert T % 64 and T % 32 and set(n.tolist()) == set(range(K + 1))
    assert n[ALL_ONES] == 8 and (ss[ALL_ONES] == 1).all() and (ds[ALL_ONES] == 1).all() and s[ALL_ONES][8] == FIRST_DS + 16
    for edge in (64, 128):
        assert any(s[STRADDLES][k] < edge < s[STRADDLES][k] + ss[STRADDLES, k] for k in range(3)), edge
    assert s[CUT_BY_T][n[CUT_BY_T]] > T and (plans[0]["contact"][CUT_BY_T, T - 1] & 3) != 3
    assert ds[LAST_DS, 1] == 19 and plans[0]["starts"][LAST_DS][2] - plans[7]["starts"][LAST_DS][2] == 19 - 7
    taken = np.arange(K)[None, :] < n[:, None]
    assert len(np.unique(ss[taken])) > 10 and len(np.unique(ds[taken])) > 10
    M, kind, rp, plan1 = replans
    assert {"first", "inside", "last", "standing"} <= set(kind) and (M == -1).sum() >= 7 and (M >= 1).sum() >= 15
    short = [i for i in range(B35) if kind[i] == "inside"]
    assert any(min(s[i][k + 1] - s[i][k] - ss[i, k] for k in range(n[i])) <= 4 for i in short)
    for i in np.nonzero(M >= 1)[0]:
        assert (plans[0]["contact"][i, M[i]] & 3) == 3
        assert np.abs(plan1["ref_traj"][i, M[i]] - plans[0]["ref_traj"][i, M[i]]).max() <= 1e-9, i       # (the DCM reference is continuous there)


def test_synth_timed_walk_is_the_walk_with_other_durations(wca):
    """synth_timed_footstep_walk_batch: synth_footstep_walk_batch's footsteps, durations that differ per robot and per step within the
    spread, shard-invariant; with no spread the timed restatement gives the untimed plan of the walk"""
    kb = wca.synth.synth_walk_kin_batch(6)
    poses = pt.poses_host(wca.synth.icub_like_model(), kb)
    a = wca.synth.synth_footstep_walk_batch(6, 300, poses, kb)
    b = wca.synth.synth_timed_footstep_walk_batch(6, 300, poses, kb)
    for k in ("n_steps", "side", "target", "state0", "q0", "com0"):
        assert np.array_equal(a[k], b[k]), k
    ss, ds = b["ss_ticks"], b["ds_ticks"]
    assert ss.shape == ds.shape == a["side"].shape and ss.dtype == np.int32 and b["final_ds_ticks"] == a["final_ds_ticks"]
    assert (np.abs(ss - a["ss_ticks"]) <= 0.2 * a["ss_ticks"] + 0.5).all() and (np.abs(ds - a["ds_ticks"]) <= 0.2 * a["ds_ticks"] + 0.5).all()
    assert len(np.unique(ss)) > 6 and len(np.unique(ds)) > 6 and (ss >= 1).all() and (ds >= 1).all()
    kb2 = {k: v[2:5] for k, v in kb.items() if isinstance(v, np.ndarray) and v.shape[:1] == (6,)}
    part = wca.synth.synth_timed_footstep_walk_batch(3, 300, poses[2:5], dict(kb, **kb2), first=2)
    assert np.array_equal(part["ss_ticks"], ss[2:5]) and np.array_equal(part["ds_ticks"], ds[2:5]) and np.array_equal(part["target"], b["target"][2:5])
    flat = wca.synth.synth_timed_footstep_walk_batch(6, 300, poses, kb, spread=0.0)
    pa, pf = fp.footstep_plan(a, a["state0"], 351, 300), ft.footstep_plan_timed(flat, flat["state0"], 351, 300)
    for k in pa:
        assert np.array_equal(pa[k], pf[k]), k


def test_null_refusals(wca):
    """the library exports the two entry points, which refuse a NULL handle and a NULL timing"""
    lib = wca.capi.lib()
    ins, fs, rp, tm = wca.capi.TickInputs(), wca.capi.TickFootsteps(), wca.capi.TickReplan(), wca.capi.TickStepTiming()
    assert lib.wcqp_tick_upload_footsteps_timed(None, C.byref(ins), C.byref(fs), C.byref(tm)) == WCQP_E_INVALID
    assert lib.wcqp_tick_upload_footsteps_timed(None, C.byref(ins), C.byref(fs), None) == WCQP_E_INVALID
    assert lib.wcqp_tick_replan_footsteps_timed(None, C.byref(rp), C.byref(tm), None) == WCQP_E_INVALID
    pipe = object.__new__(wca.TickPipeline)
    pipe.planned, pipe.batch, pipe._h = True, 3, None
    bad = dict(n_steps=np.zeros(3, np.int32), side=np.zeros((3, 2), np.uint8), target=np.zeros((3, 2, 3)), ss_ticks=np.ones((3, 3), np.int32),
               ds_ticks=np.ones((3, 2), np.int32))
    with pytest.raises(ValueError):
        pipe.replan_footsteps(np.full(3, -1), bad, 5)


# ---------------------------------------------------------------------------------------------------------------- GPU

def _same_window(wa, wb):
    assert set(wa) == set(wb)
    for k in wb:
        assert np.array_equal(wa[k], wb[k]), k


def _window_against(wca, w, plan, rows=None):
    """a plan window against a restated plan: contact flags and hull_nc exact, the rest within TOL; the hull rows in force at every stage
    are those of the last change of contact pair at a stage <= max_ticks, built from THAT stage's feet (the set a stage names)"""
    from oracle import hull_spec as hs
    rows = range(B35) if rows is None else rows
    gap = {}
    for i in rows:
        assert np.array_equal(w["contact"][i], plan["contact"][i]), i
        for k, kr in WINDOW:
            gap[k] = max(gap.get(k, 0.0), float(np.abs(w[k][i] - plan[kr][i]).max()))
        pair = plan["contact"][i] & 3
        c, built = 0, {}
        for t in range(T):
            if 0 < t <= MAXT and pair[t] != pair[t - 1]:
                c = t
            if c not in built:
                built[c] = hs.hull_from_feet(wca.synth.FOOT_RECT, plan["left_traj"][i, c], plan["right_traj"][i, c], int(pair[c]))
            A, b, nc = built[c]
            assert w["hull_nc"][i, t] == nc, (i, t)
            gap["hull"] = max(gap.get("hull", 0.0), float(np.abs(w["hull_A"][i, t] - A).max()), float(np.abs(w["hull_b"][i, t, :nc] - b[:nc]).max()))
            assert (w["hull_b"][i, t, nc:] == 1e30).all()
    print("gap", gap)
    assert max(gap.values()) <= TOL, gap
    return gap


@pytest.fixture(scope="module")
def timed(wca, scen):
    """the scenario's timed plan on a reactive handle with gain scheduling (keeps dcm_vel): (handle, its whole plan)"""
    pipe = _pipe(wca)
    pipe.upload_footsteps(scen[1], scen[1])
    return pipe, pipe.plan_window()


@pytest.mark.gpu
def test_uniform_timed_upload_equals_the_untimed_upload(wca, scen):
    """ANCHOR, no tolerance: the timed upload with every ss_k = 30, ds_k = 20 and the untimed upload of the same footsteps - records,
    ref_traj, dcm_vel_traj, hull rows, u_init - bit for bit, with final_ds_ticks 0 and 7; the flag tells the two plans apart"""
    fs = scen[0]
    for final in (0, 7):
        f = dict(fs, final_ds_ticks=final)
        a, b = _pipe(wca), _pipe(wca)
        a.upload_footsteps(f, f)
        b.upload_footsteps(f, ft.uniform(f))
        _same_window(b.plan_window(), a.plan_window())
        assert a.info()["plan_timed"] is False and b.info()["plan_timed"] is True and b.info()["plan_generated"] is True


@pytest.mark.gpu
def test_uniform_timed_replan_equals_the_untimed_replan(wca, scen):
    """ANCHOR, no tolerance: a replan at merge stages of the uniform timeline - the first stage of a double support, inside one, the last
    one, standing, robots with -1 - with uniform durations on the timed handle, and the untimed replan of the untimed handle: bit for bit"""
    fs = scen[0]
    uni = ft.uniform(fs)
    plan0 = fp.footstep_plan(fs, fs["state0"], T, MAXT)
    starts = [ft.step_starts(FIRST_DS, uni["ss_ticks"][i], uni["ds_ticks"][i], int(fs["n_steps"][i]), 0) for i in range(B35)]
    M, kind = _merge_stages(starts, uni["ss_ticks"], fs["n_steps"])
    assert {"first", "inside", "last", "standing"} <= set(kind)
    n_new = np.array([(i * 3) % 5 for i in range(B35)], np.int32)
    sides = ((np.arange(4)[None, :] + np.arange(B35)[:, None] // 2) % 2).astype(np.uint8)
    rp = fr.new_steps(plan0, M, n_new, sides, 9, 23)
    a, b = _pipe(wca), _pipe(wca)
    a.upload_footsteps(fs, fs)
    b.upload_footsteps(fs, uni)
    a.replan_footsteps(M, rp, 9)
    b.replan_footsteps(M, ft.uniform(dict(rp, ss_ticks=SS, ds_ticks=DS)), 9)
    wa, wb = a.plan_window(), b.plan_window()
    _same_window(wb, wa)
    assert not np.array_equal(wa["ref_traj"], plan0["ref_traj"])          # (the replan replanned)


@pytest.mark.gpu
@pytest.mark.parametrize("final", [0, 7])
def test_timed_upload_matches_the_restatement(wca, scen, timed, final):
    """contact flags (fixed frame included), hull_nc and the set a stage names exact; feet, twists, heights, ref_traj, dcm_vel_traj and
    hull rows within 1e-9 (the gap is printed) - final_ds_ticks = 0: every robot's own last ds; 7: that"""
    fs, tfs, plans = scen
    if final == 0:
        w = timed[1]
    else:
        pipe = _pipe(wca)
        pipe.upload_footsteps(fs, dict(tfs, final_ds_ticks=final))
        w = pipe.plan_window()
    assert w["contact"].shape == (B35, T)
    _window_against(wca, w, plans[final])
    assert np.abs(w["u_init"] - plans[final]["zmp_ref"][:, 0]).max() <= TOL


@pytest.mark.gpu
def test_timed_replan_matches_the_restatement(wca, scen, replans):
    """per-robot merge stages of the timed timeline - the first stage of a double support, inside a short one, the last one, standing, -1:
    stages below M_i and the robots with -1 are bit-identical to before, from M_i on the plan matches the restatement as the upload does,
    ref_traj[M_i] is continuous to 1e-9; then a second timed replan, of the plans the first one left, standing robots walking on"""
    fs, tfs, plans = scen
    M, kind, rp, plan1 = replans
    pipe = _pipe(wca)
    pipe.upload_footsteps(fs, tfs)
    w0 = pipe.plan_window()
    pipe.replan_footsteps(M, rp, rp["first_ds_ticks"])
    w1 = pipe.plan_window()
    for i in range(B35):
        m = T if M[i] < 0 else int(M[i])
        for k in w1:
            if k != "u_init":
                assert np.array_equal(w1[k][i, :m], w0[k][i, :m]), (k, i)
        if M[i] >= 1:
            assert np.abs(w1["ref_traj"][i, m] - w0["ref_traj"][i, m]).max() <= TOL, i
    assert np.array_equal(w1["u_init"], w0["u_init"])
    _window_against(wca, w1, plan1)
    # the second replan is checked against the NEW plan in force: a stage inside a new single support is refused, the handle unchanged
    s1 = {int(i): ft.step_starts(int(M[i]) + rp["first_ds_ticks"], rp["ss_ticks"][i], rp["ds_ticks"][i], int(rp["n_steps"][i]), 0) for i in np.nonzero(M >= 1)[0]}
    i = next(i for i in s1 if rp["n_steps"][i] >= 2 and s1[i][1] + 1 < MAXT)
    M2 = np.full(B35, -1, np.int32)
    rp2 = fr.new_steps(plan1, np.where(np.arange(B35) == i, s1[i][0] + int(rp["ss_ticks"][i, 0]), -1), np.full(B35, 2, np.int32),
                       np.tile(np.array([1, 0], np.uint8), (B35, 1)), 6, 24)
    rp2.update(ss_ticks=np.full((B35, 2), 5, np.int32), ds_ticks=np.full((B35, 2), 2, np.int32))
    M2[i] = s1[i][1]                                                      # the first stage of the new plan's second single support
    with pytest.raises(wca.WcqpError, match="invalid|INVALID"):
        pipe.replan_footsteps(M2, rp2, 6)
    M2[i] = s1[i][0] + int(rp["ss_ticks"][i, 0]) - 1                      # the last stage of its first
    with pytest.raises(wca.WcqpError, match="invalid|INVALID"):
        pipe.replan_footsteps(M2, rp2, 6)
    _same_window(pipe.plan_window(), w1)
    M2[i] = s1[i][0] + int(rp["ss_ticks"][i, 0])                          # the first stage of the double support behind it
    pipe.replan_footsteps(M2, rp2, 6)
    _window_against(wca, pipe.plan_window(), ft.footstep_replan_timed(plan1, tfs, M2, rp2, T, MAXT))


@pytest.mark.gpu
def test_refusals_leave_the_plan_unchanged(wca, scen, timed, replans):
    """on the host, the handle unchanged: a NULL pointer in the timing, ss = 0 or ds = 0 of a step the robot takes (of one it does not
    take: fine), a timeline past 2^30 stages, a merge stage inside a single support of the timed timeline, the untimed replan and the goal
    replan on a timed plan, the timed replan on an untimed plan"""
    fs, tfs, plans = scen
    pipe, w = timed
    M, kind, rp, _ = replans
    lib = wca.capi.lib()

    def bad_upload(**kw):
        with pytest.raises(wca.WcqpError, match="invalid|INVALID"):
            pipe.upload_footsteps(fs, dict(tfs, **kw))
    zero = np.array(tfs["ss_ticks"], copy=True); zero[ALL_ONES, 7] = 0
    bad_upload(ss_ticks=zero)
    bad_upload(ds_ticks=zero)
    huge = np.array(tfs["ds_ticks"], copy=True); huge[CUT_BY_T, 2] = 1 << 30
    bad_upload(ds_ticks=huge)
    bad_upload(final_ds_ticks=-1)
    n_steps, side, target = (np.ascontiguousarray(tfs[k]) for k in ("n_steps", "side", "target"))
    st = {k: np.ascontiguousarray(fs[k], dtype=np.float64) for k in ("state0", "q0", "com0")}
    steps = wca.capi.TickFootsteps(K, n_steps.ctypes.data, side.ctypes.data, target.ctypes.data, FIRST_DS, 0, 0, 0, 0.02, (C.c_double * 2)(0.03, -0.005),
                                   (C.c_double * 2)(0.03, 0.005))
    ins = wca.capi.TickInputs(**{k: v.ctypes.data for k, v in st.items()})
    for tm in (None, wca.capi.TickStepTiming(None, tfs["ds_ticks"].ctypes.data), wca.capi.TickStepTiming(tfs["ss_ticks"].ctypes.data, None)):
        assert lib.wcqp_tick_upload_footsteps_timed(pipe._h, C.byref(ins), C.byref(steps), None if tm is None else C.byref(tm)) == WCQP_E_INVALID
    # merge stages inside single supports of the timed timeline: the first and the last stage of one
    s = plans[0]["starts"]
    i = STRADDLES
    for stage in (s[i][1], s[i][1] + int(tfs["ss_ticks"][i, 1]) - 1):
        Mb = np.where(np.arange(B35) == i, stage, -1).astype(np.int32)
        with pytest.raises(wca.WcqpError, match="invalid|INVALID"):
            pipe.replan_footsteps(Mb, dict(rp, n_steps=np.zeros(B35, np.int32)), 9)
    zero_rp = np.array(rp["ss_ticks"], copy=True)
    j = next(j for j in np.nonzero(M >= 1)[0] if rp["n_steps"][j] >= 1)
    zero_rp[j, 0] = 0
    with pytest.raises(wca.WcqpError, match="invalid|INVALID"):
        pipe.replan_footsteps(M, dict(rp, ss_ticks=zero_rp), 9)
    rpc = wca.capi.TickReplan(M.ctypes.data, 4, rp["n_steps"].ctypes.data, rp["side"].ctypes.data, rp["target"].ctypes.data, 9)
    assert lib.wcqp_tick_replan_footsteps_timed(pipe._h, C.byref(rpc), None, None) == WCQP_E_INVALID
    # a plan is timed or not from its upload on
    with pytest.raises(wca.WcqpError, match="unsupported|UNSUPPORTED"):
        pipe.replan_footsteps(M, {k: rp[k] for k in ("n_steps", "side", "target")}, 9)
    planner = wca.UnicyclePlanner(step_ticks=SS + DS, max_steps=4, nominal_width=0.118, min_width=0.10)
    with pytest.raises(wca.WcqpError, match="unsupported|UNSUPPORTED"):
        pipe.replan_goals(np.zeros((B35, 2)), planner, 9)
    assert pipe.info()["plan_timed"] is True
    _same_window(pipe.plan_window(), w)
    plain = _pipe(wca)
    plain.upload_footsteps(fs, fs)
    w_plain = plain.plan_window()
    with pytest.raises(wca.WcqpError, match="unsupported|UNSUPPORTED"):
        plain.replan_footsteps(np.full(B35, -1, np.int32), dict(rp, ss_ticks=np.ones((B35, 4), np.int32), ds_ticks=np.ones((B35, 4), np.int32)), 9)
    _same_window(plain.plan_window(), w_plain)
    # an untimed upload makes the handle's plan untimed again
    pipe2 = _pipe(wca)
    pipe2.upload_footsteps(fs, tfs)
    pipe2.upload_footsteps(fs, fs)
    assert pipe2.info()["plan_timed"] is False
    pipe2.replan_footsteps(np.full(B35, -1, np.int32), {k: rp[k] for k in ("n_steps", "side", "target")}, 9)


# seconds for the child process below.  Measured once on an MI355X: 1.2 s for the process, 0.44 s of it between the first import's end and
# the last comparison (0.26 s to create the two handles).  Twice the process's time, and a margin for a cold start of the GPU runtime.
SECOND_SLAB_LIMIT = 30


@pytest.mark.gpu
def test_uploads_past_65535_robots_take_the_second_record_launch():
    """B = 65536, the smallest batch with a robot on the record pass's second launch (robots lie on grid.y), on the smallest handle
    (max_ticks = 1, MPC horizon 1), K = 1, n_steps alternating 0 and 1, every robot at its own offset: robots 0, 65533, 65534 and 65535 of
    the untimed and of the timed upload - whose durations differ for 65534 and 65535 - equal the restatements (flags and hull_nc exact,
    the rest within 1e-9) and, bit for bit, a handle of those four robots alone.  tests/helpers/footstep_second_slab_check.py in a
    process of its own, under a time limit."""
    r = subprocess.run(["timeout", "-k", "10", str(SECOND_SLAB_LIMIT), sys.executable,
                        os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "footstep_second_slab_check.py")], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("footstep second slab ok"), r.stdout[-3000:] + r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-2])
    print(res)
    assert res["batch"] == 65536 and max(res["untimed"].values()) <= TOL and max(res["timed"].values()) <= TOL
