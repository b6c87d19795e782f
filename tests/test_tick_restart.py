"""Stopped robots of a running fleet restarted on the device, per robot (wcqp_tick_restart_robots), on the GPU: the restarted
plan against the restatement (helpers/plan_restart.py); a restarted robot ticking bit for bit like a freshly uploaded one; robots the
oracle stops walking again; stream order; rebases around a restart and the set slots; refusals.  The small workload of
tests/test_tick_replan.py: 13 robots, three full waves and a lone robot in the fourth."""
import ctypes as C

import numpy as np
import pytest
from walking_controllers_amd.capi import (E_INVALID as WCQP_E_INVALID, E_UNSUPPORTED as WCQP_E_UNSUPPORTED, TICK_RESTART_ALWAYS as ALWAYS,
                                          TICK_RESTART_IF_STOPPED as IF_STOPPED, TICK_RESTART_KEEP as KEEP)

import robots
from helpers import footstep_plan as fp
from helpers import footstep_replan as fr
from helpers import plan_restart as prs
from helpers import planned_tick as pt
from helpers import position_tick as pk
from helpers import streamed_tick as stt
from helpers import zmp_gains as zg

ROBOT, K_DCM, N = "iCubGazeboV2_5", 1.0, 50
B13, MAXT, T = fr.B13, fr.MAXT, fr.MAXT + 51
SET = (2, 4, 5, 6, 7, 9, 12)         # a whole wave (4..7), single robots of two other waves, and robot 12, alone in its wave
KEPT = tuple(i for i in range(B13) if i not in SET)
STATE = ("q_des", "dcm", "com", "ik_fail", "mpc_fail", "hot_try", "hot_hit", "active_lower", "active_upper", "zmp_gains", "ik_iters")
LOGS = ("u0_log", "dq_log", "q_log")
FD = 12                              # the double support a restarted robot's new steps start behind
COPIED = ("left_traj", "right_traj", "left_twist", "right_twist", "contact", "com_height", "com_height_vel", "dcm_vel_traj")


def _ik(wca):
    R = robots.ROBOTS[ROBOT]
    return wca.IkSolver(form=wca.IK_FORM_QPOASES, neck_weight=R["neck_weight"] * np.eye(3), joint_reg_weights=np.array(R["reg_w"], float),
                        joint_reg_gains=np.array(R["reg_k"], float), joint_reg_rad=np.deg2rad(wca.synth.WALK_POSTURE_DEG),
                        v_max=wca.synth.WALK_VMAX.copy(), k_pos_com=R["k_pos_com"], k_pos_foot=R["k_pos_foot"], k_att_foot=R["k_att_foot"],
                        k_neck=R["k_neck"])


def _pipe(wca, maxt, controller="mpc", gs=False, tpl=0, kind="planned", B=B13):
    """kind: "planned" (the planned velocity tick), "position" (the POSITION tick), "resident" (the streamed EXTERNAL handle with a
    resident plan), "plain" (no planned trajectories)"""
    R = robots.ROBOTS[ROBOT]
    ctl = dict(dcm_controller="reactive", k_dcm=K_DCM) if controller == "reactive" else {}
    sch = dict(zmp_gain_scheduling=True, **zg.ZMP_SCHEDULE[ROBOT]) if gs else {}
    position = kind == "position"
    mode = dict(ik_mode="position", position_ik=dict(q_reg=pk.scenario()["q_reg"], max_iter=12)) if position else {}
    how = dict(external_feedback=True, streamed_trajectories=True, resident_plan=True) if kind == "resident" else \
        (dict(ticks_per_launch=tpl) if kind == "plain" else dict(planned_trajectories=True, ticks_per_launch=tpl))
    mpc = wca.MpcSolver(horizon=N, com_height=pk.H) if position else wca.MpcSolver(horizon=N)
    kin = wca.KinModel(pk.scenario()["model"] if position else wca.synth.icub_like_model())
    return wca.TickPipeline(B, maxt, mpc, _ik(wca), log_ticks=maxt, k_com=R["k_com"], k_zmp=R["k_zmp"], noise=0.0, kin=kin,
                            neck_additional_rotation=pk.ADD_ROT if position else np.array(R["additional_rotation"]), **ctl, **sch, **mode, **how)


def _classic_upload(pipe, d, w):
    e = dict(d, ref_traj=w["ref_traj"])
    pipe.upload(e, dcm_vel_traj=w.get("dcm_vel_traj"), left_traj=w["left_traj"], right_traj=w["right_traj"], left_twist=w["left_twist"],
                right_twist=w["right_twist"], contact=w["contact"], com_height_traj=w.get("com_height", w.get("com_height_traj")),
                com_height_vel=w["com_height_vel"])


def _steps(w, M, n_steps, fd, seed, lo=0.015, hi=0.03):
    """footsteps from the soles the plan (or window) `w` holds at each robot's merge stage: n_steps[i] steps of lo..hi metres along the
    swinging foot's new heading, sides alternating from the right foot, yaw increments of both signs; rows not taken hold 1e3"""
    rng = np.random.default_rng(seed)
    B, Kp = len(M), 2
    sides = np.tile(np.array([1, 0], np.uint8), (B, 1))
    target = np.full((B, Kp, 3), 1e3)
    for i in range(B):
        if M[i] < 0:
            continue
        L, Rr = w["left_traj"][i, M[i]], w["right_traj"][i, M[i]]
        p = [L[:2].copy(), Rr[:2].copy()]
        yaw = [np.arctan2(L[6], L[3]), np.arctan2(Rr[6], Rr[3])]
        for k in range(int(n_steps[i])):
            sw = int(sides[i][k])
            inc = rng.uniform(0.01, 0.03) * (1.0 if (i + k) % 2 else -1.0)
            yaw[sw] += inc
            p[sw] = p[sw] + rng.uniform(lo, hi) * np.array([np.cos(yaw[sw]), np.sin(yaw[sw])])
            target[i, k] = (p[sw][0], p[sw][1], inc)
    return dict(n_steps=np.asarray(n_steps, np.int32), side=sides, target=target, first_ds_ticks=int(fd))


def _rows(fs, roll=1):
    """the rows a restart takes: another robot's start posture, so that a restarted robot does not merely return to its own"""
    return {k: np.ascontiguousarray(np.roll(fs[k], -roll, axis=0)) for k in ("state0", "q0", "com0")}


def _mode(robots_, how=ALWAYS):
    m = np.full(B13, KEEP, np.uint8)
    m[list(robots_)] = how
    return m


def _merge(robots_, M):
    m = np.full(B13, -1, np.int32)
    m[list(robots_)] = M
    return m


def _same(a, b, rows=None, keys=STATE + LOGS):
    for k in keys:
        if k in a:
            x, y = (a[k], b[k]) if rows is None else (a[k][..., rows, :] if a[k].ndim == 3 else a[k][rows], b[k][..., rows, :] if b[k].ndim == 3 else b[k][rows])
            assert np.array_equal(x, y), k


def _same_window(wa, wb, rows=slice(None)):
    assert set(wa) == set(wb)
    for k in wb:
        assert np.array_equal(wa[k][rows], wb[k][rows]), k


@pytest.fixture(scope="module")
def small(wca):
    return fr.small_footsteps(wca, pt)


# ---------------------------------------------------------------------------------------------------------------- (1) the plan

@pytest.mark.gpu
@pytest.mark.parametrize("S", [41, 64])
def test_restarted_plan_matches_the_restatement(wca, small, S):
    """upload_footsteps, run(S), restart the set, plan_window() over all T stages, on a handle that keeps dcm_vel.  S = 41 lies mid-swing
    of the old plans and inside the first 64-stage tile; S = 64 is a tile's first stage.  Restarted robots: stages below S bit for bit what
    they were; from S on the restatement - copied and zero entries bit for bit, ref_traj to 1e-12 (the tolerance a replanned plan is held
    to), the rows of every stage those of the classic rule on the standing feet.  Kept robots, and u_init: bit for bit."""
    from oracle import hull_spec as hs
    fs = small
    pipe = _pipe(wca, MAXT, "reactive", True)
    pipe.upload_footsteps(fs, fs)
    pipe.run(S)
    w0 = pipe.plan_window()
    rows = _rows(fs)
    pipe.restart_robots(_mode(SET), rows)
    res = pipe.restart_result()
    assert res["stage"] == S and np.array_equal(res["restarted"], _mode(SET) == ALWAYS) and not res["stopped_ticks"][list(KEPT)].any()
    w1 = pipe.plan_window()
    want = prs.restart(w0, SET, S, rows["state0"], fs["zmp_delta_left"], fs["zmp_delta_right"])
    assert set(w1) == set(w0) and "dcm_vel_traj" in w1
    _same_window(w1, w0, list(KEPT))
    assert np.array_equal(w1["u_init"], w0["u_init"])
    for i in SET:
        for k in w1:
            if k != "u_init":
                assert np.array_equal(w1[k][i, :S], w0[k][i, :S]), (k, i)
        for k in COPIED:
            assert np.array_equal(w1[k][i, S:], want[k][i, S:]), (k, i)
        err = np.abs(w1["ref_traj"][i, S:] - want["ref_traj"][i, S:]).max()
        print(i, "ref_traj", err)
        assert err <= 1e-12, (i, err)
        A, b, nc = hs.hull_from_feet(wca.synth.FOOT_RECT, rows["state0"][i, 24:36], rows["state0"][i, 36:48], 3)
        assert np.all(w1["hull_nc"][i, S:] == nc)
        assert np.abs(w1["hull_A"][i, S:] - A).max() < 1e-12 and np.abs(w1["hull_b"][i, S:, :nc] - b[:nc]).max() < 1e-12, i
        for k in ("hull_A", "hull_b"):
            assert np.all(w1[k][i, S:] == w1[k][i, S]), (k, i)
    # NULL dcm0 / u_init: the robot's DCM is the standing stage's reference, bit for bit
    out = pipe.download()
    assert np.array_equal(out["dcm"][list(SET)], w1["ref_traj"][list(SET), S]) and not out["ik_fail"][list(SET)].any()


@pytest.mark.gpu
def test_restart_on_a_timed_plan_with_a_swing_profile(wca, small):
    """Per-step timings and a swing profile in force change nothing of a standing stage: the same restatement, stage 41 mid-swing of the
    shaped plan; the timed replan that follows is accepted and the handle runs on."""
    S = 41
    i, k = np.indices(small["side"].shape)
    fs = dict(small, ss_ticks=(fr.SS - 2 + (i + k) % 5).astype(np.int32), ds_ticks=(fr.DS - 2 + (3 * i + k) % 4).astype(np.int32))
    pipe = _pipe(wca, MAXT, "reactive", True)
    pipe.set_swing_profile(apex_ratio=0.4, landing_velocity=-0.02, pitch_delta=0.05, com_height_delta=0.004)
    pipe.upload_footsteps(fs, fs)
    assert pipe.info()["plan_timed"]
    pipe.run(S)
    w0 = pipe.plan_window()
    assert w0["com_height_vel"][:, :S].any() and w0["com_height_vel"][list(SET), S:].any()      # (the profile is in force)
    rows = _rows(fs)
    pipe.restart_robots(_mode(SET), rows)
    w1 = pipe.plan_window()
    want = prs.restart(w0, SET, S, rows["state0"], fs["zmp_delta_left"], fs["zmp_delta_right"])
    _same_window(w1, w0, list(KEPT))
    for r in SET:
        for key in w1:
            if key != "u_init":
                assert np.array_equal(w1[key][r, :S], w0[key][r, :S]), (key, r)
        for key in COPIED:
            assert np.array_equal(w1[key][r, S:], want[key][r, S:]), (key, r)
        assert np.abs(w1["ref_traj"][r, S:] - want["ref_traj"][r, S:]).max() <= 1e-12, r
    M = _merge(SET, S + 5)
    rp = _steps(w1, M, np.where(M >= 0, 2, 0), FD, 15)
    rp.update(ss_ticks=np.full((B13, 2), 28, np.int32), ds_ticks=np.full((B13, 2), 18, np.int32))
    pipe.replan_footsteps(M, rp, FD)
    pipe.run(MAXT - S)
    w2 = pipe.plan_window()
    assert all((w2["contact"][r, S + 5 + FD] & 3) != 3 and np.all(w2["contact"][r, S:S + 5 + FD] == 7) for r in SET)
    _same_window(w2, w0, list(KEPT))


# ---------------------------------------------------------------------------------------------------------------- (2) like a fresh robot

CFGS = {"mpc": dict(), "reactive_gs": dict(controller="reactive", gs=True), "position": dict(kind="position"), "mpc_tpl1": dict(tpl=1),
        "mpc_rows": dict(explicit=True), "reactive_gs_rows": dict(controller="reactive", gs=True, explicit=True)}


def _scenario(wca, small, cfg):
    """(footsteps, max_ticks, the two restart stages odd / even, step lengths): the small workload, or the POSITION scenario's own"""
    if CFGS[cfg].get("kind") == "position":
        return dict(pk.scenario()["fs"]), pk.T, (21, 30), (0.006, 0.012)
    return small, MAXT, (41, 64), (0.015, 0.03)


@pytest.mark.gpu
@pytest.mark.parametrize("odd", [True, False], ids=["S_odd", "S_even"])
@pytest.mark.parametrize("cfg", sorted(CFGS))
def test_a_restarted_robot_ticks_like_a_fresh_one(wca, small, cfg, odd):
    """Handle A: upload_footsteps, run(S), restart the set (NULL dcm0 / u_init; the `_rows` configurations: explicit dcm0 / u_init rows a
    few millimetres off the standing ZMP, each robot its own, NaN for the kept robots), replan the restarted robots at M = S + 5,
    run to max_ticks.  Handle B is fresh, with max_ticks - S ticks: uploaded classically with A's final window [S, T) and the restart's
    rows, run in one go.  For the restarted robots A's log rows [S:] and final state are B's rows [0:] and state bit for bit - the same
    kernels on the same records from the same state, so a difference names an array the reset missed; S odd and even: both parities of the
    hand-off record and both tick phases.  The kept robots equal a twin that never saw the calls."""
    fs, maxt, stages, (lo, hi) = _scenario(wca, small, cfg)
    S = stages[0 if odd else 1]
    assert S % 2 == (1 if odd else 0)
    kw = {k: v for k, v in CFGS[cfg].items() if k != "explicit"}
    a, twin = _pipe(wca, maxt, **kw), _pipe(wca, maxt, **kw)
    rows = _rows(fs)
    listed = np.isin(np.arange(B13), SET)[:, None]
    start = {}
    if CFGS[cfg].get("explicit"):
        zmp = np.array([prs.standing_zmp(rows["state0"][i], fs["zmp_delta_left"], fs["zmp_delta_right"]) for i in range(B13)])
        off = 1e-3 * (1.0 + np.arange(B13)[:, None] % 4)
        start = dict(dcm0=np.where(listed, zmp + off * np.array([1.0, -0.5]), np.nan), u_init=np.where(listed, zmp - off * np.array([0.5, 0.25]), np.nan))
    for p in (a, twin):
        p.upload_footsteps(fs, fs)
        p.run(S, use_graph=True)
    a.restart_robots(_mode(SET), dict(rows, **start))
    w = a.plan_window()
    if start:      # the rows took effect: the robot's DCM is dcm0, not the standing stage's reference
        now = a.download()["dcm"]
        assert np.array_equal(now[list(SET)], start["dcm0"][list(SET)]) and not np.any(now[list(SET)] == w["ref_traj"][list(SET), S])
    M = _merge(SET, S + 5)
    a.replan_footsteps(M, _steps(w, M, np.where(M >= 0, 2, 0), FD, 11, lo, hi), FD)
    for p in (a, twin):
        p.run(maxt - S, use_graph=True)
    oa, ot = a.download(), twin.download()
    _same(oa, ot, list(KEPT))
    wa = a.plan_window()
    _same_window(wa, twin.plan_window(), list(KEPT))
    b = _pipe(wca, maxt - S, **kw)
    wb = {k: np.ascontiguousarray(v[:, S:]) for k, v in wa.items() if k != "u_init"}
    at_S = np.ascontiguousarray(wa["ref_traj"][:, S])
    d = {k: np.where(listed, rows[k], fs[k]) for k in rows}
    d.update({k: np.where(listed, start[k], at_S) if start else at_S for k in ("dcm0", "u_init")})
    _classic_upload(b, d, wb)
    b.run(maxt - S, use_graph=True)
    ob = b.download()
    r = list(SET)
    for k in STATE:
        if k in oa:
            assert np.array_equal(oa[k][r], ob[k][r]), k
    seen = 0
    for k in LOGS:
        if k in oa:
            assert oa[k].shape[0] == maxt and ob[k].shape[0] == maxt - S
            assert np.array_equal(oa[k][S:, r], ob[k][:, r]), k
            seen += 1
    assert seen >= 2
    print(cfg, S, "ik_fail of the restarted robots", oa["ik_fail"][r])


# ---------------------------------------------------------------------------------------------------------------- (3) stopped robots walk again

OUT_OF_REACH, BAD = 0.6, (2, 4, 5, 6, 9, 12)      # metres ahead of the swinging foot; the robots whose first step lies there


def _unreachable(fs):
    tg = fs["target"].copy()
    for i in BAD:
        sw = int(fs["side"][i, 0])
        tg[i, 0, :2] = fs["state0"][i, 24 + 12 * sw:26 + 12 * sw] + np.array([OUT_OF_REACH, 0.0])
    return dict(fs, target=tg)


@pytest.mark.gpu
def test_stopped_robots_walk_again(wca, qs, small):
    """Six robots' first step lies 0.6 m ahead: the swing (stages 20 .. 50) asks for more than the joints' velocity bounds give, and the
    velocity IK gives up.  oracle/tick_spec.py alone says so first, on the CPU, for two of them beside two whose steps are reachable.
    restart_robots(IF_STOPPED for every robot) at S = 41 then restarts exactly the robots whose ik_fail > 0, and reports that count; the
    others are bit for bit a twin that never saw the call.  The restarted robots are replanned to reachable steps at M = 46 - inside a
    single support of the OLD plan, accepted because their plan stands now, and refused for a robot that was not restarted - and end the
    run with ik_fail == 0 and joints that moved.  On the reactive controller: under the MPC this workload's start transient (the CoM starts
    4 cm from the DCM) makes the velocity IK give up on some robots whatever their steps, in the oracle as on the device."""
    from oracle import tick_spec as ts
    S = 41
    fs = _unreachable(small)
    plan = fp.footstep_plan(fs, fs["state0"], T, MAXT)
    sel = [2, 12, 1, 3]
    sub = {k: (v[sel] if isinstance(v, np.ndarray) and v.shape[:1] == (B13,) else v) for k, v in fs.items()}
    pl = {k: v[sel] for k, v in plan.items() if isinstance(v, np.ndarray) and v.shape[:1] == (B13,)}
    R = robots.ROBOTS[ROBOT]
    ipar = robots.ik_params(qs, ROBOT, v_max=wca.synth.WALK_VMAX.copy())
    ipar.joint_reg_deg = wca.synth.WALK_POSTURE_DEG.copy()
    d = dict(sub, ref_traj=pl["ref_traj"], dcm_vel_traj=pl["dcm_vel_traj"], dcm0=pl["ref_traj"][:, 0].copy(), u_init=pl["zmp_ref"][:, 0].copy())
    ref = ts.run_ticks(ts.TickParams(horizon=N, k_com=R["k_com"], k_zmp=R["k_zmp"], noise=0.0), d, S, ipar, kin_model=wca.synth.icub_like_model(),
                       foot_rect=wca.synth.FOOT_RECT, stages=stt.stages_of(pl, S), neck_additional_rotation=R["additional_rotation"],
                       dcm_controller="reactive", k_dcm=K_DCM, dcm_vel=pl["dcm_vel_traj"])
    print("the oracle's ik_fail at tick", S, ref["ik_fail"])
    assert (ref["ik_fail"][:2] > 0).all() and (ref["ik_fail"][2:] == 0).all()

    a, twin = _pipe(wca, MAXT, "reactive"), _pipe(wca, MAXT, "reactive")
    for p in (a, twin):
        p.upload_footsteps(fs, fs)
        p.run(S)
    before = a.download()["ik_fail"]
    print("the device's", before)
    assert np.array_equal(before[sel] > 0, ref["ik_fail"] > 0)
    stopped = before > 0
    assert stopped.sum() >= 2 and (~stopped).sum() >= 2 and set(np.nonzero(stopped)[0]) <= set(BAD)
    rows = {k: np.ascontiguousarray(fs[k]) for k in ("state0", "q0", "com0")}       # (prepareRobot: back to the start posture)
    a.restart_robots(np.full(B13, IF_STOPPED, np.uint8), rows)
    # the bookkeeping, while the host is still owed the decision: stage 46 lies in the old plans' first single support
    walking = [i for i in np.nonzero(~stopped)[0] if fs["n_steps"][i] > 0]
    w = a.plan_window()
    M = _merge(np.nonzero(stopped)[0], S + 5)
    rp = _steps(w, M, np.where(M >= 0, 2, 0), FD, 12)
    lib = wca.capi.lib()

    def call(Mx):
        Mx = np.ascontiguousarray(Mx, np.int32)
        t = wca.capi.TickReplan(Mx.ctypes.data, 2, rp["n_steps"].ctypes.data, rp["side"].ctypes.data, rp["target"].ctypes.data, FD)
        return lib.wcqp_tick_replan_footsteps(a._h, C.byref(t), None)
    assert call(_merge(walking[:1], S + 5)) == WCQP_E_INVALID
    assert call(M) == 0
    res = a.restart_result()
    assert res["stage"] == S and np.array_equal(res["restarted"], stopped) and np.array_equal(res["stopped_ticks"], np.where(stopped, before, 0))
    for p in (a, twin):
        p.run(MAXT - S)
    oa, ot = a.download(), twin.download()
    keep = list(np.nonzero(~stopped)[0])
    _same(oa, ot, keep)
    _same_window(a.plan_window(), twin.plan_window(), keep)
    r = list(np.nonzero(stopped)[0])
    assert not oa["ik_fail"][r].any() and (ot["ik_fail"][r] == before[r] + MAXT - S).all()
    assert all(np.abs(oa["dq_log"][S:, i]).max() > 1e-3 for i in r) and not ot["dq_log"][S:, r].any()


# ---------------------------------------------------------------------------------------------------------------- (4) enqueue-only

@pytest.mark.gpu
def test_restart_on_a_stream_copies_its_arrays_at_the_call(wca, small):
    """run, restart_robots, replan_footsteps, run on one non-blocking stream with no host synchronisation in between, every input array
    overwritten with NaN as soon as its call returns: bit for bit the synchronous sequence."""
    fs, S = small, 41
    rows = _rows(fs)
    sync = _pipe(wca, MAXT)
    sync.upload_footsteps(fs, fs)
    sync.run(S)
    sync.restart_robots(_mode(SET), rows)
    M = _merge(SET, S + 5)
    rp = _steps(sync.plan_window(), M, np.where(M >= 0, 2, 0), FD, 13)
    sync.replan_footsteps(M, rp, FD)
    sync.run(MAXT - S)
    s = wca.capi.stream_create()
    try:
        pipe = _pipe(wca, MAXT)
        pipe.upload_footsteps(fs, fs)
        pipe.run(S, stream=s)
        mode, mine = _mode(SET), {k: v.copy() for k, v in rows.items()}
        pipe.restart_robots(mode, mine, stream=s)
        mode[:] = 9
        for v in mine.values():
            v[:] = np.nan
        Mc, rc = M.copy(), {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in rp.items()}
        pipe.replan_footsteps(Mc, rc, FD, stream=s)
        Mc[:] = 3; rc["n_steps"][:] = 1; rc["target"][:] = np.nan
        pipe.run(MAXT - S, stream=s)
        wca.capi.stream_synchronize(s)
        _same(sync.download(), pipe.download())
        _same_window(sync.plan_window(), pipe.plan_window())
    finally:
        wca.capi.stream_destroy(s)


# ---------------------------------------------------------------------------------------------------------------- (5) with rebase

LIFT = 0.008
SHORT = dict(first_ds_ticks=10, ss_ticks=24, ds_ticks=12, final_ds_ticks=0)      # at most three steps: standing from stage 118 on


def _short_footsteps(wca, n_max=3):
    """tests/test_plan_rebase.py's walk: plans that end inside max_ticks, as a rebase asks"""
    fs = dict(fr.small_footsteps(wca, pt), lift=LIFT, **SHORT)
    fs["n_steps"] = np.minimum(fs["n_steps"], n_max).astype(np.int32)
    w = dict(left_traj=fs["state0"][:, None, 24:36], right_traj=fs["state0"][:, None, 36:48])
    tg = np.full((B13, fs["side"].shape[1], 3), 1e3)
    rng = np.random.default_rng(5)
    for i in range(B13):
        p = [fs["state0"][i, 24:26].copy(), fs["state0"][i, 36:38].copy()]
        yaw = [np.arctan2(fs["state0"][i, 30], fs["state0"][i, 27]), np.arctan2(fs["state0"][i, 42], fs["state0"][i, 39])]
        for k in range(int(fs["n_steps"][i])):
            sw = int(fs["side"][i, k])
            inc = rng.uniform(0.01, 0.03) * (1.0 if (i + k) % 2 else -1.0)
            yaw[sw] += inc
            p[sw] = p[sw] + rng.uniform(0.006, 0.012) * np.array([np.cos(yaw[sw]), np.sin(yaw[sw])])
            tg[i, k] = (p[sw][0], p[sw][1], inc)
    fs["target"] = tg
    return fs


@pytest.mark.gpu
def test_restart_around_a_rebase(wca):
    """Handle A has room for the whole run; handle B, with max_ticks 135, rebases by 40 after 60 ticks, restarts the set (A at stage 60, B
    at stage 20), replans it, runs 50 ticks, rebases again - a rebase admits the restarted robots, they stand or their new plans end in
    time - and runs 60 more: the state and the log rows of every tick are A's, read at B's own indices, and B's plan is A's from its shift on."""
    fs = _short_footsteps(wca)
    rows = _rows(fs)
    a, b = _pipe(wca, 300), _pipe(wca, MAXT)
    for p in (a, b):
        p.upload_footsteps(fs, fs)
        p.run(60)
    shift = b.rebase_plan(40)
    assert shift == 40

    def same(t0, done):
        oa, ob = a.download(), b.download()
        assert ob["tick"] == oa["tick"] - shift == done - shift
        _same(oa, ob, keys=STATE)
        for k in LOGS:
            if k in oa:
                assert np.array_equal(oa[k][t0:done], ob[k][t0 - shift:done - shift]), (k, done)
        wa, wb = a.plan_window(), b.plan_window()
        for k in wb:
            if k != "u_init":
                assert np.array_equal(wb[k], wa[k][:, shift:shift + T]), (k, done)
    a.restart_robots(_mode(SET), rows)
    b.restart_robots(_mode(SET), rows)
    assert a.restart_result()["stage"] == 60 and b.restart_result()["stage"] == 20
    M = _merge(SET, 66)
    rp = _steps(a.plan_window(), M, np.where(M >= 0, 2, 0), 6, 14, 0.006, 0.012)
    a.replan_footsteps(M, rp, 6)
    b.replan_footsteps(np.where(M >= 0, M - shift, -1).astype(np.int32), rp, 6)
    for p in (a, b):
        p.run(50)
    same(60, 110)
    shift += b.rebase_plan(None)
    assert shift == 110
    # ... and a restart right behind that rebase, at B's stage 0
    a.restart_robots(_mode((4, 12)), rows)
    b.restart_robots(_mode((4, 12)), rows)
    assert b.restart_result()["stage"] == 0
    for p in (a, b):
        p.run(60)
    same(110, 170)


@pytest.mark.gpu
def test_set_slots_run_out_and_a_rebase_frees_them(wca):
    """A handle of 20 ticks gives every robot three set slots.  A robot restarted between single ticks takes one more each time: the third
    call is refused with WCQP_E_INVALID and changes nothing - plan, state, the last result -, a KEEP for that robot still passes, and after
    a rebase, which frees the slots of past stages, the restart is accepted again.  With its slots full the robot's replans are refused
    too - a goal call's steps are the device's, so the host bounds their sets - and accepted again after the rebase."""
    fs = _short_footsteps(wca, n_max=0)
    rows = _rows(fs)
    pipe = _pipe(wca, 20)
    pipe.upload_footsteps(fs, fs)
    for k in range(2):
        pipe.restart_robots(_mode((5,)), rows)
        pipe.run(1)
    w, out, res = pipe.plan_window(), pipe.download(), pipe.restart_result()
    with pytest.raises(wca.WcqpError):
        pipe.restart_robots(_mode((5,)), rows)
    with pytest.raises(wca.WcqpError):
        pipe.restart_robots(_mode((5, 7), IF_STOPPED), rows)
    _same_window(pipe.plan_window(), w)
    _same(pipe.download(), out)
    assert pipe.restart_result()["stage"] == res["stage"] == 1 and np.array_equal(pipe.restart_result()["restarted"], res["restarted"])
    # robot 5's slots are full: a replan - footsteps from goals or from a list - has no room for its sets and is refused, where it would
    # write them into robot 6's slots - also next to robot 3, never restarted, which has the room
    from helpers import goal_replan as gr
    planner = wca.UnicyclePlanner(**dict(gr.WALK, step_ticks=SHORT["ss_ticks"] + SHORT["ds_ticks"], max_steps=2))
    goals = fs["com0"] + np.array([0.3, 0.0])
    for timing_free_call in (lambda: pipe.replan_goals(goals, planner, 6, merge_stage=_merge((5,), 2)),
                             lambda: pipe.replan_goals(goals, planner, 6, merge_stage=_merge((3, 5), 2)),
                             lambda: pipe.replan_footsteps(_merge((5,), 2), _steps(w, _merge((5,), 2), np.where(np.arange(B13) == 5, 1, 0), 6, 16, 0.006, 0.012), 6)):
        with pytest.raises(wca.WcqpError):
            timing_free_call()
        _same_window(pipe.plan_window(), w)
    pipe.restart_robots(_mode((7,)), rows)
    assert pipe.rebase_plan(2) == 2
    # the rebase freed robot 5's slots: its goal call has room again, and nobody else's plan changes by it
    w_r = pipe.plan_window()
    pipe.replan_goals(goals, planner, 6, merge_stage=_merge((3, 5), 1))
    res_g = pipe.goal_result()
    assert (res_g["status"][[3, 5]] >= 0).all() and (res_g["merge_stage"][[3, 5]] == 1).all()
    _same_window(pipe.plan_window(), w_r, [i for i in range(B13) if i not in (3, 5)])
    pipe.restart_robots(_mode((5,)), rows)
    assert pipe.restart_result()["restarted"][5] and pipe.restart_result()["stage"] == 0
    pipe.run(20)
    assert not np.delete(pipe.download()["ik_fail"], 3).any()      # (robot 3 walks to its goal: its steps are the planner's, not this test's)


# ---------------------------------------------------------------------------------------------------------------- (6) refusals

@pytest.mark.gpu
def test_refusals(wca, small):
    """Every refusal that needs a device; after the refused calls the plan is what it was and the run equals a twin's.  NaN rows of KEPT
    robots are accepted: none of them is read."""
    fs = small
    rows = _rows(fs)
    lib, capi = wca.capi.lib(), wca.capi

    def call(pipe, mode, d, drop=()):
        m = np.ascontiguousarray(mode, np.uint8)
        keep = {k: np.ascontiguousarray(v, float) for k, v in d.items()}
        f = dict(mode=m.ctypes.data, **{k: v.ctypes.data for k, v in keep.items()})
        return lib.wcqp_tick_restart_robots(pipe._h, C.byref(capi.TickRestart(**{k: v for k, v in f.items() if k not in drop})), None)

    assert call(_pipe(wca, MAXT, kind="plain"), _mode(SET), rows) == WCQP_E_UNSUPPORTED            # a handle that holds no plan
    assert call(_pipe(wca, MAXT, kind="resident"), _mode(SET), rows) == WCQP_E_UNSUPPORTED         # EXTERNAL, a resident plan
    fresh = _pipe(wca, MAXT)
    assert call(fresh, _mode(SET), rows) == WCQP_E_INVALID                                       # before an upload
    assert lib.wcqp_tick_get_restart_result(fresh._h, C.byref(capi.TickRestartResult())) == WCQP_E_INVALID      # ... and before any call
    plan0 = fp.footstep_plan(fs, fs["state0"], T, MAXT)
    _classic_upload(fresh, dict(fs, dcm0=plan0["ref_traj"][:, 0].copy(), u_init=plan0["zmp_ref"][:, 0].copy()), plan0)
    assert call(fresh, _mode(SET), rows) == WCQP_E_UNSUPPORTED                                   # a plan that was not generated

    pipe, twin = _pipe(wca, MAXT), _pipe(wca, MAXT)
    for p in (pipe, twin):
        p.upload_footsteps(fs, fs)
        p.run(41)
    w_ref = twin.plan_window()

    def arr(key, idx, val):
        e = dict(rows); e[key] = np.array(rows[key], copy=True); e[key][idx] = val
        return e
    two = dict(rows, dcm0=rows["com0"].copy(), u_init=rows["com0"].copy())
    bad = [(_mode(SET), rows, ("mode",)), (_mode(SET), rows, ("state0",)), (_mode(SET), rows, ("q0",)), (_mode(SET), rows, ("com0",)),
           (_mode((3,), 3), rows, ()), (_mode((3,), 255), rows, ()),
           (_mode(SET), arr("state0", (4, 30), np.nan), ()), (_mode(SET), arr("state0", (4, 68), np.inf), ()), (_mode(SET), arr("state0", (12, 2), np.nan), ()),
           (_mode(SET), arr("q0", (12, 22), np.nan), ()), (_mode(SET), arr("com0", (2, 1), -np.inf), ()),
           (_mode(SET, IF_STOPPED), arr("q0", (9, 0), np.nan), ()),
           (_mode(SET), dict(two, dcm0=arr("com0", (6, 0), np.nan)["com0"]), ()), (_mode(SET), dict(two, u_init=arr("com0", (7, 1), np.nan)["com0"]), ())]
    for mode, d, drop in bad:
        assert call(pipe, mode, d, drop) == WCQP_E_INVALID, (mode, drop)
        _same_window(pipe.plan_window(), w_ref)
    assert lib.wcqp_tick_restart_robots(pipe._h, None, None) == WCQP_E_INVALID
    # a call that lists nobody is accepted and enqueues nothing; KEPT robots' rows may hold anything
    nan = {k: np.full_like(v, np.nan) for k, v in rows.items()}
    assert call(pipe, _mode(()), nan) == 0
    res = pipe.restart_result()
    assert res["stage"] == 41 and not res["restarted"].any()
    mixed = {k: np.where(np.isin(np.arange(B13), SET)[:, None], rows[k], np.nan) for k in rows}
    assert call(pipe, _mode(SET), mixed) == 0 and call(twin, _mode(SET), rows) == 0
    for p in (pipe, twin):
        p.run(MAXT - 41)
    _same(pipe.download(), twin.download())
    _same_window(pipe.plan_window(), twin.plan_window())
