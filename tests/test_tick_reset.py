"""Robots of a sensor-fed fleet reset on the device, per robot (wcqp_tick_reset_robots), on the GPU: a reset robot ticking
bit for bit like a freshly uploaded one - plain and sensor feedback, filters on and off, with and without a resident plan -, its plan
against the restatement, the run against oracle/tick_spec.py, IF_STOPPED and who stops, a rejected first reading, streams, rebases, set
slots and refusals.  The scenario of helpers/resident_plan.py: 13 robots, three full waves and a lone robot in the fourth."""
import ctypes as C

import numpy as np
import pytest
from walking_controllers_amd.capi import E_INVALID as WCQP_E_INVALID, E_UNSUPPORTED as WCQP_E_UNSUPPORTED

import robots
from helpers import footstep_replan as fr
from helpers import plan_restart as prs
from helpers import resident_plan as rs
from helpers import streamed_tick as stt
from helpers import tick_reset as tr
from helpers import zmp_gains as zg

B, MAXT, T = rs.B, rs.MAXT, rs.T
SET, KEPT = list(tr.ROBOTS), list(tr.KEPT)
AFTER = 70            # ticks a reset robot is compared over (the issue asks for 60 at least)
PRE = 10              # the sensor cases: the last PRE ticks below S are sensor-fed, so the filters are running when the call comes
COPIED = ("left_traj", "right_traj", "left_twist", "right_twist", "contact", "com_height", "com_height_vel", "dcm_vel_traj")


def _pipe(wca, cfg, maxt=MAXT, resident=True, filters=None, planned=False):
    controller, gs = rs.CONFIGS[cfg]
    R = robots.ROBOTS[rs.ROBOT]
    ctl = dict(dcm_controller="reactive", k_dcm=rs.K_DCM) if controller == "reactive" else {}
    sch = dict(zmp_gain_scheduling=True, **zg.ZMP_SCHEDULE[rs.ROBOT]) if gs else {}
    ik = wca.IkSolver(form=wca.IK_FORM_QPOASES, neck_weight=R["neck_weight"] * np.eye(3), joint_reg_weights=np.array(R["reg_w"], float),
                      joint_reg_gains=np.array(R["reg_k"], float), joint_reg_rad=np.deg2rad(wca.synth.WALK_POSTURE_DEG),
                      v_max=wca.synth.WALK_VMAX.copy(), k_pos_com=R["k_pos_com"], k_pos_foot=R["k_pos_foot"], k_att_foot=R["k_att_foot"],
                      k_neck=R["k_neck"])
    how = dict(planned_trajectories=True, noise=0.0) if planned else \
        dict(external_feedback=True, streamed_trajectories=True, resident_plan=resident, sensor_filters=filters)
    return wca.TickPipeline(B, maxt, wca.MpcSolver(horizon=50), ik, log_ticks=maxt, k_com=R["k_com"], k_zmp=R["k_zmp"],
                            kin=wca.KinModel(wca.synth.icub_like_model()), neck_additional_rotation=np.array(R["additional_rotation"]), **ctl, **sch, **how)


def _stage(stages, t):
    return tuple(stages[k][t] for k in ("left_pose", "right_pose", "left_twist", "right_twist", "contact", "com_height", "com_height_vel"))


def P(*a):
    """a tick's feedback in the plain form: dcm, com, zmp, q"""
    return ("plain", tuple(a))


def Sn(*a):
    """... in the sensor form: q, dq, wrench_left, wrench_right"""
    return ("sensor", tuple(a))


def _rowp(ext, t):
    return P(*(ext[k][t] for k in ("dcm", "com", "zmp", "q")))


def _give(pipe, fb):
    kind, args = fb
    (pipe.set_sensor_feedback_host if kind == "sensor" else pipe.set_feedback_host)(*args)


def _tick(pipe, fb, stage=None):
    """one tick in the order of the header: the stage (out of the plan, or handed over), the feedback (P or Sn), the tick"""
    if stage is None:
        pipe.set_desired_from_plan()
    else:
        pipe.set_desired_host(*stage)
    _give(pipe, fb)
    pipe.run(1)


class Feed:
    """What a handle is fed: below S resident_plan.disturbed's feed (the sensor cases: the last PRE ticks below S a seeded sensor feed),
    from S on fixed arrays - the reset robots' are what the restatement's robot in the loop recorded from the reset rows
    (helpers/tick_reset.restated: its readings in the sensor form, what it evaluated from them in the plain form), so a reset robot is fed
    a robot that stands where it was put back; the kept robots' are a seeded sensor feed or, in the plain form, still disturbed's."""

    def __init__(self, wca, qs, cfg, S, form, n_after=AFTER):
        fs = rs.scenario(wca)[0]
        self.S, self.form = S, form
        self.ext = rs.disturbed(wca, qs, cfg)[0]
        self.pre = tr.sensor_feed(fs, PRE, seed=8)
        run = tr.restated(wca, qs, cfg, S) if S > 0 else None          # (S = 0: seeded feeds alone)
        if form == "sensor":
            self.post = [tuple(np.array(x, copy=True) for x in r) for r in tr.sensor_feed(fs, n_after)]
            for k in range(n_after if run else 0):
                for x, y in zip(self.post[k], run["readings"][k]):
                    x[SET] = y
        else:
            p = tr.plain_feed(fs, n_after)
            on = np.isin(np.arange(B), SET)[None, :, None]
            self.post = {k: np.where(on, p[k], self.ext[k][S:S + n_after]) for k in p}
            for k, v in (stt.external_of_sensors(run) if run else {}).items():
                self.post[k][:, SET] = v[:n_after]

    def below(self, t):
        if self.form == "sensor" and t >= self.S - PRE:
            return Sn(*self.pre[t - (self.S - PRE)])
        return _rowp(self.ext, t)

    def after(self, k):
        return Sn(*self.post[k]) if self.form == "sensor" else _rowp(self.post, k)

    def at(self, t):
        return self.below(t) if t < self.S else self.after(t - self.S)


def _same_rows(a, b, rows, keys=tr.STATE + tr.LOGS, a0=0, b0=0, n=None):
    for k in keys:
        if k.endswith("_log"):
            x, y = a[k][a0:(None if n is None else a0 + n), rows], b[k][b0:(None if n is None else b0 + n), rows]
        else:
            x, y = a[k][rows], b[k][rows]
        assert np.array_equal(x, y), k


def _same_window(wa, wb, rows=slice(None), upto=None):
    assert set(wa) == set(wb)
    for k in wb:
        if k == "u_init":
            assert np.array_equal(wa[k][rows], wb[k][rows]), k
        else:
            assert np.array_equal(wa[k][rows, :upto], wb[k][rows, :upto]), k


def _twin_check(wca, qs, cfg, S, form, explicit, filters=None):
    """THE COMPARISON: H walks 0 .. S - 1, is reset, walks on; H0 is H without the call; H2 is fresh, classically uploaded with H's window
    [S, T) and the reset's rows, fed H's feed from its tick 0"""
    fs = rs.scenario(wca)[0]
    feed = Feed(wca, qs, cfg, S, form)
    h, h0 = _pipe(wca, cfg, filters=filters), _pipe(wca, cfg, filters=filters)
    for p in (h, h0):
        p.upload_footsteps(fs, fs)
        for t in range(S):
            _tick(p, feed.at(t))
    w_before = h.plan_window()
    h.reset_robots(tr.mode(), tr.rows(fs, explicit))
    res = h.restart_result()
    # (stopped_ticks: the robot's ik_fail just before - the seeded sensor feed below S stops a walking robot now and then)
    assert res["stage"] == S and np.array_equal(res["restarted"], tr.mode() == tr.ALWAYS)
    assert np.array_equal(res["stopped_ticks"], np.where(res["restarted"], h0.download()["ik_fail"], 0))
    with pytest.raises(wca.WcqpError, match=r"\(-1\)"):
        h.recover_result()                                    # (as after a plain restart)
    w_after = h.plan_window()
    start = tr.start_rows(fs, explicit)
    now = h.download()
    assert np.array_equal(now["measured"][SET], np.concatenate([start["dcm0"], fs["com0"], start["u_init"]], 1)[SET])      # (where a rejected reading finds them)
    assert np.array_equal(now["measured"][KEPT], h0.download()["measured"][KEPT]) and now["tick"] == S
    for p in (h, h0):
        for t in range(S, S + AFTER):
            _tick(p, feed.at(t))
    oh, o0 = h.download(), h0.download()
    # the nine other robots, and every window below S: the run without the call
    _same_rows(oh, o0, KEPT)
    _same_window(h.plan_window(), h0.plan_window(), KEPT)
    _same_window(w_after, w_before, SET, upto=S)
    # the fresh twin
    h2 = _pipe(wca, cfg, maxt=MAXT - S, filters=filters)
    d, wb = tr.twin_upload(w_after, S, fs, explicit)
    h2.upload(dict(d, ref_traj=wb["ref_traj"]), dcm_vel_traj=wb.get("dcm_vel_traj"), left_traj=wb["left_traj"], right_traj=wb["right_traj"],
              left_twist=wb["left_twist"], right_twist=wb["right_twist"], contact=wb["contact"], com_height_traj=wb["com_height"],
              com_height_vel=wb["com_height_vel"])
    for k in range(AFTER):
        _tick(h2, feed.after(k))
    o2 = h2.download()
    _same_rows(oh, o2, SET, a0=S, b0=0, n=AFTER)
    assert not oh["ik_fail"][SET].any() and not oh["feedback_fail"][SET].any() and np.abs(oh["dq_log"][S:S + AFTER, SET]).max() > 1e-4
    return oh, o2


# ---------------------------------------------------------------------------------------------------------------- (1) like a fresh robot

@pytest.mark.gpu
@pytest.mark.parametrize("explicit", [False, True], ids=["null_rows", "explicit_rows"])
@pytest.mark.parametrize("form", ["plain", "sensor"])
@pytest.mark.parametrize("S", tr.STAGES)
@pytest.mark.parametrize("cfg", list(rs.CONFIGS))
def test_a_reset_robot_ticks_like_a_fresh_one(wca, qs, cfg, S, form, explicit):
    """For robots 0, 3, 5, 12 the log rows S + k of H equal rows k of the fresh twin bit for bit over AFTER ticks, and so do q_des,
    measured, ik_fail, mpc_fail and feedback_fail; the nine others and every plan window below S are a run of H without the call.  S odd
    and even: both parities of the hand-off record.  A difference names an array the reset missed."""
    _twin_check(wca, qs, cfg, S, form, explicit)


# ---------------------------------------------------------------------------------------------------------------- (2) the plan

@pytest.mark.gpu
@pytest.mark.parametrize("S", tr.STAGES)
def test_the_plan_is_the_restarted_robots(wca, qs, S):
    """Every window of the four robots after the call is helpers/plan_restart.restart on H's window: copied and zero entries bit for bit,
    ref_traj within 1e-12, the hull rows those of the classic rule on the standing feet; the plan in force is "generated from S, no
    steps": a replan at M >= S is accepted for a reset robot at a stage inside its OLD swing."""
    from oracle import hull_spec as hs
    cfg = "reactive_gs"
    fs = rs.scenario(wca)[0]
    feed = Feed(wca, qs, cfg, S, "plain")
    pipe = _pipe(wca, cfg)
    pipe.upload_footsteps(fs, fs)
    for t in range(S):
        _tick(pipe, feed.at(t))
    w0 = pipe.plan_window()
    pipe.reset_robots(tr.mode(), tr.rows(fs))
    w1 = pipe.plan_window()
    want = tr.reset_plan(w0, S, fs)
    assert set(w1) == set(w0) and "dcm_vel_traj" in w1
    _same_window(w1, w0, KEPT)
    assert np.array_equal(w1["u_init"], w0["u_init"])
    for i in SET:
        for k in COPIED:
            assert np.array_equal(w1[k][i, S:], want[k][i, S:]), (k, i)
        err = np.abs(w1["ref_traj"][i, S:] - want["ref_traj"][i, S:]).max()
        print(i, "ref_traj", err)
        assert err <= 1e-12, (i, err)
        A, b, nc = hs.hull_from_feet(wca.synth.FOOT_RECT, fs["state0"][i, 24:36], fs["state0"][i, 36:48], 3)
        assert np.all(w1["hull_nc"][i, S:] == nc)
        assert np.abs(w1["hull_A"][i, S:] - A).max() < 1e-12 and np.abs(w1["hull_b"][i, S:, :nc] - b[:nc]).max() < 1e-12, i
    if S == 41:
        assert (int(w0["contact"][0, S + 2]) & 3) != 3           # (robot 0's old plan swings there)
        M = np.full(B, -1, np.int32); M[0] = S + 2
        rp = fr.new_steps(dict(w1, zmp_ref=w1["ref_traj"]), M, np.where(M >= 0, 1, 0).astype(np.int32), np.tile(np.array([1, 0], np.uint8), (B, 1)), 12, 3)
        pipe.replan_footsteps(M, rp, 12)
        assert (int(pipe.plan_window()["contact"][0, S + 2 + 12]) & 3) != 3


# ---------------------------------------------------------------------------------------------------------------- (3) the restatement

@pytest.mark.gpu
def test_against_the_restatement(wca, qs):
    """The MPC, sensor form, S = 41: the four robots from S on against oracle/tick_spec.run_ticks on the window with the reset rows, fed
    the recorded readings of its robot in the loop, at 1e-9.  Measured on an MI355X: DESIGN §8.28."""
    cfg, S = "mpc", 41
    fs = rs.scenario(wca)[0]
    ref = tr.restated(wca, qs, cfg, S)
    n = MAXT - S
    feed = Feed(wca, qs, cfg, S, "sensor", n_after=n)
    pipe = _pipe(wca, cfg)
    pipe.upload_footsteps(fs, fs)
    for t in range(S):
        _tick(pipe, feed.at(t))
    pipe.reset_robots(tr.mode(), tr.rows(fs))
    for k in range(n):
        assert all(np.array_equal(x[SET], y) for x, y in zip(feed.after(k)[1], ref["readings"][k]))      # (Feed: the recording)
        _tick(pipe, feed.after(k))
    out = pipe.download()
    assert np.array_equal(out["ik_fail"][SET], ref["ik_fail"]) and np.array_equal(out["mpc_fail"][SET], ref["mpc_fail"]) and not out["feedback_fail"][SET].any()
    errs = {"u0_log": np.abs(out["u0_log"][S:, SET] - ref["u0_log"]).max(), "dq_log": np.abs(out["dq_log"][S:, SET] - ref["dq_log"]).max(),
            "q_des": np.abs(out["q_des"][SET] - ref["q_des"]).max(), "measured": np.abs(out["measured"][SET] - ref["measured_log"][-1]).max()}
    print("against the restatement:", errs)
    for k, e in errs.items():
        assert e <= 1e-9, (k, e)


# ---------------------------------------------------------------------------------------------------------------- (4) who stops

@pytest.mark.gpu
def test_if_stopped_resets_who_stopped_and_they_walk_again(wca, qs):
    """Robots 2 and 12 read zero normal force on tick S - 3: feedback_fail = 1 and ik_fail counts.  reset_robots(IF_STOPPED for every
    robot) resets exactly those two and reports their ik_fail; the others are bit for bit a run without the call.  Before the result is
    fetched a replan_footsteps for robot 2 at M >= S is accepted - the owed decision was settled - and robot 2 takes its new steps with
    ik_fail == 0 to MAXT, fed the states the restatement's internal plant has on the stitched plan from the reset rows.  The reactive
    controller, as in the restart's walk-again test."""
    from oracle import tick_spec as ts
    cfg, S, BAD = "reactive_gs", 41, [2, 12]
    fs, plan, _ = rs.scenario(wca)
    feed = Feed(wca, qs, cfg, S, "plain", n_after=MAXT - S)
    kept = [i for i in range(B) if i not in BAD]
    # robot 2's new steps and what it is fed while it takes them: the restatement with the internal plant, from the reset rows
    after = tr.reset_plan(plan, S, fs, BAD)
    M = np.full(B, -1, np.int32); M[2] = S + 5
    rp = fr.new_steps(after, M, np.where(M >= 0, 2, 0).astype(np.int32), np.tile(np.array([1, 0], np.uint8), (B, 1)), 12, 3)
    stitched = fr.footstep_replan(after, fs, M, rp, T, MAXT)
    win = {k: v[[2]][:, S:] for k, v in stitched.items() if k not in prs.NOT_STAGED}
    R = robots.ROBOTS[rs.ROBOT]
    start = tr.start_rows(fs, False)
    d = {k: (v[[2]] if isinstance(v, np.ndarray) and v.shape[:1] == (B,) else v) for k, v in fs.items()}
    d.update(ref_traj=win["ref_traj"], dcm_vel_traj=win["dcm_vel_traj"], dcm0=start["dcm0"][[2]], u_init=start["u_init"][[2]])
    walk = ts.run_ticks(ts.TickParams(horizon=50, k_com=R["k_com"], k_zmp=R["k_zmp"]), d, MAXT - S, rs.ik_params(wca, qs), kin_model=wca.synth.icub_like_model(),
                        foot_rect=wca.synth.FOOT_RECT, stages=stt.stages_of(win, MAXT - S), neck_additional_rotation=R["additional_rotation"],
                        dcm_controller="reactive", k_dcm=rs.K_DCM, dcm_vel=win["dcm_vel_traj"], zmp_gain_schedule=zg.ZMP_SCHEDULE[rs.ROBOT])
    assert not walk["ik_fail"].any() and np.abs(walk["dq_log"]).max() > 1e-2
    post = {k: v.copy() for k, v in feed.post.items()}
    p12 = stt.external_of_sensors(tr.restated(wca, qs, cfg, S, (12,)))          # robot 12 stands where it was put back
    for k, log in (("dcm", "dcm_log"), ("com", "com_log"), ("zmp", "zmp_log"), ("q", "q_log")):
        post[k][:, 2] = walk[log][:, 0]
        post[k][:, 12] = p12[k][:, 0]
    nof = Sn(*tr.bad_force(tr.sensor_feed(fs, 1, seed=9)[0], BAD))
    h, h0 = _pipe(wca, cfg), _pipe(wca, cfg)
    for p in (h, h0):
        p.upload_footsteps(fs, fs)
        for t in range(S):
            _tick(p, nof if t == S - 3 else feed.at(t))
    before = h.download()
    assert np.array_equal(before["feedback_fail"], np.isin(np.arange(B), BAD).astype(np.int64))
    assert np.array_equal(before["ik_fail"] > 0, np.isin(np.arange(B), BAD)) and (before["ik_fail"][BAD] == 4).all()
    rows = {k: np.ascontiguousarray(fs[k]) for k in ("state0", "q0", "com0")}
    h.reset_robots(np.full(B, tr.IF_STOPPED, np.uint8), rows)
    h.replan_footsteps(M, rp, 12)                            # (robot 2's old plan swings at stage 46: accepted because it stands now)
    res = h.restart_result()
    assert res["stage"] == S and np.array_equal(res["restarted"], np.isin(np.arange(B), BAD))
    assert np.array_equal(res["stopped_ticks"], np.where(res["restarted"], before["ik_fail"], 0))
    assert not h.download()["feedback_fail"].any()
    for p in (h, h0):
        for k in range(MAXT - S):
            _tick(p, _rowp(post, k))
    oh, o0 = h.download(), h0.download()
    _same_rows(oh, o0, kept)
    _same_window(h.plan_window(), h0.plan_window(), kept)
    assert not oh["ik_fail"][BAD].any() and not oh["feedback_fail"][BAD].any() and (o0["ik_fail"][BAD] == 4 + MAXT - S).all()
    assert np.abs(oh["dq_log"][S:, 2]).max() > 1e-2 and not o0["dq_log"][S:, BAD].any()
    err = np.abs(oh["dq_log"][S:, 2] - walk["dq_log"][:, 0]).max()
    print("robot 2 walking again against the restatement:", err)
    assert err <= 1e-8


# ---------------------------------------------------------------------------------------------------------------- (5) a rejected first reading

@pytest.mark.gpu
@pytest.mark.parametrize("form", ["plain", "sensor"])
@pytest.mark.parametrize("S", [0, 41, 64])
def test_a_rejected_first_reading_keeps_the_reset_rows(wca, qs, form, S):
    """A reset robot whose tick-S feedback is non-finite: `measured` of that tick is (dcm0, com0, u_init), it is stopped with
    feedback_fail == 1, its measured joints are q0, and its wave-mates are bit for bit a run in which its feedback was fine.  S = 0: the
    rows the host reports before any tick are the reset rows."""
    cfg, r = "mpc", 3
    fs = rs.scenario(wca)[0]
    feed = Feed(wca, qs, cfg, S, form, n_after=3)
    start = tr.start_rows(fs, True)
    want = np.concatenate([start["dcm0"], fs["com0"], start["u_init"]], 1)
    outs = []
    for bad in (True, False):
        p = _pipe(wca, cfg)
        p.upload_footsteps(fs, fs)
        for t in range(S):
            _tick(p, feed.at(t))
        p.reset_robots(tr.mode(), tr.rows(fs, True))
        assert np.array_equal(p.download()["measured"][SET], want[SET])
        for k in range(3):
            kind, args = feed.after(k)
            fb = [np.array(x, copy=True) for x in args]
            if bad and k == 0:
                fb[0][r, 1] = np.nan
            _tick(p, (kind, tuple(fb)))
            if k == 0:
                first = p.download()
        outs.append((first, p.download()))
    (f_bad, o_bad), (f_ok, o_ok) = outs
    assert np.array_equal(f_bad["measured"][r], want[r]) and f_bad["feedback_fail"][r] == 1 and f_bad["ik_fail"][r] == 2
    assert not np.array_equal(f_ok["measured"][r], want[r]) and f_ok["feedback_fail"][r] == 0 and f_ok["ik_fail"][r] == 0
    assert o_bad["ik_fail"][r] == 4 and np.array_equal(o_bad["q_des"][r], fs["q0"][r]) and not o_bad["dq_log"][S:S + 3, r].any()
    others = [i for i in range(B) if i != r]
    _same_rows(o_bad, o_ok, others)
    # (p: the run in which nobody stopped) IF_STOPPED resets nobody there
    p.reset_robots(tr.mode(SET, tr.IF_STOPPED), tr.rows(fs, True))
    res = p.restart_result()
    assert not res["restarted"].any() and res["stage"] == S + 3


# ---------------------------------------------------------------------------------------------------------------- (6) filters

@pytest.mark.gpu
@pytest.mark.parametrize("S", tr.STAGES)
def test_filters_start_at_a_reset_robots_next_reading(wca, qs, S):
    """Sensor filters on (10 Hz each): the sensor case of (1) is bit for bit the fresh twin's - the reset robot's joint-velocity and wrench
    filters start AT its next accepted reading, its CoM filter at com0, although the handle's filters have long been running - and the
    nine robots not reset are bit for bit the run without the call: the kernel change moves nothing."""
    _twin_check(wca, qs, "mpc", S, "sensor", S == 64, filters=tr.FILTERS)


@pytest.mark.gpu
def test_a_rejected_reading_leaves_the_robot_fresh(wca, qs):
    """Filters on.  Robot 5's reading of tick S has no normal force: rejected, its mark stays.  A second sensor call for tick S + 1
    replaces a first one and starts from the same state.  `measured` after tick S + 1 - robot 5 is stopped, but its reading is
    evaluated - is what a fresh twin evaluates from that reading at its tick 0: the filters started AT it."""
    cfg, S, r = "mpc", 41, 5
    fs = rs.scenario(wca)[0]
    feed = Feed(wca, qs, cfg, S, "sensor", n_after=3)
    h = _pipe(wca, cfg, filters=tr.FILTERS)
    h.upload_footsteps(fs, fs)
    for t in range(S):
        _tick(h, feed.at(t))
    h.reset_robots(tr.mode(), tr.rows(fs))
    w_after = h.plan_window()
    _tick(h, Sn(*tr.bad_force(feed.after(0)[1], (r,))))
    o = h.download()
    assert o["feedback_fail"][r] == 1 and o["ik_fail"][r] == 2
    h.set_desired_from_plan()
    _give(h, feed.after(2))                                  # replaced by the next call: it advances nothing
    _give(h, feed.after(1))
    h.run(1)
    got = h.download()["measured"][r]
    h2 = _pipe(wca, cfg, maxt=MAXT - S, filters=tr.FILTERS)
    d, wb = tr.twin_upload(w_after, S, fs, False)
    h2.upload(dict(d, ref_traj=wb["ref_traj"]), left_traj=wb["left_traj"], right_traj=wb["right_traj"], left_twist=wb["left_twist"],
              right_twist=wb["right_twist"], contact=wb["contact"], com_height_traj=wb["com_height"], com_height_vel=wb["com_height_vel"])
    _tick(h2, feed.after(1))
    assert np.array_equal(got, h2.download()["measured"][r])
    # (a filter that had run on would give another DCM: the twin's next tick, fed the same reading again, does)
    _tick(h2, feed.after(1))
    assert not np.array_equal(got, h2.download()["measured"][r])


# ---------------------------------------------------------------------------------------------------------------- (7) no resident plan

@pytest.mark.gpu
@pytest.mark.parametrize("explicit", [False, True], ids=["null_rows", "explicit_rows"])
def test_a_streamed_handle_without_a_plan(wca, qs, explicit):
    """A streamed handle without a resident plan, its stages handed over by set_desired_host: the same twin comparison.  There is no plan
    part - the caller's next stage is the robot's -, and with dcm0 / u_init NULL the standing ZMP is the midpoint of the sole origins (the
    handle knows no zmp_delta_*)."""
    cfg, S = "mpc", 41
    fs, plan, _ = rs.scenario(wca)
    feed = Feed(wca, qs, cfg, S, "plain")
    src = _pipe(wca, cfg)
    src.upload_footsteps(fs, fs)
    w = src.plan_window()
    after = tr.reset_plan(w, S, fs)                           # the stages the caller hands over from S on: the reset robots stand
    stages = stt.stages_of(dict(after, com_height_traj=after["com_height"]), MAXT)
    zero = (0.0, 0.0)
    start = tr.start_rows(fs, True) if explicit else {k: np.array([tr.standing_zmp(fs["state0"][i], zero, zero) for i in range(B)]) for k in ("dcm0", "u_init")}
    h, h0 = _pipe(wca, cfg, resident=False), _pipe(wca, cfg, resident=False)
    for p in (h, h0):
        p.upload(dict(state0=fs["state0"], q0=fs["q0"], com0=fs["com0"], ref_traj=w["ref_traj"], dcm0=w["ref_traj"][:, 0].copy(), u_init=w["u_init"]))
        for t in range(S):
            _tick(p, feed.at(t), _stage(stages, t))
    h.reset_robots(tr.mode(), tr.rows(fs, explicit))
    assert h.restart_result()["restarted"][SET].all()
    assert np.array_equal(h.download()["measured"][SET], np.concatenate([start["dcm0"], fs["com0"], start["u_init"]], 1)[SET])
    for p in (h, h0):
        for t in range(S, S + AFTER):
            _tick(p, feed.at(t), _stage(stages, t))
    oh, o0 = h.download(), h0.download()
    _same_rows(oh, o0, KEPT)
    h2 = _pipe(wca, cfg, maxt=MAXT - S, resident=False)
    h2.upload(dict(state0=fs["state0"], q0=fs["q0"], com0=fs["com0"], ref_traj=np.ascontiguousarray(w["ref_traj"][:, S:]), **start))
    for k in range(AFTER):
        _tick(h2, feed.after(k), _stage(stages, S + k))
    _same_rows(oh, h2.download(), SET, a0=S, b0=0, n=AFTER)
    assert not oh["ik_fail"][SET].any()


# ---------------------------------------------------------------------------------------------------------------- (8) streams

@pytest.mark.gpu
def test_reset_on_a_stream_with_the_host_forms(wca, qs):
    """One non-blocking stream: run, reset_robots, set_desired_host, set_sensor_feedback_host, run with no synchronisation of the caller's,
    every input buffer overwritten right after its call - the HOST forms wait for the reset's kernels themselves.  Bit for bit the
    blocking run."""
    cfg, S, n = "mpc", 41, 12
    fs = rs.scenario(wca)[0]
    feed = Feed(wca, qs, cfg, S, "sensor", n_after=n)
    outs = []
    s = wca.capi.stream_create()
    try:
        for stream in (None, s):
            p = _pipe(wca, cfg)
            p.upload_footsteps(fs, fs)
            for t in range(S):
                p.set_desired_from_plan(stream=stream)
                if stream:
                    wca.capi.stream_synchronize(stream)
                _give(p, feed.at(t))
                p.run(1, stream=stream)
            if not outs:
                stages = stt.stages_of(dict(tr.reset_plan(p.plan_window(), S, fs), com_height_traj=p.plan_window()["com_height"]), MAXT)
            mode, rows = tr.mode(), tr.rows(fs, True)
            p.reset_robots(mode, rows, stream=stream)
            mode[:] = 9
            for v in rows.values():
                v[:] = np.nan
            for k in range(n):
                st = [np.array(x, copy=True) for x in _stage(stages, S + k)]
                p.set_desired_host(*st)
                for x in st:
                    x[...] = 77 if x.dtype == np.uint8 else np.nan
                fb = [np.array(x, copy=True) for x in feed.after(k)[1]]
                p.set_sensor_feedback_host(*fb)
                for x in fb:
                    x[:] = np.nan
                p.run(1, stream=stream)
            if stream:
                wca.capi.stream_synchronize(stream)
            outs.append((p.download(), p.plan_window()))
    finally:
        wca.capi.stream_synchronize(s)
        wca.capi.stream_destroy(s)
    _same_rows(outs[0][0], outs[1][0], slice(None))
    _same_window(outs[0][1], outs[1][1])
    assert not outs[0][0]["ik_fail"][SET].any() and not outs[0][0]["feedback_fail"].any()


# ---------------------------------------------------------------------------------------------------------------- (9) with rebase

@pytest.mark.gpu
def test_reset_around_a_rebase(wca, qs):
    """Handle A has room for the whole run; handle B, with max_ticks 130, is reset at stage 40, rebased by 60 after 90 ticks - a rebase
    admits the reset robots: they stand - and reset again right behind it (A at stage 90, B at stage 30): the state and the log rows of
    every tick are A's, read at B's own indices, and B's plan is A's from its shift on.  One-step plans, which stand in time for the rebase."""
    cfg = "mpc"
    fs0 = rs.scenario(wca)[0]
    fs = dict(fs0, n_steps=np.minimum(fs0["n_steps"], 1).astype(np.int32))
    ext = tr.plain_feed(fs, 150, seed=12)
    a, b = _pipe(wca, cfg, maxt=MAXT), _pipe(wca, cfg, maxt=130)
    shift = 0

    def walk(t0, t1):
        for p in (a, b):
            for t in range(t0, t1):
                _tick(p, _rowp(ext, t))

    def same(t0, done):
        oa, ob = a.download(), b.download()
        assert ob["tick"] == oa["tick"] - shift == done - shift
        _same_rows(oa, ob, slice(None), keys=tr.STATE)
        for k in tr.LOGS:
            assert np.array_equal(oa[k][t0:done], ob[k][t0 - shift:done - shift]), (k, done)
        wa, wb = a.plan_window(), b.plan_window()
        for k in wb:
            if k != "u_init":
                assert np.array_equal(wb[k], wa[k][:, shift:shift + wb[k].shape[1]]), (k, done)
    for p in (a, b):
        p.upload_footsteps(fs, fs)
    walk(0, 40)
    for p in (a, b):
        p.reset_robots(tr.mode(), tr.rows(fs, True))
    walk(40, 90)
    same(0, 90)
    shift = b.rebase_plan(60)
    assert shift == 60
    for p in (a, b):
        p.reset_robots(tr.mode((3, 12)), tr.rows(fs, False, (3, 12)))
    assert a.restart_result()["stage"] == 90 and b.restart_result()["stage"] == 30
    assert np.array_equal(a.download()["measured"], b.download()["measured"])
    walk(90, 150)
    same(90, 150)


# ---------------------------------------------------------------------------------------------------------------- (10) set slots

@pytest.mark.gpu
def test_set_slots_run_out_and_a_rebase_frees_them(wca, qs):
    """A resident handle of 20 ticks gives every robot three set slots.  A robot reset between single ticks takes one more each time: the
    third call is refused with WCQP_E_INVALID and changes nothing - plan, state, the last result -, and after a rebase, which frees the
    slots of past stages, the reset is accepted again."""
    cfg = "mpc"
    fs0 = rs.scenario(wca)[0]
    fs = dict(fs0, n_steps=np.zeros(B, np.int32), first_ds_ticks=5, final_ds_ticks=5)      # (a plan that stands within the 20 ticks, as a rebase asks)
    ext = tr.plain_feed(fs, 20, seed=13)
    pipe = _pipe(wca, cfg, maxt=20)
    pipe.upload_footsteps(fs, fs)
    for k in range(2):
        pipe.reset_robots(tr.mode((5,)), tr.rows(fs, False, (5,)))
        _tick(pipe, _rowp(ext, k))
    w, out, res = pipe.plan_window(), pipe.download(), pipe.restart_result()
    for m in (tr.mode((5,)), tr.mode((5, 7), tr.IF_STOPPED)):
        with pytest.raises(wca.WcqpError, match=r"\(-1\)"):
            pipe.reset_robots(m, tr.rows(fs, False, (5, 7)))
    _same_window(pipe.plan_window(), w)
    _same_rows(pipe.download(), out, slice(None))
    assert pipe.restart_result()["stage"] == res["stage"] == 1 and np.array_equal(pipe.restart_result()["restarted"], res["restarted"])
    pipe.reset_robots(tr.mode((7,)), tr.rows(fs, False, (7,)))        # (a robot with room)
    assert pipe.rebase_plan(2) == 2
    pipe.reset_robots(tr.mode((5,)), tr.rows(fs, False, (5,)))
    assert pipe.restart_result()["restarted"][5] and pipe.restart_result()["stage"] == 0
    for k in range(2, 12):
        _tick(pipe, _rowp(ext, k))
    assert not pipe.download()["ik_fail"].any()


# ---------------------------------------------------------------------------------------------------------------- (11) refusals

@pytest.mark.gpu
def test_refusals(wca, qs):
    """Every refusal of the header; each leaves the handle unchanged - a window and a download() compared before and after.  The restart
    and the recover call still refuse the resident handle."""
    cfg, S = "mpc", 41
    fs, plan, _ = rs.scenario(wca)
    lib, capi = wca.capi.lib(), wca.capi
    rows = tr.rows(fs, nan_kept=False)
    feed = Feed(wca, qs, cfg, S, "plain", n_after=2)

    def call(pipe, mode, d, drop=(), fn="wcqp_tick_reset_robots"):
        m = np.ascontiguousarray(mode, np.uint8)
        keep = {k: np.ascontiguousarray(v, float) for k, v in d.items()}
        f = dict(mode=m.ctypes.data, **{k: v.ctypes.data for k, v in keep.items()})
        return getattr(lib, fn)(pipe._h, C.byref(capi.TickRestart(**{k: v for k, v in f.items() if k not in drop})), None)

    # a handle that is not streamed: a planned handle (internal plant), the synthetic-gait EXTERNAL handle; a POSITION streamed handle
    from helpers import position_external as px
    R = robots.ROBOTS[rs.ROBOT]
    gait = wca.TickPipeline(B, MAXT, wca.MpcSolver(horizon=50), wca.IkSolver(form=wca.IK_FORM_QPOASES), k_com=R["k_com"], k_zmp=R["k_zmp"],
                            kin=wca.KinModel(wca.synth.icub_like_model()), external_feedback=True)
    assert not gait.info()["streamed_trajectories"]
    position = px.pipe(wca, "mpc", B=B)
    assert position.info()["streamed_trajectories"] and position.info()["ik_mode"] == "position"
    for refused in (_pipe(wca, cfg, planned=True), gait, position):
        assert call(refused, tr.mode(), rows) == WCQP_E_UNSUPPORTED
    fresh = _pipe(wca, cfg)
    assert call(fresh, tr.mode(), rows) == WCQP_E_INVALID                                        # not uploaded
    assert call(_pipe(wca, cfg, resident=False), tr.mode(), rows) == WCQP_E_INVALID              # ... without a plan too
    src = _pipe(wca, cfg)
    src.upload_footsteps(fs, fs)
    w = src.plan_window()
    fresh.upload(dict(state0=fs["state0"], q0=fs["q0"], com0=fs["com0"], ref_traj=w["ref_traj"], dcm0=w["ref_traj"][:, 0].copy(), u_init=w["u_init"]),
                 left_traj=w["left_traj"], right_traj=w["right_traj"], left_twist=w["left_twist"], right_twist=w["right_twist"], contact=w["contact"],
                 com_height_traj=w["com_height"], com_height_vel=w["com_height_vel"])
    assert call(fresh, tr.mode(), rows) == WCQP_E_UNSUPPORTED                                    # a resident plan that was not generated

    pipe, twin = src, _pipe(wca, cfg)           # (twin: the same walk without a single refused call)
    twin.upload_footsteps(fs, fs)
    for p in (pipe, twin):
        for t in range(S):
            _tick(p, feed.at(t))
    w_ref, o_ref = pipe.plan_window(), pipe.download()

    def unchanged():
        _same_window(pipe.plan_window(), w_ref)
        o = pipe.download()
        _same_rows(o, o_ref, slice(None))
        assert o["tick"] == o_ref["tick"]

    def arr(key, idx, val):
        e = dict(rows); e[key] = np.array(rows[key], copy=True); e[key][idx] = val
        return e
    two = dict(rows, dcm0=rows["com0"].copy(), u_init=rows["com0"].copy())
    bad = [(tr.mode(), rows, ("mode",)), (tr.mode(), rows, ("state0",)), (tr.mode(), rows, ("q0",)), (tr.mode(), rows, ("com0",)),
           (tr.mode((3,), 3), rows, ()), (tr.mode((3,), 255), rows, ()),
           (tr.mode(), arr("state0", (3, 30), np.nan), ()), (tr.mode(), arr("q0", (12, 22), np.nan), ()), (tr.mode(), arr("com0", (0, 1), -np.inf), ()),
           (tr.mode(SET, tr.IF_STOPPED), arr("q0", (5, 0), np.nan), ()),
           (tr.mode(), dict(two, dcm0=arr("com0", (5, 0), np.nan)["com0"]), ()), (tr.mode(), dict(two, u_init=arr("com0", (12, 1), np.nan)["com0"]), ())]
    for mode, d, drop in bad:
        assert call(pipe, mode, d, drop) == WCQP_E_INVALID, (mode, drop)
        unchanged()
    assert lib.wcqp_tick_reset_robots(pipe._h, None, None) == WCQP_E_INVALID
    # the restart and the recover call keep their refusal of this handle
    assert call(pipe, tr.mode(), rows, fn="wcqp_tick_restart_robots") == WCQP_E_UNSUPPORTED
    assert lib.wcqp_tick_recover_robots(pipe._h, None, C.byref(capi.TickRecover()), None) == WCQP_E_UNSUPPORTED
    unchanged()
    # a stage in hand; a stage and a feedback in hand: the handle is what it was, and tick S runs on both as on the twin
    pipe.set_desired_from_plan()
    assert call(pipe, tr.mode(), rows) == WCQP_E_INVALID
    unchanged()
    _give(pipe, feed.at(S))
    assert call(pipe, tr.mode(), rows) == WCQP_E_INVALID
    _same_window(pipe.plan_window(), w_ref)
    pipe.run(1)
    _tick(twin, feed.at(S))
    w_ref, o_ref = twin.plan_window(), twin.download()
    unchanged()
    # a call that lists nobody is accepted and enqueues nothing; kept robots' rows may hold anything
    nan = {k: np.full_like(v, np.nan) for k, v in rows.items()}
    assert call(pipe, tr.mode(()), nan) == 0
    res = pipe.restart_result()
    assert res["stage"] == S + 1 and not res["restarted"].any()
    unchanged()
    # S > max_ticks cannot be reached by this call - S is the ticks enqueued, and wcqp_tick_run refuses a tick past max_ticks -: a handle
    # whose every tick has run takes a reset at S = max_ticks
    short = _pipe(wca, cfg, maxt=4)
    fs4 = dict(fs, n_steps=np.zeros(B, np.int32))
    short.upload_footsteps(fs4, fs4)
    e4 = tr.plain_feed(fs, 4)
    for t in range(4):
        _tick(short, _rowp(e4, t))
    assert call(short, tr.mode(), rows) == 0 and short.restart_result()["stage"] == 4
