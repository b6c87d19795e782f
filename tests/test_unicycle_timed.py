"""The planner chooses every step's duration (wcqp_unicycle_plan_timed_*).  CPU: properties of the numpy restatement
(helpers/unicycle_plan_timed.py), its decision margins, the closed loop on its timed plans, and the refusals that need no device.  GPU:
the kernel against the restatement, batch sizes, non-finite inputs next to healthy robots, the two forms, a fuzz batch, and
upload_goal / replan_goal with `timing` end to end against oracle/tick_spec.py, on the planned, the POSITION and a resident-plan handle."""
import ctypes as C

import numpy as np
import pytest
from walking_controllers_amd.capi import E_INVALID as WCQP_E_INVALID, E_HIP as WCQP_E_HIP

import robots
from helpers import footstep_plan_timed as ft
from helpers import planned_tick as pt
from helpers import position_tick as pk
from helpers import streamed_tick as stt
from helpers import unicycle_plan as up
from helpers import unicycle_plan_timed as ut
from helpers import zmp_gains as zg

OUT = ("n_steps", "side", "target", "status", "desired_point", "unicycle_end", "ss_ticks", "ds_ticks")
MARGIN = 1e-9           # a robot the restatement decided by less may be decided otherwise by the device: it is left out of a comparison
# the scenario of the GPU tests: 13 robots (a wave with dead lanes), K = 8 steps of 20 .. 30 samples, nominally 25.  The thresholds are set
# for steps of 0.25 s, as the untimed planner's tests set them; a turn at 0.7 rad/s passes max_angle_variation (10 degrees) within 25
# samples, so a turning robot's steps are shorter than nominal.  The handle's step_ticks is not read: 1 would end every untimed plan STUCK
SCEN = dict(step_ticks=1, max_steps=8, max_linear_velocity=0.2, max_angular_velocity=0.7, min_step_length=0.01, min_angle_variation=0.02)
# the reference's weights and ratio (plannerParams.ini: timeWeight 2.5, positionWeight 1.0, switchOverSwingRatio 0.7) ...
TIMING = dict(min_step_ticks=20, max_step_ticks=30, nominal_step_ticks=25, time_weight=2.5, position_weight=1.0, switch_over_swing_ratio=0.7)
# ... and a position weight at which the two terms of a candidate's score are of one size (|r - r_nom|^2 ~ 0.05^2, the time term ~ 1)
HEAVY = dict(TIMING, position_weight=2000.0)
FUZZ_SEED, FUZZ_B, FUZZ_RADIUS = 7, 256, 0.4
# the walk of the closed-loop tests: the untimed planner tests' small robot (feet 0.114 .. 0.123 m apart, steps of 30 + 20 stages behind
# 20) with the reference's timing scaled to it - 0.8 / 0.9 / 1.0 s there, 40 / 50 / 60 ticks here -, its weights and its ratio.  A step
# may turn a foot by 0.07 rad at most: at 0.15 rad/s the turning robot passes that after 46 samples, so its steps are shorter than nominal
FIRST_DS, K_WALK, MAXT = 20, 6, 400
WALK = dict(step_ticks=1, max_steps=K_WALK, nominal_width=0.118, min_width=0.10, max_linear_velocity=0.03, max_angular_velocity=0.15,
            min_step_length=0.005, min_angle_variation=0.01, max_angle_variation=0.07)
WALK_TIMING = dict(min_step_ticks=40, max_step_ticks=60, nominal_step_ticks=50, time_weight=2.5, position_weight=1.0, switch_over_swing_ratio=0.7)
GOALS0 = np.array([[0.04, 0.0], [0.03, 0.03], [0.05, -0.01]])      # straight, a turn, and the robot that is replanned
FD_REPLAN, GOAL1 = 15, (0.02, 0.02)
K_DCM = 1.0
KEYS = ("u0_log", "dq_log", "q_des", "dcm", "com")


def _params(wca, **kw):
    return dict(wca.UnicyclePlanner.DEFAULTS, **kw)


def _replay(p, g, r, i):
    """the feet of robot i walked through the steps of plan r: per step (swing side, its three constraint margins against the stance foot)"""
    feet = [(g["left0"][i, 0], g["left0"][i, 1], np.arctan2(g["left0"][i, 6], g["left0"][i, 3])),
            (g["right0"][i, 0], g["right0"][i, 1], np.arctan2(g["right0"][i, 6], g["right0"][i, 3]))]
    rows = []
    for k in range(int(r["n_steps"][i])):
        sw = int(r["side"][i, k])
        st = feet[1 - sw]
        c, yaw = r["target"][i, k, :2], feet[sw][2] + r["target"][i, k, 2]
        d = c - np.array(st[:2])
        rlon = np.cos(st[2]) * d[0] + np.sin(st[2]) * d[1]
        rlat = np.cos(st[2]) * d[1] - np.sin(st[2]) * d[0]
        rows.append((sw, p["max_step_length"] - np.hypot(rlon, rlat), (1.0 if sw == 0 else -1.0) * rlat - p["min_width"],
                     p["max_angle_variation"] - abs(up.wrap(yaw - st[2]))))
        feet[sw] = (c[0], c[1], yaw)
    return rows


def _plan(p, tm, g):
    return ut.unicycle_plan_timed(p, tm, g["left0"], g["right0"], g["goals"], g["first_side"])


@pytest.fixture(scope="module")
def scen(wca):
    """the 13 scenario robots and their restated plans, at the reference's weights and at the heavy position weight"""
    g = wca.synth.synth_goal_batch(13)
    p = _params(wca, **SCEN)
    return g, p, _plan(p, TIMING, g), _plan(p, HEAVY, g)


@pytest.fixture(scope="module")
def fuzz(wca):
    """256 robots heading anywhere with goals from the disc of 0.4 m (some arrive within K steps, most do not), at the heavy position
    weight: the weight at which the choice among feasible candidates is not the nominal one"""
    g = wca.synth.synth_goal_batch(FUZZ_B, seed=FUZZ_SEED, cases=False, radius=FUZZ_RADIUS)
    p = _params(wca, **SCEN)
    return g, p, _plan(p, HEAVY, g)


@pytest.fixture(scope="module")
def walk3(wca, qs):
    """Three robots of the walk tests sent to GOALS0 by the timed planner, robot 2 sent on to GOAL1 by a timed replan five stages into the
    double support behind its second step: the restated footsteps with their durations, the timed plans (before and after the replan) and
    oracle/tick_spec.py's run over each - reactive controller, gain scheduling."""
    from oracle import tick_spec as ts
    robot = "iCubGazeboV2_5"
    R = robots.ROBOTS[robot]
    model = wca.synth.icub_like_model()
    kb = wca.synth.synth_walk_kin_batch(3)
    fs = wca.synth.synth_footstep_walk_batch(3, MAXT, pt.poses_host(model, kb), kb)
    st = fs["state0"]
    p = _params(wca, **WALK)
    T = MAXT + 51
    r0 = ut.unicycle_plan_timed(p, WALK_TIMING, st[:, 24:36], st[:, 36:48], GOALS0, 1)
    fs.update(n_steps=r0["n_steps"], side=r0["side"], target=r0["target"], first_ds_ticks=FIRST_DS, ss_ticks=r0["ss_ticks"], ds_ticks=r0["ds_ticks"],
              final_ds_ticks=0, lift=0.02)
    plan0 = ft.footstep_plan_timed(fs, st, T, MAXT)
    m_replan = plan0["starts"][2][1] + int(r0["ss_ticks"][2, 1]) + 5
    M = np.array([-1, -1, m_replan], np.int32)
    r1 = ut.unicycle_plan_timed(p, WALK_TIMING, plan0["left_traj"][2:, m_replan], plan0["right_traj"][2:, m_replan], np.array([GOAL1]), 1)
    rp = dict(n_steps=np.zeros(3, np.int32), side=np.zeros((3, K_WALK), np.uint8), target=np.zeros((3, K_WALK, 3)), ss_ticks=np.zeros((3, K_WALK), np.int32),
              ds_ticks=np.zeros((3, K_WALK), np.int32), first_ds_ticks=FD_REPLAN)
    for k in ("n_steps", "side", "target", "ss_ticks", "ds_ticks"):
        rp[k][2] = r1[k][0]
    plan1 = ft.footstep_replan_timed(plan0, fs, M, rp, T, MAXT)
    ipar = robots.ik_params(qs, robot, v_max=wca.synth.WALK_VMAX.copy())
    ipar.joint_reg_deg = wca.synth.WALK_POSTURE_DEG.copy()

    def run(plan, n=MAXT):
        d = dict(fs, ref_traj=plan["ref_traj"], dcm_vel_traj=plan["dcm_vel_traj"], dcm0=plan["ref_traj"][:, 0].copy(), u_init=plan0["zmp_ref"][:, 0].copy())
        return ts.run_ticks(ts.TickParams(horizon=50, k_com=R["k_com"], k_zmp=R["k_zmp"]), d, n, ipar, kin_model=model, foot_rect=wca.synth.FOOT_RECT,
                            stages=stt.stages_of(plan, MAXT), neck_additional_rotation=R["additional_rotation"], dcm_controller="reactive",
                            k_dcm=K_DCM, dcm_vel=plan["dcm_vel_traj"], zmp_gain_schedule=zg.ZMP_SCHEDULE[robot])
    return dict(fs=fs, p=p, r0=r0, r1=r1, M=M, m_replan=m_replan, rp=rp, plan0=plan0, plan1=plan1, ref0=run(plan0), ref1=run(plan1), robot=robot, T=T)


# ---------------------------------------------------------------------------------------------------------------- CPU

def test_closed_loop_on_the_timed_footsteps(walk3):
    """(straight, turn, replanned) the timed plan of the timed planner's footsteps and oracle/tick_spec.py walk the whole plan - every
    robot stands before max_ticks - with no IK or MPC failure, before and after robot 2 is sent on inside a double support"""
    w = walk3
    assert (w["r0"]["status"] == up.DONE).all() and (w["r0"]["n_steps"] >= 3).all() and w["r1"]["status"][0] == up.DONE and w["r1"]["n_steps"][0] >= 2
    assert (w["r0"]["margin"] >= MARGIN).all() and w["r1"]["margin"][0] >= MARGIN
    assert abs(w["r0"]["target"][1, :, 2]).max() > 0.05                       # (the turn turns)
    m0 = w["r0"]["ss_ticks"] + w["r0"]["ds_ticks"]
    print("step durations", m0.tolist(), (w["r1"]["ss_ticks"] + w["r1"]["ds_ticks"]).tolist())
    assert len(set(m0[m0 > 0].tolist())) >= 2                                 # (the robots do not march to one metronome)
    assert all(s[-1] < MAXT for s in w["plan0"]["starts"])
    assert w["m_replan"] + FD_REPLAN + int((w["r1"]["ss_ticks"] + w["r1"]["ds_ticks"]).sum()) < MAXT
    assert (w["plan0"]["contact"][2, w["m_replan"]] & 3) == 3 and (w["plan0"]["contact"][2, w["m_replan"] - 6] & 3) != 3
    for ref in (w["ref0"], w["ref1"]):
        assert (ref["ik_fail"] == 0).all() and (ref["mpc_fail"] == 0).all()
    for k in KEYS:                                                            # (the replan changed robot 2's walk, and only that)
        ax = 1 if k in ("u0_log", "dq_log") else 0
        assert np.array_equal(np.take(w["ref0"][k], [0, 1], axis=ax), np.take(w["ref1"][k], [0, 1], axis=ax)), k
    assert not np.array_equal(w["ref0"]["q_des"][2], w["ref1"]["q_des"][2])


def test_steps_satisfy_the_constraints_and_the_duration_rules(scen, fuzz):
    """every step taken satisfies the three constraints against its stance foot (replayed from the outputs alone), lasts min .. max ticks
    split into ss, ds >= 1 by the ratio, sides alternate from first_side, rows of steps not taken are zero, goal (0, 0) gives no step"""
    g, p, r, rh = scen
    for gg, r_, tm in ((g, r, TIMING), (g, rh, HEAVY), (fuzz[0], fuzz[2], HEAVY)):
        for i in range(len(r_["n_steps"])):
            rows = _replay(p, gg, r_, i)
            n = int(r_["n_steps"][i])
            assert [sw for sw, *_ in rows] == [(int(gg["first_side"][i]) + k) % 2 for k in range(n)], i
            assert all(min(m[1:]) >= -1e-12 for m in rows), (i, rows)
            for k in ("side", "target", "ss_ticks", "ds_ticks"):
                assert not r_[k][i, n:].any(), (k, i)
            assert (r_["status"][i] == up.TRUNCATED) == (n == p["max_steps"])
            ss, ds = r_["ss_ticks"][i, :n], r_["ds_ticks"][i, :n]
            assert (ss >= 1).all() and (ds >= 1).all() and (ss + ds >= tm["min_step_ticks"]).all() and (ss + ds <= tm["max_step_ticks"]).all()
            assert [(int(a), int(b)) for a, b in zip(ss, ds)] == [ut.durations(int(a + b), tm["switch_over_swing_ratio"]) for a, b in zip(ss, ds)]
            assert [s["m"] for s in r_["steps"][i]] == (ss + ds).tolist()
    case = {c: i for i, c in enumerate(g["case"])}
    for r_ in (r, rh):
        assert r_["n_steps"][case["origin"]] == 0 and r_["status"][case["origin"]] == up.DONE
        assert r_["n_steps"][case["below_a_step"]] == 0 and r_["status"][case["below_a_step"]] == up.DONE
        for c in ("far", "far_turn"):
            assert r_["n_steps"][case[c]] == p["max_steps"] and r_["status"][case[c]] == up.TRUNCATED
        for c in ("straight", "turn_left", "turn_right", "behind"):
            assert 0 < r_["n_steps"][case[c]] < p["max_steps"] and r_["status"][case[c]] == up.DONE, c
        assert (r_["target"][..., 2] > 1e-3).any() and (r_["target"][..., 2] < -1e-3).any()
    # the durations differ per robot and per step: the turning robots step faster than nominal, and the heavy weight shortens straight steps
    assert set(np.unique(r["ss_ticks"] + r["ds_ticks"])) >= {0, 24, 25} and set(np.unique(rh["ss_ticks"] + rh["ds_ticks"])) >= {0, 23, 24, 25}
    assert len(set(np.unique(fuzz[2]["ss_ticks"] + fuzz[2]["ds_ticks"])) - {0}) >= 3
    assert set(np.unique(fuzz[2]["status"])) >= {up.DONE, up.TRUNCATED}


def test_the_ratio_splits_a_step(wca):
    """ds = min(max(floor(m rho + 0.5), 1), m - 1): the reference's 0.7 gives 37 of 90 and 10 of 25; the clamps hold at the extremes"""
    assert ut.durations(90, 0.7) == (53, 37) and ut.durations(25, 0.7) == (15, 10) and ut.durations(2, 0.7) == (1, 1)
    assert ut.durations(20, 1e-6) == (19, 1) and ut.durations(20, 1e6) == (1, 19) and ut.durations(3, 1.0) == (1, 2)


def test_without_a_position_weight_a_feasible_nominal_step_is_taken(scen):
    """position_weight = 0: the score is the time term alone, smallest at nominal_step_ticks - every step whose nominal candidate is
    feasible lasts exactly that, and every other step the feasible duration nearest to it in 1 / m"""
    g, p, _, _ = scen
    r = _plan(p, dict(TIMING, position_weight=0.0), g)
    seen = 0
    for i in range(13):
        for s in r["steps"][i]:
            if TIMING["nominal_step_ticks"] in s["feasible"]:
                assert s["m"] == TIMING["nominal_step_ticks"], (i, s["m"])
                seen += 1
            else:
                assert s["m"] == min(s["feasible"], key=lambda m: (abs(1.0 / m - 1.0 / TIMING["nominal_step_ticks"]), m))
    assert seen >= 20 and (r["ss_ticks"] + r["ds_ticks"] == 24).any()


def test_mirrored_inputs_give_mirrored_footsteps_of_equal_durations(scen, fuzz):
    """y -> -y with the sides swapped (d_y = 0): the same steps, mirrored, each as long as before"""
    def mirror(pose):
        yaw = np.arctan2(pose[:, 6], pose[:, 3])
        out = np.zeros_like(pose)
        out[:, 0], out[:, 1], out[:, 2] = pose[:, 0], -pose[:, 1], pose[:, 2]
        c, s = np.cos(-yaw), np.sin(-yaw)
        out[:, 3], out[:, 4], out[:, 6], out[:, 7], out[:, 11] = c, -s, s, c, 1.0
        return out
    for g, p, r, tm in ((scen[0], scen[1], scen[2], TIMING), (scen[0], scen[1], scen[3], HEAVY), (fuzz[0], fuzz[1], fuzz[2], HEAVY)):
        m = ut.unicycle_plan_timed(p, tm, mirror(g["right0"]), mirror(g["left0"]), g["goals"] * np.array([1.0, -1.0]), 1 - g["first_side"])
        ok = np.minimum(r["margin"], m["margin"]) >= MARGIN
        assert ok.mean() >= 0.98
        for k in ("n_steps", "status", "ss_ticks", "ds_ticks"):
            assert np.array_equal(m[k][ok], r[k][ok]), k
        taken = (np.arange(p["max_steps"])[None, :] < r["n_steps"][:, None]) & ok[:, None]
        assert np.array_equal(m["side"][taken], 1 - r["side"][taken])
        err = np.abs(m["target"][taken] - r["target"][taken] * np.array([1.0, -1.0, -1.0])).max()
        print("mirror", err)
        assert err <= 1e-12


def test_decision_margins_stay_inside_the_caps(scen, fuzz):
    """the restatement alone, for the committed seeds: no scenario robot and at most 2 % of the fuzz batch is decided by less than 1e-9 -
    feasibility of any candidate, the score's gap between the step taken and any other feasible candidate, the two arrival thresholds"""
    print("scenario", np.sort(scen[2]["margin"])[:3], np.sort(scen[3]["margin"])[:3], "fuzz", np.sort(fuzz[2]["margin"])[:5])
    assert (scen[2]["margin"] >= MARGIN).all() and (scen[3]["margin"] >= MARGIN).all()
    assert (fuzz[2]["margin"] < MARGIN).mean() <= 0.02
    # the margin sees a tie: two candidates of one score (no weights at all: every feasible candidate scores 0, the first one is taken)
    g, p = scen[0], scen[1]
    flat = _plan(p, dict(TIMING, time_weight=0.0, position_weight=0.0), g)
    moved = flat["n_steps"] > 0
    assert (flat["margin"][moved] == 0.0).all() and all(s["m"] == s["feasible"][0] for i in np.nonzero(moved)[0] for s in flat["steps"][i])


def test_refusals_without_a_device(wca, scen):
    """what the timed forms refuse before they look for a device: a NULL timing, tick counts out of order or below 2, a negative or
    non-finite weight, a ratio that is not a positive number, missing duration rows - and everything the untimed forms refuse"""
    lib = wca.capi.lib()
    g = scen[0]
    pl = wca.UnicyclePlanner(**SCEN)
    B, K = 13, SCEN["max_steps"]
    o = dict(n_steps=np.full(B, 77, np.int32), side=np.full((B, K), 9, np.uint8), target=np.full((B, K, 3), 5.0), status=np.full(B, 77, np.int32),
             desired_point=np.full((B, 2), 5.0), unicycle_end=np.full((B, 3), 5.0))
    ss, ds = np.full((B, K), 77, np.int32), np.full((B, K), 77, np.int32)
    a = {k: np.ascontiguousarray(g[k]) for k in ("left0", "right0", "goals", "first_side")}

    def call(timing=TIMING, null_tm=False, rows=(True, True), batch=B, goals=None, handle=True, device=True):
        """the codes of the host form and - only for calls it refuses before it launches, the arrays being HOST memory - the device form"""
        tm = wca.capi.UnicycleTiming(*(timing[k] for k, _ in wca.capi.UnicycleTiming._fields_))
        gl = a["goals"] if goals is None else np.ascontiguousarray(goals)
        ins = wca.capi.UnicycleInputs(a["left0"].ctypes.data, a["right0"].ctypes.data, gl.ctypes.data, a["first_side"].ctypes.data)
        outs = wca.capi.UnicycleOutputs(**{k: v.ctypes.data for k, v in o.items()})
        args = (pl._h if handle else None, None if null_tm else C.byref(tm), batch, C.byref(ins), C.byref(outs),
                ss.ctypes.data if rows[0] else None, ds.ctypes.data if rows[1] else None)
        rc = lib.wcqp_unicycle_plan_timed_host(*args)
        return (rc, lib.wcqp_unicycle_plan_timed_device(*args, None)) if device else rc
    both = (WCQP_E_INVALID, WCQP_E_INVALID)
    assert call(null_tm=True) == both and call(handle=False) == both and call(batch=-1) == both and call(batch=0) == (0, 0)
    assert call(rows=(False, True)) == both and call(rows=(True, False)) == both
    for bad in (dict(min_step_ticks=26), dict(min_step_ticks=1), dict(min_step_ticks=0, nominal_step_ticks=0, max_step_ticks=0), dict(max_step_ticks=24),
                dict(nominal_step_ticks=31), dict(time_weight=-1.0), dict(position_weight=-1e-300), dict(time_weight=np.nan), dict(position_weight=np.inf),
                dict(switch_over_swing_ratio=np.nan), dict(switch_over_swing_ratio=0.0), dict(switch_over_swing_ratio=-0.7),
                dict(switch_over_swing_ratio=np.inf)):
        assert call(timing=dict(TIMING, **bad)) == both, bad
    # the host form reads its arrays first, as the untimed one does; nothing is written by any refused call
    assert call(goals=np.where(np.arange(B)[:, None] == 6, np.nan, a["goals"]), device=False) == WCQP_E_INVALID
    assert (o["n_steps"] == 77).all() and (o["status"] == 77).all() and (o["target"] == 5.0).all() and (ss == 77).all() and (ds == 77).all()
    # what is allowed: min = nominal = max = 2, zero weights
    ok = dict(TIMING, min_step_ticks=2, nominal_step_ticks=2, max_step_ticks=2, time_weight=0.0, position_weight=0.0)
    rc = call(timing=ok, device=False)
    if wca.device_count() == 0:
        assert rc == WCQP_E_HIP and call(device=False) == WCQP_E_HIP          # no device: an error, never a plan from somewhere else
    else:
        assert rc == 0


def test_binding_takes_the_timing(wca, scen):
    g = scen[0]
    pl = wca.UnicyclePlanner(**SCEN)
    assert pl.timing is None
    with pytest.raises(TypeError):
        pl.plan_host(g["left0"], g["right0"], g["goals"], g["first_side"], timing=dict(step_time=3))
    with pytest.raises(TypeError):
        wca.UnicyclePlanner(timing=dict(nominal=3))
    if wca.device_count() == 0:
        with pytest.raises(wca.WcqpError, match="invalid|INVALID"):         # (refused before a device is looked for)
            pl.plan_host(g["left0"], g["right0"], g["goals"], g["first_side"], timing=dict(TIMING, min_step_ticks=1))
    empty = pl.plan_host(g["left0"][:0], g["right0"][:0], g["goals"][:0], g["first_side"][:0], timing=TIMING)
    assert empty["ss_ticks"].shape == (0, 8) and empty["ds_ticks"].dtype == np.int32
    assert "ss_ticks" not in pl.plan_host(g["left0"][:0], g["right0"][:0], g["goals"][:0], g["first_side"][:0])
    # plannerParams.ini's values: durations in seconds there, ticks of dT here
    ini = dict(unicycleGain=10.0, referencePosition=(0.1, 0.0), minStepDuration=0.8, maxStepDuration=1.0, nominalDuration=0.9, timeWeight=2.5,
               positionWeight=1.0, switchOverSwingRatio=0.7)
    a = wca.UnicyclePlanner.from_ini_values(ini)
    assert a.timing == wca.UnicyclePlanner.TIMING_DEFAULTS == dict(min_step_ticks=80, max_step_ticks=100, nominal_step_ticks=90, time_weight=2.5,
                                                                   position_weight=1.0, switch_over_swing_ratio=0.7)
    b = wca.UnicyclePlanner.from_ini_values(dict(ini, nominalDuration=0.25, minStepDuration=0.2, maxStepDuration=0.3), dT=0.005)
    assert (b.timing["min_step_ticks"], b.timing["nominal_step_ticks"], b.timing["max_step_ticks"]) == (40, 50, 60)
    assert wca.UnicyclePlanner.from_ini_values(dict(unicycleGain=10.0)).timing is None


# ---------------------------------------------------------------------------------------------------------------- GPU

def _device(wca, pl, tm, g, B=None, stream=0, overwrite=False):
    """wcqp_unicycle_plan_timed_device on device arrays -> the outputs as numpy arrays (prefilled with junk: every row is written).  The
    arrays come from the HIP runtime libwcqp itself is linked against, reached through the library's own handle: one runtime in the process."""
    L = wca.capi.lib()
    L.hipMalloc.argtypes, L.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p]
    L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    B = len(g["goals"]) if B is None else B
    K = pl.max_steps
    host = {k: np.ascontiguousarray(g[k][:B]) for k in ("left0", "right0", "goals", "first_side")}
    host.update(n_steps=np.full(B, 77, np.int32), side=np.full((B, K), 9, np.uint8), target=np.full((B, K, 3), np.nan), status=np.full(B, 77, np.int32),
                desired_point=np.full((B, 2), np.nan), unicycle_end=np.full((B, 3), np.nan), ss_ticks=np.full((B, K), 77, np.int32),
                ds_ticks=np.full((B, K), 77, np.int32))
    assert host["first_side"].dtype == np.uint8 and host["goals"].dtype == np.float64
    ptr = {}
    try:
        for k, v in host.items():
            ptr[k] = C.c_void_p()
            assert L.hipMalloc(C.byref(ptr[k]), max(v.nbytes, 8)) == 0
            assert L.hipMemcpy(ptr[k], v.ctypes.data, v.nbytes, 1) == 0
        t = wca.capi.UnicycleTiming(*(tm[k] for k, _ in wca.capi.UnicycleTiming._fields_))
        ins = wca.capi.UnicycleInputs(ptr["left0"], ptr["right0"], ptr["goals"], ptr["first_side"])
        outs = wca.capi.UnicycleOutputs(**{k: ptr[k] for k in OUT[:6]})
        wca.capi.check(L.wcqp_unicycle_plan_timed_device(pl._h, C.byref(t), B, C.byref(ins), C.byref(outs), ptr["ss_ticks"], ptr["ds_ticks"], stream or None))
        if overwrite:          # the three structs are read at the call
            C.memset(C.byref(ins), 0, C.sizeof(ins)); C.memset(C.byref(outs), 0, C.sizeof(outs)); C.memset(C.byref(t), 0, C.sizeof(t))
        wca.capi.stream_synchronize(stream)
        for k in OUT:
            assert L.hipMemcpy(host[k].ctypes.data, ptr[k], host[k].nbytes, 2) == 0
    finally:
        for v in ptr.values():
            L.hipFree(v)
    return {k: host[k] for k in OUT}


def _against_the_restatement(dev, r, rows=None):
    """decisions and durations equal, numbers to 1e-9 - on `rows` (default: all)"""
    rows = np.arange(len(r["n_steps"])) if rows is None else rows
    for k in ("n_steps", "side", "status", "ss_ticks", "ds_ticks"):
        assert np.array_equal(dev[k][rows], r[k][rows]), k
    for k in ("target", "desired_point", "unicycle_end"):
        err = np.abs(dev[k][rows] - r[k][rows]).max()
        print(k, err)
        assert err <= 1e-9, (k, err)


def _same_rows(a, b, rows):
    for k in OUT:
        assert np.array_equal(a[k][rows], b[k][rows]), k


@pytest.fixture(scope="module")
def scen_dev(wca, scen):
    return _device(wca, wca.UnicyclePlanner(**SCEN), TIMING, scen[0])


@pytest.mark.gpu
def test_scenario_matches_the_restatement(wca, scen, scen_dev):
    """13 robots, K = 8, 20 / 25 / 30 ticks: n_steps, side, status and both duration rows equal, target, desired_point and unicycle_end
    to 1e-9 (the gap printed: both sides do the same RK4 in binary64) - at the reference's weights and at the heavy position weight"""
    _against_the_restatement(scen_dev, scen[2])
    _against_the_restatement(_device(wca, wca.UnicyclePlanner(**SCEN), HEAVY, scen[0]), scen[3])
    assert all(np.isfinite(scen_dev[k]).all() for k in OUT)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [70, 1])
def test_other_batch_sizes_are_bit_identical(wca, scen, scen_dev, B):
    """a full wave plus six lanes, and one robot: the first 13 rows equal the 13-robot run bit for bit; rows of steps not taken are zero"""
    g = wca.synth.synth_goal_batch(B)
    assert np.array_equal(g["goals"][:13], scen[0]["goals"][:B]) and np.array_equal(g["left0"][:13], scen[0]["left0"][:B])
    d = _device(wca, wca.UnicyclePlanner(**SCEN), TIMING, g)
    _same_rows(d, scen_dev, np.arange(min(B, 13)))
    idle = np.arange(SCEN["max_steps"])[None, :] >= d["n_steps"][:, None]
    for k in ("side", "target", "ss_ticks", "ds_ticks"):
        assert not d[k][idle].any(), k
    taken = d["ss_ticks"][~idle] + d["ds_ticks"][~idle]
    assert (taken >= TIMING["min_step_ticks"]).all() and (taken <= TIMING["max_step_ticks"]).all() and (d["ss_ticks"][~idle] >= 1).all()
    assert all(np.isfinite(d[k]).all() for k in OUT) and (d["status"] <= up.STUCK).all() and (d["n_steps"] <= SCEN["max_steps"]).all()


@pytest.mark.gpu
def test_stuck_robots_next_to_healthy_ones(wca, scen):
    """a turn of 1 rad/s passes max_angle_variation before min_step_ticks samples: the turning robots have no feasible candidate and end
    STUCK with no step; the others equal the batch in which the stuck ones stand still (goal 0, 0), bit for bit"""
    g = scen[0]
    par = dict(SCEN, max_angular_velocity=1.0)
    r = _plan(_params(wca, **par), TIMING, g)
    stuck = r["status"] == up.STUCK
    assert 3 <= stuck.sum() <= 9 and (r["margin"] >= MARGIN).all()
    pl = wca.UnicyclePlanner(**par)
    d = _device(wca, pl, TIMING, g)
    _against_the_restatement(d, r)
    assert (d["n_steps"][stuck] == 0).all() and not d["target"][stuck].any() and not d["ss_ticks"][stuck].any()
    calm = dict(g, goals=np.where(stuck[:, None], 0.0, g["goals"]))
    _same_rows(d, _device(wca, pl, TIMING, calm), np.nonzero(~stuck)[0])


@pytest.mark.gpu
def test_a_nan_goal_on_the_device_form(wca, scen, scen_dev):
    """robots with a NaN goal, an Inf sole and a first_side of 2: INVALID_INPUT with zero steps and zero rows; the wave's other robots are
    bit-identical and nothing stored is non-finite"""
    g = {k: np.array(v, copy=True) for k, v in scen[0].items() if k != "case"}
    g["goals"][4, 1] = np.nan; g["left0"][9, 6] = np.inf; g["first_side"][11] = 2
    bad = np.array([4, 9, 11])
    d = _device(wca, wca.UnicyclePlanner(**SCEN), TIMING, g)
    assert (d["status"][bad] == up.INVALID_INPUT).all() and (d["n_steps"][bad] == 0).all()
    for k in ("side", "target", "desired_point", "unicycle_end", "ss_ticks", "ds_ticks"):
        assert not d[k][bad].any(), k
    _same_rows(d, scen_dev, np.setdiff1d(np.arange(13), bad))
    assert all(np.isfinite(d[k]).all() for k in OUT)


@pytest.mark.gpu
def test_forms_agree(wca, scen, scen_dev):
    """the host form, and the device form on a non-blocking stream with the host structs overwritten as soon as the call returns: bit for
    bit; the untimed form of the same handle is untouched by the timing"""
    g = scen[0]
    pl = wca.UnicyclePlanner(**SCEN)
    h = pl.plan_host(g["left0"], g["right0"], g["goals"], g["first_side"], timing=TIMING)
    _same_rows(h, scen_dev, np.arange(13))
    s = wca.capi.stream_create()
    try:
        _same_rows(_device(wca, pl, TIMING, g, stream=s, overwrite=True), scen_dev, np.arange(13))
    finally:
        wca.capi.stream_destroy(s)
    with pytest.raises(wca.WcqpError, match="invalid|INVALID"):
        pl.plan_host(g["left0"], g["right0"], np.where(np.arange(13)[:, None] == 6, np.nan, g["goals"]), g["first_side"], timing=TIMING)
    # step_ticks is not read by the timed form (1 here), and is by the untimed one: D = 25 gives the untimed scenario's plan
    u = wca.UnicyclePlanner(**dict(SCEN, step_ticks=25)).plan_host(g["left0"], g["right0"], g["goals"], g["first_side"])
    ru = up.unicycle_plan(_params(wca, **dict(SCEN, step_ticks=25)), g["left0"], g["right0"], g["goals"], g["first_side"])
    assert np.array_equal(u["n_steps"], ru["n_steps"]) and np.array_equal(u["status"], ru["status"]) and "ss_ticks" not in u


@pytest.mark.gpu
def test_fuzz_against_the_restatement(wca, fuzz):
    """256 robots, goals from the disc of 0.4 m, any heading, the heavy position weight: robots the restatement decided by 1e-9 or more
    agree with it, and those are at least 98 % of the batch"""
    g, p, r = fuzz
    d = _device(wca, wca.UnicyclePlanner(**SCEN), HEAVY, g)
    keep = r["margin"] >= MARGIN
    print("left out", int((~keep).sum()), "of", FUZZ_B)
    assert (~keep).mean() <= 0.02
    _against_the_restatement(d, r, np.nonzero(keep)[0])
    assert all(np.isfinite(d[k]).all() for k in OUT)


def _ik(wca, robot):
    R = robots.ROBOTS[robot]
    return wca.IkSolver(form=wca.IK_FORM_QPOASES, neck_weight=R["neck_weight"] * np.eye(3), joint_reg_weights=np.array(R["reg_w"], float),
                        joint_reg_gains=np.array(R["reg_k"], float), joint_reg_rad=np.deg2rad(wca.synth.WALK_POSTURE_DEG),
                        v_max=wca.synth.WALK_VMAX.copy(), k_pos_com=R["k_pos_com"], k_pos_foot=R["k_pos_foot"], k_att_foot=R["k_att_foot"],
                        k_neck=R["k_neck"])


def _pipe(wca, B, robot, **kw):
    """a reactive handle with gain scheduling and its own (fused) kinematics; kw: planned_trajectories=True, or the streamed form"""
    R = robots.ROBOTS[robot]
    return wca.TickPipeline(B, MAXT, wca.MpcSolver(horizon=50), _ik(wca, robot), log_ticks=MAXT, k_com=R["k_com"], k_zmp=R["k_zmp"],
                            kin=wca.KinModel(wca.synth.icub_like_model()), dcm_controller="reactive", k_dcm=K_DCM, zmp_gain_scheduling=True,
                            **zg.ZMP_SCHEDULE[robot], neck_additional_rotation=np.array(R["additional_rotation"]), **kw)


def _run_against(out, ref, n=MAXT):
    assert (ref["ik_fail"] == 0).all() and (out["ik_fail"] == 0).all()
    for k in KEYS:
        a, b = (out[k][:n], ref[k][:n]) if k.endswith("_log") else (out[k], ref[k])
        err = np.abs(a - b).max()
        print(k, err)
        assert err <= 1e-9, (k, err)
    assert np.array_equal(out["mpc_fail"], ref["mpc_fail"])


@pytest.mark.gpu
def test_upload_goal_and_replan_goal_with_timing_end_to_end(wca, walk3):
    """upload_goal(timing=) and 1 + the whole plan of run on a planned handle (reactive law, fused kinematics) against oracle/tick_spec.py
    on the restated timed plan to 1e-9; then, on a second handle, replan_goal(timing=) for robot 2 inside a double support of its timed
    timeline (-1 for the others), run on, against the restatement on the stitched plan; the robots with -1 are bit-identical to the run
    without the replan, plan_timed is reported, and the two replans that know one common timing are refused with the plan unchanged"""
    w = walk3
    fs = w["fs"]
    pl = wca.UnicyclePlanner(**WALK)
    kw = dict(lift=fs["lift"], zmp_delta_left=fs["zmp_delta_left"], zmp_delta_right=fs["zmp_delta_right"], timing=WALK_TIMING)
    a = _pipe(wca, 3, w["robot"], planned_trajectories=True)
    assert a.info()["plan_timed"] is False
    got = a.upload_goal(fs, GOALS0, pl, 1, FIRST_DS, **kw)
    _against_the_restatement(got, w["r0"])
    assert a.info()["plan_timed"] is True and a.info()["kin_handoff"] == "fused" and a.info()["dcm_controller"] == "reactive"
    a.run(1)
    a.run(MAXT - 1)
    out_a = a.download()
    _run_against(out_a, w["ref0"])
    b = _pipe(wca, 3, w["robot"], planned_trajectories=True)
    b.upload_goal(fs, GOALS0, pl, 1, FIRST_DS, **kw)
    b.run(w["m_replan"])
    before = b.plan_window()
    with pytest.raises(wca.WcqpError, match="unsupported|UNSUPPORTED"):
        b.replan_goals(np.zeros((3, 2)), pl, FD_REPLAN)
    with pytest.raises(wca.WcqpError, match="unsupported|UNSUPPORTED"):
        b.replan_footsteps(w["M"], {k: w["rp"][k] for k in ("n_steps", "side", "target")}, FD_REPLAN)
    after = b.plan_window()
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    goals1 = np.array([[9.0, 9.0], [np.nan, 0.0], GOAL1])                     # (rows of robots that keep their plan are not read)
    got = b.replan_goal(w["M"], goals1, pl, 1, FD_REPLAN, timing=WALK_TIMING)
    assert (got["status"][:2] == -1).all() and not got["target"][:2].any() and not got["ss_ticks"][:2].any()
    _against_the_restatement(got, dict(w["r1"], **{k: np.concatenate([got[k][:2], w["r1"][k]]) for k in OUT}), np.array([2]))
    b.run(MAXT - w["m_replan"])
    out_b = b.download()
    _run_against(out_b, w["ref1"])
    for k in KEYS:
        ax = 1 if k in ("u0_log", "dq_log") else 0
        assert np.array_equal(np.take(out_a[k], [0, 1], axis=ax), np.take(out_b[k], [0, 1], axis=ax)), k
    win = b.plan_window()
    for k in ("left_traj", "right_traj", "ref_traj", "dcm_vel_traj"):
        err = np.abs(win[k] - w["plan1"][k]).max()
        print(k, err)
        assert err <= 1e-9, (k, err)
    assert np.array_equal(win["contact"], w["plan1"]["contact"]) and b.info()["plan_timed"] is True


@pytest.mark.gpu
def test_the_position_tick_and_a_resident_plan_take_the_timed_goal(wca, walk3):
    """A timed plan on the POSITION tick - its own tests' 13 prepared robots, their three steps given durations of their own: the plan
    matches the restatement and the whole run equals, bit for bit, that of a POSITION handle given the plan through the classic upload,
    with no IK failure - and the walk test's upload_goal(timing=) as the resident plan of a streamed handle, staged tick by tick and fed
    the restatement's internal-plant states for 45 ticks (into the first timed single support), against oracle/tick_spec.py to 1e-9"""
    w = walk3
    fs, robot, n = w["fs"], w["robot"], 45
    R = robots.ROBOTS[robot]
    pl = wca.UnicyclePlanner(**WALK)
    kw = dict(lift=fs["lift"], zmp_delta_left=fs["zmp_delta_left"], zmp_delta_right=fs["zmp_delta_right"], timing=WALK_TIMING)
    assert FIRST_DS + 10 < n and w["plan0"]["contact"][0, n - 1] & 3 != 3
    ref = _pipe(wca, 3, robot, planned_trajectories=True)
    ref.upload_goal(fs, GOALS0, pl, 1, FIRST_DS, **kw)
    w_ref = ref.plan_window()
    # the POSITION tick, on the scenario its own tests walk (13 prepared robots, 70 ticks, CoM height 0.42 m): its three steps of 15 + 10
    # stages given durations of their own
    sc = pk.scenario()
    pfs = sc["fs"]
    dur = dict(ss_ticks=np.tile(np.array([12, 17, 9], np.int32), (pk.B13, 1)) + (np.arange(pk.B13)[:, None] % 3).astype(np.int32),
               ds_ticks=np.tile(np.array([8, 5, 11], np.int32), (pk.B13, 1)) + (np.arange(pk.B13)[:, None] % 2).astype(np.int32))
    assert pfs["side"].shape == (pk.B13, 3)

    def position_pipe():
        Rk = robots.ROBOTS[pk.ROBOT]
        return wca.TickPipeline(pk.B13, pk.T, wca.MpcSolver(horizon=pk.N, com_height=pk.H), _ik(wca, pk.ROBOT), log_ticks=pk.T, k_com=Rk["k_com"],
                                k_zmp=Rk["k_zmp"], kin=wca.KinModel(sc["model"]), planned_trajectories=True, neck_additional_rotation=pk.ADD_ROT,
                                ik_mode="position", position_ik=dict(q_reg=sc["q_reg"], max_iter=30), **pk.controller_kwargs("reactive_gs"))
    a, b = position_pipe(), position_pipe()
    a.upload_footsteps(pfs, dict(pfs, **dur))
    wa = a.plan_window()
    restated = ft.footstep_plan_timed(dict(pfs, **dur), pfs["state0"], pk.T + pk.N + 1, pk.T, com_height=pk.H)
    assert np.array_equal(wa["contact"], restated["contact"]) and np.abs(wa["ref_traj"] - restated["ref_traj"]).max() <= 1e-9
    assert a.info()["plan_timed"] is True and a.info()["ik_mode"] == "position"
    b.upload(dict(pfs, ref_traj=wa["ref_traj"], dcm0=wa["ref_traj"][:, 0].copy(), u_init=wa["u_init"]), dcm_vel_traj=wa["dcm_vel_traj"],
             left_traj=wa["left_traj"], right_traj=wa["right_traj"], left_twist=wa["left_twist"], right_twist=wa["right_twist"], contact=wa["contact"],
             com_height_traj=wa["com_height"], com_height_vel=wa["com_height_vel"])
    a.run(pk.T); b.run(pk.T)
    oa, ob = a.download(), b.download()
    assert (oa["ik_fail"] == 0).all() and np.abs(oa["q_des"] - pfs["q0"]).max() > 1e-3 and (np.unique(wa["contact"][:, :pk.T] & 3).size == 3)
    for k in oa:
        assert np.array_equal(np.asarray(oa[k]), np.asarray(ob[k])), k
    # a resident plan: the stage out of the timed plan every tick, the plant states of the restatement's internal run as the feedback
    s = _pipe(wca, 3, robot, external_feedback=True, streamed_trajectories=True, resident_plan=True)
    s.upload_goal(fs, GOALS0, pl, 1, FIRST_DS, **kw)
    ws = s.plan_window()
    for k in ("left_traj", "right_traj", "contact", "ref_traj", "dcm_vel_traj", "hull_A", "hull_b", "hull_nc"):
        assert np.array_equal(ws[k], w_ref[k]), k
    assert s.info()["plan_timed"] is True and s.info()["resident_plan"] is True
    ext = stt.external_of(w["ref0"])
    for t in range(n):
        s.set_desired_from_plan()
        s.set_feedback_host(ext["dcm"][t], ext["com"][t], ext["zmp"][t], None)
        s.run(1)
    _run_against_first(s.download(), w["ref0"], n)


def _run_against_first(out, ref, n):
    """the first n ticks' logs of a run against a longer reference run"""
    assert (out["ik_fail"] == 0).all()
    for k in ("u0_log", "dq_log"):
        err = np.abs(out[k][:n] - ref[k][:n]).max()
        print(k, err)
        assert err <= 1e-9, (k, err)
