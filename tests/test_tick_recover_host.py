"""Stopped robots stood up on the device (wcqp_tick_recover_robots), without a device: the ABI, what the binding refuses
before it reaches the library, the target rule of helpers/plan_recover.py on helpers/footstep_plan.py's plan, and THE CONDITION the GPU
tests of tests/test_tick_recover.py rest on - the posture IK converges from the joints the stopped robots stopped at."""
import ctypes as C
import functools

import numpy as np
import pytest
from walking_controllers_amd.capi import E_INVALID as WCQP_E_INVALID

import robots
import test_tick_restart as rt
from helpers import footstep_plan as fp
from helpers import footstep_replan as fr
from helpers import plan_recover as prc
from helpers import plan_restart as prs
from helpers import planned_tick as pt
from helpers import position_tick as pk
from helpers import prepare_spec as ps
from helpers import streamed_tick as stt

B13, MAXT, T, S = fr.B13, fr.MAXT, fr.MAXT + 51, 41


def test_the_symbols_exist_and_refuse_null(wca):
    capi = wca.capi
    lib = capi.lib()
    for s in ("wcqp_tick_recover_robots", "wcqp_tick_get_recover_result"):
        assert s in capi.ABI_SYMBOLS and getattr(lib, s)
    assert (capi.RECOVER_KEPT, capi.RECOVER_NOT_STOPPED, capi.RECOVER_NOT_STANDING) == (prc.KEPT, prc.NOT_STOPPED, prc.NOT_STANDING) == (-1, -2, -3)
    assert (prc.KEEP, prc.ALWAYS, prc.IF_STOPPED) == (capi.TICK_RESTART_KEEP, capi.TICK_RESTART_ALWAYS, capi.TICK_RESTART_IF_STOPPED)
    assert lib.wcqp_tick_recover_robots(None, None, C.byref(capi.TickRecover()), None) == WCQP_E_INVALID
    assert lib.wcqp_tick_get_recover_result(None, C.byref(capi.TickRecoverResult())) == WCQP_E_INVALID
    assert [k for k, _ in capi.TickRecover._fields_] == ["mode", "left_d", "right_d", "com_d", "Rd_neck", "q_guess", "dcm0", "u_init"]
    assert [k for k, _ in capi.TickRecoverResult._fields_] == ["restarted", "stopped_ticks", "status", "iters", "residual", "stage"]
    assert "wcqp_tick_recover" in capi.ABI_STRUCTS and "WCQP_RECOVER_NOT_STANDING" in capi.ABI_CONSTANTS


def test_binding_refusals_without_a_device(wca):
    """What TickPipeline.recover_robots refuses before it reaches the library: a handle without a plan, something that is no
    PrepareSolver, arrays of the wrong shape."""
    pipe = object.__new__(wca.TickPipeline)
    pipe.planned, pipe.batch, pipe._h = False, 3, None
    prep = object.__new__(wca.PrepareSolver)
    prep._h = None
    m = np.zeros(3, np.uint8)
    with pytest.raises(ValueError):
        pipe.recover_robots(m, prep)
    pipe.planned = True
    with pytest.raises(TypeError):
        pipe.recover_robots(m, None)
    for bad in (dict(left_d=np.zeros((3, 11)), right_d=np.zeros((3, 12))), dict(com_d=np.zeros((3, 2))), dict(Rd_neck=np.zeros((3, 3, 3))),
                dict(q_guess=np.zeros((4, 23))), dict(dcm0=np.zeros((3, 3))), dict(u_init=np.zeros(3))):
        with pytest.raises(AssertionError):
            pipe.recover_robots(m, prep, **bad)
    with pytest.raises(AssertionError):
        pipe.recover_robots(np.zeros(4, np.uint8), prep)
    pipe._h = prep._h = None      # (nothing to destroy)


def test_target_rule_on_the_restated_plan(wca):
    """helpers/plan_recover.targets on the small scenario's plan (first double support 20 stages, steps of 30 + 20): stage 10 lies in the
    first double support, stage 41 mid-swing of every robot that walks, stage 60 in the double support behind the first step, and the
    robots without steps stand throughout.  The soles and the height are the stage's, the CoM x, y are prs.standing_zmp of those soles
    bit for bit - at stage 10, where nothing has moved, the standing ZMP of state0 - and agree with the plan's own ZMP of a standing stage."""
    fs = fr.small_footsteps(wca, pt)
    plan = fp.footstep_plan(fs, fs["state0"], T, MAXT)
    dl, dr = fs["zmp_delta_left"], fs["zmp_delta_right"]
    walks = fs["n_steps"] > 0
    assert walks.sum() >= 9 and (~walks).sum() >= 2
    for stage, want in ((10, np.ones(B13, bool)), (S, ~walks), (60, np.ones(B13, bool))):
        t = prc.targets(plan, stage, dl, dr)
        assert np.array_equal(t["standing"], want), stage
        assert np.array_equal(t["standing"], (plan["contact"][:, stage] & 3) == 3)
        assert np.array_equal(t["left_d"], plan["left_traj"][:, stage]) and np.array_equal(t["right_d"], plan["right_traj"][:, stage])
        assert np.array_equal(t["com_d"][:, 2], plan["com_height_traj"][:, stage])
        for i in range(B13):
            row = np.zeros(87); row[24:36] = plan["left_traj"][i, stage]; row[36:48] = plan["right_traj"][i, stage]
            assert np.array_equal(t["com_d"][i, :2], prs.standing_zmp(row, dl, dr)), (stage, i)
    t = prc.targets(plan, 10, dl, dr)
    for i in range(B13):
        assert np.array_equal(t["com_d"][i, :2], prs.standing_zmp(fs["state0"][i], dl, dr)), i
    last = prc.targets(plan, MAXT, dl, dr)
    for i in np.nonzero(~walks)[0]:
        assert last["standing"][i] and np.abs(last["com_d"][i, :2] - plan["zmp_ref"][i, MAXT]).max() <= 1e-15, i
    # the window's key for the height, and the restart's own restatement: a restarted robot's stage S gives back the rows it stands on
    win = dict(left_traj=plan["left_traj"], right_traj=plan["right_traj"], contact=plan["contact"], com_height=plan["com_height_traj"])
    assert np.array_equal(prc.targets(win, S, dl, dr)["com_d"], prc.targets(plan, S, dl, dr)["com_d"])
    st = np.roll(fs["state0"], -1, axis=0)
    again = prc.targets(prs.restart({k: plan[k] for k in fr.PLAN_KEYS}, range(B13), S, st, dl, dr), S, dl, dr)
    assert again["standing"].all() and np.array_equal(again["left_d"], st[:, 24:36]) and np.array_equal(again["com_d"][:, 2], st[:, 68])
    assert np.array_equal(again["com_d"][:, :2], np.array([prs.standing_zmp(st[i], dl, dr) for i in range(B13)]))


def _start_targets(fs, i):
    """the recover call of the GPU tests: back onto the start soles, the start CoM at the start height, no neck target"""
    return dict(left_d=fs["state0"][i, 24:36], right_d=fs["state0"][i, 36:48], com_d=np.array([*fs["com0"][i], fs["state0"][i, 68]]), Rd_neck=None)


def test_the_posture_ik_converges_from_where_the_velocity_robots_stopped(wca, qs):
    """THE CONDITION of tests/test_tick_recover.py on the planned reactive handle.  oracle/tick_spec.run_ticks walks the six robots whose
    first step lies out of reach to tick 41: all of them are stopped there.  From the joints each stopped at, helpers/prepare_spec.solve
    towards the start soles and the start CoM ends SOLVED within the solver's max_iter (100, PrepareSolver's default) - and a CoM one metre
    up, the unsolvable target of the GPU tests, does not."""
    from oracle import tick_spec as ts
    fs = rt._unreachable(fr.small_footsteps(wca, pt))
    plan = fp.footstep_plan(fs, fs["state0"], T, MAXT)
    sel = list(rt.BAD)
    sub = {k: (v[sel] if isinstance(v, np.ndarray) and v.shape[:1] == (B13,) else v) for k, v in fs.items()}
    pl = {k: v[sel] for k, v in plan.items() if isinstance(v, np.ndarray) and v.shape[:1] == (B13,)}
    R = robots.ROBOTS[rt.ROBOT]
    ipar = robots.ik_params(qs, rt.ROBOT, v_max=wca.synth.WALK_VMAX.copy())
    ipar.joint_reg_deg = wca.synth.WALK_POSTURE_DEG.copy()
    d = dict(sub, ref_traj=pl["ref_traj"], dcm_vel_traj=pl["dcm_vel_traj"], dcm0=pl["ref_traj"][:, 0].copy(), u_init=pl["zmp_ref"][:, 0].copy())
    ref = ts.run_ticks(ts.TickParams(horizon=rt.N, k_com=R["k_com"], k_zmp=R["k_zmp"], noise=0.0), d, S, ipar, kin_model=wca.synth.icub_like_model(),
                       foot_rect=wca.synth.FOOT_RECT, stages=stt.stages_of(pl, S), neck_additional_rotation=R["additional_rotation"],
                       dcm_controller="reactive", k_dcm=rt.K_DCM, dcm_vel=pl["dcm_vel_traj"])
    print("the oracle's ik_fail at tick", S, ref["ik_fail"])
    assert (ref["ik_fail"] > 0).all()
    model, par = wca.synth.icub_like_model(), ps.Params(q_reg=np.deg2rad(wca.synth.WALK_POSTURE_DEG))
    assert par.max_iter == 100
    for n, i in enumerate(sel):
        s = ps.solve(model, _start_targets(fs, i), ref["q_des"][n], par)
        print(i, s["status"], s["iters"])
        assert s["status"] == ps.SOLVED and s["iters"] <= par.max_iter, i
    for n, i in ((sel.index(5), 5), (sel.index(12), 12)):
        tg = _start_targets(fs, i)
        tg["com_d"][2] = 1.0
        s = ps.solve(model, tg, ref["q_des"][n], par)
        print(i, "com z = 1:", s["status"], s["iters"])
        assert s["status"] in (ps.MAX_ITER, ps.INFEASIBLE), i


@functools.lru_cache(maxsize=None)
def _position_plan():
    sc = pk.scenario()
    fs = rt._unreachable(dict(sc["fs"]))
    return fs, fp.footstep_plan(fs, fs["state0"], pk.T + pk.N + 1, pk.T, com_height=pk.H)


@pytest.mark.parametrize("i", range(B13))
def test_the_posture_ik_converges_from_where_the_position_robots_stopped(i):
    """THE CONDITION on the POSITION handle, for every robot - at 12 iterations a tick the device stops more robots than the six sent out of
    reach, so whoever it finds stopped at tick 41 is covered.  The restatement of the tick (helpers/position_tick.walk, 12 iterations as the
    handle of the GPU tests) walks robot i to tick 41 - the six are stopped there -, and from the joints it holds then the posture IK ends
    SOLVED within 100 iterations."""
    sc = pk.scenario()
    fs, plan = _position_plan()
    par = ps.Params(q_reg=sc["q_reg"])
    w = pk.walk(pk.chain("mpc", i, plan=plan), fs["q0"][i], ps.Params(q_reg=sc["q_reg"], max_iter=12), n_ticks=S)
    s = ps.solve(sc["model"], _start_targets(fs, i), w["q_log"][S - 1], par)
    print(i, "stopped for", w["ik_fail"], "ticks;", s["status"], s["iters"])
    assert (w["ik_fail"] > 0 or i not in rt.BAD) and s["status"] == ps.SOLVED and s["iters"] <= par.max_iter
