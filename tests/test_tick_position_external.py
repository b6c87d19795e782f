"""The POSITION tick on the measured robot, from streamed stages (WCQP_TICK_OPT_POSITION_STREAMED, wcqp_tick_create_opts).
CPU: the option list's ABI and every refusal that needs no device, the binding's refusals, and the restatement (helpers/position_external.py)
as a fair yardstick - fed its own logs it is the internal one bit for bit, under the disturbed feed every tick is SOLVED and p_star moves.
GPU: the kernel against the restatement through the hand-over form, under the disturbed feed, from a resident plan, against the plan by the
stand-alone kinematics, through the sensor form, with rejected robots, in its forms and across a replan."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
from walking_controllers_amd.capi import E_HIP as WCQP_E_HIP, E_INVALID as WCQP_E_INVALID, E_UNSUPPORTED as WCQP_E_UNSUPPORTED

import robots
from helpers import footstep_replan as fr
from helpers import position_external as px
from helpers import position_tick as pk
from helpers import prepare_spec as ps
from helpers import streamed_tick as stt

B13, T, SEL = px.B13, px.T, px.SEL
RES, POS = px.OPT_RESIDENT_PLAN, px.OPT_POSITION_STREAMED


# ---------------------------------------------------------------------------------------------------------------- CPU

def _params(wca, **kw):
    """the wcqp_tick_params of a POSITION handle on streamed stages that every check in front of the device passes, with fields replaced
    (pik_*: of position_ik; ik_algorithm; horizon) -> (params, what it points to)"""
    cp = wca.capi
    R = robots.ROBOTS[pk.ROBOT]
    q_reg = np.ascontiguousarray(pk.scenario()["q_reg"])
    p = cp.TickParams(3, 0, T, T, 180, 110, R["k_com"], R["k_zmp"], 1e-4, 99, wca.MpcSolver(horizon=kw.pop("horizon", pk.N), com_height=pk.H).params,
                      px.ik_solver(wca).params, 0, 1, wca.KinModel(pk.scenario()["model"]).params,
                      (C.c_double * 8)(*np.asarray(wca.synth.FOOT_RECT, float).reshape(8)))
    p.plant, p.streamed_trajectories = 1, 1
    p.neck_additional_rotation = (C.c_double * 9)(*np.eye(3).reshape(9))
    p.ik_mode = cp.TICK_IK_POSITION
    p.position_ik = cp.PrepareParams(0.5, 1.0, 0.3, 1e-12, 1e-10, 30, q_reg.ctypes.data, None, None)
    keep = [q_reg]
    for k, v in kw.items():
        if k.startswith("pik_"):
            if isinstance(v, np.ndarray):
                keep.append(v)
                v = v.ctypes.data
            setattr(p.position_ik, k[4:], v)
        elif k == "ik_algorithm":
            p.ik.algorithm = v
        else:
            setattr(p, k, v)
    return p, keep


def _opts(wca, pairs):
    return (wca.capi.TickOption * max(len(pairs), 1))(*(wca.capi.TickOption(k, v) for k, v in pairs))


def _create(wca, pairs, n=None, null_opts=False, **kw):
    """wcqp_tick_create_opts -> the return code; a handle that comes back is checked to exist only with WCQP_OK, and destroyed"""
    lib = wca.capi.lib()
    p, keep = _params(wca, **kw)
    h = C.c_void_p()
    rc = lib.wcqp_tick_create_opts(C.byref(p), None if null_opts else _opts(wca, pairs), len(pairs) if n is None else n, C.byref(h))
    assert bool(h) == (rc == 0), (rc, h)
    if rc == 0:
        assert lib.wcqp_tick_destroy(h) == 0
    return rc


def test_option_list_abi_and_refusals_need_no_device(wca):
    """The new struct, macros and symbols are in the binding's ABI tables and exported; every refusal of wcqp_tick_create_opts comes back
    with its code and no handle, before anything touches the device (this test runs without one): the list itself, each key's values, what
    WCQP_TICK_OPT_POSITION_STREAMED needs, the position_ik checks, and POSITION on streamed stages or the EXTERNAL plant WITHOUT the option
    through all three entry points.  A fully valid block fails only where the device is asked for (WCQP_E_HIP here; a handle with one)."""
    cp = wca.capi
    lib = cp.lib()
    assert cp.VERSION == 400
    assert cp.ABI_STRUCTS["wcqp_tick_option"] is cp.TickOption and [k for k, _ in cp.TickOption._fields_] == ["key", "value"] and C.sizeof(cp.TickOption) == 8
    assert cp.ABI_CONSTANTS["WCQP_TICK_OPT_RESIDENT_PLAN"] == 1 == RES and cp.ABI_CONSTANTS["WCQP_TICK_OPT_POSITION_STREAMED"] == 2 == POS
    for sym in ("wcqp_tick_create_opts", "wcqp_tick_get_option"):
        assert sym in cp.ABI_SYMBOLS and getattr(lib, sym)
    # ---- the list itself
    p, keep = _params(wca)
    h = C.c_void_p()
    assert lib.wcqp_tick_create_opts(None, _opts(wca, [(POS, 1)]), 1, C.byref(h)) == WCQP_E_INVALID and not h
    assert lib.wcqp_tick_create_opts(C.byref(p), _opts(wca, [(POS, 1)]), 1, None) == WCQP_E_INVALID
    assert _create(wca, [(POS, 1)], n=-1) == WCQP_E_INVALID
    assert _create(wca, [], n=1, null_opts=True) == WCQP_E_INVALID
    for key in (0, 3, -1, 1 << 20):
        assert _create(wca, [(key, 1)]) == WCQP_E_INVALID, key
        assert _create(wca, [(POS, 1), (key, 0)]) == WCQP_E_INVALID, key
    assert _create(wca, [(POS, 1), (POS, 1)]) == WCQP_E_INVALID and _create(wca, [(RES, 0), (POS, 1), (RES, 0)]) == WCQP_E_INVALID
    for key in (RES, POS):
        for value in (2, -1):
            assert _create(wca, [(key, value)] + ([(POS, 1)] if key == RES else [])) == WCQP_E_INVALID, (key, value)
    assert lib.wcqp_tick_get_option(None, POS, C.byref(C.c_int32())) == WCQP_E_INVALID
    # ---- what the option needs
    on = [(POS, 1)]
    assert _create(wca, on, ik_mode=cp.TICK_IK_VELOCITY) == WCQP_E_UNSUPPORTED
    assert _create(wca, on, streamed_trajectories=0, plant=0, planned_trajectories=1) == WCQP_E_UNSUPPORTED      # a valid planned POSITION handle
    assert _create(wca, on, streamed_trajectories=0) == WCQP_E_UNSUPPORTED
    assert _create(wca, on, plant=0) == WCQP_E_UNSUPPORTED
    assert _create(wca, on, use_kinematics=0) == WCQP_E_UNSUPPORTED
    assert _create(wca, on, kin_handoff=wca.KIN_HANDOFF_DENSE) == WCQP_E_UNSUPPORTED and _create(wca, on, kin_handoff=wca.KIN_HANDOFF_COMPACT) == WCQP_E_UNSUPPORTED
    assert _create(wca, on, ik_algorithm=wca.IK_ALG_NULLSPACE_16L) == WCQP_E_UNSUPPORTED
    assert _create(wca, on, logger_ticks=4) == WCQP_E_UNSUPPORTED
    assert _create(wca, on, horizon=56) == WCQP_E_UNSUPPORTED                                   # the kGainsLdsStages rule of every streamed handle
    assert _create(wca, on, planned_trajectories=1) == WCQP_E_UNSUPPORTED
    assert _create(wca, on + [(RES, 1)], streamed_trajectories=0) == WCQP_E_UNSUPPORTED
    # ---- the position_ik checks apply unchanged
    for k in ("w_q", "w_n", "step_cap", "tol_step", "tol_constraint"):
        assert _create(wca, on, **{"pik_" + k: np.nan}) == WCQP_E_INVALID, k
    assert _create(wca, on, pik_max_iter=0) == WCQP_E_INVALID and _create(wca, on, pik_q_reg=None) == WCQP_E_INVALID
    assert _create(wca, on, pik_q_min=-np.ones(23)) == WCQP_E_INVALID
    assert _create(wca, on, ik_mode=2) == WCQP_E_INVALID
    # ---- without the option: today's answer, through all three entry points
    for kw in (dict(), dict(streamed_trajectories=0), dict(streamed_trajectories=0, planned_trajectories=1)):
        p, keep = _params(wca, **kw)
        for call in (lambda: lib.wcqp_tick_create(C.byref(p), C.byref(h)), lambda: lib.wcqp_tick_create_ext(C.byref(p), None, C.byref(h)),
                     lambda: lib.wcqp_tick_create_ext(C.byref(p), C.byref(cp.TickParamsExt(0)), C.byref(h)),
                     lambda: lib.wcqp_tick_create_ext(C.byref(p), C.byref(cp.TickParamsExt(1)), C.byref(h)),
                     lambda: lib.wcqp_tick_create_opts(C.byref(p), None, 0, C.byref(h)),
                     lambda: lib.wcqp_tick_create_opts(C.byref(p), _opts(wca, [(POS, 0)]), 1, C.byref(h)),
                     lambda: lib.wcqp_tick_create_opts(C.byref(p), _opts(wca, [(RES, 1), (POS, 0)]), 2, C.byref(h))):
            assert call() == WCQP_E_UNSUPPORTED and not h, kw
    # ---- a fully valid block, alone and with a resident plan: every host check passes
    expect = 0 if wca.device_count() > 0 else WCQP_E_HIP
    assert _create(wca, on) == expect and _create(wca, [(RES, 1), (POS, 1)]) == expect and _create(wca, [(POS, 1), (RES, 0)]) == expect


RESIDENT_CASES = [(dict(resident_plan=1, streamed_trajectories=0), WCQP_E_UNSUPPORTED),
                  (dict(resident_plan=1, streamed_trajectories=0, plant=0), WCQP_E_UNSUPPORTED),
                  (dict(resident_plan=1, streamed_trajectories=0, planned_trajectories=1, plant=0), WCQP_E_UNSUPPORTED),
                  (dict(resident_plan=1, planned_trajectories=1), WCQP_E_UNSUPPORTED),
                  (dict(resident_plan=1, streamed_trajectories=0, planned_trajectories=1), WCQP_E_UNSUPPORTED),
                  (dict(resident_plan=1, logger_ticks=5), WCQP_E_UNSUPPORTED),
                  (dict(resident_plan=2), WCQP_E_INVALID), (dict(resident_plan=-1), WCQP_E_INVALID)]


@pytest.mark.parametrize("case,rc", RESIDENT_CASES)
def test_create_opts_with_the_resident_key_answers_as_create_ext(wca, case, rc):
    """the cases of test_tick_resident_plan.py::test_create_refuses_before_the_device (its parameter block, restated): wcqp_tick_create_opts
    with the one key WCQP_TICK_OPT_RESIDENT_PLAN gives wcqp_tick_create_ext's answer"""
    lib = wca.capi.lib()
    case = dict(case)
    value = case.pop("resident_plan")
    prm = wca.capi.TickParams()
    prm.batch, prm.max_ticks, prm.step_ticks, prm.ds_ticks = 4, 10, 180, 110
    prm.mpc.horizon, prm.mpc.sampling_time, prm.mpc.com_height, prm.mpc.gravity = 50, 0.01, 0.53, 9.81
    prm.ik.dof, prm.use_kinematics, prm.kin_handoff, prm.streamed_trajectories, prm.plant = 23, 1, 0, 1, 1
    for k in range(9):
        prm.neck_additional_rotation[k] = float(k % 4 == 0)
    for k, v in case.items():
        setattr(prm, k, v)
    h = C.c_void_p()
    a = lib.wcqp_tick_create_ext(C.byref(prm), C.byref(wca.capi.TickParamsExt(value)), C.byref(h))
    b = lib.wcqp_tick_create_opts(C.byref(prm), _opts(wca, [(RES, value)]), 1, C.byref(h))
    assert a == b == rc and not h


def test_binding_refusals(wca):
    """what TickPipeline refuses before it reaches the library: POSITION with neither planned nor streamed trajectories (pinned), streamed
    ones without the external plant, no q_reg"""
    mk = lambda **kw: wca.TickPipeline(3, T, wca.MpcSolver(horizon=pk.N), px.ik_solver(wca), kin=wca.KinModel(pk.scenario()["model"]), **kw)
    st = dict(streamed_trajectories=True, external_feedback=True, neck_additional_rotation=np.eye(3))
    with pytest.raises(ValueError, match="planned"):
        mk(ik_mode="position", position_ik=dict(q_reg=np.zeros(23)))
    with pytest.raises(ValueError, match="planned"):
        mk(ik_mode="position", position_ik=dict(q_reg=np.zeros(23)), external_feedback=True)
    with pytest.raises(ValueError, match="external"):
        mk(ik_mode="position", position_ik=dict(q_reg=np.zeros(23)), streamed_trajectories=True, neck_additional_rotation=np.eye(3))
    with pytest.raises(ValueError, match="q_reg"):
        mk(ik_mode="position", position_ik=dict(w_q=0.5), **st)
    with pytest.raises(ValueError, match="position_ik"):
        mk(position_ik=dict(q_reg=np.zeros(23)), **st)
    with pytest.raises(ValueError, match="exclude"):
        mk(ik_mode="position", position_ik=dict(q_reg=np.zeros(23)), planned_trajectories=True, **st)


@pytest.mark.parametrize("controller", pk.CONTROLLERS)
def test_restatement_is_a_fair_yardstick(controller):
    """Fed its own internal logs, the restatement with external feedback reproduces the internal one's u0_log and p_star bit for bit (so its
    walk is helpers/position_tick.reference's); under the disturbed feed every tick of robots 0, 5 and 12 ends SOLVED within the budget of
    30 iterations, the MPC never fails, and p_star differs from the undisturbed run's by more than 1e-4."""
    base = pk.reference(controller)
    ownr = px.reference(controller, "own")
    dist = px.reference(controller, "disturbed")
    for i in SEL:
        assert np.array_equal(ownr[i]["chain"]["u0_log"], base[i]["chain"]["u0_log"]), i
        assert np.array_equal(ownr[i]["chain"]["p_star"], base[i]["chain"]["p_star"]), i
        assert np.array_equal(ownr[i]["walk"]["q_log"], base[i]["walk"]["q_log"]), i
        w = dist[i]["walk"]
        moved = np.abs(dist[i]["chain"]["p_star"] - base[i]["chain"]["p_star"]).max()
        print(controller, i, "iters", w["iters"].min(), w["iters"].max(), "p_star moves by", moved)
        assert (w["status"] == ps.SOLVED).all() and w["ik_fail"] == 0 and (w["iters"] >= 1).all() and (w["iters"] <= 30).all()
        assert dist[i]["chain"]["mpc_fail"] == 0 and (dist[i]["run"]["feedback_fail"] == 0).all()
        assert moved > 1e-4


# ---------------------------------------------------------------------------------------------------------------- GPU

POSITION_KEYS = ("u0_log", "q_log", "q_des", "ik_fail", "mpc_fail", "ik_iters", "measured", "feedback_fail", "active_lower", "active_upper", "dcm", "com",
                 "zmp_gains", "tick")


def _same(a, b, keys=POSITION_KEYS, rows=None, n=None):
    """bit for bit (rows: only these robots; n: only the first n ticks of the logs)"""
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if n is not None and k.endswith("_log"):
            x, y = x[:n], y[:n]
        if rows is not None and x.ndim >= 1 and B13 in x.shape:
            ax = x.shape.index(B13)
            x, y = np.take(x, rows, ax), np.take(y, rows, ax)
        assert np.array_equal(x, y), k


def _finite(o):
    for k, v in o.items():
        assert np.isfinite(np.asarray(v, float)).all(), k


@pytest.fixture(scope="module")
def walks(wca):
    """per (controller, feed): the hand-over form on the scenario's restated plan - stages_of(plan) through set_desired_host, the feed
    through set_feedback_host, run(1) - once -> the downloaded outputs"""
    cache = {}

    def get(controller, feed):
        if (controller, feed) not in cache:
            ext = px.own(controller)[0] if feed == "own" else px.disturbed(controller)
            p = px.pipe(wca, controller)
            px.upload_streamed(p, pk.scenario()["plan"])
            px.handed_over(p, stt.stages_of(pk.scenario()["plan"], T), ext)
            cache[(controller, feed)] = p.download()
            info = p.info()
            assert info["ik_mode"] == "position" and info["streamed_trajectories"] and not info["planned_trajectories"] and not info["resident_plan"]
            assert info["kin_handoff"] == "fused" and info["ticks_per_launch"] == 1
            assert p.option(POS) == 1 and p.option(RES) == 0
            p.close()
        return cache[(controller, feed)]
    return get


def _against(o, reference, ext, label, n=T):
    assert "dq_log" not in o and o["tick"] == n
    assert not o["ik_fail"].any() and not o["mpc_fail"].any() and not o["feedback_fail"].any()
    assert (o["ik_iters"] >= n).all() and (o["ik_iters"] <= 30 * n).all()
    last = np.concatenate([ext["dcm"][n - 1], ext["com"][n - 1], ext["zmp"][n - 1]], 1)
    assert np.array_equal(o["measured"], last)
    errs = {}
    for i, r in reference.items():
        assert (r["walk"]["status"] == ps.SOLVED).all()
        errs[i] = (np.abs(o["q_log"][:n, i] - r["walk"]["q_log"]).max(), np.abs(o["u0_log"][:n, i] - r["chain"]["u0_log"]).max())
        print(label, i, "q_log", errs[i][0], "u0_log", errs[i][1], "iters", int(o["ik_iters"][i]), "restatement", int(r["walk"]["iters"].sum()))
    for i, (eq, eu) in errs.items():
        assert eq <= 1e-9 and eu <= 1e-9, (i, eq, eu)
        if n == T:
            assert np.abs(o["q_des"][i] - reference[i]["walk"]["q_log"][-1]).max() <= 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("controller", pk.CONTROLLERS)
def test_hand_over_form(walks, controller):
    """(1) stages through set_desired_host, the restatement's internal logs through set_feedback_host: q_log and u0_log of robots 0, 5, 12
    within 1e-9 of the restatement, no IK failure in any of the 13.  Measured on an MI355X: see DESIGN 8.19."""
    _against(walks(controller, "own"), px.reference(controller, "own"), px.own(controller)[0], controller + " own")


@pytest.mark.gpu
@pytest.mark.parametrize("controller", pk.CONTROLLERS)
def test_disturbed_feed(walks, controller):
    """(2) the same under the disturbed feed, against the disturbed restatement; q_log differs from (1)'s by more than 1e-6: the feed is read"""
    o = walks(controller, "disturbed")
    _against(o, px.reference(controller, "disturbed"), px.disturbed(controller), controller + " disturbed")
    moved = np.abs(o["q_log"] - walks(controller, "own")["q_log"]).max()
    print(controller, "q_log moves by", moved)
    assert moved > 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("controller", pk.CONTROLLERS)
def test_resident_plan_form(wca, controller):
    """(3) upload_footsteps on the handle, then set_desired_from_plan per tick: bit for bit the hand-over form fed that handle's
    plan_window() stages; option() reports both keys"""
    fs = pk.scenario()["fs"]
    ext = px.own(controller)[0]
    a = px.pipe(wca, controller, resident=True)
    assert a.option(POS) == 1 and a.option(RES) == 1 and a.info()["resident_plan"]
    a.upload_footsteps(fs, fs)
    w = a.plan_window()
    px.from_plan(a, ext)
    oa = a.download()
    b = px.pipe(wca, controller)
    px.upload_streamed(b, w)
    px.handed_over(b, px.window_stages(w), ext)
    ob = b.download()
    _same(oa, ob)
    assert oa["tick"] == T and not oa["ik_fail"].any() and not oa["feedback_fail"].any()
    for i, r in px.reference(controller, "own").items():
        assert np.abs(oa["q_log"][:, i] - r["walk"]["q_log"]).max() <= 1e-9, i


@pytest.mark.gpu
def test_soles_sit_on_the_plan(wca, walks):
    """(4) knows no restatement: at q_log[t] with the left sole anchored on stage t's pose, the stand-alone kinematics put the right sole on
    stage t's pose and the CoM at stage t's height, to 1e-9 - all 13 robots, every tick, under the disturbed feed"""
    plan = pk.scenario()["plan"]
    kin = wca.KinModel(pk.scenario()["model"])
    q = walks("mpc", "disturbed")["q_log"]                       # [T][B][23]
    qf = np.ascontiguousarray(q.reshape(T * B13, 23))
    ident = np.tile(np.concatenate([np.zeros(3), np.eye(3).reshape(9)]), (T * B13, 1))
    k0 = kin.jacobians_host(ident, qf, state=np.zeros((T * B13, 87)))["state"]      # the soles in the base frame
    left = np.swapaxes(plan["left_traj"][:, :T], 0, 1).reshape(T * B13, 12)
    pL, RL = k0[:, 0:3], k0[:, 3:12].reshape(-1, 3, 3)
    Rb = left[:, 3:12].reshape(-1, 3, 3) @ np.swapaxes(RL, 1, 2)
    base = np.concatenate([left[:, :3] - np.einsum("bij,bj->bi", Rb, pL), Rb.reshape(-1, 9)], axis=1)
    k = kin.jacobians_host(np.ascontiguousarray(base), qf, state=np.zeros((T * B13, 87)))["state"]
    right = np.swapaxes(plan["right_traj"][:, :T], 0, 1).reshape(T * B13, 12)
    height = np.swapaxes(plan["com_height_traj"][:, :T], 0, 1).reshape(T * B13)
    e_left, e_right, e_h = np.abs(k[:, 0:12] - left).max(), np.abs(k[:, 12:24] - right).max(), np.abs(k[:, 68] - height).max()
    print("left sole", e_left, "right sole", e_right, "CoM height", e_h)
    assert e_left <= 1e-9 and e_right <= 1e-9 and e_h <= 1e-9


def _sensor_walk(p, readings, spoil=None, watch=()):
    """SENSOR_T ticks of the sensor form on the scenario's stages -> (outputs, {t: download() after tick t} for t in watch)"""
    stages = stt.stages_of(pk.scenario()["plan"], px.SENSOR_T)
    px.upload_streamed(p, pk.scenario()["plan"])
    seen = {}
    for t in range(px.SENSOR_T):
        p.set_desired_host(*px.stage(stages, t))
        r = [np.array(x, copy=True) for x in readings[t]]
        if spoil is not None:
            spoil(t, r)
        p.set_sensor_feedback_host(*r)
        p.run(1)
        if t in watch:
            seen[t] = p.download()
    return p.download(), seen


@pytest.fixture(scope="module")
def sensor_run(wca):
    """the sensor form on the recording, MPC handle, once: (outputs, the downloads after the ticks around the switch of the fixed-frame foot)"""
    cache = []

    def get():
        if not cache:
            cache.append(_sensor_walk(px.pipe(wca, "mpc"), px.sensor_recording()["readings"], watch=(0, 33, 34, 35, 36, 37, px.SENSOR_T - 1)))
        return cache[0]
    return get


@pytest.mark.gpu
def test_sensor_form(sensor_run):
    """(5) the recording built beforehand (helpers/position_external.sensor_recording) through set_sensor_feedback_host, across the switch of
    the fixed-frame foot at tick 35: download()["measured"] within 1e-12 of oracle/sensor_spec.sensor_measured on the ticks around it (the
    sensor kernel's own bar, tests/test_tick_resident_plan.py), q_log and u0_log of robots 0, 5, 12 within 1e-9 of the restatement fed the
    evaluated states, no robot stopped"""
    o, seen = sensor_run()
    ext = px.sensor_recording()["external"]
    flags = pk.scenario()["plan"]["contact"][:, :px.SENSOR_T]
    assert ((flags[:, 34] & 4) != (flags[:, 36] & 4)).all()
    for t, d in seen.items():
        err = np.abs(d["measured"] - np.concatenate([ext["dcm"][t], ext["com"][t], ext["zmp"][t]], 1)).max()
        print("tick", t, "measured error", err)
        assert err <= 1e-12, (t, err)
    assert "dq_log" not in o and o["tick"] == px.SENSOR_T and not o["ik_fail"].any() and not o["feedback_fail"].any() and not o["mpc_fail"].any()
    ref = px.reference("mpc", "sensor")
    for i, r in ref.items():
        assert (r["walk"]["status"] == ps.SOLVED).all()
        eq = np.abs(o["q_log"][:px.SENSOR_T, i] - r["walk"]["q_log"]).max()
        eu = np.abs(o["u0_log"][:px.SENSOR_T, i] - r["chain"]["u0_log"]).max()
        print("sensor", i, "q_log", eq, "u0_log", eu)
        assert eq <= 1e-9 and eu <= 1e-9, (i, eq, eu)


def _stopped_at(o, before, i, t, n):
    """robot i was stopped by a rejection on tick t of n: its joints and its iteration count are those tick t - 1 left"""
    assert np.array_equal(o["q_log"][t:n, i], np.tile(o["q_log"][t - 1, i], (n - t, 1))) and np.array_equal(o["q_des"][i], o["q_log"][t - 1, i])
    assert o["ik_iters"][i] == before["ik_iters"][i] and np.array_equal(before["q_des"][i], o["q_log"][t - 1, i])
    assert o["ik_fail"][i] == n - t + 1 and o["feedback_fail"][i] == 1
    _finite(o)


@pytest.mark.gpu
def test_rejection_by_the_plain_form(wca, walks):
    """(6a) a NaN in robot 5's dcm_meas at tick 20: its q_log stays constant from that tick on, ik_iters stops growing, ik_fail and
    feedback_fail of every robot equal a streamed VELOCITY handle's under the same stages and feed (with the wide velocity limits of
    helpers/position_external.py: nothing but the rejection stops a robot there), every other robot is bit for bit the run without the
    rejection, nothing is non-finite"""
    i, t0 = 5, 20
    ext = {k: v.copy() for k, v in px.own("mpc")[0].items()}
    ext["dcm"][t0, i, 1] = np.nan
    stages = stt.stages_of(pk.scenario()["plan"], T)
    out = {}
    for position in (True, False):
        p = px.pipe(wca, "mpc", position=position)
        px.upload_streamed(p, pk.scenario()["plan"])
        px.handed_over(p, stages, ext, t1=t0)
        before = p.download()
        px.handed_over(p, stages, ext, t0=t0)
        out[position] = (p.download(), before)
        p.close()
    o, before = out[True]
    v = out[False][0]
    print("position ik_fail", o["ik_fail"], "feedback_fail", o["feedback_fail"], "velocity ik_fail", v["ik_fail"])
    _stopped_at(o, before, i, t0, T)
    assert np.array_equal(o["ik_fail"], v["ik_fail"]) and np.array_equal(o["feedback_fail"], v["feedback_fail"])
    _finite(v)
    _same(o, walks("mpc", "own"), rows=[r for r in range(B13) if r != i])


@pytest.mark.gpu
def test_rejection_by_the_sensor_form(wca, sensor_run):
    """(6b) a total normal force below 0.1 for robot 9 at tick 30 of the recording: the same checks against the sensor-fed run without it"""
    i, t0, n = 9, 30, px.SENSOR_T
    readings = px.sensor_recording()["readings"]

    def spoil(t, r):
        if t == t0:
            r[2][i, 2] = 0.03; r[3][i, 2] = 0.04
    out = {}
    for position in (True, False):
        out[position] = _sensor_walk(px.pipe(wca, "mpc", position=position), readings, spoil=spoil, watch=(t0 - 1,))
    o, seen = out[True]
    v = out[False][0]
    print("position ik_fail", o["ik_fail"], "feedback_fail", o["feedback_fail"], "velocity ik_fail", v["ik_fail"])
    _stopped_at(o, seen[t0 - 1], i, t0, n)
    assert np.array_equal(o["ik_fail"], v["ik_fail"]) and np.array_equal(o["feedback_fail"], v["feedback_fail"])
    _finite(v)
    _same(o, sensor_run()[0], rows=[r for r in range(B13) if r != i])


@pytest.mark.gpu
def test_forms(wca, walks):
    """(7) a non-blocking stream and one robot against thirteen (robot 0) are bit for bit the hand-over walk; run without feedback, run(2)
    and run before a desired stage are WCQP_E_INVALID and leave the handle as it was; the device form of the feedback against the host form
    runs in a process of its own (torch initialises its runtime first)"""
    base = walks("mpc", "own")
    ext = px.own("mpc")[0]
    plan = pk.scenario()["plan"]
    stages = stt.stages_of(plan, T)
    s = wca.capi.stream_create()
    try:
        a = px.pipe(wca, "mpc")
        px.upload_streamed(a, plan)
        for t in range(T):
            a.set_desired_host(*px.stage(stages, t))
            if t in (0, 40):
                with pytest.raises(wca.WcqpError, match=r"\(-1\)"):
                    a.run(1, stream=s)                      # a stage, but no feedback
            px.feed(a, ext, t)
            if t in (0, 40):
                with pytest.raises(wca.WcqpError, match=r"\(-1\)"):
                    a.run(2, stream=s)                      # one tick per call
            a.run(1, stream=s)
            if t in (0, 40):
                px.feed(a, ext, t + 1)
                with pytest.raises(wca.WcqpError, match=r"\(-1\)"):
                    a.run(1, stream=s)                      # feedback, but no stage
        wca.capi.stream_synchronize(s)
        _same(a.download(), base)
    finally:
        wca.capi.stream_synchronize(s)
        wca.capi.stream_destroy(s)
    one = px.pipe(wca, "mpc", B=1)
    px.upload_streamed(one, plan, rows=slice(0, 1))
    px.handed_over(one, stages, ext, rows=slice(0, 1))
    o1 = one.download()
    for k in POSITION_KEYS:
        if k != "tick":
            x = np.asarray(base[k])
            assert np.array_equal(o1[k], np.take(x, [0], x.shape.index(B13))), k
    r = subprocess.run([sys.executable, os.path.abspath(px.__file__)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "position external device ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.gpu
def test_replan_between_two_ticks(wca):
    """(8) the resident form on the reactive handle with gain scheduling: replan_footsteps at stage 30 - inside the double support [25, 35) -
    enqueued between ticks 29 and 30 is bit for bit the hand-over of the stitched plan's stages (the handle's plan_window() afterwards),
    and robot 0 within 1e-9 of the restatement on the stitched plan; a replan with M = t after tick t was staged is WCQP_E_INVALID and
    leaves the run unchanged"""
    c = "reactive_gs"
    sc = pk.scenario()
    fs, plan0 = sc["fs"], sc["plan"]
    M = np.full(B13, -1, np.int32); M[[0, 3, 6]] = 30
    n_new = np.where(M >= 0, 2, 0).astype(np.int32)
    sides = np.tile(np.array([0, 1], np.uint8), (B13, 1))
    assert np.all(plan0["contact"][M >= 0, 30] & 3 == 3)
    rp = fr.new_steps(plan0, M, n_new, sides, 8, 31)
    stitched = fr.footstep_replan(plan0, fs, M, rp, T + pk.N + 1, T, com_height=pk.H)
    ext = stt.external_of(px.run(c, stitched))                # (the reactive chain reads stage t alone: one run on the stitched plan)
    a = px.pipe(wca, c, resident=True)
    a.upload_footsteps(fs, fs)
    px.from_plan(a, ext, t1=30)
    a.replan_footsteps(M, rp, rp["first_ds_ticks"])
    px.from_plan(a, ext, t1=52, t0=30)
    # tick 52 - in the double support [50, 60) of robot 9, which keeps its plan - is staged: a replan at that very stage comes one too late
    t, late_robot = 52, 9
    assert (int(stitched["contact"][late_robot, t]) & 3) == 3
    late = np.full(B13, -1, np.int32); late[late_robot] = t
    step = dict(n_steps=np.where(late >= 0, 1, 0).astype(np.int32), side=np.zeros((B13, 1), np.uint8), target=np.full((B13, 1, 3), 1e3), first_ds_ticks=5)
    step["target"][late_robot, 0] = (stitched["left_traj"][late_robot, t, 0] + 0.01, stitched["left_traj"][late_robot, t, 1], 0.0)
    a.set_desired_from_plan()
    with pytest.raises(wca.WcqpError, match=r"\(-1\)"):
        a.replan_footsteps(late, step, 5)
    px.feed(a, ext, t)
    a.run(1)
    px.from_plan(a, ext, t0=t + 1)
    oa = a.download()
    w = a.plan_window()
    assert np.array_equal(w["contact"], stitched["contact"])
    b = px.pipe(wca, c)
    px.upload_streamed(b, w)
    px.handed_over(b, px.window_stages(w), ext)
    _same(oa, b.download())
    assert oa["tick"] == T and not oa["ik_fail"].any() and not oa["feedback_fail"].any()
    r0 = px.restate(c, 0, ext, plan=stitched)
    err = np.abs(oa["q_log"][:, 0] - r0["walk"]["q_log"]).max()
    moved = np.abs(r0["walk"]["q_log"] - px.reference(c, "own")[0]["walk"]["q_log"]).max()
    print("robot 0 against the stitched restatement", err, "the replan moves its joints by", moved)
    assert (r0["walk"]["status"] == ps.SOLVED).all() and err <= 1e-9 and moved > 1e-4
