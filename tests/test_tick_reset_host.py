"""Robots of a sensor-fed fleet reset per robot (wcqp_tick_reset_robots), without a device: the ABI, what the binding
refuses before it reaches the library, the restatement's own properties (helpers/tick_reset.py), and the condition the GPU tests rest on:
the restatement, started from the reset rows and fed the robot in the loop, stops none of the reset robots."""
import ctypes as C

import numpy as np
import pytest
from walking_controllers_amd.capi import E_INVALID as WCQP_E_INVALID

from helpers import plan_restart as prs
from helpers import resident_plan as rs
from helpers import tick_reset as tr

B, MAXT = rs.B, rs.MAXT


def test_the_symbol_exists_and_refuses_null(wca):
    capi = wca.capi
    lib = capi.lib()
    assert "wcqp_tick_reset_robots" in capi.ABI_SYMBOLS and lib.wcqp_tick_reset_robots
    assert lib.wcqp_tick_reset_robots(None, C.byref(capi.TickRestart()), None) == WCQP_E_INVALID
    assert lib.wcqp_tick_reset_robots(None, None, None) == WCQP_E_INVALID
    # it reuses the restart's struct and modes: nothing grew
    assert [k for k, _ in capi.TickRestart._fields_] == ["mode", "state0", "q0", "com0", "dcm0", "u_init"]
    assert (tr.KEEP, tr.ALWAYS, tr.IF_STOPPED) == (capi.TICK_RESTART_KEEP, capi.TICK_RESTART_ALWAYS, capi.TICK_RESTART_IF_STOPPED)


def test_binding_refusals_without_a_device(wca):
    """What TickPipeline.reset_robots refuses before it reaches the library: arrays of the wrong shape, a missing row."""
    pipe = object.__new__(wca.TickPipeline)
    pipe.planned, pipe.streamed, pipe.batch, pipe._h = False, True, 3, None
    d = dict(state0=np.zeros((3, 87)), q0=np.zeros((3, 23)), com0=np.zeros((3, 2)))
    for bad in (dict(d, state0=np.zeros((3, 86))), dict(d, q0=np.zeros((4, 23))), dict(d, com0=np.zeros((3, 3))), dict(d, dcm0=np.zeros((2, 2))),
                dict(d, u_init=np.zeros(3))):
        with pytest.raises(AssertionError):
            pipe.reset_robots(np.zeros(3, np.uint8), bad)
    with pytest.raises(AssertionError):
        pipe.reset_robots(np.zeros(4, np.uint8), d)
    with pytest.raises(KeyError):
        pipe.reset_robots(np.zeros(3, np.uint8), dict(state0=d["state0"], q0=d["q0"]))
    with pytest.raises(wca.WcqpError, match=r"\(-1\)"):
        pipe.reset_robots(np.zeros(3, np.uint8), d)           # (no handle: the library's own refusal)
    pipe._h = None      # (nothing to destroy)


def test_the_standing_zmp_is_the_restarts(wca):
    """helpers/tick_reset.standing_zmp, written out operation by operation, equals helpers/plan_restart.standing_zmp bit for bit on every
    robot of the scenario and on rotated soles"""
    fs = rs.scenario(wca)[0]
    dl, dr = fs["zmp_delta_left"], fs["zmp_delta_right"]
    assert np.any(np.asarray(dl) != 0.0) or np.any(np.asarray(dr) != 0.0)
    rng = np.random.default_rng(2)
    for i in range(B):
        st = fs["state0"][i].copy()
        assert np.array_equal(tr.standing_zmp(st, dl, dr), prs.standing_zmp(st, dl, dr)), i
        st[24:48] += 0.1 * rng.normal(size=24)
        assert np.array_equal(tr.standing_zmp(st, dl, dr), prs.standing_zmp(st, dl, dr)), i
    start = tr.start_rows(fs, False)
    assert np.array_equal(start["dcm0"], start["u_init"]) and np.array_equal(start["dcm0"][3], prs.standing_zmp(fs["state0"][3], dl, dr))
    ex = tr.start_rows(fs, True)
    for i in tr.ROBOTS:
        assert 5e-4 <= np.abs(ex["dcm0"][i] - start["dcm0"][i]).max() <= 5e-3 and not np.array_equal(ex["dcm0"][i], ex["u_init"][i])


def test_a_fresh_filter_starts_at_its_input(wca):
    """The per-robot filter reset of the restatement: a reset robot's first filtered joint velocities and wrenches ARE its readings,
    whatever the filters held; a rejected reading leaves it fresh; the CoM filter starts at com0; the other robots' filters go on as
    if nothing had happened."""
    fs, _, stages = rs.scenario(wca)
    model = wca.synth.icub_like_model()
    omega = np.sqrt(9.81 / 0.53)
    feed = tr.sensor_feed(fs, 6)
    a = tr.ResetFilters(B, 0.01, fs["com0"], **tr.FILTERS)
    b = tr.ResetFilters(B, 0.01, fs["com0"], **tr.FILTERS)
    for t in range(3):
        for f in (a, b):
            f.step_stages(model, stages, t, *feed[t], omega)
    i, j = 3, 5
    for r in (i, j):
        a.reset(r, fs["com0"][r])
    assert np.array_equal(a.com.y[i], fs["com0"][i]) and not a.vel.y[i].any() and a.fresh[i]
    # robot j's first reading after the reset is rejected (no force): it stays fresh, its filters hold
    ma, ra = a.step_stages(model, stages, 3, *tr.bad_force(feed[3], (j,)), omega)
    mb, rb = b.step_stages(model, stages, 3, *feed[3], omega)
    assert ra[j] and not ra[i] and a.fresh[j] and not a.fresh[i] and not rb.any()
    assert np.array_equal(a.dq.y[i], feed[3][1][i]) and np.array_equal(a.dq.u[i], feed[3][1][i])
    assert np.array_equal(a.w.y[i], np.concatenate([feed[3][2][i, [2, 3, 4]], feed[3][3][i, [2, 3, 4]]]))
    assert not np.array_equal(b.dq.y[i], feed[3][1][i])
    kept = [r for r in range(B) if r not in (i, j)]
    assert np.array_equal(ma[kept], mb[kept])
    ma, ra = a.step_stages(model, stages, 4, *feed[4], omega)
    assert not ra.any() and np.array_equal(a.dq.y[j], feed[4][1][j]) and not a.fresh.any()
    assert not np.array_equal(a.dq.y[i], feed[4][1][i])          # (robot i's filter is running by now)
    # a robot reset before any reading equals a fresh restatement's robot
    c = tr.ResetFilters(B, 0.01, fs["com0"], **tr.FILTERS)
    d = tr.ResetFilters(B, 0.01, fs["com0"], **tr.FILTERS)
    c.reset(i, fs["com0"][i])
    mc, _ = c.step_stages(model, stages, 0, *feed[0], omega)
    md, _ = d.step_stages(model, stages, 0, *feed[0], omega)
    assert np.array_equal(mc, md)


def test_the_rows_and_the_plan(wca):
    """the rows of the kept robots hold NaN, those of the listed robots the scenario's own; the plan after the call stands from S on the
    soles of state0 and is untouched below S and for every kept robot"""
    fs, plan, _ = rs.scenario(wca)
    for explicit in (False, True):
        rows = tr.rows(fs, explicit)
        assert set(rows) == {"state0", "q0", "com0"} | ({"dcm0", "u_init"} if explicit else set())
        for k, v in rows.items():
            assert np.isnan(v[list(tr.KEPT)]).all() and np.isfinite(v[list(tr.ROBOTS)]).all(), k
        assert np.array_equal(rows["q0"][list(tr.ROBOTS)], fs["q0"][list(tr.ROBOTS)])
    for S in tr.STAGES:
        after = tr.reset_plan(plan, S, fs)
        for i in range(B):
            upto = S if i in tr.ROBOTS else rs.T
            for k in after:
                if k not in prs.NOT_STAGED:
                    assert np.array_equal(after[k][i, :upto], plan[k][i, :upto]), (k, i)
        for i in tr.ROBOTS:
            assert np.all(after["contact"][i, S:] == 7) and np.all(after["left_traj"][i, S:] == fs["state0"][i, 24:36])
    # S = 41 lies inside the first swing of the walkers among the four
    assert any((int(plan["contact"][i, 41]) & 3) != 3 for i in tr.ROBOTS) and tr.STAGES[0] % 2 == 1 and tr.STAGES[1] % 2 == 0


@pytest.mark.parametrize("S", tr.STAGES)
@pytest.mark.parametrize("cfg", list(rs.CONFIGS))
def test_the_restatement_walks_on_from_the_reset_rows(wca, qs, cfg, S):
    """THE CONDITION the GPU tests rest on: oracle/tick_spec.run_ticks, started from the reset rows on the plan window [S, T) and fed the
    robot-in-the-loop sensors from there, stops none of the four robots before MAXT, under both controller configurations."""
    run = tr.restated(wca, qs, cfg, S)
    assert run["u0_log"].shape == (MAXT - S, len(tr.ROBOTS), 2) and len(run["readings"]) == MAXT - S
    assert (run["ik_fail"] == 0).all() and (run["mpc_fail"] == 0).all() and (run["feedback_fail"] == 0).all()
    assert np.isfinite(run["dq_log"]).all() and np.abs(run["dq_log"]).max() > 1e-4          # (the robots move: the noise is followed)
