"""Stopped robots restarted per robot (wcqp_tick_restart_robots), without a device: the ABI, what the binding refuses before
it reaches the library, the refusals that need no handle, and the numpy restatement's own properties (helpers/plan_restart.py)."""
import ctypes as C

import numpy as np
import pytest
from walking_controllers_amd.capi import E_INVALID as WCQP_E_INVALID

from helpers import footstep_plan as fp
from helpers import footstep_replan as fr
from helpers import plan_restart as prs
from helpers import planned_tick as pt

B13, MAXT, T = fr.B13, fr.MAXT, fr.MAXT + 51
SET = (2, 4, 5, 6, 7, 9, 12)


def test_the_symbols_exist_and_refuse_null(wca):
    capi = wca.capi
    lib = capi.lib()
    for s in ("wcqp_tick_restart_robots", "wcqp_tick_get_restart_result"):
        assert s in capi.ABI_SYMBOLS and getattr(lib, s)
    assert (capi.TICK_RESTART_KEEP, capi.TICK_RESTART_ALWAYS, capi.TICK_RESTART_IF_STOPPED) == (0, 1, 2)
    assert lib.wcqp_tick_restart_robots(None, C.byref(capi.TickRestart()), None) == WCQP_E_INVALID
    assert lib.wcqp_tick_get_restart_result(None, C.byref(capi.TickRestartResult())) == WCQP_E_INVALID
    assert [k for k, _ in capi.TickRestart._fields_] == ["mode", "state0", "q0", "com0", "dcm0", "u_init"]
    assert [k for k, _ in capi.TickRestartResult._fields_] == ["restarted", "stopped_ticks", "stage"]


def test_binding_refusals_without_a_device(wca):
    """What TickPipeline.restart_robots refuses before it reaches the library: a handle without a plan, arrays of the wrong shape."""
    pipe = object.__new__(wca.TickPipeline)
    pipe.planned, pipe.batch, pipe._h = False, 3, None
    d = dict(state0=np.zeros((3, 87)), q0=np.zeros((3, 23)), com0=np.zeros((3, 2)))
    with pytest.raises(ValueError):
        pipe.restart_robots(np.zeros(3, np.uint8), d)
    pipe.planned = True
    for bad in (dict(d, state0=np.zeros((3, 86))), dict(d, q0=np.zeros((4, 23))), dict(d, com0=np.zeros((3, 3))), dict(d, dcm0=np.zeros((2, 2))),
                dict(d, u_init=np.zeros(3))):
        with pytest.raises(AssertionError):
            pipe.restart_robots(np.zeros(3, np.uint8), bad)
    with pytest.raises(AssertionError):
        pipe.restart_robots(np.zeros(4, np.uint8), d)
    with pytest.raises(KeyError):
        pipe.restart_robots(np.zeros(3, np.uint8), dict(state0=d["state0"], q0=d["q0"]))
    pipe._h = None      # (nothing to destroy)


@pytest.mark.parametrize("S", [0, 41, 64, MAXT])
def test_restatement_properties(wca, S):
    """ref == zmp and dcm_vel == 0 from S on, the DCM recursion holds there, the soles are state0's, stages below S and robots that are
    not restarted are untouched, the standing stage is a valid one - on a plan dict and on a window's key names alike."""
    fs = fr.small_footsteps(wca, pt)
    plan0 = {k: v for k, v in fp.footstep_plan(fs, fs["state0"], T, MAXT).items() if k in fr.PLAN_KEYS}
    st = np.roll(fs["state0"], -1, axis=0)
    out = prs.restart(plan0, SET, S, st, fs["zmp_delta_left"], fs["zmp_delta_right"])
    assert set(out) == set(plan0)
    a = np.exp(np.sqrt(9.81 / 0.53) * 0.01)
    for i in range(B13):
        for k in plan0:
            if i not in SET:
                assert np.array_equal(out[k][i], plan0[k][i]), (k, i)
                continue
            assert np.array_equal(out[k][i, :S], plan0[k][i, :S]), (k, i)
        if i not in SET:
            continue
        assert np.array_equal(out["ref_traj"][i, S:], out["zmp_ref"][i, S:]) and not out["dcm_vel_traj"][i, S:].any()
        xi, z = out["ref_traj"][i, S:], out["zmp_ref"][i, S:]
        assert np.abs(xi[1:] - a * xi[:-1] - (1.0 - a) * z[:-1]).max(initial=0.0) <= 1e-15
        assert np.all(out["contact"][i, S:] == 7)
        assert np.all(out["left_traj"][i, S:] == st[i, 24:36]) and np.all(out["right_traj"][i, S:] == st[i, 36:48])
        assert not out["left_twist"][i, S:].any() and not out["right_twist"][i, S:].any() and not out["com_height_vel"][i, S:].any()
        assert np.all(out["com_height_traj"][i, S:] == st[i, 68])
        mid = 0.5 * (st[i, 24:26] + st[i, 27:36].reshape(3, 3)[:2, :2] @ np.asarray(fs["zmp_delta_left"]) +
                     st[i, 36:38] + st[i, 39:48].reshape(3, 3)[:2, :2] @ np.asarray(fs["zmp_delta_right"]))
        assert np.abs(out["ref_traj"][i, S] - mid).max() <= 1e-15
    # the window's names, with entries that are not per stage and rows the restatement leaves to the hull rule
    win = dict(com_height=plan0["com_height_traj"], contact=plan0["contact"], ref_traj=plan0["ref_traj"], u_init=np.ones((B13, 2)),
               hull_nc=np.zeros((B13, T), np.int32))
    ow = prs.restart(win, SET, S, st, fs["zmp_delta_left"], fs["zmp_delta_right"])
    assert set(ow) == {"com_height", "contact", "ref_traj", "u_init"} and np.array_equal(ow["u_init"], win["u_init"])
    assert np.array_equal(ow["com_height"], out["com_height_traj"]) and np.array_equal(ow["ref_traj"], out["ref_traj"])
    with pytest.raises(KeyError):
        prs.restart(dict(unknown=np.zeros((B13, T))), SET, S, st, fs["zmp_delta_left"], fs["zmp_delta_right"])


def test_a_replan_continues_the_restarted_plan(wca):
    """The restated plan is one helpers/footstep_replan.py stitches new steps onto: a restarted robot replanned at M > S walks from the
    soles it was restarted on, and its DCM reference arrives at the standing stage's ZMP at M."""
    fs = fr.small_footsteps(wca, pt)
    plan0 = {k: v for k, v in fp.footstep_plan(fs, fs["state0"], T, MAXT).items() if k in fr.PLAN_KEYS}
    S = 41
    st = np.roll(fs["state0"], -1, axis=0)
    plan1 = prs.restart(plan0, SET, S, st, fs["zmp_delta_left"], fs["zmp_delta_right"])
    M = np.full(B13, -1, np.int32); M[list(SET)] = S + 5          # (inside a single support of the OLD plan: [20, 50))
    n = np.where(M >= 0, 2, 0).astype(np.int32)
    rp = fr.new_steps(plan1, M, n, np.tile(np.array([1, 0], np.uint8), (B13, 1)), 12, 3)
    plan2 = fr.footstep_replan(plan1, fs, M, rp, T, MAXT)
    for i in SET:
        assert np.array_equal(plan2["left_traj"][i, S + 5], st[i, 24:36]) and np.abs(plan2["ref_traj"][i, S + 5] - plan1["ref_traj"][i, S + 5]).max() <= 1e-12
        assert (plan2["contact"][i, S + 5 + 12] & 3) != 3 and np.all(plan2["contact"][i, S:S + 5 + 12] == 7)
