"""CPU restatement of the closed-loop tick with the REACTIVE DCM controller (wcqp_tick_params.dcm_controller = REACTIVE): oracle/tick_spec.py's
run_ticks with its MPC solve replaced by WalkingDCMReactiveController::evaluateControl (WM/src/WalkingDCMReactiveController.cpp:63-82),

    zmp_des = dcm_des - dcm_des_dot / omega - kDCM (dcm_des - dcm_measured),      omega = sqrt(gravity / com_height)

The replacement is a patch of tick_spec.qs.mpc_exact for the duration of one run_ticks call (restored on the way out, exceptions
included).  run_ticks calls the solve as mpc_exact(c, dcm[i], ref[i, t:t + N + 1], u_prev[i], hull rows) - window[0] is the tick's
reference stage, window[1] the next one - so without an explicit velocity the law takes the forward difference of the window.
With an explicit velocity array vel[B][stages][2] the patch has to know (i, t): it relies on run_ticks calling the solve exactly once
per robot and tick, in the fixed order `for t: for i in range(B)`, and counts the calls.  A change of that order in tick_spec breaks
this helper (the count check at the end catches a different NUMBER of calls, not a different order)."""
import contextlib

import numpy as np

from oracle import tick_spec


def reactive_law(dcm_des, dcm_des_dot, dcm_meas, omega, k_dcm):
    """WalkingDCMReactiveController.cpp:75-78, elementwise."""
    return dcm_des - dcm_des_dot / omega - k_dcm * (dcm_des - dcm_meas)


@contextlib.contextmanager
def reactive_solve(p, k_dcm, B, vel=None):
    """tick_spec.qs.mpc_exact replaced by the reactive law while the block runs; `calls` counts the solves."""
    omega = np.sqrt(p.gravity / p.com_height)
    state = {"calls": 0}

    def solve(c, x0, window, u_prev, hA, hb, nc):
        k = state["calls"]
        state["calls"] = k + 1
        if vel is None:
            v = (window[1] - window[0]) / p.dT
        else:
            t, i = divmod(k, B)           # run_ticks: `for t: for i in range(B)`, one solve per robot-tick
            v = vel[i, t]
        return {"u0": reactive_law(np.asarray(window[0]), np.asarray(v), np.asarray(x0), omega, k_dcm)}

    saved = tick_spec.qs.mpc_exact
    tick_spec.qs.mpc_exact = solve
    try:
        yield state
    finally:
        tick_spec.qs.mpc_exact = saved


def run_ticks_reactive(p, data, n_ticks, ik_params, k_dcm, dcm_vel=None, **kw):
    """tick_spec.run_ticks under reactive_solve.  Logger columns 4-5 are the velocity the law used (run_ticks writes the forward
    difference there, which is that velocity when dcm_vel is None)."""
    B = data["q0"].shape[0]
    with reactive_solve(p, k_dcm, B, dcm_vel) as st:
        out = tick_spec.run_ticks(p, data, n_ticks, ik_params, **kw)
    assert st["calls"] == n_ticks * B, (st["calls"], n_ticks, B)
    L = out["logger"].shape[0]
    if dcm_vel is not None and L > 0:
        out["logger"][:, :, 4:6] = np.transpose(np.asarray(dcm_vel)[:, :L], (1, 0, 2))
    return out
