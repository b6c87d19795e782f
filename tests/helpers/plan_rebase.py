"""The plan wcqp_tick_rebase_plan leaves behind (include/wcqp.h states THE REBASED PLAN), restated in plain numpy on the dicts
TickPipeline.plan_window returns - and on any dict of per-stage arrays [B][T][...], helpers/footstep_plan.py's plans among them -, and the
admission rule csrc/goal_merge.h holds as rebase_allowed."""
import math

import numpy as np

OMEGA = math.sqrt(9.81 / 0.53)          # the tests' handles: gravity / CoM height of the tick parameters' defaults
NOT_STAGED = ("u_init", "change", "a")  # entries of a window or a restated plan that are not [B][T][...]


def rebase(w, R, omega=OMEGA, dT=0.01):
    """Stages [0, T - R) are the old stages [R, T), stages [T - R, T) copies of the old stage T - 1 - the support-polygon rows per stage
    with them, which is what the compaction of the set slots must leave unchanged.  u_init, where the dict has one, becomes the ZMP of the
    new stage 0 recovered from old stage R: ref - dcm_vel / omega where the dict keeps the velocity, else the recursion solved for it."""
    R = int(R)
    T = next(v for k, v in w.items() if k not in NOT_STAGED).shape[1]
    assert 1 <= R <= T - 2, (R, T)
    out = {}
    for k, v in w.items():
        if k in NOT_STAGED:
            continue
        out[k] = np.concatenate([v[:, R:], np.repeat(v[:, -1:], R, axis=1)], axis=1)
    if "u_init" in w:
        xi = w["ref_traj"]
        if "dcm_vel_traj" in w:
            out["u_init"] = xi[:, R] - w["dcm_vel_traj"][:, R] / omega
        else:
            a = math.exp(omega * dT)
            out["u_init"] = (xi[:, R + 1] - a * xi[:, R]) / (1.0 - a)
    return out


def stands_from(origin, first_ds, ss, ds, final_ds):
    """the first standing stage of a plan generated from stage `origin`: behind first_ds stages of double support and its steps, step k of
    ss[k] + ds[k] stages, the last double support lasting final_ds stages where that is > 0"""
    n = len(ss)
    s = origin + first_ds
    for k in range(n):
        s += ss[k] + (final_ds if k == n - 1 and final_ds > 0 else ds[k])
    return s


def rebase_allowed(origin, first_ds, ss, ds, final_ds, shift, ticks_enqueued, max_ticks):
    """even, 2 at least, no more than the ticks enqueued, and the plan stands from a stage <= max_ticks on"""
    return shift >= 2 and shift % 2 == 0 and shift <= ticks_enqueued and stands_from(origin, first_ds, ss, ds, final_ds) <= max_ticks


def rebase_auto(ticks_enqueued):
    """WCQP_TICK_REBASE_AUTO: the largest even shift <= the ticks enqueued"""
    return ticks_enqueued - ticks_enqueued % 2
