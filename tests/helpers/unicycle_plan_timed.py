"""The timed unicycle planner of wcqp_unicycle_plan_timed_* (include/wcqp.h states it), restated from that definition in plain Python
floats with one loop per robot and a stored path.  Start, unicycle law, RK4, candidate geometry, the three constraints and the arrival
test are helpers/unicycle_plan.py's; here the candidates of a step are the samples min_step_ticks .. max_step_ticks, every feasible one
is scored, the best-scored one (the first of equals) is the step, and the step's two durations follow from its length in samples.
Outputs: those of unicycle_plan plus ss_ticks, ds_ticks [B][K], and `margin` [B], the smallest margin of any decision the robot's plan
took: for the candidate taken every constraint's |margin|; for every other candidate either - infeasible - the largest of the constraints
it violates (all of them would have to flip), or - feasible - every constraint's margin and its score's distance c(m) - c(m*) from the
best; and the two arrival thresholds.  A robot whose margin is below 1e-9 may be decided otherwise by arithmetic that rounds otherwise."""
import math

import numpy as np

from helpers import unicycle_plan as up

DONE, TRUNCATED, STUCK, INVALID_INPUT = up.DONE, up.TRUNCATED, up.STUCK, up.INVALID_INPUT
TIMING_KEYS = ("min_step_ticks", "max_step_ticks", "nominal_step_ticks", "time_weight", "position_weight", "switch_over_swing_ratio")


def durations(m, ratio):
    """(ss, ds) of a step of m samples: ds = min(max(floor(m rho + 0.5), 1), m - 1), rho = r / (1 + r)"""
    rho = ratio / (1.0 + ratio)
    ds = min(max(int(math.floor(m * rho + 0.5)), 1), m - 1)
    return m - ds, ds


def _score(p, tm, m, c, stance, sgn):
    """c(m) of candidate c (x, y) after m samples, seen from the stance foot (x, y, th)"""
    ct, st = math.cos(stance[2]), math.sin(stance[2])
    ex, ey = c[0] - stance[0], c[1] - stance[1]
    rlon, rlat = ct * ex + st * ey, ct * ey - st * ex
    dt = 1.0 / (m * p["dT"]) - 1.0 / (tm["nominal_step_ticks"] * p["dT"])
    dl = rlat - sgn * p["nominal_width"]
    return tm["time_weight"] * (dt * dt) + tm["position_weight"] * (rlon * rlon + dl * dl)


def plan_robot(p, tm, left0, right0, goal, first_side):
    K, half_w = int(p["max_steps"]), 0.5 * p["nominal_width"]
    m_min, m_max = int(tm["min_step_ticks"]), int(tm["max_step_ticks"])
    out = dict(n_steps=0, side=np.zeros(K, np.uint8), target=np.zeros((K, 3)), status=INVALID_INPUT, desired_point=np.zeros(2),
               unicycle_end=np.zeros(3), ss_ticks=np.zeros(K, np.int32), ds_ticks=np.zeros(K, np.int32), margin=np.inf, steps=[])
    read = [left0[0], left0[1], left0[3], left0[6], right0[0], right0[1], right0[3], right0[6], goal[0], goal[1]]
    if not all(math.isfinite(v) for v in read) or first_side > 1:
        return out
    feet = [(left0[0], left0[1], math.atan2(left0[6], left0[3])), (right0[0], right0[1], math.atan2(right0[6], right0[3]))]
    sw = int(first_side)
    stance = feet[1 - sw]
    off = -half_w if sw == 1 else half_w              # a left stance foot (the right one swings): (0, -w/2)
    u = up._foot(stance, 1.0, off) + (stance[2],)
    dx, dy = p["reference_position"]
    ax, ay = dx + goal[0], dy + goal[1]
    ys = (u[0] + (math.cos(u[2]) * ax - math.sin(u[2]) * ay), u[1] + (math.sin(u[2]) * ax + math.cos(u[2]) * ay))
    if not (math.isfinite(ys[0]) and math.isfinite(ys[1])):
        return out
    out["desired_point"][:] = ys
    status, margin, n = TRUNCATED, math.inf, 0
    for k in range(K):
        sgn = 1.0 if sw == 0 else -1.0
        stance, swing = feet[1 - sw], feet[sw]
        path = [u]
        for m in range(m_max):
            path.append(up._rk4(p, path[-1], ys))
        ms_all = range(m_min, m_max + 1)
        cand = {m: up._foot(path[m], sgn, half_w) for m in ms_all}
        cons = {m: up._constraints(p, cand[m], path[m][2], stance, sgn) for m in ms_all}
        cost = {m: _score(p, tm, m, cand[m], stance, sgn) for m in ms_all}
        feas = [m for m in ms_all if min(cons[m]) >= 0.0]
        ms = min(feas, key=lambda m: (cost[m], m)) if feas else 0
        for m in ms_all:
            if m == ms:
                margin = min(margin, min(abs(v) for v in cons[m]))
            elif m in feas:
                margin = min(margin, min(cons[m]), cost[m] - cost[ms])
            else:
                margin = min(margin, max(abs(v) for v in cons[m] if not v >= 0.0))
        if ms == 0:
            status = STUCK
            break
        c, th_u = cand[ms], path[ms][2]
        dist = math.sqrt((c[0] - swing[0]) ** 2 + (c[1] - swing[1]) ** 2)
        dyaw = up.wrap(th_u - swing[2])
        margin = min(margin, abs(dist - p["min_step_length"]), abs(abs(dyaw) - p["min_angle_variation"]))
        if dist < p["min_step_length"] and abs(dyaw) < p["min_angle_variation"]:
            status = DONE
            break
        out["side"][k] = sw
        out["target"][k] = (c[0], c[1], dyaw)
        out["ss_ticks"][k], out["ds_ticks"][k] = durations(ms, tm["switch_over_swing_ratio"])
        # what the step was chosen from, for the tests: m*, the feasible candidates, every candidate's score
        out["steps"].append(dict(m=ms, feasible=feas, cost=cost))
        n += 1
        feet[sw] = (c[0], c[1], th_u)
        u = path[ms]
        sw = 1 - sw
    out.update(n_steps=n, status=status, margin=margin, feet=feet)
    out["unicycle_end"][:] = u
    return out


def unicycle_plan_timed(params, timing, left0, right0, goals, first_side):
    """params: the dict of wcqp_unicycle_params' fields (capi.UnicyclePlanner.values; step_ticks is not read), timing: the dict of
    wcqp_unicycle_timing's.  -> the arrays of the device's outputs (ss_ticks, ds_ticks among them), `margin` [B], `feet` [B][2][3] and
    `steps`, per robot the list of its steps' choices."""
    assert set(timing) == set(TIMING_KEYS), sorted(timing)
    left0, right0, goals = (np.asarray(a, float) for a in (left0, right0, goals))
    B = goals.shape[0]
    fs = np.broadcast_to(np.asarray(first_side), (B,))
    rows = [plan_robot(params, timing, left0[i].tolist(), right0[i].tolist(), goals[i].tolist(), int(fs[i])) for i in range(B)]
    K = int(params["max_steps"])
    out = dict(n_steps=np.array([r["n_steps"] for r in rows], np.int32), side=np.array([r["side"] for r in rows], np.uint8).reshape(B, K),
               target=np.array([r["target"] for r in rows], float).reshape(B, K, 3), status=np.array([r["status"] for r in rows], np.int32),
               desired_point=np.array([r["desired_point"] for r in rows], float).reshape(B, 2),
               unicycle_end=np.array([r["unicycle_end"] for r in rows], float).reshape(B, 3),
               ss_ticks=np.array([r["ss_ticks"] for r in rows], np.int32).reshape(B, K),
               ds_ticks=np.array([r["ds_ticks"] for r in rows], np.int32).reshape(B, K), margin=np.array([r["margin"] for r in rows], float))
    out["feet"] = np.array([r.get("feet", [(0.0,) * 3] * 2) for r in rows], float).reshape(B, 2, 3)
    out["steps"] = [r["steps"] for r in rows]
    return out
