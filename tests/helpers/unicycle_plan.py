"""The unicycle planner of wcqp_unicycle_* (include/wcqp.h states it), restated from that definition in plain Python floats with one loop
per robot and a stored path: from the soles, the goal and the first swing side to n_steps, side, target, status, desired_point and
unicycle_end - plus `margin` [B], the smallest absolute margin of any decision the robot's plan took: the three constraints of the
candidates m* and m* + 1 (and, for a later candidate, the largest margin among the constraints it violates: all of them would have to
flip), and the two arrival thresholds.  A robot whose margin is below 1e-9 may be decided otherwise by arithmetic that rounds otherwise."""
import math

import numpy as np

DONE, TRUNCATED, STUCK, INVALID_INPUT = range(4)
TWO_PI = 2.0 * math.pi


def wrap(a):
    return a - TWO_PI * round(a / TWO_PI)          # (Python's round of a float ties to even, as rint does)


def _rate(p, x, y, th, ys):
    dx, dy = p["reference_position"]
    c, s = math.cos(th), math.sin(th)
    ex = (x + (c * dx - s * dy)) - ys[0]
    ey = (y + (s * dx + c * dy)) - ys[1]
    kd = p["unicycle_gain"] / dx                    # B^-1 = [[d_x c - d_y s, d_x s + d_y c], [-s, c]] / d_x
    v = -kd * ((dx * c - dy * s) * ex + (dx * s + dy * c) * ey)
    w = -kd * (c * ey - s * ex)
    v = min(max(v, -p["max_linear_velocity"]), p["max_linear_velocity"])
    w = min(max(w, -p["max_angular_velocity"]), p["max_angular_velocity"])
    v = v / (1.0 + p["slow_when_turning_gain"] * abs(w))
    return v * c, v * s, w


def _rk4(p, u, ys):
    h = p["dT"]
    k1 = _rate(p, u[0], u[1], u[2], ys)
    k2 = _rate(p, u[0] + 0.5 * h * k1[0], u[1] + 0.5 * h * k1[1], u[2] + 0.5 * h * k1[2], ys)
    k3 = _rate(p, u[0] + 0.5 * h * k2[0], u[1] + 0.5 * h * k2[1], u[2] + 0.5 * h * k2[2], ys)
    k4 = _rate(p, u[0] + h * k3[0], u[1] + h * k3[1], u[2] + h * k3[2], ys)
    return tuple(u[j] + h / 6.0 * (k1[j] + 2.0 * k2[j] + 2.0 * k3[j] + k4[j]) for j in range(3))


def _foot(u, sgn, half_w):
    """the foot beside the unicycle u: R(th) (0, sgn w/2) from it"""
    return u[0] - math.sin(u[2]) * sgn * half_w, u[1] + math.cos(u[2]) * sgn * half_w


def _constraints(p, c, th_u, stance, sgn):
    """the three margins (>= 0: satisfied) of candidate c with yaw th_u against the stance foot (x, y, th)"""
    ct, st = math.cos(stance[2]), math.sin(stance[2])
    ex, ey = c[0] - stance[0], c[1] - stance[1]
    rlon, rlat = ct * ex + st * ey, ct * ey - st * ex
    return (p["max_step_length"] - math.sqrt(rlon * rlon + rlat * rlat), sgn * rlat - p["min_width"],
            p["max_angle_variation"] - abs(wrap(th_u - stance[2])))


def plan_robot(p, left0, right0, goal, first_side):
    K, D, half_w = int(p["max_steps"]), int(p["step_ticks"]), 0.5 * p["nominal_width"]
    out = dict(n_steps=0, side=np.zeros(K, np.uint8), target=np.zeros((K, 3)), status=INVALID_INPUT, desired_point=np.zeros(2),
               unicycle_end=np.zeros(3), margin=np.inf)
    read = [left0[0], left0[1], left0[3], left0[6], right0[0], right0[1], right0[3], right0[6], goal[0], goal[1]]
    if not all(math.isfinite(v) for v in read) or first_side > 1:
        return out
    feet = [(left0[0], left0[1], math.atan2(left0[6], left0[3])), (right0[0], right0[1], math.atan2(right0[6], right0[3]))]
    sw = int(first_side)
    stance = feet[1 - sw]
    off = -half_w if sw == 1 else half_w              # a left stance foot (the right one swings): (0, -w/2)
    u = _foot(stance, 1.0, off) + (stance[2],)
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
        for m in range(D):
            path.append(_rk4(p, path[-1], ys))
        cand = [None] + [_foot(path[m], sgn, half_w) for m in range(1, D + 1)]
        cons = [None] + [_constraints(p, cand[m], path[m][2], stance, sgn) for m in range(1, D + 1)]
        feas = [m for m in range(1, D + 1) if min(cons[m]) >= 0.0]
        ms = feas[-1] if feas else 0
        for m in range(ms + 1, D + 1):                # an infeasible candidate past m*: feasible only if every violated constraint flips
            viol = [abs(v) for v in cons[m] if not v >= 0.0]
            margin = min(margin, max(viol) if viol else math.inf)
        if ms == 0:
            status = STUCK
            break
        margin = min(margin, min(abs(v) for v in cons[ms]))
        if ms < D:
            margin = min(margin, min(abs(v) for v in cons[ms + 1]))
        c, th_u = cand[ms], path[ms][2]
        dist = math.sqrt((c[0] - swing[0]) ** 2 + (c[1] - swing[1]) ** 2)
        dyaw = wrap(th_u - swing[2])
        margin = min(margin, abs(dist - p["min_step_length"]), abs(abs(dyaw) - p["min_angle_variation"]))
        if dist < p["min_step_length"] and abs(dyaw) < p["min_angle_variation"]:
            status = DONE
            break
        out["side"][k] = sw
        out["target"][k] = (c[0], c[1], dyaw)
        n += 1
        feet[sw] = (c[0], c[1], th_u)
        u = path[ms]
        sw = 1 - sw
    out.update(n_steps=n, status=status, margin=margin, feet=feet)
    out["unicycle_end"][:] = u
    return out


def unicycle_plan(params, left0, right0, goals, first_side):
    """params: the dict of wcqp_unicycle_params' fields (capi.UnicyclePlanner.values).  -> the arrays of the device's outputs, `margin` [B]
    and `feet` [B][2][3], both soles' (x, y, yaw) at the end."""
    left0, right0, goals = (np.asarray(a, float) for a in (left0, right0, goals))
    B = goals.shape[0]
    fs = np.broadcast_to(np.asarray(first_side), (B,))
    rows = [plan_robot(params, left0[i].tolist(), right0[i].tolist(), goals[i].tolist(), int(fs[i])) for i in range(B)]
    K = int(params["max_steps"])
    out = dict(n_steps=np.array([r["n_steps"] for r in rows], np.int32), side=np.array([r["side"] for r in rows], np.uint8).reshape(B, K),
               target=np.array([r["target"] for r in rows], float).reshape(B, K, 3), status=np.array([r["status"] for r in rows], np.int32),
               desired_point=np.array([r["desired_point"] for r in rows], float).reshape(B, 2),
               unicycle_end=np.array([r["unicycle_end"] for r in rows], float).reshape(B, 3), margin=np.array([r["margin"] for r in rows], float))
    out["feet"] = np.array([r.get("feet", [(0.0,) * 3] * 2) for r in rows], float).reshape(B, 2, 3)
    return out
