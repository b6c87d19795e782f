"""CPU restatement of ZMP-CoM gain scheduling (wcqp_tick_params.zmp_gain_scheduling): the reference's `useGainScheduling 1`.

Every tick, before the ZMP-CoM law, WalkingModule calls WalkingZMPController::setPhase(stance) (WM/src/WalkingModule.cpp:657-662) with
stance = |dcm_des_dot| < 0.001, and setPhase moves kCoM and kZMP - each through a smoother of its own - towards the stance or the walking
value (WM/src/WalkingZMPController.cpp:29-125); both smoothers start at rest at the stance gains.  The smoother upstream is
iCub::ctrl::minJerkTrajGen; the project's restatement of it (include/wcqp.h) is the third-order minimum-jerk approximation

    H(s) = (150/T^3) / (s^3 + (9/T) s^2 + (60/T^2) s + 150/T^3),   T = smoothingTime,

discretised with the bilinear (Tustin) transform at the tick's sampling time.  Here it is built from the polynomial algebra
(not the device's closed-form coefficients) and run in direct form I, and the gains are filtered as TWO separate smoothers on the gains
themselves, as the reference does - the device runs one filter of the walking indicator and maps it onto both gains.

scheduled_gains wraps tick_spec.qs.mpc_exact: run_ticks calls it exactly once per robot and tick, in the order `for t: for i`, right
before the ZMP-CoM law, and reads p.k_com / p.k_zmp in that law - so the wrapper advances robot i's smoothers (BEFORE it delegates: a
QPOracleError of the MPC still follows a setPhase) and writes the robot's gains into p.k_com[i] / p.k_zmp[i] ([B][1] arrays while the
block runs).  It composes with reactive_tick.reactive_solve (enter that one first)."""
import contextlib

import numpy as np
from numpy.polynomial import polynomial as P

from oracle import tick_spec

STANCE_THRESHOLD = 0.001      # WM/src/WalkingModule.cpp:657-658

# zmpControllerParams.ini of the three shipped robots: smoothingTime, kCoM_stance, kZMP_stance (useGainScheduling 1 on all three;
# the walking gains are tests/robots.py's k_com / k_zmp)
ZMP_SCHEDULE = {
    "iCubGazeboV2_5": dict(zmp_smoothing_time=0.05, k_com_stance=6.0, k_zmp_stance=0.9),
    "iCubGenova04": dict(zmp_smoothing_time=0.1, k_com_stance=6.0, k_zmp_stance=0.9),
    "icubGazeboSim": dict(zmp_smoothing_time=0.1, k_com_stance=5.0, k_zmp_stance=1.2),
}


def is_stance(v):
    """WalkingModule.cpp:657-658 - the norm, not its square, compared with 0.001 (numpy does not contract into FMAs)."""
    v = np.asarray(v, float)
    return np.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) < STANCE_THRESHOLD


def tustin_coeffs(T, dT):
    """(b[0..3], a[0..3]) of H(z) = sum b_k z^-k / sum a_k z^-k, a[0] = 1: s^n -> K^n (1 - q)^n (1 + q)^(3 - n), q = z^-1, K = 2 / dT."""
    K = 2.0 / dT
    den_s = [150.0 / T ** 3, 60.0 / T ** 2, 9.0 / T, 1.0]          # coefficients of s^0 .. s^3
    den = np.zeros(4)
    for n, c in enumerate(den_s):
        den = den + c * K ** n * P.polymul(P.polypow([1.0, -1.0], n), P.polypow([1.0, 1.0], 3 - n))[:4]
    num = den_s[0] * P.polypow([1.0, 1.0], 3)
    return num / den[0], den / den[0]


class MinJerkSmoother:
    """The smoother in direct form I, at rest at y0 (input and output histories y0)."""

    def __init__(self, T, dT, y0):
        self.b, self.a = tustin_coeffs(T, dT)
        self.u = [float(y0)] * 3
        self.y = [float(y0)] * 3

    def step(self, target):
        b, a = self.b, self.a
        y = (b[0] * target + b[1] * self.u[0] + b[2] * self.u[1] + b[3] * self.u[2]
             - a[1] * self.y[0] - a[2] * self.y[1] - a[3] * self.y[2])
        self.u = [float(target)] + self.u[:2]
        self.y = [y] + self.y[:2]
        return y


class GainSchedule:
    """The two smoothers of WalkingZMPController (kCoM, kZMP), at rest at the stance gains."""

    def __init__(self, dT, k_com, k_zmp, k_com_stance, k_zmp_stance, zmp_smoothing_time):
        self.walk = (k_com, k_zmp)
        self.stance = (k_com_stance, k_zmp_stance)
        self.f = [MinJerkSmoother(zmp_smoothing_time, dT, k_com_stance), MinJerkSmoother(zmp_smoothing_time, dT, k_zmp_stance)]

    def set_phase(self, stance):
        goal = self.stance if stance else self.walk
        return self.f[0].step(goal[0]), self.f[1].step(goal[1])


def gain_sequence(vel, dT, k_com, k_zmp, sched):
    """vel [T][2] -> the gains [T][2] of every tick (two filters)."""
    g = GainSchedule(dT, k_com, k_zmp, **sched)
    return np.array([g.set_phase(bool(is_stance(v))) for v in np.asarray(vel, float)])


def gain_sequence_one_filter(vel, dT, k_com, k_zmp, sched):
    """The same with ONE filter of the walking indicator, k = k_stance + (k_walking - k_stance) s."""
    f = MinJerkSmoother(sched["zmp_smoothing_time"], dT, 0.0)
    s = np.array([f.step(0.0 if is_stance(v) else 1.0) for v in np.asarray(vel, float)])
    kc, kz = sched["k_com_stance"], sched["k_zmp_stance"]
    return np.stack([kc + (k_com - kc) * s, kz + (k_zmp - kz) * s], axis=1)


def forward_difference(ref, dT):
    """The velocity the tick uses without an uploaded one: (ref[t + 1] - ref[t]) / dT (the last stage 0)."""
    v = np.zeros_like(ref)
    v[:, :-1] = (ref[:, 1:] - ref[:, :-1]) / dT
    return v


@contextlib.contextmanager
def scheduled_gains(p, B, sched, vel=None):
    """While the block runs, run_ticks' ZMP-CoM law uses each robot's scheduled gains (p.k_com / p.k_zmp: the walking ones on entry).
    vel [B][stages][2]: the velocity the stance flag reads (None: the forward difference of the window, as the device forms it).
    Yields a dict: `calls` and `gains` (a list, per call, of (t, i, kCoM, kZMP))."""
    k_com, k_zmp = float(p.k_com), float(p.k_zmp)
    g = [GainSchedule(p.dT, k_com, k_zmp, **sched) for _ in range(B)]
    inner = tick_spec.qs.mpc_exact
    state = {"calls": 0, "gains": []}

    def solve(c, x0, window, u_prev, hA, hb, nc):
        k = state["calls"]
        state["calls"] = k + 1
        t, i = divmod(k, B)           # run_ticks: `for t: for i in range(B)`, one solve per robot-tick
        v = np.asarray(vel[i, t]) if vel is not None else (np.asarray(window[1]) - np.asarray(window[0])) / p.dT
        kc, kz = g[i].set_phase(bool(is_stance(v)))         # setPhase first: it precedes the controller's result either way
        p.k_com[i, 0] = kc
        p.k_zmp[i, 0] = kz
        state["gains"].append((t, i, kc, kz))
        return inner(c, x0, window, u_prev, hA, hb, nc)

    p.k_com = np.full((B, 1), k_com)
    p.k_zmp = np.full((B, 1), k_zmp)
    tick_spec.qs.mpc_exact = solve
    try:
        yield state
    finally:
        tick_spec.qs.mpc_exact = inner
        p.k_com, p.k_zmp = k_com, k_zmp


def run_ticks_scheduled(p, data, n_ticks, ik_params, sched, dcm_vel=None, **kw):
    """tick_spec.run_ticks under scheduled_gains; out["zmp_gains"] [T][B][2] the gains of every tick."""
    B = data["q0"].shape[0]
    with scheduled_gains(p, B, sched, dcm_vel) as st:
        out = tick_spec.run_ticks(p, data, n_ticks, ik_params, **kw)
    assert st["calls"] == n_ticks * B, (st["calls"], n_ticks, B)
    gains = np.zeros((n_ticks, B, 2))
    for t, i, kc, kz in st["gains"]:
        gains[t, i] = (kc, kz)
    out["zmp_gains"] = gains
    return out


def pause_reference(ref, pauses):
    """ref [B][stages][2] with robot i's reference held still over its pauses [(start, length), ...] and resumed where it stopped (a stop
    and a restart of the planned walk; the stages run out at the end).  Returns the new array and the index map."""
    B, S, _ = ref.shape
    out = np.empty_like(ref)
    idx = np.zeros((B, S), np.int64)
    for i in range(B):
        m = 0
        for s in range(S):
            held = any(a <= s < a + n for a, n in pauses.get(i, ()))
            idx[i, s] = m
            if not held:
                m = min(m + 1, S - 1)
        out[i] = ref[i, idx[i]]
    return out, idx
