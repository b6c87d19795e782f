"""
ORACLE — TEST INFRASTRUCTURE ONLY.

CPU restatement of ZMP-CoM gain scheduling (wcqp_tick_params.zmp_gain_scheduling): the reference's `useGainScheduling 1`.

Every tick, before the ZMP-CoM law, WalkingModule calls WalkingZMPController::setPhase(stance) (WM/src/WalkingModule.cpp:657-662) with
stance = |dcm_des_dot| < 0.001, and setPhase moves kCoM and kZMP - each through a smoother of its own - towards the stance or the walking
value (WM/src/WalkingZMPController.cpp:29-125); both smoothers start at rest at the stance gains.  The smoother upstream is
iCub::ctrl::minJerkTrajGen; the project's restatement of it (include/wcqp.h) is the third-order minimum-jerk approximation

    H(s) = (150/T^3) / (s^3 + (9/T) s^2 + (60/T^2) s + 150/T^3),   T = smoothingTime,

discretised with the bilinear (Tustin) transform at the tick's sampling time.  Here it is built from the polynomial algebra
(not the device's closed-form coefficients) and run in direct form I, and the gains are filtered as TWO separate smoothers on the gains
themselves, as the reference does - the device runs one filter of the walking indicator and maps it onto both gains.

oracle/tick_spec.py::run_ticks(zmp_gain_schedule=...) keeps one GainSchedule per robot and advances it once per tick.
"""
import numpy as np
from numpy.polynomial import polynomial as P

STANCE_THRESHOLD = 0.001      # WM/src/WalkingModule.cpp:657-658


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
