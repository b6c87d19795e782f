"""THE SHAPED SWING (wcqp_tick_set_swing_profile) as helpers/swing_profile.py restates it - no GPU: the shape is C1 at the
apex, its end values, the analytic twists against central differences of the restated pose, the overlay of a zero profile, the monotone
descent condition the header states, and the binding's own refusals."""
import numpy as np
import pytest

from helpers import footstep_plan as fp
from helpers import footstep_plan_timed as ft
from helpers import footstep_replan as fr
from helpers import planned_tick as pt
from helpers import swing_profile as sp

LIFT, D = 0.02, 0.3
WITH_APEX = [k for k, p in sp.PROFILES.items() if p["apex_ratio"] > 0]


@pytest.mark.parametrize("name", WITH_APEX)
def test_shape_is_c1_at_the_apex(name):
    """at x = r both branches give the same six values - c0 = 1 with slope 0, the landing term 0 with slope 0 -, so the branch taken at
    equality does not matter; with ss = 30 and r = 0.8 stage u = 23 sits exactly on the joint"""
    p = sp.PROFILES[name]
    r = p["apex_ratio"]
    rise, fall = sp.shape(p, r, D, LIFT, "rise"), sp.shape(p, r, D, LIFT, "fall")
    for a, b in zip(rise, fall):
        assert float(a) == float(b), (a, b)
    assert float(rise[0]) == LIFT and float(rise[1]) == 0.0 and float(rise[2]) == p["pitch_delta"] and float(rise[3]) == 0.0
    assert (23 + 1) / 30.0 == 0.8
    assert [float(a) for a in sp.shape(sp.SHIPPED, 24 / 30.0, D, LIFT)] == [float(a) for a in sp.shape(sp.SHIPPED, 24 / 30.0, D, LIFT, "fall")]


@pytest.mark.parametrize("name", sorted(sp.PROFILES))
def test_end_values(name):
    """x = 1, the landing stage: z offset 0, vertical velocity exactly landing_velocity, theta 0, height offset 0 - for every duration"""
    p = sp.PROFILES[name]
    for d in (0.02, 0.3, 1.7):
        dz, vz, th, dth, dh, vh = (float(a) for a in sp.shape(p, 1.0, d, LIFT))
        assert dz == 0.0 and vz == p["landing_velocity"] and th == 0.0 and dh == 0.0 and vh == 0.0, (d, dz, vz, th, dh, vh)


def _pose(p, x, dyaw, R0):
    """the restated swing pose at phase x (an array): z offset [n], rotation [n][3][3] = Rz(dyaw m) R0 Ry(theta), CoM height offset [n]"""
    dz, _, th, _, dh, _ = sp.shape(p, x, D, LIFT)
    m = x ** 3 * (10.0 - 15.0 * x + 6.0 * x * x)
    R = np.stack([fp._rz(dyaw * mm) @ R0 @ sp._ry(t) for mm, t in zip(m, th)])
    return dz, R, dh


@pytest.mark.parametrize("name", sorted(sp.PROFILES))
def test_analytic_twists_are_the_derivatives_of_the_pose(name):
    """Central differences with h = 1e-5 in x of the restated pose - height, rotation (the antisymmetric part of R(x + h) R(x - h)^T over
    2 h), CoM height - against the analytic twists, relative to each twist's largest value over the swing: 1e-6.  The truncation error is
    h^2 / 6 times the third derivative, at most 12 / (1 - r)^3 = 1500 for r = 0.8 against first derivatives of order 1.5 / (1 - r) = 7.5: a
    relative 3e-9; rounding adds 1e-16 / h = 1e-11.  The second derivative jumps at x = r (the shape is C1, not C2), so grid points within
    2 h of r are left out: a difference across the joint is first order."""
    p = sp.PROFILES[name]
    h, dyaw = 1e-5, 0.07
    R0 = fp._rz(0.3) @ sp._ry(0.02)
    x = np.linspace(0.001, 0.999, 1997)
    x = x[np.abs(x - p["apex_ratio"]) > 2 * h]
    _, vz, _, dth, _, vh = sp.shape(p, x, D, LIFT)
    (za, Ra, ha), (zb, Rb, hb) = _pose(p, x - h, dyaw, R0), _pose(p, x + h, dyaw, R0)
    m1 = 30.0 * x * x * (1.0 - x) ** 2
    A = np.stack([fp._rz(dyaw * mm) @ R0 for mm in x ** 3 * (10.0 - 15.0 * x + 6.0 * x * x)])
    omega = np.array([0.0, 0.0, 1.0])[None, :] * (dyaw * m1 / D)[:, None] + A[:, :, 1] * dth[:, None]
    S = np.einsum("nij,nkj->nik", Rb, Ra)
    num = np.stack([S[:, 2, 1] - S[:, 1, 2], S[:, 0, 2] - S[:, 2, 0], S[:, 1, 0] - S[:, 0, 1]], 1) / 2.0 / (2.0 * h * D)
    for what, got, want in (("vz", (zb - za) / (2.0 * h * D), vz), ("omega", num, omega), ("vh", (hb - ha) / (2.0 * h * D), vh)):
        scale = np.abs(want).max()
        err = np.abs(got - want).max() / scale if scale > 0 else np.abs(got).max()
        print(name, what, err)
        assert err <= 1e-6, (what, err)


def test_zero_profile_leaves_a_plan_as_it_is(wca):
    """the overlay of the all-zero profile returns the unshaped plan bit for bit: untimed, timed and stitched"""
    fs = fr.small_footsteps(wca, pt)
    T = fr.MAXT + 51
    plan0, (M1, rp1, plan1), _ = fr.small_replans(fs)
    steps0 = sp.uniform_steps(0, fr.FIRST_DS, fs["n_steps"], fr.SS, fr.DS, fs["side"])
    steps1 = sp.stitched_steps(steps0, M1, sp.uniform_steps(M1, fr.FD1, rp1["n_steps"], fr.SS, fr.DS, rp1["side"]))
    tfs = sp.timed_small_footsteps(fs)
    tplan = ft.footstep_plan_timed(tfs, fs["state0"], T, fr.MAXT)
    tsteps = sp.timed_steps(0, fr.FIRST_DS, tfs["n_steps"], tfs["ss_ticks"], tfs["ds_ticks"], tfs["side"])
    assert [s[:-1] for s in tplan["starts"]] == tsteps[0] and min(min(r) for r in tsteps[1] if r) == 2
    for plan, steps in ((plan0, steps0), (plan1, steps1), (tplan, tsteps)):
        got = sp.apply_profile(plan, *steps, sp.ZERO, fs["lift"], 0.01)
        for k in fr.PLAN_KEYS:
            assert np.array_equal(got[k], plan[k]), k
        # ... and a profile moves swing stages only, none of ZMP and DCM
        shaped = sp.apply_profile(plan, *steps, sp.ALL_FIELDS, fs["lift"], 0.01)
        both = (plan["contact"] & 3) == 3
        for k in fr.PLAN_KEYS:
            assert np.array_equal(shaped[k][both], plan[k][both]), k
        for k in ("contact", "ref_traj", "dcm_vel_traj", "zmp_ref"):
            assert np.array_equal(shaped[k], plan[k]), k
        for k in ("left_traj", "right_traj"):
            assert np.array_equal(shaped[k][..., :2], plan[k][..., :2]), k
        assert not np.array_equal(shaped["com_height_traj"], plan["com_height_traj"])


def test_monotone_descent_condition():
    """the descent from the apex is monotone iff |landing_velocity| (1 - r) D <= 3 lift: with V = v (1 - r) D <= 0 the derivative of the
    height in y is y (-6 lift (1 - y) + V (3 y - 2)), whose bracket is linear in y, V <= 0 at y = 1 and -6 lift - 2 V at y = 0"""
    r = 0.8
    x = np.linspace(r, 1.0, 4001)[1:]
    for factor, monotone in ((0.0, True), (2.9, True), (3.0, True), (3.1, False), (6.0, False)):
        v = -factor * LIFT / ((1.0 - r) * D)
        p = dict(sp.ZERO, apex_ratio=r, landing_velocity=v)
        dz, vz = sp.shape(p, x, D, LIFT)[:2]
        assert (vz.max() <= 1e-15) == monotone, (factor, vz.max())
        assert (np.diff(dz).max() <= 1e-18) == monotone, factor


def test_binding(wca):
    """the symbols are exported and refuse NULL; synth ships plannerParams.ini's profile"""
    import ctypes as C
    lib = wca.capi.lib()
    p = wca.capi.TickSwingProfile()
    assert lib.wcqp_tick_set_swing_profile(None, C.byref(p)) == wca.capi.E_INVALID
    assert lib.wcqp_tick_get_swing_profile(None, C.byref(p)) == wca.capi.E_INVALID
    assert wca.synth.shipped_swing_profile() == sp.SHIPPED
    assert wca.capi.TICK_OPT_SWING_PROFILE == 5
