"""THE SHAPED SWING of wcqp_tick_set_swing_profile (include/wcqp.h states it), restated in plain numpy from that definition: `shape`, the
six scalar functions of the swing phase, and `apply_profile`, which overlays a profile on an UNSHAPED restated plan - the dict
footstep_plan, footstep_plan_timed, footstep_replan or footstep_replan_timed returns.  The overlay is exact: a profile touches the swing
foot's height, rotation and twist and the CoM height of single-support stages and nothing else - neither ZMP and DCM nor a stage with both
feet down -, so it commutes with stitching and one overlay serves uploads and replans.  Also the profiles and the timed scenario of the GPU
tests."""
import numpy as np

ZERO = dict(apex_ratio=0.0, landing_velocity=0.0, pitch_delta=0.0, com_height_delta=0.0)
SHIPPED = dict(apex_ratio=0.8, landing_velocity=0.0, pitch_delta=0.0, com_height_delta=0.01)        # plannerParams.ini
ALL_FIELDS = dict(apex_ratio=0.8, landing_velocity=-0.05, pitch_delta=0.03, com_height_delta=0.01)
QUARTIC_PITCH = dict(apex_ratio=0.0, landing_velocity=0.0, pitch_delta=0.03, com_height_delta=0.0)
EARLY_APEX = dict(apex_ratio=0.3, landing_velocity=0.0, pitch_delta=0.0, com_height_delta=-0.005)
PROFILES = dict(shipped=SHIPPED, all_fields=ALL_FIELDS, quartic_pitch=QUARTIC_PITCH, early_apex=EARLY_APEX)


def _h(y):
    return 3.0 * y * y - 2.0 * y * y * y


def shape(profile, x, D, lift, branch=None):
    """At swing phase x in (0, 1] of a single support of duration D [s] with apex height `lift`: (z offset over p_z, vertical velocity,
    theta, theta rate, CoM height offset over h0, CoM height velocity), arrays like x.  branch: None - the definition's (x <= r rises) -,
    or "rise" / "fall" to evaluate that branch's formula wherever x lies (the two agree at x = r)."""
    x = np.asarray(x, float)
    r, v, pitch, dh = (float(profile[k]) for k in ("apex_ratio", "landing_velocity", "pitch_delta", "com_height_delta"))
    quartic, dquartic = 16.0 * x * x * (1.0 - x) ** 2, 32.0 * x * (1.0 - x) * (1.0 - 2.0 * x)
    land, vland = np.zeros_like(x), np.zeros_like(x)
    if r == 0.0:
        c, dc = quartic, dquartic
    else:
        ya = x / r
        yb = (x - r) / (1.0 - r)
        rise = (x <= r) if branch is None else np.full(x.shape, branch == "rise")
        c = np.where(rise, _h(ya), 1.0 - _h(yb))
        dc = np.where(rise, 6.0 * ya * (1.0 - ya) / r, -6.0 * yb * (1.0 - yb) / (1.0 - r))
        land = np.where(rise, 0.0, v * (1.0 - r) * D * (yb ** 3 - yb ** 2))
        vland = np.where(rise, 0.0, v * (3.0 * yb * yb - 2.0 * yb))           # d/dt: (1 - r) D (3 y^2 - 2 y) / ((1 - r) D)
    return lift * c + land, lift * dc / D + vland, pitch * c, pitch * dc / D, dh * quartic, dh * dquartic / D


def _ry(t):
    c, s = np.cos(t), np.sin(t)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def apply_profile(plan, starts, ss, side, profile, lift, dT):
    """plan: an unshaped restated plan; per robot i the steps whose single supports lie in it: starts[i][k] the first stage of step k's
    single support (a stage index of the plan's arrays), ss[i][k] its length, side[i][k] the foot that swings.  Returns the plan with the
    profile laid over those stages (a copy; every other entry the input's)."""
    out = dict(plan)
    for k in ("left_traj", "right_traj", "left_twist", "right_twist", "com_height_traj", "com_height_vel"):
        out[k] = np.array(plan[k], float, copy=True)
    T = out["com_height_traj"].shape[1]
    traj, twist = (out["left_traj"], out["right_traj"]), (out["left_twist"], out["right_twist"])
    for i in range(len(starts)):
        for s, n, sw in zip(starts[i], ss[i], side[i]):
            s, n, sw = int(s), int(n), int(sw)
            if s >= T:                                                                  # (a plan cut off by T)
                continue
            assert s >= 1 and (int(plan["contact"][i, s - 1]) & 3) == 3, (i, s)         # (the stage before: the foot on the ground, z = p_z)
            pz = plan[("left_traj", "right_traj")[sw]][i, s - 1, 2]
            for u in range(n):
                t = s + u
                if t >= T:
                    break
                assert (int(plan["contact"][i, t]) & 3) == (1 if sw == 1 else 2), (i, t)
                dz, vz, th, dth, dh, vh = (float(a) for a in shape(profile, (u + 1) / float(n), n * dT, lift))
                A = traj[sw][i, t, 3:].reshape(3, 3).copy()                             # Rz(dyaw m) R
                traj[sw][i, t, 2] = pz + dz
                traj[sw][i, t, 3:] = (A @ _ry(th)).reshape(9)
                twist[sw][i, t, 2] = vz
                twist[sw][i, t, 3:] = twist[sw][i, t, 3:] + A[:, 1] * dth
                out["com_height_traj"][i, t] = plan["com_height_traj"][i, t] + dh
                out["com_height_vel"][i, t] = vh
    return out


def uniform_steps(origin, first_ds, n_steps, ss, ds, sides):
    """(starts, ss, side) of untimed plans generated at stage origin[i] with n_steps[i] steps of ss + ds stages behind first_ds"""
    B = len(n_steps)
    org = np.broadcast_to(np.asarray(origin), (B,))
    return ([[int(org[i]) + first_ds + k * (ss + ds) for k in range(int(n_steps[i]))] for i in range(B)],
            [[ss] * int(n_steps[i]) for i in range(B)], [[int(sides[i][k]) for k in range(int(n_steps[i]))] for i in range(B)])


def timed_steps(origin, first_ds, n_steps, ssk, dsk, sides, final_ds=0):
    """the same of timed plans: step k lasts ssk[i][k] + dsk[i][k] stages (final_ds only moves the first standing stage)"""
    B = len(n_steps)
    org = np.broadcast_to(np.asarray(origin), (B,))
    starts = []
    for i in range(B):
        s, row = int(org[i]) + first_ds, []
        for k in range(int(n_steps[i])):
            row.append(s)
            s += int(ssk[i][k]) + int(dsk[i][k])
        starts.append(row)
    return (starts, [[int(ssk[i][k]) for k in range(int(n_steps[i]))] for i in range(B)],
            [[int(sides[i][k]) for k in range(int(n_steps[i]))] for i in range(B)])


def stitched_steps(old, merge_stage, new):
    """the steps of a stitched plan: robot i keeps the old steps whose single support ends at or below its merge stage (a merge stage lies
    in no single support) and takes the new ones; merge_stage -1: the old ones"""
    out = ([], [], [])
    for i, M in enumerate(merge_stage):
        M = int(M)
        keep = [k for k in range(len(old[0][i])) if M < 0 or old[0][i][k] + old[1][i][k] <= M]
        for a in range(3):
            out[a].append([old[a][i][k] for k in keep] + (list(new[a][i]) if M >= 0 else []))
    return out


def timed_small_footsteps(fs):
    """the timed counterpart of helpers/footstep_replan.small_footsteps (`fs`): the same 13 robots and footsteps, every step with durations
    of its own - single supports of 2 to 30 stages (robot 4's only step, and robot 1's second, last 2), double supports of 1 to 20"""
    rng = np.random.default_rng(31)
    shape_ = np.asarray(fs["side"]).shape
    ss = rng.integers(3, 31, size=shape_).astype(np.int32)
    ds = rng.integers(1, 21, size=shape_).astype(np.int32)
    ss[4, 0] = 2; ss[1, 1] = 2
    return dict(fs, ss_ticks=ss, ds_ticks=ds)
