"""The plan wcqp_tick_replan_footsteps leaves behind (include/wcqp.h states it), restated in plain numpy on top of helpers/footstep_plan.py:
`footstep_replan` takes a plan (the dict footstep_plan returns) and gives back the stitched one.  Also the small scenario of the GPU tests:
13 robots whose replans cover every case the record and DCM passes distinguish."""
import numpy as np

from helpers import footstep_plan as fp

PLAN_KEYS = ("left_traj", "right_traj", "left_twist", "right_twist", "contact", "com_height_traj", "com_height_vel", "ref_traj", "dcm_vel_traj",
             "zmp_ref")
# the small scenario (tests/test_tick_footsteps.py's): steps of 30 + 20 stages behind 20, T = 186 with N = 50
B13, MAXT, FIRST_DS, SS, DS, K = 13, 135, 20, 30, 20, 4


def changes_of(contact, max_ticks):
    """per robot the last stage <= max_ticks at which the contact pair changes (the classic upload's rule; stage 0 counts)"""
    pair = contact[:, :max_ticks + 1] & 3
    out = np.zeros(contact.shape[0], np.int64)
    for i in range(contact.shape[0]):
        ch = np.nonzero(pair[i, 1:] != pair[i, :-1])[0]
        out[i] = ch[-1] + 1 if ch.size else 0
    return out


def footstep_replan(plan, fs, merge_stage, rp, T, max_ticks, dT=0.01, com_height=0.53, gravity=9.81):
    """plan: the plan in force; fs: the handle's footstep parameters (ss_ticks, ds_ticks, final_ds_ticks, lift, zmp_delta_*);
    merge_stage [B] (-1: the robot keeps its plan); rp: n_steps [B], side [B][K'], target [B][K'][3], first_ds_ticks.
    Returns the stitched plan (same keys, `change` recomputed) and `a` [B][2], the solved start point of the first double support's ramp."""
    out = {k: np.array(plan[k], copy=True) for k in PLAN_KEYS}
    B = out["contact"].shape[0]
    fd = int(rp["first_ds_ticks"])
    omega = np.sqrt(gravity / com_height)
    A = np.exp(omega * dT)
    delta = (np.asarray(fs["zmp_delta_left"], float), np.asarray(fs["zmp_delta_right"], float))
    a_sol = np.full((B, 2), np.nan)
    for i in range(B):
        M = int(merge_stage[i])
        if M < 0:
            continue
        assert 1 <= M < T and (int(plan["contact"][i, M]) & 3) == 3, (i, M)
        n = int(rp["n_steps"][i])
        # the rules of the upload with stage 0 moved to M: the start footprints are record M's desired soles
        st = np.zeros((1, 87))
        st[0, 24:36] = plan["left_traj"][i, M]; st[0, 36:48] = plan["right_traj"][i, M]; st[0, 68] = plan["com_height_traj"][i, M]
        sub_fs = dict(fs, n_steps=np.array([n]), side=np.asarray(rp["side"])[i:i + 1], target=np.asarray(rp["target"], float)[i:i + 1],
                      first_ds_ticks=fd)
        Ts = max(T - M, fd + 1)
        sub = fp.footstep_plan(sub_fs, st, Ts, max(max_ticks - M, 0), dT, com_height, gravity)
        m = T - M
        for k in ("left_traj", "right_traj", "left_twist", "right_twist", "com_height_traj", "com_height_vel"):
            out[k][i, M:] = sub[k][0, :m]
        # the fixed-frame bit keeps stage M - 1's value before the first new single support (everywhere when no step is taken)
        c = sub["contact"][0, :m].copy()
        keep = m if n == 0 else min(fd, m)
        c[:keep] = (c[:keep] & 3) | (int(plan["contact"][i, M - 1]) & 4)
        out["contact"][i, M:] = c
        # the first double support's ZMP ramp a -> b, a such that the recursion arrives at the old ref[M]
        zp = [st[0, 24:26] + st[0, 27:36].reshape(3, 3)[:2, :2] @ delta[0], st[0, 36:38] + st[0, 39:48].reshape(3, 3)[:2, :2] @ delta[1]]
        b = zp[1 - int(rp["side"][i][0])] if n > 0 else 0.5 * (zp[0] + zp[1])
        X = sub["ref_traj"][0, fd]
        q = 1.0 / A
        S0 = sum(q ** j for j in range(1, fd + 1))
        S1 = sum(j * q ** j for j in range(1, fd + 1)) / (fd + 1.0)
        a = (X * q ** fd + (A - 1.0) * b * S1 - plan["ref_traj"][i, M]) / (-(A - 1.0) * (S0 - S1))
        a_sol[i] = a
        zmp = np.array(sub["zmp_ref"][0]); xi = np.array(sub["ref_traj"][0])
        for u in range(fd - 1, -1, -1):
            zmp[u] = a + (u + 1) / float(fd + 1) * (b - a)
            xi[u] = (xi[u + 1] - (1.0 - A) * zmp[u]) / A
        out["ref_traj"][i, M:] = xi[:m]; out["zmp_ref"][i, M:] = zmp[:m]
        out["dcm_vel_traj"][i, M:] = omega * (xi[:m] - zmp[:m])
    out["change"] = changes_of(out["contact"], max_ticks)
    out["a"] = a_sol
    return out


def small_footsteps(wca, pt):
    """the 13-robot scenario of tests/test_tick_footsteps.py: 0 to K steps, a foot twice in a row, both signs of yaw"""
    kb = wca.synth.synth_walk_kin_batch(B13)
    poses = pt.poses_host(wca.synth.icub_like_model(), kb)
    fs = wca.synth.synth_footstep_walk_batch(B13, MAXT, poses, kb)
    rng = np.random.default_rng(5)
    n_steps = np.array([0, 4, 4, 2, 1, 3, 4, 0, 2, 4, 3, 1, 4], np.int32)
    side = np.tile(np.array([1, 0, 1, 0], np.uint8), (B13, 1))
    side[2] = (1, 1, 0, 0); side[5] = (0, 0, 0, 1); side[9] = (0, 1, 1, 0)
    target = np.zeros((B13, K, 3))
    st = fs["state0"]
    for i in range(B13):
        p = [st[i, 24:26].copy(), st[i, 36:38].copy()]
        yaw = [np.arctan2(st[i, 33], st[i, 27]), np.arctan2(st[i, 45], st[i, 39])]
        for k in range(K):
            sw = side[i, k]
            inc = rng.uniform(0.02, 0.06) * (1.0 if (i + k) % 3 else -1.0)
            yaw[sw] += inc
            p[sw] = p[sw] + rng.uniform(0.015, 0.03) * np.array([np.cos(yaw[sw]), np.sin(yaw[sw])])
            target[i, k] = (p[sw][0], p[sw][1], inc)
    target[n_steps[:, None] <= np.arange(K)[None, :]] = 1e3
    fs.update(n_steps=n_steps, side=side, target=target, first_ds_ticks=FIRST_DS, ss_ticks=SS, ds_ticks=DS, final_ds_ticks=0, lift=0.02)
    return fs


def new_steps(plan, merge_stage, n_steps, sides, first_ds_ticks, seed):
    """footsteps from the footprints the plan holds at each robot's merge stage: short steps along the swinging foot's new heading, yaw
    increments of both signs; rows of robots that keep their plan, and steps a robot does not take, hold 1e3 (they are not read)"""
    rng = np.random.default_rng(seed)
    B, Kp = len(merge_stage), np.asarray(sides).shape[1]
    target = np.full((B, Kp, 3), 1e3)
    for i in range(B):
        M = int(merge_stage[i])
        if M < 0:
            continue
        L, R = plan["left_traj"][i, M], plan["right_traj"][i, M]
        p = [L[:2].copy(), R[:2].copy()]
        yaw = [np.arctan2(L[6], L[3]), np.arctan2(R[6], R[3])]
        for k in range(int(n_steps[i])):
            sw = int(sides[i][k])
            inc = rng.uniform(0.02, 0.06) * (1.0 if (i + k) % 2 else -1.0)
            yaw[sw] += inc
            p[sw] = p[sw] + rng.uniform(0.015, 0.03) * np.array([np.cos(yaw[sw]), np.sin(yaw[sw])])
            target[i, k] = (p[sw][0], p[sw][1], inc)
    return dict(n_steps=np.asarray(n_steps, np.int32), side=np.asarray(sides, np.uint8), target=target, first_ds_ticks=int(first_ds_ticks))


# The two replans of the small scenario (old timeline: single supports [20, 50) [70, 100) [120, 150) [170, 200), double supports between).
#   robot  old n   M1                                           new steps
#   0      0       -1   keeps its plan
#   1      4       60   the middle of a double support            2
#   2      4       50   the first stage of a double support       2, the left foot twice in a row
#   3      2       64   a tile edge of the record pass            3
#   4      1       128  a tile edge; standing, the old plan over  1
#   5      3       65   just past a tile edge                     2
#   6      4       110                                            0: come to a stop
#   7      0       100  standing                                  3: cut by T mid-swing (162..192 of 186), changes of pair at 142, 162 > max_ticks
#   8      2       129  just past a tile edge; standing           1
#   9      4       -1   keeps its plan
#   10     3       105                                            2
#   11     1       55                                             4
#   12     4       100  the first stage of a double support       1
M1 = np.array([-1, 60, 50, 64, 128, 65, 110, 100, 129, -1, 105, 55, 100], np.int32)
N1 = np.array([0, 2, 2, 3, 1, 2, 0, 3, 1, 0, 2, 4, 1], np.int32)
S1 = np.tile(np.array([0, 1, 0, 1], np.uint8), (B13, 1))
S1[2] = (0, 0, 1, 0); S1[7] = (1, 0, 1, 0); S1[10] = (1, 0, 1, 0)
FD1 = 12
# the second replan, of robots the first one touched, at a later stage of their NEW plans (robot 1: 60 + 12 + 30 = 102 .. 122 is a double
# support; robot 11: 55 + 12 + 30 = 97 .. 117; robot 7: 142 .. 162, past max_ticks; robot 6 stands) - and robot 9's first
M2 = np.array([-1, 110, -1, -1, -1, -1, 140, 150, -1, 100, -1, 100, -1], np.int32)
N2 = np.array([0, 1, 0, 0, 0, 0, 2, 1, 0, 2, 0, 0, 0], np.int32)
S2 = np.tile(np.array([1, 0], np.uint8), (B13, 1))
FD2 = 7


def small_replans(fs, T=MAXT + 51):
    """the small scenario's plan, its two replans' arguments and the stitched plans after each: (plan0, (M1, rp1, plan1), (M2, rp2, plan2))"""
    plan0 = fp.footstep_plan(fs, fs["state0"], T, MAXT)
    rp1 = new_steps(plan0, M1, N1, S1, FD1, 21)
    plan1 = footstep_replan(plan0, fs, M1, rp1, T, MAXT)
    rp2 = new_steps(plan1, M2, N2, S2, FD2, 22)
    plan2 = footstep_replan(plan1, fs, M2, rp2, T, MAXT)
    return plan0, (M1, rp1, plan1), (M2, rp2, plan2)
