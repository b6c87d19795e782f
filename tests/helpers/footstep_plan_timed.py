"""The timed plan of wcqp_tick_upload_footsteps_timed and the timed replan of wcqp_tick_replan_footsteps_timed (include/wcqp.h states both),
restated in plain numpy with per-robot loops next to helpers/footstep_plan.py and helpers/footstep_replan.py, whose wording they keep:
step k of robot i lasts fs["ss_ticks"][i, k] + fs["ds_ticks"][i, k] stages, the last step's double support final_ds_ticks stages or -
0 / missing - its own ds; fs["ss_ticks"] / fs["ds_ticks"] are [B][K] arrays here.  With every step's durations equal the results are
those of footstep_plan / footstep_replan, bit for bit."""
import numpy as np

from helpers import footstep_plan as fp
from helpers import footstep_replan as fr


def step_starts(first_ds, ss, ds, n, final_ds):
    """[n + 1]: s_k, the first stage of step k's single support on the plan's own timeline, then the first standing stage"""
    s = [int(first_ds)]
    for k in range(n):
        s.append(s[-1] + int(ss[k]) + (int(final_ds) if (k == n - 1 and final_ds > 0) else int(ds[k])))
    return s


def footstep_plan_timed(fs, state0, T, max_ticks, dT=0.01, com_height=0.53, gravity=9.81):
    n_steps, side, target = np.asarray(fs["n_steps"]), np.asarray(fs["side"]), np.asarray(fs["target"], float)
    ssk, dsk = np.asarray(fs["ss_ticks"]), np.asarray(fs["ds_ticks"])
    B = n_steps.shape[0]
    assert ssk.shape == side.shape and dsk.shape == side.shape, (ssk.shape, dsk.shape, side.shape)
    first_ds = int(fs["first_ds_ticks"])
    final_ds = int(fs.get("final_ds_ticks", 0))
    lift = float(fs["lift"])
    delta = (np.asarray(fs["zmp_delta_left"], float), np.asarray(fs["zmp_delta_right"], float))
    omega = np.sqrt(gravity / com_height)
    a = np.exp(omega * dT)
    feet = np.zeros((B, 2, T, 12)); tw = np.zeros((B, 2, T, 6))
    contact = np.zeros((B, T), np.uint8)
    ref = np.zeros((B, T, 2)); zmp_ref = np.zeros((B, T, 2))
    change = np.zeros(B, np.int64)
    starts = []
    for i in range(B):
        n = int(n_steps[i])
        assert all(ssk[i, k] >= 1 and dsk[i, k] >= 1 for k in range(n)), i
        # the footprint chain: both feet after j landed steps, and their ZMP points
        p = [state0[i, 24:27].copy(), state0[i, 36:39].copy()]
        R = [state0[i, 27:36].reshape(3, 3).copy(), state0[i, 39:48].reshape(3, 3).copy()]
        chain = [([p[0].copy(), p[1].copy()], [R[0].copy(), R[1].copy()])]
        for k in range(n):
            sw = int(side[i, k])
            p[sw] = np.array([target[i, k, 0], target[i, k, 1], p[sw][2]])
            R[sw] = fp._rz(target[i, k, 2]) @ R[sw]
            chain.append(([p[0].copy(), p[1].copy()], [R[0].copy(), R[1].copy()]))
        zp = [[c[0][f][:2] + c[1][f][:2, :2] @ delta[f] for f in range(2)] for c in chain]
        s = step_starts(first_ds, ssk[i], dsk[i], n, final_ds)
        starts.append(s)
        s_end = s[n]                                                               # the first standing stage
        step_of = np.full(max(T, s_end + 1), -1)                                   # the step a stage lies in: -1 before the first, n - 1 from the last on
        for k in range(n):
            step_of[s[k]:] = k
        Tz = max(T, s_end + 1)
        zmp = np.zeros((Tz, 2))
        for t in range(Tz):
            if t >= s_end:
                zmp[t] = 0.5 * (zp[n][0] + zp[n][1])
            elif t < first_ds:
                za = 0.5 * (zp[0][0] + zp[0][1])
                zb = zp[0][1 - int(side[i, 0])] if n > 0 else za
                zmp[t] = za + (t + 1) / float(first_ds + 1) * (zb - za)
            else:
                k = int(step_of[t])
                u = t - s[k]
                ss = int(ssk[i, k])
                if u < ss:
                    zmp[t] = zp[k][1 - int(side[i, k])]
                else:
                    za = zp[k + 1][1 - int(side[i, k])]
                    zb = zp[k + 1][1 - int(side[i, k + 1])] if k < n - 1 else 0.5 * (zp[n][0] + zp[n][1])
                    nds = s[k + 1] - s[k] - ss                                     # (the last step's: final_ds_ticks, or its own ds)
                    zmp[t] = za + (u - ss + 1) / float(nds + 1) * (zb - za)
        xi = np.zeros((Tz, 2))
        xi[s_end:] = zmp[s_end:]
        for t in range(min(s_end, Tz) - 1, -1, -1):
            xi[t] = (xi[t + 1] - (1.0 - a) * zmp[t]) / a
        ref[i] = xi[:T]; zmp_ref[i] = zmp[:T]
        prev_pair = -1
        for t in range(T):
            k = int(step_of[t])
            u = t - s[k] if k >= 0 else 0
            ss = int(ssk[i, k]) if k >= 0 else 1
            swinging = k >= 0 and u < ss
            j = 0 if k < 0 else k + (0 if swinging else 1)
            pos = [chain[j][0][0].copy(), chain[j][0][1].copy()]; rot = [chain[j][1][0].copy(), chain[j][1][1].copy()]
            flags = 3
            fixed = 1 - int(side[i, k]) if k >= 0 else 0
            if swinging:
                sw = int(side[i, k])
                p0, R0, p1 = chain[k][0][sw], chain[k][1][sw], chain[k + 1][0][sw]
                x = (u + 1) / float(ss)
                m = x ** 3 * (10.0 - 15.0 * x + 6.0 * x * x); dm = 30.0 * x * x * (1.0 - x) ** 2
                lz = 16.0 * x * x * (1.0 - x) ** 2; dlz = 32.0 * x * (1.0 - x) * (1.0 - 2.0 * x)
                dyaw = target[i, k, 2]
                pos[sw] = p0 + (p1 - p0) * m + np.array([0.0, 0.0, lift * lz])
                rot[sw] = fp._rz(dyaw * m) @ R0
                v = ((p1 - p0) * dm + np.array([0.0, 0.0, lift * dlz])) / (ss * dT)
                tw[i, sw, t] = np.concatenate([v, [0.0, 0.0, dyaw * dm / (ss * dT)]])
                flags = 1 if sw == 1 else 2
            contact[i, t] = flags | (4 if fixed == 0 else 0)
            for f in range(2):
                feet[i, f, t, :3] = pos[f]; feet[i, f, t, 3:] = rot[f].reshape(9)
            if t <= max_ticks and flags != prev_pair:
                change[i] = t
                prev_pair = flags
    vel = omega * (ref - zmp_ref)
    h0 = np.repeat(state0[:, 68:69], T, axis=1)
    return dict(left_traj=np.ascontiguousarray(feet[:, 0]), right_traj=np.ascontiguousarray(feet[:, 1]),
                left_twist=np.ascontiguousarray(tw[:, 0]), right_twist=np.ascontiguousarray(tw[:, 1]), contact=contact,
                com_height_traj=np.ascontiguousarray(h0), com_height_vel=np.zeros((B, T)), ref_traj=ref, dcm_vel_traj=vel, zmp_ref=zmp_ref,
                change=change, starts=starts)


def uniform(fs, K=None):
    """fs with its two common tick counts spread over [B][K] arrays: the timed call's arguments for an untimed walk"""
    shape = np.asarray(fs["side"]).shape if K is None else (np.asarray(fs["n_steps"]).shape[0], K)
    return dict(fs, ss_ticks=np.full(shape, int(fs["ss_ticks"]), np.int32), ds_ticks=np.full(shape, int(fs["ds_ticks"]), np.int32))


def footstep_replan_timed(plan, fs, merge_stage, rp, T, max_ticks, dT=0.01, com_height=0.53, gravity=9.81):
    """footstep_replan on per-step timelines.  plan: the plan in force (merge stages are checked against ITS contact flags: both feet
    down); fs: the handle's footstep parameters (final_ds_ticks, lift, zmp_delta_*; its ss_ticks / ds_ticks are not read); merge_stage [B]
    (-1: the robot keeps its plan); rp: n_steps [B], side [B][K'], target [B][K'][3], ss_ticks, ds_ticks [B][K'], first_ds_ticks.
    Returns the stitched plan (same keys, `change` recomputed) and `a` [B][2], the solved start point of the first double support's ramp."""
    out = {k: np.array(plan[k], copy=True) for k in fr.PLAN_KEYS}
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
                      ss_ticks=np.asarray(rp["ss_ticks"])[i:i + 1], ds_ticks=np.asarray(rp["ds_ticks"])[i:i + 1], first_ds_ticks=fd)
        Ts = max(T - M, fd + 1)
        sub = footstep_plan_timed(sub_fs, st, Ts, max(max_ticks - M, 0), dT, com_height, gravity)
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
    out["change"] = fr.changes_of(out["contact"], max_ticks)
    out["a"] = a_sol
    return out
