"""The plan wcqp_tick_upload_footsteps generates (include/wcqp.h states it), restated in plain numpy with per-robot loops: from the footstep
arrays to the arrays wcqp_tick_upload takes - left_traj, right_traj, left_twist, right_twist, contact, com_height_traj, com_height_vel,
ref_traj, dcm_vel_traj - plus zmp_ref and, for the checks, `change` [B]: the last stage <= max_ticks at which the contact pair changes."""
import numpy as np


def _rz(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def footstep_plan(fs, state0, T, max_ticks, dT=0.01, com_height=0.53, gravity=9.81):
    n_steps, side, target = np.asarray(fs["n_steps"]), np.asarray(fs["side"]), np.asarray(fs["target"], float)
    B = n_steps.shape[0]
    first_ds, ss, ds = int(fs["first_ds_ticks"]), int(fs["ss_ticks"]), int(fs["ds_ticks"])
    final_ds = int(fs.get("final_ds_ticks", 0)) or ds
    lift = float(fs["lift"])
    delta = (np.asarray(fs["zmp_delta_left"], float), np.asarray(fs["zmp_delta_right"], float))
    per = ss + ds
    omega = np.sqrt(gravity / com_height)
    a = np.exp(omega * dT)
    feet = np.zeros((B, 2, T, 12)); tw = np.zeros((B, 2, T, 6))
    contact = np.zeros((B, T), np.uint8)
    ref = np.zeros((B, T, 2)); zmp_ref = np.zeros((B, T, 2))
    change = np.zeros(B, np.int64)
    for i in range(B):
        n = int(n_steps[i])
        # the footprint chain: both feet after j landed steps, and their ZMP points
        p = [state0[i, 24:27].copy(), state0[i, 36:39].copy()]
        R = [state0[i, 27:36].reshape(3, 3).copy(), state0[i, 39:48].reshape(3, 3).copy()]
        chain = [([p[0].copy(), p[1].copy()], [R[0].copy(), R[1].copy()])]
        for k in range(n):
            sw = int(side[i, k])
            p[sw] = np.array([target[i, k, 0], target[i, k, 1], p[sw][2]])
            R[sw] = _rz(target[i, k, 2]) @ R[sw]
            chain.append(([p[0].copy(), p[1].copy()], [R[0].copy(), R[1].copy()]))
        zp = [[c[0][f][:2] + c[1][f][:2, :2] @ delta[f] for f in range(2)] for c in chain]
        s_end = first_ds + n * per - ds + final_ds if n > 0 else first_ds          # the first standing stage
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
                k = min((t - first_ds) // per, n - 1)
                u = t - first_ds - k * per
                if u < ss:
                    zmp[t] = zp[k][1 - int(side[i, k])]
                else:
                    za = zp[k + 1][1 - int(side[i, k])]
                    zb = zp[k + 1][1 - int(side[i, k + 1])] if k < n - 1 else 0.5 * (zp[n][0] + zp[n][1])
                    nds = final_ds if k == n - 1 else ds
                    zmp[t] = za + (u - ss + 1) / float(nds + 1) * (zb - za)
        xi = np.zeros((Tz, 2))
        xi[s_end:] = zmp[s_end:]
        for t in range(min(s_end, Tz) - 1, -1, -1):
            xi[t] = (xi[t + 1] - (1.0 - a) * zmp[t]) / a
        ref[i] = xi[:T]; zmp_ref[i] = zmp[:T]
        prev_pair = -1
        for t in range(T):
            k = (t - first_ds) // per if t >= first_ds else -1
            u = (t - first_ds) - k * per if k >= 0 else 0
            swinging = 0 <= k < n and u < ss
            j = 0 if k < 0 else (k + (0 if swinging else 1) if k < n else n)
            pos = [chain[j][0][0].copy(), chain[j][0][1].copy()]; rot = [chain[j][1][0].copy(), chain[j][1][1].copy()]
            flags = 3
            fixed = 1 - int(side[i, min(k, n - 1)]) if (k >= 0 and n > 0) else 0
            if swinging:
                sw = int(side[i, k])
                p0, R0, p1 = chain[k][0][sw], chain[k][1][sw], chain[k + 1][0][sw]
                x = (u + 1) / float(ss)
                m = x ** 3 * (10.0 - 15.0 * x + 6.0 * x * x); dm = 30.0 * x * x * (1.0 - x) ** 2
                lz = 16.0 * x * x * (1.0 - x) ** 2; dlz = 32.0 * x * (1.0 - x) * (1.0 - 2.0 * x)
                dyaw = target[i, k, 2]
                pos[sw] = p0 + (p1 - p0) * m + np.array([0.0, 0.0, lift * lz])
                rot[sw] = _rz(dyaw * m) @ R0
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
                change=change)
