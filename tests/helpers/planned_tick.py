"""CPU restatement of the closed-loop tick in planned-trajectory mode (wcqp_tick_params.planned_trajectories): oracle/tick_spec.py's
run_ticks with per-tick kinematics, where everything the synthetic gait supplies comes from the planner's stage t instead - what
WalkingModule::updateTrajectories (WM/src/WalkingModule.cpp:1085-1145) pulls from TrajectoryGenerator:

  desired feet / twists        left_traj, right_traj [B][T][12], left_twist, right_twist [B][T][6]     (state 24..47, 75..86)
  desired CoM height, velocity com_height_traj / com_height_vel [B][T] (None: state0[68], 0)           (state 71, 74; :689, :695)
  desired neck orientation     RotZ(atan2(sin yL + sin yR, cos yL + cos yR)) @ additional_rotation,
                               y_f = atan2(R10, R00) of the desired foot rotation                       (57..65; :697-707, :383)
  floating-base anchor         the desired pose of the fixed-frame foot (contact bit 2)                 (:1147-1165)
  contact pair                 contact bits 0-1; a change of pair rebuilds the hull rows from that tick's desired feet

The loop is run_ticks' own, step for step, built from its pieces (qs, ks, hs, disturbance); the DCM controller is called as
tick_spec.qs.mpc_exact and the ZMP-CoM law reads p.k_com / p.k_zmp at the time of use, so reactive_tick.reactive_solve and
zmp_gains.scheduled_gains apply to it unchanged (`for t: for i` order, one solve per robot and tick).  No logger rows, no splices, no
external plant (the mode refuses them)."""
import numpy as np

from oracle import tick_spec

qs, ks, hs = tick_spec.qs, tick_spec.ks, tick_spec.hs

STATE = dict(pd_left=24, Rd_left=27, pd_right=36, Rd_right=39, Rd_neck=57, com_des_z=71, com_vel_z=74, twist_left=75, twist_right=81)


def neck_orientation(Rl, Rr, add_rot):
    """RotZ(meanYaw) @ add_rot for desired foot rotations Rl, Rr (row-major 9 or 3 x 3)."""
    Rl = np.asarray(Rl, float).reshape(3, 3); Rr = np.asarray(Rr, float).reshape(3, 3)
    yl, yr = np.arctan2(Rl[1, 0], Rl[0, 0]), np.arctan2(Rr[1, 0], Rr[0, 0])       # the asRPY yaw of run_ticks' rpy helper
    y = np.arctan2(np.sin(yl) + np.sin(yr), np.cos(yl) + np.cos(yr))
    c, s = np.cos(y), np.sin(y)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]) @ np.asarray(add_rot, float).reshape(3, 3)


def poses_host(model, kin_batch):
    """The pose block [B][87] the kinematics give at tick 0 (kin_spec, the oracle's twin of KinModel.jacobians_host)."""
    B = kin_batch["q"].shape[0]
    out = np.zeros((B, 87))
    for i in range(B):
        K = ks.jacobians(model, kin_batch["base"][i], kin_batch["q"][i])
        s = out[i]
        s[0:3] = K["p_left"]; s[3:12] = K["R_left"].reshape(9); s[12:15] = K["p_right"]; s[15:24] = K["R_right"].reshape(9)
        s[48:57] = K["R_neck"].reshape(9); s[66:69] = K["com"]
    return out


def synthetic_as_planned(p, data, T, add_rot):
    """The synthetic gait of `data` (synth_walk_batch) written out as planned trajectories over T stages: constant feet, the swing_profile
    twists, flags from contact_code and the stance side, constant height.  Returns (planned arrays, data with state0's Rd_neck set to the
    mean-yaw formula - what both runs then use).  Vectorised over robots and stages (tools/tick_controller_timing.py --planned uses it at
    8192 robots); the twists are run_ticks' products, operation for operation."""
    B = data["q0"].shape[0]
    st0 = np.array(data["state0"], float, copy=True)
    cyc = (np.arange(T)[None, :] + np.asarray(data["phase0"])[:, None]) % (2 * p.step_ticks)
    side, sidx = cyc // p.step_ticks, cyc % p.step_ticks
    code = np.where(sidx < p.ds_ticks, 2, side)                 # tick_spec.contact_code
    swing = sidx >= p.ds_ticks
    x = np.where(swing, (sidx - p.ds_ticks) / float(p.step_ticks - p.ds_ticks), 0.0)
    prof = np.where(swing, 10.392304845413264 * x * (1.0 - x) * (1.0 - 2.0 * x), 0.0)
    tw = np.asarray(data["swing_twist"], float)[:, None, :] * prof[..., None]
    ltw = np.where(((code == 0) | (code == 2))[..., None], 0.0, tw)
    rtw = np.where(((code == 1) | (code == 2))[..., None], 0.0, tw)
    contact = (np.choose(code, [1, 2, 3]) | np.where(side == 0, 4, 0)).astype(np.uint8)
    for i in range(B):
        st0[i, 57:66] = neck_orientation(st0[i, 27:36], st0[i, 39:48], add_rot).reshape(9)
    d = dict(data); d["state0"] = st0
    plan = dict(left_traj=np.repeat(st0[:, None, 24:36], T, axis=1), right_traj=np.repeat(st0[:, None, 36:48], T, axis=1),
                left_twist=np.ascontiguousarray(ltw), right_twist=np.ascontiguousarray(rtw), contact=np.ascontiguousarray(contact),
                com_height_traj=np.repeat(st0[:, 68:69], T, axis=1), com_height_vel=np.zeros((B, T)))
    return plan, d


def run_ticks_planned(p, data, plan, n_ticks, ik_params, kin_model, foot_rect, add_rot, ik_form="qpoases"):
    """run_ticks(kin_model=...) with the synthetic gait replaced by `plan` (left_traj, right_traj, left_twist, right_twist, contact and
    optionally com_height_traj / com_height_vel).  Returns run_ticks' per-tick logs and final states."""
    B = data["q0"].shape[0]
    N = p.horizon
    mp = qs.MPCParams(horizon=N, sampling_time=p.dT, com_height=p.com_height, gravity=p.gravity)
    c = qs.mpc_constants(mp)
    omega = np.sqrt(p.gravity / p.com_height)
    inst = np.arange(B, dtype=np.uint64) + np.uint64(data.get("first", 0))
    dcm = data["dcm0"].copy(); com = data["com0"].copy(); zmp_meas = data["u_init"].copy()
    u_prev = data["u_init"].copy()
    c_ref = data["com0"].copy(); v_ref_prev = np.zeros((B, 2))
    p_star = data["com0"].copy(); v_star_prev = np.zeros((B, 2))
    q_des = data["q0"].copy(); dq_prev = np.zeros((B, 23))
    u0_log = np.zeros((n_ticks, B, 2)); dq_log = np.zeros((n_ticks, B, 23))
    mpc_fail = np.zeros(B, np.int64); ik_fail = np.zeros(B, np.int64)
    state_now = data["state0"].copy()
    hull_cur = [None] * B; hull_code = -np.ones(B, np.int64)
    J_now = [None] * B
    h_traj = plan.get("com_height_traj"); h_vel = plan.get("com_height_vel")
    ident = np.concatenate([np.zeros(3), np.eye(3).reshape(9)])
    for t in range(n_ticks):
        flags = np.asarray(plan["contact"])[:, t].astype(np.int64)
        code = (flags & 3) - 1
        for i in range(B):
            s = state_now[i]
            s[24:36] = plan["left_traj"][i, t]; s[36:48] = plan["right_traj"][i, t]
            s[57:66] = neck_orientation(s[27:36], s[39:48], add_rot).reshape(9)
            side = 0 if flags[i] & 4 else 1
            pa, Ra = ks.forward(kin_model, ident, q_des[i])["frames"][side]
            sd = s[36:48] if side else s[24:36]
            Rb = sd[3:12].reshape(3, 3) @ Ra.T
            base = np.concatenate([sd[0:3] - Rb @ pa, Rb.reshape(9)])
            K = ks.jacobians(kin_model, base, q_des[i])
            J_now[i] = K
            s[0:3] = K["p_left"]; s[3:12] = K["R_left"].reshape(9); s[12:15] = K["p_right"]; s[15:24] = K["R_right"].reshape(9)
            s[48:57] = K["R_neck"].reshape(9); s[66:69] = K["com"]
            if int(code[i]) != hull_code[i]:
                k = int(code[i])
                hull_cur[i] = hs.hull_from_feet(foot_rect, s[24:36], s[36:48], {0: 1, 1: 2, 2: 3}[k])
                hull_code[i] = k
        r_t = data["ref_traj"][:, t, :]
        v_ref = -omega * (c_ref - r_t)
        c_ref = c_ref + 0.5 * p.dT * (v_ref + v_ref_prev); v_ref_prev = v_ref
        u0 = np.zeros((B, 2))
        for i in range(B):
            hA, hb, nc = hull_cur[i]
            try:
                u0[i] = tick_spec.qs.mpc_exact(c, dcm[i], data["ref_traj"][i, t:t + N + 1], u_prev[i], hA, hb, nc)["u0"]
            except qs.QPOracleError:
                u0[i] = u_prev[i]; mpc_fail[i] += 1
        v_star = p.k_com * (c_ref - com) - p.k_zmp * (u0 - zmp_meas) + v_ref
        p_star = p_star + 0.5 * p.dT * (v_star + v_star_prev); v_star_prev = v_star
        dq = np.zeros((B, 23))
        for i in range(B):
            s = state_now[i].copy()
            s[69:71] = p_star[i]
            s[71] = h_traj[i, t] if h_traj is not None else data["state0"][i][68]
            s[72:74] = v_star[i]
            s[74] = h_vel[i, t] if h_vel is not None else 0.0
            s[75:81] = plan["left_twist"][i, t]; s[81:87] = plan["right_twist"][i, t]
            one = dict(q=q_des[i:i + 1], state=s[None, :], **{n: J_now[i][n][None] for n in ("J_left", "J_right", "J_neck", "J_com")})
            if ik_fail[i] > 0:
                ik_fail[i] += 1
                continue
            try:
                dq[i] = qs.ik_exact(ik_params, qs.ik_inputs_from_batch(one, 0), ik_form)["dq"]
            except qs.QPOracleError:
                ik_fail[i] += 1
        q_des = q_des + 0.5 * p.dT * (dq + dq_prev); dq_prev = dq
        w = np.stack([tick_spec.disturbance(p.seed, inst, t, 0), tick_spec.disturbance(p.seed, inst, t, 1)], 1)
        com = com + p.dT * (-omega * (com - dcm))
        dcm = c.a * dcm + c.b * u0 + p.noise * w
        zmp_meas = u0.copy(); u_prev = u0.copy()
        u0_log[t] = u0; dq_log[t] = dq
    return dict(u0_log=u0_log, dq_log=dq_log, q_des=q_des, dcm=dcm, com=com, mpc_fail=mpc_fail, ik_fail=ik_fail)


def sole_poses(kin_model, q, plan, t):
    """Both soles' world poses at joint positions q[B][23] with the base anchored as tick t anchors it: (p [B][2][3], R [B][2][3][3])."""
    B = q.shape[0]
    ident = np.concatenate([np.zeros(3), np.eye(3).reshape(9)])
    P = np.zeros((B, 2, 3)); Rw = np.zeros((B, 2, 3, 3))
    for i in range(B):
        side = 0 if int(plan["contact"][i, t]) & 4 else 1
        fr = ks.forward(kin_model, ident, q[i])["frames"]
        pa, Ra = fr[side]
        sd = (plan["right_traj"] if side else plan["left_traj"])[i, t]
        Rb = sd[3:12].reshape(3, 3) @ Ra.T
        pb = sd[0:3] - Rb @ pa
        for f in range(2):
            P[i, f] = pb + Rb @ fr[f][0]; Rw[i, f] = Rb @ fr[f][1]
    return P, Rw
