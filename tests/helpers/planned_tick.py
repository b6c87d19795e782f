"""Scenario builders for the planned-trajectory mode of the closed-loop tick (wcqp_tick_params.planned_trajectories).  The restatement
is oracle/tick_spec.py::run_ticks(stages=...): these build what it and the device are fed (the synthetic gait written out as the planner's
arrays, the pose block of tick 0) and read a finished walk back (sole_poses)."""
import numpy as np

from oracle import kin_spec as ks
from oracle.tick_spec import neck_orientation


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
