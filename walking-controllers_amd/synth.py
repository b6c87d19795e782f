"""
Synthetic iCub-shaped workloads in the batch
layouts of the C ABI (`include/wcqp.h`).

Every number depends only on (seed, global instance index, slot), through a
counter-based 64-bit mixer, so any shard [first, first+count) of a batch is
bit-identical to the same rows of the full batch whatever the shard count —
this is what lets the multi-GPU path be checked for shard-count invariance.

The constants are the values shipped in the reference's
app/robots/iCubGazeboV2_5/{controllerParams,qpInverseKinematics,plannerParams}.ini
(values only; no parser is reproduced here).
"""
from __future__ import annotations

import numpy as np

HULL_ROWS = 8            # hull rows are padded to 8 per instance (n_c in 4..8)
HULL_PAD_B = 1e30        # padded rows: 0*u <= +OsqpEigen::INFTY
IK_STATE_LEN = 87        # packed pose block, see IK_STATE_OFFSETS

# offsets inside the packed per-instance IK state block (doubles)
IK_STATE_OFFSETS = dict(
    p_left=0, R_left=3, p_right=12, R_right=15,
    pd_left=24, Rd_left=27, pd_right=36, Rd_right=39,
    R_neck=48, Rd_neck=57,
    com=66, com_des=69, com_vel_des=72,
    twist_left=75, twist_right=81,
)

FOOT_X = (-0.02, 0.05)       # controllerParams.ini:7  foot_size
FOOT_Y = (-0.025, 0.025)
# the four corners (x, y) of the foot rectangle in the foot frame, in the order foot_corners() walks them
FOOT_RECT = np.array([FOOT_X[1], FOOT_Y[1], FOOT_X[1], FOOT_Y[0], FOOT_X[0], FOOT_Y[0], FOOT_X[0], FOOT_Y[1]])
NOMINAL_WIDTH = 0.16         # plannerParams.ini:27

ICUB_JOINT_REG_DEG = np.array([15, 0, 0,
                               -7, 22, 11, 30,
                               -7, 22, 11, 30,
                               5.082, 0.406, -0.131, -45.249, -26.454, -0.351,
                               5.082, 0.406, -0.131, -45.249, -26.454, -0.351], float)

# Posture the WALK scenario (synth_walk_batch, per-tick kinematics) starts from and regularises to.  The shipped
# jointRegularization (ICUB_JOINT_REG_DEG) belongs to the real iCub URDF, which is not in the repository: on the
# iCub-SHAPED tree of icub_like_model() it puts the soles 15 cm ahead of the centre of mass and tilts them by 65 degrees,
# a robot no LIPM can balance.  This is the tree's own crouch: thighs 50 deg forward, knees 100 deg, soles flat under the
# CoM.  The depth is what keeps every leg away from its straight (singular) configuration while the pelvis sways over the
# other foot: tools/walk_diag.py, 65536 robots x 1024 ticks - the straightest knee stays above 31 deg and no IK becomes
# infeasible (at 35 / 70 deg 5.8 % of the robots over-stretched a leg at some point and their IK had no solution).
WALK_POSTURE_DEG = np.array([5, 0, 0,
                             -7, 22, 11, 30,
                             -7, 22, 11, 30,
                             -50.0, 0.406, -0.131, 100.0, -50.0, -0.351,
                             -50.0, 0.406, -0.131, 100.0, -50.0, -0.351], float)
# Joint velocity limits of the walk scenario [rad/s] (the reference reads them from the robot at run time,
# RobotHelper.cpp:288-298; there is no value in the repository): legs 1.5, torso and arms 0.3.  The twelve leg joints are
# all but determined by the 15 task rows, so a leg joint on its limit soon leaves the QP without a solution, while the
# upper body is where the QP has freedom: with these limits a bound is active on ~12 % of the robot-ticks (the upper
# body's, mostly while the pelvis changes sides) and none of 65536 robots fails in 1024 ticks.
WALK_VMAX = np.array([0.3] * 11 + [1.5] * 12, float)
# Swing foot of the walk scenario: LIFTED - the vertical twist amplitude is positive (the zero-net-displacement profile of
# tick_device.h: up in the first half of the single support, down in the second; 0.04-0.08 m/s peak = 0.9-1.8 cm of lift),
# small horizontal / angular scatter.  (An isotropic random twist pushes the foot down and outwards as often as up: that
# stretches the leg.)
WALK_SWING_LIFT = (0.04, 0.08)
WALK_SWING_LIN_SIGMA = 0.01
WALK_SWING_ANG_SIGMA = 0.02

_M1 = np.uint64(0x9E3779B97F4A7C15)
_M2 = np.uint64(0xBF58476D1CE4E5B9)
_M3 = np.uint64(0x94D049BB133111EB)


def _mix(x: np.ndarray) -> np.ndarray:
    x = x.astype(np.uint64, copy=True)
    x ^= x >> np.uint64(30)
    x *= _M2
    x ^= x >> np.uint64(27)
    x *= _M3
    x ^= x >> np.uint64(31)
    return x


class CounterRNG:
    """Stateless counter-based generator: value(seed, instance, slot)."""

    def __init__(self, seed: int, first: int, count: int):
        self.seed = np.uint64(seed & 0xFFFFFFFFFFFFFFFF)
        self.inst = np.arange(first, first + count, dtype=np.uint64)
        self._slot = 0

    def _bits(self, k: int) -> np.ndarray:
        slots = np.arange(self._slot, self._slot + k, dtype=np.uint64)
        self._slot += k
        with np.errstate(over="ignore"):
            base = _mix(self.inst * _M1 + self.seed)[:, None]
            return _mix(base + (slots[None, :] + np.uint64(1)) * _M3)

    def uniform(self, k: int, lo: float = 0.0, hi: float = 1.0) -> np.ndarray:
        u = (self._bits(k) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
        return lo + (hi - lo) * u

    def normal(self, k: int, sigma: float = 1.0) -> np.ndarray:
        k2 = (k + 1) // 2
        u1 = 1.0 - self.uniform(k2)          # (0, 1]
        u2 = self.uniform(k2)
        r = np.sqrt(-2.0 * np.log(u1))
        z = np.concatenate([r * np.cos(2 * np.pi * u2), r * np.sin(2 * np.pi * u2)], axis=1)
        return sigma * z[:, :k]


# --------------------------------------------------------------------------------------
# support polygon -> hull rows  (our own convention, SURVEY Appendix D-4:
# CCW hull, unit outward normals, rows a.u <= b, padded to 8 with 0.u <= 1e30)
# --------------------------------------------------------------------------------------
def convex_hull_ccw(pts: np.ndarray) -> np.ndarray:
    """Andrew monotone chain; returns CCW vertices without collinear points."""
    P = sorted(map(tuple, np.asarray(pts, float)))
    if len(P) <= 2:
        return np.array(P)

    def cross(o, a, b):
        return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])

    lo, up = [], []
    for p in P:
        while len(lo) >= 2 and cross(lo[-2], lo[-1], p) <= 0:
            lo.pop()
        lo.append(p)
    for p in reversed(P):
        while len(up) >= 2 and cross(up[-2], up[-1], p) <= 0:
            up.pop()
        up.append(p)
    return np.array(lo[:-1] + up[:-1])


def hull_rows(pts: np.ndarray):
    """rows (A[8,2], b[8], nc) of the convex hull of 2-D points."""
    V = convex_hull_ccw(pts)
    nc = len(V)
    assert 3 <= nc <= HULL_ROWS, nc
    A = np.zeros((HULL_ROWS, 2))
    b = np.full(HULL_ROWS, HULL_PAD_B)
    for k in range(nc):
        v0, v1 = V[k], V[(k + 1) % nc]
        d = v1 - v0
        nrm = np.array([d[1], -d[0]]) / np.hypot(d[0], d[1])
        A[k] = nrm
        b[k] = nrm @ v0
    return A, b, nc


def foot_corners(pos_xy: np.ndarray, yaw: float) -> np.ndarray:
    c, s = np.cos(yaw), np.sin(yaw)
    R = np.array([[c, -s], [s, c]])
    loc = np.array([[FOOT_X[1], FOOT_Y[1]], [FOOT_X[1], FOOT_Y[0]],
                    [FOOT_X[0], FOOT_Y[0]], [FOOT_X[0], FOOT_Y[1]]])
    return loc @ R.T + pos_xy


def synth_mpc_batch(count: int, seed: int = 1234, horizon: int = 50, first: int = 0,
                    dT: float = 0.01, x0_sigma: float = 0.01, uprev_sigma: float = 0.005):
    """SURVEY.md §8d config 2.  Returns dict of C-contiguous arrays."""
    N = horizon
    rng = CounterRNG(seed, first, count)
    u_state = rng.uniform(1)[:, 0]
    yaw = rng.uniform(2, -0.3, 0.3)
    other_x = rng.uniform(1, -0.1, 0.1)[:, 0]
    other_y = rng.uniform(1, -0.02, 0.02)[:, 0]
    x0_n = rng.normal(2, x0_sigma)
    v = rng.uniform(2, -0.2, 0.2)
    up_n = rng.normal(2, uprev_sigma)
    ref_n = rng.normal(2 * (N + 1), 1e-4).reshape(count, N + 1, 2)

    hull_A = np.zeros((count, HULL_ROWS, 2))
    hull_b = np.zeros((count, HULL_ROWS))
    hull_nc = np.zeros(count, np.int32)
    centroid = np.zeros((count, 2))
    contact = np.zeros(count, np.int32)       # 0 = left only, 1 = right only, 2 = both
    for i in range(count):
        st = 0 if u_state[i] < 0.35 else (1 if u_state[i] < 0.70 else 2)
        contact[i] = st
        # stance foot at the origin; the other foot nominal-width away (left is +y)
        if st == 0:
            pts = foot_corners(np.zeros(2), yaw[i, 0])
        elif st == 1:
            pts = foot_corners(np.zeros(2), yaw[i, 1])
        else:
            left = foot_corners(np.zeros(2), yaw[i, 0])
            right = foot_corners(np.array([other_x[i], -NOMINAL_WIDTH + other_y[i]]), yaw[i, 1])
            pts = np.vstack([left, right])
        A, b, nc = hull_rows(pts)
        hull_A[i], hull_b[i], hull_nc[i] = A, b, nc
        centroid[i] = convex_hull_ccw(pts).mean(axis=0)
    x0 = centroid + x0_n
    stage = np.arange(N + 1, dtype=float)[None, :, None]
    ref = x0[:, None, :] + stage * v[:, None, :] * dT + ref_n
    u_prev = centroid + up_n
    return dict(x0=np.ascontiguousarray(x0), ref=np.ascontiguousarray(ref),
                u_prev=np.ascontiguousarray(u_prev), hull_A=hull_A, hull_b=hull_b,
                hull_nc=hull_nc, contact=contact, centroid=centroid)


# --------------------------------------------------------------------------------------
def _skew(p: np.ndarray) -> np.ndarray:
    z = np.zeros(p.shape[0])
    return np.stack([np.stack([z, -p[:, 2], p[:, 1]], -1),
                     np.stack([p[:, 2], z, -p[:, 0]], -1),
                     np.stack([-p[:, 1], p[:, 0], z], -1)], -2)


def _small_rot(w: np.ndarray) -> np.ndarray:
    """Rodrigues for a batch of rotation vectors (count, 3)."""
    th = np.linalg.norm(w, axis=1)
    th_safe = np.where(th > 0, th, 1.0)
    K = _skew(w / th_safe[:, None])
    I = np.eye(3)[None]
    s = np.sin(th)[:, None, None]
    c = (1 - np.cos(th))[:, None, None]
    return I + s * K + c * (K @ K)


def _rotz(a: np.ndarray) -> np.ndarray:
    c, s, z, o = np.cos(a), np.sin(a), np.zeros_like(a), np.ones_like(a)
    return np.stack([np.stack([c, -s, z], -1), np.stack([s, c, z], -1), np.stack([z, z, o], -1)], -2)


def synth_ik_batch(count: int, seed: int = 4321, dof: int = 23, first: int = 0,
                   joint_sigma: float = 0.3, com_sigma: float = 0.05, additional_rotation=None, posture_deg=None):
    """SURVEY.md §8d config 3 (dense random joint columns, exact mixed-representation
    base blocks).  Returns dict of C-contiguous arrays in ABI layout.
    additional_rotation / posture_deg: another robot's qpInverseKinematics.ini values (default: iCubGazeboV2_5's; the
    random draws do not depend on them)."""
    n = dof + 6
    rng = CounterRNG(seed, first, count)
    o = IK_STATE_OFFSETS

    def jac6():
        p = rng.normal(3, 0.3)
        J = np.zeros((count, 6, n))
        J[:, 0:3, 0:3] = np.eye(3)
        J[:, 0:3, 3:6] = -_skew(p)
        J[:, 3:6, 3:6] = np.eye(3)
        J[:, :, 6:] = rng.normal(6 * dof, joint_sigma).reshape(count, 6, dof)
        return J

    J_left, J_right, J_neck6 = jac6(), jac6(), jac6()
    pc = rng.normal(3, 0.3)
    J_com = np.zeros((count, 3, n))
    J_com[:, :, 0:3] = np.eye(3)
    J_com[:, :, 3:6] = -_skew(pc)
    J_com[:, :, 6:] = rng.normal(3 * dof, com_sigma).reshape(count, 3, dof)

    q_reg = np.deg2rad((ICUB_JOINT_REG_DEG if posture_deg is None else np.asarray(posture_deg, float)) if dof == 23 else np.zeros(dof))
    q = q_reg[None, :] + rng.normal(dof, 0.05)

    state = np.zeros((count, IK_STATE_LEN))
    yaw = rng.uniform(3, -0.3, 0.3)
    # desired feet: left at origin-ish, right nominal-width away; small yaw
    pd_left = np.concatenate([rng.uniform(2, -0.1, 0.1), np.zeros((count, 1))], 1)
    pd_right = pd_left + np.array([0.0, -NOMINAL_WIDTH, 0.0]) + \
        np.concatenate([rng.uniform(2, -0.05, 0.05), rng.uniform(1, 0.0, 0.03)], 1)
    Rd_left, Rd_right = _rotz(yaw[:, 0]), _rotz(yaw[:, 1])
    R_left = _small_rot(rng.normal(3, 0.01)) @ Rd_left
    R_right = _small_rot(rng.normal(3, 0.01)) @ Rd_right
    p_left = pd_left + rng.normal(3, 0.005)
    p_right = pd_right + rng.normal(3, 0.005)
    # setDesiredNeckOrientation right-multiplies additional_rotation (WM/src/WalkingQPInverseKinematics.cpp:143-146)
    add_rot = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]) if additional_rotation is None else np.asarray(additional_rotation, float)
    Rd_neck = _rotz(yaw[:, 2]) @ add_rot
    R_neck = _small_rot(rng.normal(3, 0.02)) @ Rd_neck
    com_des = 0.5 * (pd_left + pd_right) + np.array([0.0, 0.0, 0.53])
    com = com_des + rng.normal(3, 0.005)
    com_vel = rng.normal(3, 0.05)
    stance_left = rng.uniform(1)[:, 0] < 0.5
    tw = rng.normal(6, 0.2)
    twist_left = np.where(stance_left[:, None], 0.0, tw)
    twist_right = np.where(stance_left[:, None], tw, 0.0)

    def put(name, arr):
        a = arr.reshape(count, -1)
        state[:, o[name]:o[name] + a.shape[1]] = a

    put("p_left", p_left); put("R_left", R_left); put("p_right", p_right); put("R_right", R_right)
    put("pd_left", pd_left); put("Rd_left", Rd_left); put("pd_right", pd_right); put("Rd_right", Rd_right)
    put("R_neck", R_neck); put("Rd_neck", Rd_neck)
    put("com", com); put("com_des", com_des); put("com_vel_des", com_vel)
    put("twist_left", twist_left); put("twist_right", twist_right)

    return dict(J_left=np.ascontiguousarray(J_left), J_right=np.ascontiguousarray(J_right),
                J_neck=np.ascontiguousarray(J_neck6[:, 3:6, :]), J_com=np.ascontiguousarray(J_com),
                q=np.ascontiguousarray(q), state=state)


# --------------------------------------------------------------------------------------
def _dcm_reference(zl, zr, phase0, T, step_ticks, ds_ticks, dT, com_height, gravity):
    """ZMP reference that sits on the stance foot's ZMP point (zl / zr) in single support and moves linearly to the
    next stance foot in double support; DCM reference integrated BACKWARDS through xi_t = (xi_{t+1} - b zmp_t) / a
    (the way the reference's planner builds it, WM/src/TrajectoryGenerator.cpp:152-154).  Returns (xi[:, :T], zmp[:, :T])."""
    count = zl.shape[0]
    Tz = T + 4 * step_ticks                                   # tail so that the backward pass has settled
    tau = np.arange(Tz)[None, :]
    cyc = (tau + phase0[:, None]) % (2 * step_ticks)
    sidx = cyc % step_ticks
    side = cyc // step_ticks                                  # 0: left is the stance foot of this step
    cur = np.where(side[..., None] == 0, zl[:, None, :], zr[:, None, :])
    prev = np.where(side[..., None] == 0, zr[:, None, :], zl[:, None, :])
    lam = np.clip(sidx / float(ds_ticks), 0.0, 1.0)[..., None]
    zmp = prev + lam * (cur - prev)
    a = np.exp(np.sqrt(gravity / com_height) * dT); b = 1.0 - a
    xi = np.zeros((count, Tz, 2))
    xi[:, -1] = zmp[:, -1]
    for t in range(Tz - 2, -1, -1):
        xi[:, t] = (xi[:, t + 1] - b * zmp[:, t]) / a
    return np.ascontiguousarray(xi[:, :T]), np.ascontiguousarray(zmp[:, :T])


def synth_tick_batch(count: int, n_ticks: int, seed: int = 2718, horizon: int = 50, first: int = 0,
                     step_ticks: int = 180, ds_ticks: int = 110, dT: float = 0.01, com_height: float = 0.53,
                     gravity: float = 9.81, additional_rotation=None):
    """Inputs of the device-resident tick pipeline (BASELINE configs 4/5): per instance a long
    DCM reference trajectory (the deque the reference consumes one stage per tick), the
    support-polygon rows of the three contact pairs (left, right, both), a random phase
    offset of the step cycle, constant Jacobians/poses for the IK, initial states.

    The DCM reference is dynamically consistent, the way the reference's planner builds it
    (WM/src/TrajectoryGenerator.cpp:152-154): a ZMP reference that sits on the stance foot
    (+ leftZMPDelta / rightZMPDelta, plannerParams.ini:39-40) in single support and moves
    linearly to the next stance foot in double support, integrated BACKWARDS through
    xi_t = (xi_{t+1} - b zmp_t) / a."""
    rng = CounterRNG(seed ^ 0x5EED, first, count)
    T = n_ticks + horizon + 1
    yaw = rng.uniform(2, -0.2, 0.2)
    dxy = np.concatenate([rng.uniform(1, -0.05, 0.05), rng.uniform(1, -0.01, 0.01)], 1)
    phase0 = (rng.uniform(1)[:, 0] * (2 * step_ticks)).astype(np.int32)
    dcm_n = rng.normal(2, 0.002)
    swing = rng.normal(6, 0.2)
    left_xy = np.zeros((count, 2)); left_xy[:, 1] = 0.5 * NOMINAL_WIDTH
    right_xy = dxy.copy(); right_xy[:, 1] -= 0.5 * NOMINAL_WIDTH
    hull_tab_A = np.zeros((count, 3, HULL_ROWS, 2)); hull_tab_b = np.zeros((count, 3, HULL_ROWS))
    hull_tab_nc = np.zeros((count, 3), np.int32)
    for i in range(count):
        L = foot_corners(left_xy[i], yaw[i, 0]); R = foot_corners(right_xy[i], yaw[i, 1])
        for k, pts in enumerate((L, R, np.vstack([L, R]))):
            A, b, nc = hull_rows(pts)
            hull_tab_A[i, k], hull_tab_b[i, k], hull_tab_nc[i, k] = A, b, nc

    def rot2(a, v):
        return np.stack([np.cos(a) * v[0] - np.sin(a) * v[1], np.sin(a) * v[0] + np.cos(a) * v[1]], -1)
    zl = left_xy + rot2(yaw[:, 0], (0.03, -0.005))            # leftZMPDelta
    zr = right_xy + rot2(yaw[:, 1], (0.03, 0.005))            # rightZMPDelta
    ref, zmp = _dcm_reference(zl, zr, phase0, T, step_ticks, ds_ticks, dT, com_height, gravity)
    ik = synth_ik_batch(count, seed=seed + 1, first=first, additional_rotation=additional_rotation)
    dcm0 = ref[:, 0, :] + dcm_n
    return dict(first=first, ref_traj=ref, zmp_ref=zmp, hull_tab_A=hull_tab_A,
                hull_tab_b=hull_tab_b, hull_tab_nc=hull_tab_nc, phase0=phase0, J_left=ik["J_left"],
                J_right=ik["J_right"], J_neck=ik["J_neck"], J_com=ik["J_com"], state0=ik["state"],
                swing_twist=np.ascontiguousarray(swing), q0=ik["q"], dcm0=np.ascontiguousarray(dcm0),
                com0=np.ascontiguousarray(dcm0.copy()), u_init=np.ascontiguousarray(zmp[:, 0].copy()))


# ------------------------------------------------------------------------------------------------
# kinematics.  The reference reads its robot model from an external URDF
# (`model.urdf`, WM/src/WalkingModule.cpp:107) that is not part of the repository, so the tree below
# is iCub-SHAPED, not iCub: same joint list and order (CFG/robotControl.ini:3-7), same chain
# topology (torso 3 -> arms 4 + 4; legs 6 + 6 from the root link), plausible link lengths, masses
# and axes.  A table derived from the real URDF has the same form and goes through the same ABI.
JOINT_NAMES = ("torso_pitch", "torso_roll", "torso_yaw",
               "l_shoulder_pitch", "l_shoulder_roll", "l_shoulder_yaw", "l_elbow",
               "r_shoulder_pitch", "r_shoulder_roll", "r_shoulder_yaw", "r_elbow",
               "l_hip_pitch", "l_hip_roll", "l_hip_yaw", "l_knee", "l_ankle_pitch", "l_ankle_roll",
               "r_hip_pitch", "r_hip_roll", "r_hip_yaw", "r_knee", "r_ankle_pitch", "r_ankle_roll")


def _rot_axis(axis, angle):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def icub_like_model() -> dict:
    """Kinematic tree in the table form of `wcqp_kin_params`: joint j has parent joint `parent[j]` (-1 = root
    link, always < j), a fixed transform (R0, p0) from the parent joint frame to its own frame at q = 0, a unit
    axis in its own frame, and carries one link (mass, centre of mass in the joint frame).  Three frames are
    attached: left sole, right sole, neck."""
    X, Y, Z = (1.0, 0, 0), (0, 1.0, 0), (0, 0, 1.0)
    parent = [-1, 0, 1, 2, 3, 4, 5, 2, 7, 8, 9, -1, 11, 12, 13, 14, 15, -1, 17, 18, 19, 20, 21]
    axis = [Y, X, Z, Y, X, Z, Y, Y, X, Z, Y, Y, X, Z, Y, Y, X, Y, X, Z, Y, Y, X]
    p0 = [(0, 0, 0.12), (0, 0, 0.03), (0, 0, 0.03),
          (0.0, 0.11, 0.14), (0, 0.02, 0), (0, 0, -0.07), (0.015, 0, -0.08),
          (0.0, -0.11, 0.14), (0, -0.02, 0), (0, 0, -0.07), (0.015, 0, -0.08),
          (0, 0.068, -0.04), (0, 0, -0.01), (0, 0, -0.03), (0, 0, -0.22), (0, 0, -0.21), (0, 0, -0.02),
          (0, -0.068, -0.04), (0, 0, -0.01), (0, 0, -0.03), (0, 0, -0.22), (0, 0, -0.21), (0, 0, -0.02)]
    R0 = [np.eye(3) for _ in range(23)]
    R0[3] = _rot_axis(X, np.deg2rad(15.0)); R0[7] = _rot_axis(X, np.deg2rad(-15.0))      # shoulders tilted outwards
    R0[13] = _rot_axis(Z, np.deg2rad(2.0)); R0[19] = _rot_axis(Z, np.deg2rad(-2.0))
    mass = [1.2, 0.9, 4.5, 1.1, 0.4, 0.9, 0.8, 1.1, 0.4, 0.9, 0.8,
            1.4, 0.6, 1.9, 1.3, 0.5, 0.7, 1.4, 0.6, 1.9, 1.3, 0.5, 0.7]
    com = [(0, 0, 0.01), (0, 0, 0.01), (0.005, 0, 0.10), (0, 0, -0.02), (0, 0, 0), (0, 0, -0.04), (0.01, 0, -0.06),
           (0, 0, -0.02), (0, 0, 0), (0, 0, -0.04), (0.01, 0, -0.06),
           (0, 0, -0.01), (0, 0, 0), (0, 0, -0.10), (0, 0, -0.10), (0, 0, -0.01), (0.02, 0, -0.03),
           (0, 0, -0.01), (0, 0, 0), (0, 0, -0.10), (0, 0, -0.10), (0, 0, -0.01), (0.02, 0, -0.03)]
    return dict(dof=23, parent=np.array(parent, np.int32), axis=np.array(axis, float), p0=np.array(p0, float),
                R0=np.stack(R0), mass=np.array(mass, float), com=np.array(com, float),
                root_mass=5.8, root_com=np.array([-0.01, 0.0, 0.02]),
                frame_joint=np.array([16, 22, 2], np.int32),          # left sole, right sole, neck
                frame_p=np.array([(0.02, 0, -0.045), (0.02, 0, -0.045), (0, 0, 0.20)], float),
                frame_R=np.stack([np.eye(3), np.eye(3), _rot_axis(Y, np.deg2rad(5.0))]))


def synth_kin_batch(count: int, seed: int = 31415, first: int = 0, joint_sigma: float = 0.25, posture_deg=None,
                    base_rot_sigma: float = 0.15) -> dict:
    """Base poses ([B][12]: position, row-major rotation) and joint angles [B][23] around the posture the
    reference regularises to (ICUB_JOINT_REG_DEG), shard-invariant like the other generators.  (A walk starts close
    to that posture - joint_sigma ~0.04 - or the regularisation term alone asks for rad/s of joint velocity.)"""
    rng = CounterRNG(seed, first, count)
    q = np.deg2rad(ICUB_JOINT_REG_DEG if posture_deg is None else posture_deg)[None, :] + rng.normal(23, joint_sigma)
    pos = rng.normal(3, 1.0) * np.array([0.05, 0.05, 0.02]) + np.array([0.0, 0.0, 0.55])
    w = rng.normal(3, base_rot_sigma)
    R = np.stack([_rot_axis(wi / (np.linalg.norm(wi) + 1e-300), np.linalg.norm(wi)) for wi in w])
    base = np.concatenate([pos, R.reshape(count, 9)], axis=1)
    return dict(q=np.ascontiguousarray(q), base=np.ascontiguousarray(base))


def synth_walk_kin_batch(count: int, first: int = 0) -> dict:
    """Base poses / joint angles the walk scenario starts from: robots standing upright on the tree's own crouch
    (WALK_POSTURE_DEG), a degree of scatter."""
    return synth_kin_batch(count, seed=27182, first=first, joint_sigma=0.015, posture_deg=WALK_POSTURE_DEG, base_rot_sigma=0.015)


def synth_walk_batch(count: int, n_ticks: int, poses: np.ndarray, kin_batch: dict, seed: int = 2718, horizon: int = 50,
                     first: int = 0, step_ticks: int = 180, ds_ticks: int = 110, dT: float = 0.01, com_height: float = 0.53,
                     gravity: float = 9.81):
    """Inputs of the tick pipeline WITH per-tick kinematics (`TickPipeline(kin=...)`): a coherent synthetic robot
    marching in place.  `kin_batch` = synth_walk_kin_batch(count, first=first) (base poses, joint angles), `poses` [count][87] =
    the pose block the kinematics produce for it at tick 0 (`KinModel.jacobians_host(base, q, state=zeros)["state"]` on
    the device, or the oracle's twin in the tests): the desired foot poses ARE the initial ones (the feet stay planted;
    the pipeline anchors the base at the stance foot, so it moves as the stance leg's joints do), the desired neck orientation is the initial one up to a small rotation, the ZMP
    reference alternates between the two feet's ZMP points (plannerParams.ini:39-40) and the DCM reference follows from it."""
    rng = CounterRNG(seed ^ 0xA11CE, first, count)
    T = n_ticks + horizon + 1
    o = IK_STATE_OFFSETS
    # the walk starts from standing in the middle of a double-support phase (either foot next), where the DCM reference
    # passes between the feet - close to where the robot's own CoM is; contact pairs then change every 70-110 ticks
    u_ph = rng.uniform(2)
    phase0 = ((u_ph[:, 0] < 0.5) * step_ticks + (0.35 + 0.2 * u_ph[:, 1]) * ds_ticks).astype(np.int32)
    dcm_n = rng.normal(2, 0.002)
    # amplitudes of the swing foot's twist profile (zero net displacement: tick_device.h): the foot is lifted
    swing = np.concatenate([rng.normal(2, WALK_SWING_LIN_SIGMA), rng.uniform(1, *WALK_SWING_LIFT), rng.normal(3, WALK_SWING_ANG_SIGMA)], axis=1)
    neck_w = rng.normal(3, 0.02)
    state0 = np.array(poses, dtype=np.float64, copy=True)
    for src, dst, k in (("p_left", "pd_left", 3), ("R_left", "Rd_left", 9), ("p_right", "pd_right", 3), ("R_right", "Rd_right", 9)):
        state0[:, o[dst]:o[dst] + k] = state0[:, o[src]:o[src] + k]
    Rn = state0[:, o["R_neck"]:o["R_neck"] + 9].reshape(count, 3, 3)
    state0[:, o["Rd_neck"]:o["Rd_neck"] + 9] = (_small_rot(neck_w) @ Rn).reshape(count, 9)

    def zmp_point(p_name, R_name, delta):
        p = state0[:, o[p_name]:o[p_name] + 2]
        R = state0[:, o[R_name]:o[R_name] + 9].reshape(count, 3, 3)
        return p + np.stack([R[:, 0, 0] * delta[0] + R[:, 0, 1] * delta[1], R[:, 1, 0] * delta[0] + R[:, 1, 1] * delta[1]], -1)
    zl = zmp_point("p_left", "R_left", (0.03, -0.005))        # leftZMPDelta
    zr = zmp_point("p_right", "R_right", (0.03, 0.005))       # rightZMPDelta
    ref, zmp = _dcm_reference(zl, zr, phase0, T, step_ticks, ds_ticks, dT, com_height, gravity)
    dcm0 = ref[:, 0, :] + dcm_n
    return dict(first=first, ref_traj=ref, zmp_ref=zmp, phase0=phase0, state0=np.ascontiguousarray(state0),
                swing_twist=np.ascontiguousarray(swing), q0=np.ascontiguousarray(kin_batch["q"]),
                dcm0=np.ascontiguousarray(dcm0),
                # the plant's CoM starts where the robot's own (kinematic) CoM is
                com0=np.ascontiguousarray(state0[:, o["com"]:o["com"] + 2].copy()), u_init=np.ascontiguousarray(zmp[:, 0].copy()))


def _min_jerk(s):
    """position, d/ds of the minimum-jerk profile 10 s^3 - 15 s^4 + 6 s^5 on [0, 1]"""
    return s ** 3 * (10.0 - 15.0 * s + 6.0 * s * s), 30.0 * s * s * (1.0 - s) ** 2


def synth_planned_walk_batch(count: int, n_ticks: int, poses: np.ndarray, kin_batch: dict, seed: int = 4242, horizon: int = 50,
                             first: int = 0, step_ticks: int = 180, ds_ticks: int = 110, n_steps: int = 4, step_length=(0.025, 0.035),
                             yaw_step=(0.0, 0.0), lift: float = 0.02, dT: float = 0.01, com_height: float = 0.53, gravity: float = 9.81) -> dict:
    """Inputs of the tick pipeline in planned-trajectory mode (`TickPipeline(planned_trajectories=True, kin=...)`): a seeded walk that goes
    somewhere.  `kin_batch` / `poses` as for synth_walk_batch (the desired feet start at the actual ones).  After a first double support of
    ds_ticks, n_steps steps of step_ticks each - single support (the swing foot lifted by `lift` and moved along a minimum-jerk profile),
    then double support - carry the swing foot `step_length` [m] (drawn per robot) ahead of the stance foot along the walking direction,
    which turns by `yaw_step` [rad] (drawn per robot) per step; the right foot swings first, and the robot stands for the rest.

      left_traj / right_traj [B][T][12]   sole pose (position, row-major rotation), T = n_ticks + horizon + 1
      left_twist / right_twist [B][T][6]  the analytic derivative of that pose (linear velocity, angular velocity about z)
      contact [B][T]                      bit 0 / 1: left / right in contact; bit 2: the left foot is the fixed frame (the stance foot of the
                                          last single support; the left one before the first)
      ref_traj / dcm_vel_traj [B][T][2]   the DCM reference by the backward recursion of _dcm_reference from the footsteps' ZMP plan (on the
                                          stance foot's ZMP point in single support, linear between the two in double support) and its
                                          velocity omega (xi - zmp)
    plus what synth_walk_batch returns (state0 with the desired neck orientation at the mean-yaw formula of the first stage, q0, dcm0,
    com0, u_init, zmp_ref) and `goal` [B][2][12], the final planned poses, and `distance` [B], how far the feet's midpoint travels."""
    rng = CounterRNG(seed ^ 0x57E95, first, count)
    T = n_ticks + horizon + 1
    o = IK_STATE_OFFSETS
    ss = step_ticks - ds_ticks
    L = step_length[0] + (step_length[1] - step_length[0]) * rng.uniform(1)[:, 0]
    dyaw = yaw_step[0] + (yaw_step[1] - yaw_step[0]) * rng.uniform(1)[:, 0]
    state0 = np.array(poses, dtype=np.float64, copy=True)
    for src, dst, k in (("p_left", "pd_left", 3), ("R_left", "Rd_left", 9), ("p_right", "pd_right", 3), ("R_right", "Rd_right", 9)):
        state0[:, o[dst]:o[dst] + k] = state0[:, o[src]:o[src] + k]
    feet = np.zeros((count, 2, T, 12)); tw = np.zeros((count, 2, T, 6))
    contact = np.zeros((count, T), np.uint8)
    zmp_pt = np.zeros((count, 2, T, 2))        # each foot's ZMP point per stage (leftZMPDelta / rightZMPDelta in the foot frame)
    delta = ((0.03, -0.005), (0.03, 0.005))
    Tz = T + 4 * step_ticks
    stance = np.zeros((count, Tz), np.int64)    # side of the ZMP plan: 0 left, 1 right, -1 double support towards `nxt`
    for i in range(count):
        p = [state0[i, o["pd_left"]:o["pd_left"] + 3].copy(), state0[i, o["pd_right"]:o["pd_right"] + 3].copy()]
        R = [state0[i, o["Rd_left"]:o["Rd_left"] + 9].reshape(3, 3).copy(), state0[i, o["Rd_right"]:o["Rd_right"] + 9].reshape(3, 3).copy()]
        heading = np.arctan2(R[0][1, 0] + R[1][1, 0], R[0][0, 0] + R[1][0, 0])
        half_w = 0.5 * np.linalg.norm((p[0] - p[1])[:2])
        mid = 0.5 * (p[0] + p[1])
        fixed = 0
        seq = []          # per stage: (pose of both feet, twists, flags)
        for t in range(T):
            k = (t - ds_ticks) // step_ticks if t >= ds_ticks else -1
            s_in = (t - ds_ticks) % step_ticks if t >= ds_ticks else 0
            pos = [p[0].copy(), p[1].copy()]; rot = [R[0].copy(), R[1].copy()]; twist = [np.zeros(6), np.zeros(6)]
            flags = 3
            if 0 <= k < n_steps and s_in < ss:
                sw = 1 - (k % 2)                  # the right foot (1) swings first
                st = 1 - sw
                # the step's target: the swing foot step_length ahead of the stance foot, the heading turned by dyaw
                h1 = heading + dyaw[i]
                fwd = np.array([np.cos(h1), np.sin(h1), 0.0]); lat = np.array([-np.sin(h1), np.cos(h1), 0.0])
                p_target = p[st] + L[i] * fwd + (2 * half_w) * lat * (1.0 if sw == 0 else -1.0)
                p_target[2] = p[sw][2]
                yaw0 = np.arctan2(R[sw][1, 0], R[sw][0, 0])
                yaw1 = yaw0 + dyaw[i]
                x = (s_in + 1) / float(ss)        # the foot lands on the last stage of the single support
                m, dm = _min_jerk(x)
                lz = 16.0 * x * x * (1.0 - x) ** 2; dlz = 32.0 * x * (1.0 - x) * (1.0 - 2.0 * x)
                pos[sw] = p[sw] + (p_target - p[sw]) * m + np.array([0.0, 0.0, lift * lz])
                rot[sw] = _rotz(np.array([(yaw1 - yaw0) * m]))[0] @ R[sw]
                v = ((p_target - p[sw]) * dm + np.array([0.0, 0.0, lift * dlz])) / (ss * dT)
                twist[sw] = np.concatenate([v, [0.0, 0.0, (yaw1 - yaw0) * dm / (ss * dT)]])
                flags = 1 if sw == 1 else 2
                fixed = st
                if s_in == ss - 1:                # touch-down: the new footprint
                    p[sw] = pos[sw].copy(); p[sw][2] = p_target[2]; R[sw] = rot[sw].copy()
                    heading = h1
                    mid = 0.5 * (p[0] + p[1])
            flags |= 4 if fixed == 0 else 0
            for f in range(2):
                feet[i, f, t, :3] = pos[f]; feet[i, f, t, 3:] = rot[f].reshape(9); tw[i, f, t] = twist[f]
                zmp_pt[i, f, t] = pos[f][:2] + rot[f][:2, :2] @ np.asarray(delta[f])
            contact[i, t] = flags
    # ZMP plan: single support on the stance foot's point, double support linear from the last stance foot to the next one
    zmp = np.zeros((count, Tz, 2))
    for i in range(count):
        fl = np.concatenate([contact[i], np.full(Tz - T, contact[i, -1])])
        zp = np.concatenate([zmp_pt[i], np.repeat(zmp_pt[i][:, -1:], Tz - T, axis=1)], axis=1)
        t = 0
        while t < Tz:
            if fl[t] & 3 != 3:
                side = 0 if fl[t] & 1 else 1
                zmp[i, t] = zp[side, t]; t += 1
                continue
            t1 = t
            while t1 < Tz and fl[t1] & 3 == 3:
                t1 += 1
            prev_side = (0 if fl[t - 1] & 1 else 1) if t > 0 else None
            next_side = (0 if fl[t1] & 1 else 1) if t1 < Tz else None
            for u in range(t, t1):
                a = zp[prev_side, u] if prev_side is not None else 0.5 * (zp[0, u] + zp[1, u])
                b = zp[next_side, u] if next_side is not None else 0.5 * (zp[0, u] + zp[1, u])
                lam = (u - t + 1) / float(t1 - t + 1)
                zmp[i, u] = a + lam * (b - a)
            t = t1
    omega = np.sqrt(gravity / com_height)
    a = np.exp(omega * dT); b = 1.0 - a
    xi = np.zeros((count, Tz, 2))
    xi[:, -1] = zmp[:, -1]
    for t in range(Tz - 2, -1, -1):
        xi[:, t] = (xi[:, t + 1] - b * zmp[:, t]) / a
    ref = np.ascontiguousarray(xi[:, :T]); zmp = np.ascontiguousarray(zmp[:, :T])
    vel = np.ascontiguousarray(omega * (ref - zmp))
    # the desired neck orientation of the first stage (planned mode recomputes it every tick; state0's copy is what the synthetic gait uses)
    left = np.ascontiguousarray(feet[:, 0]); right = np.ascontiguousarray(feet[:, 1])
    start_mid = 0.5 * (left[:, 0, :2] + right[:, 0, :2]); end_mid = 0.5 * (left[:, -1, :2] + right[:, -1, :2])
    dcm0 = ref[:, 0, :] + rng.normal(2, 0.002)
    return dict(first=first, ref_traj=ref, dcm_vel_traj=vel, zmp_ref=zmp, state0=np.ascontiguousarray(state0),
                q0=np.ascontiguousarray(kin_batch["q"]), dcm0=np.ascontiguousarray(dcm0),
                com0=np.ascontiguousarray(state0[:, o["com"]:o["com"] + 2].copy()), u_init=np.ascontiguousarray(zmp[:, 0].copy()),
                left_traj=left, right_traj=right, left_twist=np.ascontiguousarray(tw[:, 0]), right_twist=np.ascontiguousarray(tw[:, 1]),
                contact=np.ascontiguousarray(contact), goal=np.stack([left[:, -1], right[:, -1]], 1),
                distance=np.linalg.norm(end_mid - start_mid, axis=1))


ZMP_DELTA = ((0.03, -0.005), (0.03, 0.005))       # leftZMPDelta / rightZMPDelta (plannerParams.ini:39-40)


def shipped_swing_profile() -> dict:
    """The swing profile plannerParams.ini ships (footApexTime :31, stepLandingVelocity :30, pitchDelta :46 - degrees there, radians
    here -, comHeightDelta :32), as the keyword arguments of TickPipeline.set_swing_profile."""
    return dict(apex_ratio=0.8, landing_velocity=0.0, pitch_delta=0.0, com_height_delta=0.01)


def synth_footstep_walk_batch(count: int, n_ticks: int, poses: np.ndarray, kin_batch: dict, seed: int = 4242, horizon: int = 50,
                              first: int = 0, step_ticks: int = 180, ds_ticks: int = 110, n_steps: int = 4, step_length=(0.025, 0.035),
                              yaw_step=(0.0, 0.0), lift: float = 0.02, dT: float = 0.01, com_height: float = 0.53, gravity: float = 9.81) -> dict:
    """The walk of synth_planned_walk_batch (same arguments, seed and draws) as the footsteps that describe it - what
    `TickPipeline.upload_footsteps` takes (wcqp_tick_footsteps): n_steps [B], side [B][K], target [B][K][3] (x, y of the new footprint, yaw
    increment of the foot), first_ds_ticks, ss_ticks, ds_ticks, final_ds_ticks, lift, zmp_delta_left / zmp_delta_right - plus state0, q0,
    com0.  final_ds_ticks is the rest of synth_planned_walk_batch's ZMP plan, which it runs 4 step_ticks past its T stages before it lets
    the robot stand: (T + 4 step_ticks) - (the stage at which the last single support ends)."""
    rng = CounterRNG(seed ^ 0x57E95, first, count)
    T = n_ticks + horizon + 1
    o = IK_STATE_OFFSETS
    ss = step_ticks - ds_ticks
    L = step_length[0] + (step_length[1] - step_length[0]) * rng.uniform(1)[:, 0]
    dyaw = yaw_step[0] + (yaw_step[1] - yaw_step[0]) * rng.uniform(1)[:, 0]
    state0 = np.array(poses, dtype=np.float64, copy=True)
    for src, dst, k in (("p_left", "pd_left", 3), ("R_left", "Rd_left", 9), ("p_right", "pd_right", 3), ("R_right", "Rd_right", 9)):
        state0[:, o[dst]:o[dst] + k] = state0[:, o[src]:o[src] + k]
    side = np.zeros((count, n_steps), np.uint8)
    target = np.zeros((count, n_steps, 3))
    for i in range(count):
        p = [state0[i, o["pd_left"]:o["pd_left"] + 3].copy(), state0[i, o["pd_right"]:o["pd_right"] + 3].copy()]
        R = [state0[i, o["Rd_left"]:o["Rd_left"] + 9].reshape(3, 3).copy(), state0[i, o["Rd_right"]:o["Rd_right"] + 9].reshape(3, 3).copy()]
        heading = np.arctan2(R[0][1, 0] + R[1][1, 0], R[0][0, 0] + R[1][0, 0])
        half_w = 0.5 * np.linalg.norm((p[0] - p[1])[:2])
        for k in range(n_steps):
            sw = 1 - (k % 2)                      # the right foot (1) swings first
            st = 1 - sw
            h1 = heading + dyaw[i]
            fwd = np.array([np.cos(h1), np.sin(h1), 0.0]); lat = np.array([-np.sin(h1), np.cos(h1), 0.0])
            p_target = p[st] + L[i] * fwd + (2 * half_w) * lat * (1.0 if sw == 0 else -1.0)
            yaw0 = np.arctan2(R[sw][1, 0], R[sw][0, 0])
            inc = (yaw0 + dyaw[i]) - yaw0
            side[i, k] = sw
            target[i, k] = (p_target[0], p_target[1], inc)
            p[sw] = np.array([p_target[0], p_target[1], p[sw][2]])
            R[sw] = _rotz(np.array([inc]))[0] @ R[sw]
            heading = h1
    last_ss_end = ds_ticks + (n_steps - 1) * step_ticks + ss
    return dict(first=first, n_steps=np.full(count, n_steps, np.int32), side=side, target=target, first_ds_ticks=ds_ticks, ss_ticks=ss,
                ds_ticks=ds_ticks, final_ds_ticks=(T + 4 * step_ticks) - last_ss_end, lift=lift, zmp_delta_left=ZMP_DELTA[0],
                zmp_delta_right=ZMP_DELTA[1], state0=np.ascontiguousarray(state0), q0=np.ascontiguousarray(kin_batch["q"]),
                com0=np.ascontiguousarray(state0[:, o["com"]:o["com"] + 2].copy()))


def synth_timed_footstep_walk_batch(count: int, n_ticks: int, poses: np.ndarray, kin_batch: dict, spread: float = 0.2, **kw) -> dict:
    """synth_footstep_walk_batch's walk (same arguments, seed and draws: the same footsteps) with durations that differ per robot and per
    step - what `TickPipeline.upload_footsteps` routes to wcqp_tick_upload_footsteps_timed: ss_ticks / ds_ticks are [B][K] int32 arrays,
    each step's single and double support stretched or shortened by up to `spread` of the common value (never below one stage), drawn
    per (robot, step) from the robot's own counter stream; final_ds_ticks stays the common walk's."""
    fs = synth_footstep_walk_batch(count, n_ticks, poses, kin_batch, **kw)
    K = fs["side"].shape[1]
    rng = CounterRNG(kw.get("seed", 4242) ^ 0x71AED, kw.get("first", 0), count)
    u = rng.uniform(2 * K) if K else np.zeros((count, 0))
    scale = 1.0 + spread * (2.0 * u - 1.0)
    ss = np.maximum(np.rint(fs["ss_ticks"] * scale[:, :K]), 1).astype(np.int32)
    ds = np.maximum(np.rint(fs["ds_ticks"] * scale[:, K:]), 1).astype(np.int32)
    return dict(fs, ss_ticks=np.ascontiguousarray(ss), ds_ticks=np.ascontiguousarray(ds))


def synth_footstep_replan_batch(fs: dict, after_step: int = 2, ds_offset: int = 0, n_steps: int = 3, seed: int = 777,
                                step_length=(0.02, 0.03), yaw_step=(-0.04, 0.04)) -> dict:
    """A new goal for the walk of synth_footstep_walk_batch (`fs`), merged in the double support behind its step `after_step` (1-based),
    `ds_offset` stages into it - what `TickPipeline.replan_footsteps(merge_stage, footsteps, first_ds_ticks)` takes: merge_stage [B],
    n_steps [B], side [B][n_steps], target [B][n_steps][3] and first_ds_ticks, the rest of that double support.  The feet go on alternating
    from the footprints `after_step` landed steps leave, with a step length and a heading change per step drawn anew per robot."""
    count, K = fs["side"].shape
    ss, ds = int(fs["ss_ticks"]), int(fs["ds_ticks"])
    assert 1 <= after_step <= K and 0 <= ds_offset < ds and np.all(np.asarray(fs["n_steps"]) > after_step - 1)
    rng = CounterRNG(seed ^ 0x9E91A, int(fs.get("first", 0)), count)
    L = step_length[0] + (step_length[1] - step_length[0]) * rng.uniform(1)[:, 0]
    dyaw = yaw_step[0] + (yaw_step[1] - yaw_step[0]) * rng.uniform(1)[:, 0]
    o = IK_STATE_OFFSETS
    merge = np.full(count, int(fs["first_ds_ticks"]) + (after_step - 1) * (ss + ds) + ss + ds_offset, np.int32)
    side = np.zeros((count, n_steps), np.uint8)
    target = np.zeros((count, n_steps, 3))
    for i in range(count):
        st = fs["state0"][i]
        p = [st[o["pd_left"]:o["pd_left"] + 2].copy(), st[o["pd_right"]:o["pd_right"] + 2].copy()]
        yaw = [np.arctan2(st[o["Rd_left"] + 3], st[o["Rd_left"]]), np.arctan2(st[o["Rd_right"] + 3], st[o["Rd_right"]])]
        for k in range(after_step):              # the footprints at the merge stage
            sw = int(fs["side"][i, k])
            p[sw] = np.array(fs["target"][i, k, :2]); yaw[sw] += fs["target"][i, k, 2]
        sw = 1 - int(fs["side"][i, after_step - 1])
        half_w = 0.5 * np.linalg.norm(p[0] - p[1])
        heading = 0.5 * (yaw[0] + yaw[1])
        for k in range(n_steps):
            heading += dyaw[i]
            fwd = np.array([np.cos(heading), np.sin(heading)]); lat = np.array([-np.sin(heading), np.cos(heading)])
            pt = p[1 - sw] + L[i] * fwd + (2 * half_w) * lat * (1.0 if sw == 0 else -1.0)
            side[i, k] = sw
            target[i, k] = (pt[0], pt[1], heading - yaw[sw])
            p[sw] = pt; yaw[sw] = heading
            sw = 1 - sw
    return dict(merge_stage=merge, n_steps=np.full(count, n_steps, np.int32), side=side, target=target, first_ds_ticks=ds - ds_offset)


# the cases of synth_goal_batch's first robots: name, goal (x, y) in the unicycle's frame, the foot that swings first
GOAL_CASES = (("origin", (0.0, 0.0), 1), ("straight", (0.2, 0.0), 1), ("straight_left_first", (0.1, 0.0), 0), ("turn_left", (0.15, 0.1), 1),
              ("turn_right", (0.15, -0.1), 0), ("far", (2.5, 0.0), 1), ("far_turn", (2.0, 1.5), 0), ("behind", (-0.2, 0.0), 1),
              ("behind_side", (-0.15, 0.1), 0), ("sideways", (0.0, 0.2), 1), ("below_a_step", (0.008, 0.0), 0), ("straight_long", (0.3, 0.0), 1),
              ("turn_sharp", (0.1, 0.2), 0))


def synth_goal_batch(count: int, seed: int = 6021, first: int = 0, state0=None, cases: bool = True, radius: float = 1.0,
                     nominal_width: float = NOMINAL_WIDTH) -> dict:
    """Goals for `UnicyclePlanner.plan_host` / `TickPipeline.upload_goal`: left0, right0 [B][12] (the desired soles of `state0` when it is
    given; otherwise robots standing anywhere, heading anywhere, the feet nominal_width apart on the ground), goals [B][2], first_side [B]
    and case [B] (names).  With `cases` robot i < 13 of the whole batch takes GOAL_CASES[i] - straight ahead, turns, the origin (no step), far goals
    (they truncate at max_steps), goals behind and beside the robot; every other robot a goal drawn uniformly from the disc of `radius`
    and either first side."""
    rng = CounterRNG(seed ^ 0x60A15, first, count)
    o = IK_STATE_OFFSETS
    if state0 is not None:
        state0 = np.asarray(state0, float)
        left0 = np.ascontiguousarray(state0[:count, o["pd_left"]:o["pd_left"] + 12])
        right0 = np.ascontiguousarray(state0[:count, o["pd_right"]:o["pd_right"] + 12])
        rng.uniform(3)
    else:
        u = rng.uniform(3)
        mid = 4.0 * u[:, :2] - 2.0
        yaw = np.pi * (2.0 * u[:, 2] - 1.0)
        lat = np.stack([-np.sin(yaw), np.cos(yaw)], axis=1)
        R = _rotz(yaw).reshape(count, 9)
        left0 = np.concatenate([mid + 0.5 * nominal_width * lat, np.zeros((count, 1)), R], axis=1)
        right0 = np.concatenate([mid - 0.5 * nominal_width * lat, np.zeros((count, 1)), R], axis=1)
    u = rng.uniform(3)
    r, phi = radius * np.sqrt(u[:, 0]), 2.0 * np.pi * u[:, 1]
    goals = np.stack([r * np.cos(phi), r * np.sin(phi)], axis=1)
    first_side = (u[:, 2] < 0.5).astype(np.uint8)
    case = ["random"] * count
    if cases:
        for i in range(count):
            if first + i < len(GOAL_CASES):
                case[i], goals[i], first_side[i] = GOAL_CASES[first + i]
    return dict(first=first, left0=np.ascontiguousarray(left0), right0=np.ascontiguousarray(right0), goals=np.ascontiguousarray(goals),
                first_side=first_side, case=case)


def neck_target(left_d: np.ndarray, right_d: np.ndarray, additional_rotation=None) -> np.ndarray:
    """Desired neck orientation [B][9] by the mean-yaw rule of WalkingModule::prepareRobot (WM/src/WalkingModule.cpp:957-970; the tick's
    per-tick rule :697-707): RotZ(atan2(sin yL + sin yR, cos yL + cos yR)) * additional_rotation, each sole's yaw atan2(R10, R00) of its
    desired pose [B][12] (p 3 | R 9 row-major)."""
    left_d, right_d = np.asarray(left_d, float), np.asarray(right_d, float)
    yl = np.arctan2(left_d[:, 6], left_d[:, 3]); yr = np.arctan2(right_d[:, 6], right_d[:, 3])
    mean = np.arctan2(np.sin(yl) + np.sin(yr), np.cos(yl) + np.cos(yr))
    add = np.eye(3) if additional_rotation is None else np.asarray(additional_rotation, float).reshape(3, 3)
    return np.ascontiguousarray((_rotz(mean) @ add).reshape(-1, 9))


def synth_prepare_batch(count: int, first: int = 0, seed: int = 88001, com_height=(0.39, 0.45), additional_rotation=None) -> dict:
    """Targets of the batched non-linear IK (`PrepareSolver`, wcqp_prepare_*): "these robots stand with their soles here and their CoM
    there".  Left sole anywhere on the floor within a metre of the origin with a yaw of +-0.4 rad; right sole 0.12-0.18 m beside it,
    +-0.08 m fore-aft, +-0.2 rad of relative yaw; CoM between the two soles' ZMP points (ZMP_DELTA) at com_height above the floor - heights
    this tree reaches with bent knees (its legs are straight near 0.5 m, where the iteration converges slowly or not at all); neck at the
    mean yaw (neck_target).  q_guess: the joints of synth_walk_kin_batch.  Shard-invariant."""
    rng = CounterRNG(seed, first, count)
    u = rng.uniform(9)
    yl = -0.4 + 0.8 * u[:, 0]
    pl = np.stack([-1.0 + 2.0 * u[:, 1], -1.0 + 2.0 * u[:, 2], np.zeros(count)], -1)
    Rl = _rotz(yl)
    off = np.stack([-0.08 + 0.16 * u[:, 3], -(0.12 + 0.06 * u[:, 4]), np.zeros(count)], -1)
    pr = pl + np.einsum("bij,bj->bi", Rl, off)
    Rr = _rotz(yl + (-0.2 + 0.4 * u[:, 5]))
    left_d = np.concatenate([pl, Rl.reshape(count, 9)], axis=1)
    right_d = np.concatenate([pr, Rr.reshape(count, 9)], axis=1)
    zl = pl[:, :2] + np.einsum("bij,j->bi", Rl[:, :2, :2], np.array(ZMP_DELTA[0]))
    zr = pr[:, :2] + np.einsum("bij,j->bi", Rr[:, :2, :2], np.array(ZMP_DELTA[1]))
    w = (0.35 + 0.3 * u[:, 6])[:, None]
    com_d = np.concatenate([zl + w * (zr - zl), (com_height[0] + (com_height[1] - com_height[0]) * u[:, 7])[:, None]], axis=1)
    return dict(first=first, left_d=np.ascontiguousarray(left_d), right_d=np.ascontiguousarray(right_d), com_d=np.ascontiguousarray(com_d),
                Rd_neck=neck_target(left_d, right_d, additional_rotation), q_guess=synth_walk_kin_batch(count, first=first)["q"])
