"""The POSITION mode of the closed-loop tick (wcqp_tick_params.ik_mode) restated, and the scenario its tests walk.

The restatement has two parts.  The chain is oracle.tick_spec: run_ticks on the same plan gives u0_log, dcm, com and zmp_gains - it reads
nothing an IK writes - and its ten lines of LIPM reference and ZMP-CoM law are repeated here on its logs to get p_star per tick.  The IK is
helpers/prepare_spec.solve, hot-started tick to tick: the targets of tick t are the plan's soles of stage t, (p_star x, p_star y, the
plan's CoM height of stage t) and the neck rule of the planned tick; a tick that does not end SOLVED stops the robot.

The scenario: 13 robots (three full waves of four and one with three dead slots), 70 ticks of a generated walk with steps of 15 + 10 stages
behind a double support of 10 - a double support, both single supports and the switch between them - at a CoM height of 0.42 m, from the
joints prepare_spec.solve gives each robot for its own soles."""
import functools

import numpy as np

import robots
import trees
from helpers import footstep_plan as fp
from helpers import prepare_spec as ps
from helpers import streamed_tick as stt
from helpers import zmp_gains as zg
from oracle import kin_spec as ks
from oracle import tick_spec as ts

B13, T, H, N = 13, 70, 0.42, 50
STEP_TICKS, DS_TICKS, N_STEPS = 25, 10, 3
ROBOT = "iCubGazeboV2_5"
K_DCM = 1.0
ADD_ROT = np.eye(3)
SEL = (0, 5, 12)                     # the robots the restatement walks: one of the first wave, one of the second, the last one
CONTROLLERS = ("mpc", "reactive_gs")  # the MPC at N = 50; the reactive law with gain scheduling
CUT_JOINT = 17


def controller_kwargs(controller):
    """TickPipeline's keyword arguments of a controller configuration"""
    if controller == "mpc":
        return {}
    return dict(dcm_controller="reactive", k_dcm=K_DCM, zmp_gain_scheduling=True, **zg.ZMP_SCHEDULE[ROBOT])


def tree_of(tree):
    """(model, order) of a scenario's tree: "icub", the iCub-shaped one, or a variant of it in tests/trees.py whose joint k is joint order[k]"""
    from walking_controllers_amd import synth
    return (synth.icub_like_model(), list(range(23))) if tree == "icub" else (trees.named(tree), trees.ORDER[tree])


@functools.lru_cache(maxsize=None)
def scenario(tree="icub"):
    """model, q_reg, the footsteps (with state0, q0, com0: what upload_footsteps takes) and the plan of all 13 robots; on another tree
    than the iCub-shaped one everything per joint (guess, posture, v_max) is permuted with the joints"""
    from walking_controllers_amd import synth
    model, order = tree_of(tree)
    d = synth.synth_prepare_batch(B13, com_height=(H, H))
    d = dict(d, q_guess=trees.permute_joints(d["q_guess"], order))
    q_reg = trees.permute_joints(np.deg2rad(synth.WALK_POSTURE_DEG), order)
    par = ps.Params(q_reg=q_reg)
    q0 = np.zeros((B13, 23)); state0 = np.zeros((B13, 87))
    for i in range(B13):
        tg = dict(left_d=d["left_d"][i], right_d=d["right_d"][i], com_d=d["com_d"][i], Rd_neck=d["Rd_neck"][i])
        s = ps.solve(model, tg, d["q_guess"][i], par)
        assert s["status"] == ps.SOLVED, i
        q0[i] = s["q"]
        # the pose block a prepared robot starts from: the actual poses at q0, the desired ones = the targets
        K = ks.jacobians(model, s["base"], s["q"])
        st = state0[i]
        st[0:3] = K["p_left"]; st[3:12] = K["R_left"].reshape(9); st[12:15] = K["p_right"]; st[15:24] = K["R_right"].reshape(9)
        st[24:36] = d["left_d"][i]; st[36:48] = d["right_d"][i]
        st[48:57] = K["R_neck"].reshape(9); st[57:66] = d["Rd_neck"][i]; st[66:69] = K["com"]; st[69:72] = d["com_d"][i]
    fs = synth.synth_footstep_walk_batch(B13, T, state0, dict(q=q0), step_ticks=STEP_TICKS, ds_ticks=DS_TICKS, n_steps=N_STEPS, com_height=H)
    fs["state0"] = state0                # (the desired soles are the TARGETS, not copies of the actual ones)
    plan = fp.footstep_plan(fs, state0, T + N + 1, T, com_height=H)
    return dict(model=model, order=order, q_reg=q_reg, fs=fs, plan=plan, foot_rect=synth.FOOT_RECT, v_max=trees.permute_joints(synth.WALK_VMAX, order),
                posture_deg=trees.permute_joints(synth.WALK_POSTURE_DEG, order))


def chain(controller, robot, plan=None, height=None, tree="icub"):
    """The chain of one robot over T ticks on `plan` (default: the scenario's): run_ticks' u0_log, dcm, com, zmp_gains and p_star [T][2]."""
    from oracle import qp_spec as qs
    sc = scenario(tree)
    plan = sc["plan"] if plan is None else plan
    R = robots.ROBOTS[ROBOT]
    i = robot
    one = {k: (v[i:i + 1] if isinstance(v, np.ndarray) and v.shape[:1] == (B13,) else v) for k, v in sc["fs"].items()}
    p1 = {k: v[i:i + 1] for k, v in plan.items() if isinstance(v, np.ndarray) and v.shape[:1] == (B13,)}
    if height is not None:
        p1["com_height_traj"] = np.full_like(p1["com_height_traj"], height)
    e = dict(one, first=i, ref_traj=p1["ref_traj"], dcm_vel_traj=p1["dcm_vel_traj"], dcm0=p1["ref_traj"][:, 0].copy(), u_init=p1["zmp_ref"][:, 0].copy())
    ipar = robots.ik_params(qs, ROBOT, v_max=sc["v_max"])
    ipar.joint_reg_deg = sc["posture_deg"]
    ipar.joint_reg_weights = trees.permute_joints(ipar.joint_reg_weights, sc["order"])
    ipar.joint_reg_gains = trees.permute_joints(ipar.joint_reg_gains, sc["order"])
    tp = ts.TickParams(horizon=N, com_height=H, k_com=R["k_com"], k_zmp=R["k_zmp"])
    kw = {} if controller == "mpc" else dict(dcm_controller="reactive", k_dcm=K_DCM, zmp_gain_schedule=zg.ZMP_SCHEDULE[ROBOT])
    run = ts.run_ticks(tp, e, T, ipar, kin_model=sc["model"], foot_rect=sc["foot_rect"], stages=stt.stages_of(p1, T), neck_additional_rotation=ADD_ROT,
                       dcm_vel=p1["dcm_vel_traj"], **kw)
    # p_star: the LIPM reference and the ZMP-CoM law of run_ticks again, on what it logged (the plant's state at the START of each tick)
    omega = np.sqrt(tp.gravity / tp.com_height)
    ref = e["ref_traj"][0]
    c_ref = e["com0"][0].copy(); v_ref_prev = np.zeros(2)
    p_star = e["com0"][0].copy(); v_star_prev = np.zeros(2)
    out = np.zeros((T, 2))
    for t in range(T):
        v_ref = -omega * (c_ref - ref[t])
        c_ref = c_ref + 0.5 * tp.dT * (v_ref + v_ref_prev); v_ref_prev = v_ref
        g = run["zmp_gains"][t, 0]
        v_star = g[0] * (c_ref - run["com_log"][t, 0]) - g[1] * (run["u0_log"][t, 0] - run["zmp_log"][t, 0]) + v_ref
        p_star = p_star + 0.5 * tp.dT * (v_star + v_star_prev); v_star_prev = v_star
        out[t] = p_star
    return dict(u0_log=run["u0_log"][:, 0], dcm=run["dcm"][0], com=run["com"][0], zmp_gains=run["zmp_gains"][-1, 0], mpc_fail=int(run["mpc_fail"][0]),
                p_star=out, plan=p1)


def targets(p1, p_star, t, height=None):
    """the non-linear IK's targets of tick t for the one robot of plan slice p1"""
    left, right = p1["left_traj"][0, t], p1["right_traj"][0, t]
    h = p1["com_height_traj"][0, t] if height is None else height
    return dict(left_d=left, right_d=right, com_d=np.array([p_star[t, 0], p_star[t, 1], h]),
                Rd_neck=ts.neck_orientation(left[3:12], right[3:12], ADD_ROT).reshape(9))


def walk(ch, q0, par, n_ticks=T, tree="icub"):
    """The IK of the POSITION tick over the chain `ch` of one robot: prepare_spec.solve from the previous tick's joints (tick 0: q0), clipped
    into the limits; a tick that does not end SOLVED keeps the joints, stops the robot and counts, as every later tick does.
    -> q_log [T][23], iters [T], status [T], active (the joints on a limit in the last QP of each tick: {joint: side} or None), ik_fail."""
    lo, hi = ps._limits(par, 23)
    q = np.clip(np.asarray(q0, float), lo, hi)
    q_log = np.zeros((n_ticks, 23)); iters = np.zeros(n_ticks, np.int64); status = np.full(n_ticks, -1)
    active = [None] * n_ticks
    fail = 0
    for t in range(n_ticks):
        if fail == 0:
            s = ps.solve(sc_model(tree), targets(ch["plan"], ch["p_star"], t), q, par)
            iters[t] = s["iters"]; status[t] = s["status"]
            if s["status"] == ps.SOLVED:
                q = s["q"]; active[t] = s["active"]
            else:
                fail = 1
        else:
            fail += 1
        q_log[t] = q
    return dict(q_log=q_log, iters=iters, status=status, active=active, ik_fail=fail)


def sc_model(tree="icub"):
    return scenario(tree)["model"]


def params(tree="icub", **kw):
    """the IK's parameters of the scenario: the walk posture as regularisation, 30 iterations per tick, default tolerances"""
    return ps.Params(q_reg=scenario(tree)["q_reg"], max_iter=30, **kw)


@functools.lru_cache(maxsize=None)
def reference(controller, tree="icub", sel=SEL):
    """the restatement's walk of the robots `sel`, without limits: {robot: dict(chain=..., walk=...)}"""
    sc = scenario(tree)
    out = {}
    for i in sel:
        ch = chain(controller, i, tree=tree)
        out[i] = dict(chain=ch, walk=walk(ch, sc["fs"]["q0"][i], params(tree), tree=tree))
    return out


@functools.lru_cache(maxsize=None)
def cut_limits(robot):
    """The joint-17 cut of one robot: joint 17's upper limit a quarter of its range below its maximum over that robot's unlimited MPC walk
    (the other limits far away, at +-3 rad).  Per robot, because the robots stand with different knee angles: a cut taken from one robot's
    range is never reached by another, or leaves it no feasible posture.  -> (q_min, q_max)"""
    q17 = reference("mpc")[robot]["walk"]["q_log"][:, CUT_JOINT]
    lo, hi = np.full(23, -3.0), np.full(23, 3.0)
    hi[CUT_JOINT] = q17.max() - 0.25 * (q17.max() - q17.min())
    return lo, hi


@functools.lru_cache(maxsize=None)
def reference_cut():
    """the restatement's MPC walk of SEL, each robot under its own joint-17 cut: {robot: walk}"""
    sc = scenario()
    out = {}
    for i in SEL:
        lo, hi = cut_limits(i)
        out[i] = walk(reference("mpc")[i]["chain"], sc["fs"]["q0"][i], params(q_min=lo, q_max=hi))
    return out


def mask_of(active, side):
    return sum(1 << int(j) for j, s in (active or {}).items() if s * side > 0)
