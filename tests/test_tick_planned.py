"""Planned-trajectory mode of the closed-loop tick (wcqp_tick_params.planned_trajectories): the desired feet, twists, contact
flags, fixed frame and CoM height of every tick come from the planner's stage t.  CPU: the restatement's given-stages branch
(oracle/tick_spec.py::run_ticks(stages=...)) against its synthetic gait, the ABI, the binding's and the library's refusals, the generator.  GPU: the device against the restatement."""
import ctypes as C

import numpy as np
import pytest
from walking_controllers_amd.capi import E_INVALID as WCQP_E_INVALID, E_UNSUPPORTED as WCQP_E_UNSUPPORTED

import robots
from helpers import planned_tick as pt
from helpers import streamed_tick as stt
from helpers import zmp_gains as zg

K_DCM = {"iCubGazeboV2_5": 1.0, "iCubGenova04": 1.0, "icubGazeboSim": 1.5}
KEYS = ("u0_log", "dq_log", "q_des", "dcm", "com")
WALK_T = 880          # the generated walk: a double support of 110 ticks, four steps of 180, then standing
ADD_ROT = robots.ROBOTS["iCubGazeboV2_5"]["additional_rotation"]


def _walk_cpu(wca, B, T, horizon=50, planned=False, **kw):
    model = wca.synth.icub_like_model()
    kb = wca.synth.synth_walk_kin_batch(B)
    poses = pt.poses_host(model, kb)
    if planned:
        return model, wca.synth.synth_planned_walk_batch(B, T, poses, kb, horizon=horizon, **kw)
    return model, wca.synth.synth_walk_batch(B, T, poses, kb, horizon=horizon)


def _ik_params(wca, qs, robot):
    """The robot's qpInverseKinematics.ini (tests/robots.py) with the walk's velocity limits and regularisation posture."""
    ipar = robots.ik_params(qs, robot, v_max=wca.synth.WALK_VMAX.copy())
    ipar.joint_reg_deg = wca.synth.WALK_POSTURE_DEG.copy()
    return ipar


def _ik_solver(wca, robot):
    r = robots.ROBOTS[robot]
    return wca.IkSolver(form=wca.IK_FORM_QPOASES, neck_weight=r["neck_weight"] * np.eye(3), joint_reg_weights=np.array(r["reg_w"], float),
                        joint_reg_gains=np.array(r["reg_k"], float), joint_reg_rad=np.deg2rad(wca.synth.WALK_POSTURE_DEG),
                        v_max=wca.synth.WALK_VMAX.copy(), k_pos_com=r["k_pos_com"], k_pos_foot=r["k_pos_foot"], k_att_foot=r["k_att_foot"],
                        k_neck=r["k_neck"])


# ---------------------------------------------------------------------------------------------------------------- CPU

def test_restatement_reproduces_the_synthetic_gait(wca, qs):
    """The synthetic gait written out as stages: run_ticks(stages=...) reproduces its own synthetic branch to 1e-12."""
    from oracle import tick_spec as ts
    B, T = 2, 130
    p = ts.TickParams()
    model, d = _walk_cpu(wca, B, T)
    ipar = _ik_params(wca, qs, "iCubGazeboV2_5")
    plan, d2 = pt.synthetic_as_planned(p, d, T + p.horizon + 1, ADD_ROT)
    codes = np.array([ts.contact_code(t, d["phase0"], p) for t in range(T)])
    assert all(len(set(codes[:, i])) >= 2 for i in range(B)), "the run passes through a change of contact pair"
    ref = ts.run_ticks(p, d2, T, ipar, kin_model=model, foot_rect=wca.synth.FOOT_RECT)
    out = ts.run_ticks(p, d2, T, ipar, kin_model=model, foot_rect=wca.synth.FOOT_RECT, stages=stt.stages_of(plan, T), neck_additional_rotation=ADD_ROT)
    for k in KEYS:
        assert np.abs(out[k] - ref[k]).max() <= 1e-12, k
    assert np.array_equal(out["ik_fail"], ref["ik_fail"]) and np.array_equal(out["mpc_fail"], ref["mpc_fail"])
    assert np.abs(ref["dq_log"]).max() > 1e-3


def test_binding_refuses_incomplete_arguments(wca):
    mpc, ik = wca.MpcSolver.__new__(wca.MpcSolver), wca.IkSolver.__new__(wca.IkSolver)
    mpc.params = wca.capi.MpcParams(); ik.params = wca.capi.IkParams(); ik.dof = 23
    with pytest.raises(ValueError, match="neck_additional_rotation"):
        wca.TickPipeline(4, 10, mpc, ik, planned_trajectories=True)
    with pytest.raises(ValueError, match="kinematics"):
        wca.TickPipeline(4, 10, mpc, ik, planned_trajectories=True, neck_additional_rotation=np.eye(3))
    pipe = wca.TickPipeline.__new__(wca.TickPipeline)
    pipe.planned, pipe._h = True, None
    with pytest.raises(ValueError, match="left_traj"):
        pipe.upload({}, right_traj=0, left_twist=0, right_twist=0, contact=0)
    pipe.planned = False
    with pytest.raises(ValueError, match="planned"):
        pipe.upload({}, contact=np.zeros((4, 3)))


def _params(wca, **kw):
    prm = wca.capi.TickParams()
    prm.batch, prm.max_ticks, prm.step_ticks, prm.ds_ticks = 4, 10, 180, 110
    prm.mpc.horizon, prm.mpc.sampling_time, prm.mpc.com_height, prm.mpc.gravity = 50, 0.01, 0.53, 9.81
    prm.ik.dof, prm.use_kinematics, prm.kin_handoff, prm.planned_trajectories = 23, 1, 0, 1
    for k in range(9):
        prm.neck_additional_rotation[k] = float(k % 4 == 0)
    for k, v in kw.items():
        if "." in k:
            a, b = k.split(".")
            setattr(getattr(prm, a), b, v)
        else:
            setattr(prm, k, v)
    return prm


@pytest.mark.parametrize("bad", [dict(use_kinematics=0), dict(kin_handoff=1), dict(kin_handoff=2), dict(logger_ticks=5), dict(plant=1),
                                 {"ik.algorithm": 4}, {"ik.algorithm": 2}, {"mpc.horizon": 200}, {"mpc.horizon": 56}])
def test_create_refuses_before_the_device(wca, bad):
    """Every refused combination is WCQP_E_UNSUPPORTED before anything touches the device (so with or without a GPU)."""
    h = C.c_void_p()
    assert wca.capi.lib().wcqp_tick_create(C.byref(_params(wca, **bad)), C.byref(h)) == WCQP_E_UNSUPPORTED and not h


def test_create_refuses_bad_values(wca):
    h = C.c_void_p()
    assert wca.capi.lib().wcqp_tick_create(C.byref(_params(wca, planned_trajectories=2)), C.byref(h)) == WCQP_E_INVALID and not h
    prm = _params(wca)
    prm.neck_additional_rotation[4] = float("nan")
    assert wca.capi.lib().wcqp_tick_create(C.byref(prm), C.byref(h)) == WCQP_E_INVALID and not h


def test_generator_is_self_consistent(wca):
    """Twist = finite difference of the pose, flags coherent, the ZMP plan inside the support polygon at every stage, the feet advance."""
    B, T = 3, WALK_T
    _, d = _walk_cpu(wca, B, T, planned=True, yaw_step=(0.03, 0.08))
    dT = 0.01
    for f, (tr, tw) in enumerate(((d["left_traj"], d["left_twist"]), (d["right_traj"], d["right_twist"]))):
        # the pose of stage t + 1 minus that of stage t against the mean of the two stages' twists (trapezoid): O(dT^2)
        dp = (tr[:, 1:, :3] - tr[:, :-1, :3]) / dT
        assert np.abs(dp - 0.5 * (tw[:, 1:, :3] + tw[:, :-1, :3])).max() < 2e-3
        yaw = np.unwrap(np.arctan2(tr[..., 6], tr[..., 3]), axis=1)
        assert np.abs((yaw[:, 1:] - yaw[:, :-1]) / dT - 0.5 * (tw[:, 1:, 5] + tw[:, :-1, 5])).max() < 2e-2
        moving = np.abs(tw).max(-1) > 0
        assert not np.any(moving & (d["contact"] & (1 << f) > 0)), "a foot in contact does not move"
    c = d["contact"]
    assert np.all(c & 3) and np.all(np.where(c & 4, c & 1, c & 2))
    from oracle import hull_spec as hs
    for i in range(B):
        for t in range(T):
            A, b, nc = hs.hull_from_feet(wca.synth.FOOT_RECT, d["left_traj"][i, t], d["right_traj"][i, t], int(c[i, t]) & 3)
            assert np.all(A[:nc] @ d["zmp_ref"][i, t] <= b[:nc] + 1e-9), (i, t)
    assert np.all(d["distance"] > 0.08)
    omega = np.sqrt(9.81 / 0.53)
    assert np.allclose(d["dcm_vel_traj"], omega * (d["ref_traj"] - d["zmp_ref"]))
    pairs = {int(x) & 3 for x in c[0]}
    assert pairs == {1, 2, 3}


# ---------------------------------------------------------------------------------------------------------------- GPU

def _kin(wca):
    return wca.KinModel(wca.synth.icub_like_model())


def _pipe(wca, B, T, robot, controller, gs, horizon=50, planned=True, tpl=0, first=0, **kw):
    R = robots.ROBOTS[robot]
    ctl = dict(dcm_controller="reactive", k_dcm=K_DCM[robot]) if controller == "reactive" else {}
    sch = dict(zmp_gain_scheduling=True, **zg.ZMP_SCHEDULE[robot]) if gs else {}
    pl = dict(planned_trajectories=True, neck_additional_rotation=np.array(R["additional_rotation"])) if planned else {}
    ik = _ik_solver(wca, robot)
    return wca.TickPipeline(B, T, wca.MpcSolver(horizon=horizon), ik, first=first, log_ticks=T, k_com=R["k_com"], k_zmp=R["k_zmp"],
                            kin=_kin(wca), ticks_per_launch=tpl, **ctl, **sch, **pl, **kw)


def _upload(pipe, d, plan=None, vel=True):
    plan = plan if plan is not None else d
    keys = ("left_traj", "right_traj", "left_twist", "right_twist", "contact", "com_height_traj", "com_height_vel")
    pipe.upload(d, dcm_vel_traj=d.get("dcm_vel_traj") if vel else None, **{k: plan.get(k) for k in keys})


def _ref(qs, wca, robot, controller, gs, d, plan, T, horizon=50):
    from oracle import tick_spec as ts
    R = robots.ROBOTS[robot]
    p = ts.TickParams(horizon=horizon, k_com=R["k_com"], k_zmp=R["k_zmp"])
    out = ts.run_ticks(p, d, T, _ik_params(wca, qs, robot), kin_model=wca.synth.icub_like_model(), foot_rect=wca.synth.FOOT_RECT,
                       stages=stt.stages_of(plan, T), neck_additional_rotation=R["additional_rotation"], dcm_controller=controller,
                       k_dcm=K_DCM[robot], dcm_vel=d.get("dcm_vel_traj"), zmp_gain_schedule=zg.ZMP_SCHEDULE[robot] if gs else None)
    out["zmp_gains"] = out["zmp_gains"][-1]
    return out


def _close(out, ref, tol=1e-9):
    for k in KEYS + ("zmp_gains",):
        err = np.abs(out[k] - ref[k]).max()
        assert err <= tol, (k, err)
    assert np.array_equal(out["mpc_fail"], ref["mpc_fail"]) and np.array_equal(out["ik_fail"], ref["ik_fail"])


def _same(a, b):
    for k in KEYS + ("ik_fail", "mpc_fail", "hot_try", "hot_hit", "active_lower", "active_upper", "zmp_gains"):
        assert np.array_equal(a[k], b[k]), k


@pytest.fixture(scope="module")
def planned_walk(wca):
    model, d = _walk_cpu(wca, 3, WALK_T, planned=True, yaw_step=(0.03, 0.08))
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("controller", ["mpc", "reactive"])
def test_planned_synthetic_equals_the_synthetic_tick(wca, controller):
    """The planned mode fed the synthetic gait matches today's synthetic fused-kinematics tick on the same device to 1e-12."""
    from oracle import tick_spec as ts
    B, T = 8, 200
    robot = "iCubGazeboV2_5"
    _, d = _walk_cpu(wca, B, T)
    plan, d2 = pt.synthetic_as_planned(ts.TickParams(), d, T + 51, robots.ROBOTS[robot]["additional_rotation"])
    a = _pipe(wca, B, T, robot, controller, False, planned=False)
    _upload(a, d2, plan={}, vel=False)
    a.run(T)
    b = _pipe(wca, B, T, robot, controller, False)
    assert b.info()["planned_trajectories"] and not a.info()["planned_trajectories"]
    _upload(b, d2, plan=plan, vel=False)
    b.run(T)
    oa, ob = a.download(), b.download()
    for k in KEYS:
        assert np.abs(oa[k] - ob[k]).max() <= 1e-12, k
    assert np.array_equal(oa["ik_fail"], ob["ik_fail"]) and np.array_equal(oa["mpc_fail"], ob["mpc_fail"])


@pytest.mark.gpu
@pytest.mark.parametrize("gs", [False, True])
@pytest.mark.parametrize("controller,horizon", [("mpc", 50), ("reactive", 50), ("reactive", 200)])
@pytest.mark.parametrize("robot", robots.NAMES)
def test_parity_with_the_restatement(wca, qs, planned_walk, robot, controller, horizon, gs):
    """A forward-and-turning walk of 4 steps through every change of contact pair (left -> both -> right and back, the same pair again with
    the feet moved): the device against the restatement to 1e-9."""
    d = planned_walk
    B, T = d["q0"].shape[0], WALK_T
    if horizon != 50:
        _, d = _walk_cpu(wca, B, T, horizon=horizon, planned=True, yaw_step=(0.03, 0.08))
    pipe = _pipe(wca, B, T, robot, controller, gs, horizon=horizon)
    _upload(pipe, d)
    pipe.run(T)
    out = pipe.download()
    ref = _ref(qs, wca, robot, controller, gs, d, d, T, horizon)
    _close(out, ref)
    assert (ref["ik_fail"] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("controller", ["mpc", "reactive"])
def test_it_walks(wca, planned_walk, controller):
    """No IK failure; host kinematics at the final q_des put both soles on the planned final poses; the feet have advanced.  (The CPU
    restatement on the same seeded walk ends within 1e-6 m and 3e-5 rad of the final poses, its feet's midpoint within 0.001 % of the
    planned distance; the thresholds below keep a margin of 10 or more over that.)  sole_poses anchors the base at the planned pose of the
    fixed-frame foot, so the world pose of THAT foot holds by construction: what tests the walk is the other foot's world pose, the pose of
    the left sole relative to the right one (independent of the anchor) and the distance the feet's midpoint has travelled."""
    d = planned_walk
    B, T = d["q0"].shape[0], WALK_T
    pipe = _pipe(wca, B, T, "iCubGazeboV2_5", controller, False)
    _upload(pipe, d)
    pipe.run(T)
    out = pipe.download()
    assert (out["ik_fail"] == 0).all()
    P, Rw = pt.sole_poses(wca.synth.icub_like_model(), out["q_des"], d, T - 1)
    for f, tr in enumerate((d["left_traj"], d["right_traj"])):
        goal = tr[:, T - 1]
        assert np.abs(P[:, f] - goal[:, :3]).max() <= 1e-5
        dR = np.einsum("bji,bjk->bik", goal[:, 3:].reshape(B, 3, 3), Rw[:, f])
        ang = np.arccos(np.clip((np.trace(dR, axis1=1, axis2=2) - 1.0) / 2.0, -1.0, 1.0))
        assert ang.max() <= 3e-4
    # the left sole in the right sole's frame, actual against planned: no anchor in it
    gl, gr = d["left_traj"][:, T - 1], d["right_traj"][:, T - 1]
    Rgr = gr[:, 3:].reshape(B, 3, 3)
    p_rel_plan = np.einsum("bji,bj->bi", Rgr, gl[:, :3] - gr[:, :3])
    p_rel = np.einsum("bji,bj->bi", Rw[:, 1], P[:, 0] - P[:, 1])
    assert np.abs(p_rel - p_rel_plan).max() <= 2e-5
    dR = np.einsum("bji,bjk->bik", np.einsum("bji,bjk->bik", Rgr, gl[:, 3:].reshape(B, 3, 3)), np.einsum("bji,bjk->bik", Rw[:, 1], Rw[:, 0]))
    assert np.arccos(np.clip((np.trace(dR, axis1=1, axis2=2) - 1.0) / 2.0, -1.0, 1.0)).max() <= 6e-4
    mid0 = 0.5 * (d["left_traj"][:, 0, :2] + d["right_traj"][:, 0, :2])
    mid1 = 0.5 * (P[:, 0, :2] + P[:, 1, :2])
    assert np.all(np.abs(np.linalg.norm(mid1 - mid0, axis=1) / d["distance"] - 1.0) <= 1e-3)


@pytest.mark.gpu
@pytest.mark.parametrize("controller", ["mpc", "reactive"])
def test_launch_forms_agree(wca, planned_walk, controller):
    """ticks_per_launch 0 / 1 / 7, use_graph and two shards (first) give bit-identical results; splice is refused."""
    d = planned_walk
    B, T = d["q0"].shape[0], WALK_T
    outs = []
    for tpl, graph, chunks in ((0, False, [T]), (1, True, [5, 100, T - 105]), (7, False, [T]), (1, False, [T])):
        pipe = _pipe(wca, B, T, "iCubGazeboV2_5", controller, True, tpl=tpl)
        _upload(pipe, d)
        for n in chunks:
            pipe.run(n, use_graph=graph)
        outs.append(pipe.download())
    for o in outs[1:]:
        _same(outs[0], o)
    t_ = np.zeros((B, 10, 2))
    assert wca.capi.lib().wcqp_tick_splice_reference(pipe._h, 50, 10, t_.ctypes.data_as(C.c_void_p), None) == WCQP_E_UNSUPPORTED
    # two shards: robots [0, 2) and [2, 3) with first = 0 / 2
    parts = []
    for lo, hi in ((0, 2), (2, B)):
        sub = {k: (v[lo:hi] if isinstance(v, np.ndarray) and v.shape[:1] == (B,) else v) for k, v in d.items()}
        sub["first"] = lo
        pipe = _pipe(wca, hi - lo, T, "iCubGazeboV2_5", controller, True, first=lo)
        _upload(pipe, sub)
        pipe.run(T)
        parts.append(pipe.download())
    for k in ("q_des", "dcm", "com"):
        assert np.array_equal(np.concatenate([p_[k] for p_ in parts]), outs[0][k]), k
    for k in ("u0_log", "dq_log"):
        assert np.array_equal(np.concatenate([p_[k] for p_ in parts], axis=1), outs[0][k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("com_as_constraint", [False])
def test_create_refuses_where_fused_is_not_taken(wca, com_as_constraint):
    """Another IK route (CoM as a cost) with fused kinematics: WCQP_E_UNSUPPORTED (decided from the handles' host state, before the
    tick's device buffers)."""
    ik = wca.IkSolver(form=wca.IK_FORM_QPOASES, use_com_as_constraint=com_as_constraint, v_max=wca.synth.WALK_VMAX.copy())
    prm = _params(wca)
    prm.mpc = wca.MpcSolver().params
    prm.ik = ik.params
    prm.kin = _kin(wca).params
    h = C.c_void_p()
    assert wca.capi.lib().wcqp_tick_create(C.byref(prm), C.byref(h)) == WCQP_E_UNSUPPORTED and not h


@pytest.mark.gpu
def test_upload_validation(wca, planned_walk):
    d = planned_walk
    B, T = d["q0"].shape[0], WALK_T
    pipe = _pipe(wca, B, T, "iCubGazeboV2_5", "mpc", False)
    for mutate in ("no_contact", "fixed_in_air", "nan"):
        e = {k: np.array(v, copy=True) for k, v in d.items() if isinstance(v, np.ndarray)}
        e["first"] = 0
        if mutate == "no_contact":
            e["contact"][1, 200] = 4
        elif mutate == "fixed_in_air":
            e["contact"][2, 300] = 2 | 4
        else:
            e["left_twist"][0, 100, 2] = np.nan
        with pytest.raises(wca.WcqpError, match="invalid|INVALID"):
            _upload(pipe, e)
    # the checks run before the handle changes: after a refused upload a good one's state is intact and runs as a fresh handle does
    _upload(pipe, d)
    pipe.run(100)
    with pytest.raises(wca.WcqpError):
        e = {k: np.array(v, copy=True) for k, v in d.items() if isinstance(v, np.ndarray)}
        e["first"] = 0
        e["contact"][0, 300] = 0
        e["ref_traj"] += 1.0
        _upload(pipe, e)
    pipe.run(100)
    fresh = _pipe(wca, B, T, "iCubGazeboV2_5", "mpc", False)
    _upload(fresh, d)
    fresh.run(200)
    _same(pipe.download(), fresh.download())
    # a NaN beyond the stages a run can reach (max_ticks + 1 ..) is not looked at
    e = {k: np.array(v, copy=True) for k, v in d.items() if isinstance(v, np.ndarray)}
    e["first"] = 0
    e["left_traj"][0, T + 10, 0] = np.nan
    _upload(pipe, e)
