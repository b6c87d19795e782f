"""
ZMP-CoM gain scheduling in the closed-loop tick (wcqp_tick_params.zmp_gain_scheduling): the reference's `useGainScheduling 1`, set in
the zmpControllerParams.ini of all three shipped robots.  Every tick calls WalkingZMPController::setPhase(|dcm_des_dot| < 0.001) before
the ZMP-CoM law (WM/src/WalkingModule.cpp:657-662), which moves kCoM / kZMP between the stance and the walking values through a smoother
(WM/src/WalkingZMPController.cpp:29-125).  Checked against oracle/zmp_gains_spec.py: two separate smoothers per robot, advanced by
oracle/tick_spec.run_ticks(zmp_gain_schedule=...) with either DCM controller.
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest
from walking_controllers_amd.capi import E_INVALID as WCQP_E_INVALID, E_UNSUPPORTED as WCQP_E_UNSUPPORTED

import robots
from helpers import zmp_gains as zgh
from oracle import zmp_gains_spec as zg


K_DCM = {"iCubGazeboV2_5": 1.2, "iCubGenova04": 1.1, "icubGazeboSim": 1.2}   # dcmReactiveControllerParams.ini:1 (as test_tick_reactive)
VMAX = 0.45
KEYS = ("u0_log", "dq_log", "q_des", "dcm", "com")


# ---------------------------------------------------------------------------------------------------------------- CPU

def test_smoother_step_response_and_rest():
    """Unit DC gain, at rest at its initial value, the scipy cont2discrete(bilinear) check values at T = 0.05, dT = 0.01."""
    b, a = zg.tustin_coeffs(0.05, 0.01)
    assert a[0] == 1.0 and abs(b.sum() / a.sum() - 1.0) <= 1e-14
    f = zg.MinJerkSmoother(0.05, 0.01, 0.0)
    y = np.array([f.step(1.0) for _ in range(400)])
    assert np.abs(y[:6] - [0.0566, 0.2873, 0.6635, 0.9668, 1.0640, 1.0234]).max() <= 5e-5
    assert 1.05 < y.max() < 1.07 and abs(y[-1] - 1.0) <= 1e-12
    for y0 in (0.9, 6.0, 10.0):
        r = zg.MinJerkSmoother(0.1, 0.01, y0)
        assert max(abs(r.step(y0) - y0) for _ in range(300)) <= 1e-13 * y0


def test_one_filter_equals_two_filters():
    rng = np.random.default_rng(5)
    for robot, sched in zgh.ZMP_SCHEDULE.items():
        R = robots.ROBOTS[robot]
        vel = rng.normal(scale=0.01, size=(300, 2))
        vel[rng.random(300) < 0.4] = 0.0
        two = zg.gain_sequence(vel, 0.01, R["k_com"], R["k_zmp"], sched)
        one = zg.gain_sequence_one_filter(vel, 0.01, R["k_com"], R["k_zmp"], sched)
        assert np.abs(two - one).max() <= 1e-13
        assert np.abs(two[0] - [sched["k_com_stance"], sched["k_zmp_stance"]]).max() > 0 or zg.is_stance(vel[0])


def test_stance_flag_at_the_threshold():
    rng = np.random.default_rng(11)
    for _ in range(100):
        d = rng.normal(size=2)
        d /= np.linalg.norm(d)
        assert zg.is_stance(0.000999 * d) and not zg.is_stance(0.001001 * d)
    assert zg.is_stance([0.0, 0.0]) and not zg.is_stance([0.001, 0.0])


def test_wrapper_restores_the_patch_and_the_gains(wca):
    """A run with the reactive controller and a gain schedule writes nothing to `p` (field for field) and leaves oracle.qp_spec.mpc_exact
    the object it was, a run that raises included; the gains it used come back as zmp_gains."""
    from oracle import qp_spec, tick_spec as ts
    p = ts.TickParams()
    before, orig = dataclasses.replace(p), qp_spec.mpc_exact
    d = wca.synth.synth_tick_batch(2, 4)
    ipar = qp_spec.IKParams(v_max=VMAX * np.ones(23))
    kw = dict(dcm_controller="reactive", k_dcm=1.2, zmp_gain_schedule=zgh.ZMP_SCHEDULE["iCubGazeboV2_5"])
    out = ts.run_ticks(p, d, 4, ipar, **kw)
    assert out["zmp_gains"].shape == (4, 2, 2) and np.abs(out["zmp_gains"][-1] - [9.0, 3.0]).max() > 1e-3
    assert dataclasses.asdict(p) == dataclasses.asdict(before) and p.k_com == 9.0 and p.k_zmp == 3.0 and qp_spec.mpc_exact is orig
    with pytest.raises(IndexError):
        ts.run_ticks(p, d, 4, ipar, dcm_vel=np.zeros((2, 2, 2)), **kw)          # the velocities run out on tick 2: the run raises half way
    assert dataclasses.asdict(p) == dataclasses.asdict(before) and qp_spec.mpc_exact is orig and ts.qs.mpc_exact is orig


def test_binding_needs_the_schedule(wca):
    mk = lambda **kw: wca.TickPipeline(4, 10, wca.MpcSolver(), wca.IkSolver(), zmp_gain_scheduling=True, **kw)
    with pytest.raises(ValueError):
        mk(k_com_stance=6.0, k_zmp_stance=0.9)
    for bad in (dict(k_com_stance=float("nan"), k_zmp_stance=0.9, zmp_smoothing_time=0.05),
                dict(k_com_stance=6.0, k_zmp_stance=float("inf"), zmp_smoothing_time=0.05),
                dict(k_com_stance=6.0, k_zmp_stance=0.9, zmp_smoothing_time=0.0),
                dict(k_com_stance=6.0, k_zmp_stance=0.9, zmp_smoothing_time=-0.1)):
        with pytest.raises(ValueError):
            mk(**bad)


def test_create_refuses_a_bad_schedule_before_the_device(wca):
    """wcqp_tick_create checks the schedule before anything touches the device: WCQP_E_INVALID with or without a GPU."""
    pipe_params = wca.capi.TickParams()
    pipe_params.batch, pipe_params.max_ticks, pipe_params.step_ticks, pipe_params.ds_ticks = 4, 10, 180, 110
    pipe_params.ik.dof = 23
    for gs, kc, kz, T in ((1, float("nan"), 0.9, 0.05), (1, 6.0, float("-inf"), 0.05), (1, 6.0, 0.9, 0.0), (1, 6.0, 0.9, -1.0),
                          (1, 6.0, 0.9, float("nan")), (1, 6.0, 0.9, float("inf")), (2, 6.0, 0.9, 0.05)):
        prm = wca.capi.TickParams.from_buffer_copy(pipe_params)
        prm.zmp_gain_scheduling, prm.k_com_stance, prm.k_zmp_stance, prm.zmp_smoothing_time = gs, kc, kz, T
        h = C.c_void_p()
        assert wca.capi.lib().wcqp_tick_create(C.byref(prm), C.byref(h)) == WCQP_E_INVALID and not h


# ---------------------------------------------------------------------------------------------------------------- GPU

def _sched(robot):
    return zgh.ZMP_SCHEDULE[robot]


def _pipe(wca, B, T, robot, controller, ik, tpl=0, first=0, **kw):
    R = robots.ROBOTS[robot]
    ctl = dict(dcm_controller="reactive", k_dcm=K_DCM[robot]) if controller == "reactive" else {}
    return wca.TickPipeline(B, T, kw.pop("mpc", None) or wca.MpcSolver(), ik, first=first, log_ticks=T, k_com=R["k_com"], k_zmp=R["k_zmp"],
                            ticks_per_launch=tpl, zmp_gain_scheduling=True, **_sched(robot), **ctl, **kw)


def _paused(d, B, T, seed=0):
    """The robots of the batch with stance stretches: every other robot stands for a prefix, walks, stops, and walks again."""
    rng = np.random.default_rng(seed)
    pauses = {}
    for i in range(0, B, 2):
        a = int(rng.integers(3, 15))
        s = int(rng.integers(45, T - 60))
        pauses[i] = [(0, a), (s, int(rng.integers(12, 30)))]
    d = dict(d)
    d["ref_traj"], idx = zgh.pause_reference(np.asarray(d["ref_traj"]), pauses)
    if "zmp_ref" in d:
        d["zmp_ref"] = np.stack([np.asarray(d["zmp_ref"])[i, idx[i]] for i in range(B)])
    return d


def _reference(qs, p, d, T, ipar, robot, controller, vel=None, **kw):
    from oracle import tick_spec as ts
    return ts.run_ticks(p, d, T, ipar, dcm_controller=controller, k_dcm=K_DCM[robot], dcm_vel=vel, zmp_gain_schedule=_sched(robot), **kw)


def _close(out, ref, tol=1e-9, logger=False):
    for k in KEYS:
        err = np.abs(out[k] - ref[k]).max()
        assert err <= tol, (k, err)
    assert np.array_equal(out["mpc_fail"], ref["mpc_fail"]) and np.array_equal(out["ik_fail"], ref["ik_fail"])
    assert np.abs(out["zmp_gains"] - ref["zmp_gains"][-1]).max() <= 1e-13
    if logger:
        err = np.abs(out["logger"][:, :, 13:17] - ref["logger"][:, :, 13:17]).max()
        assert err <= tol, err


def _meaningful(ref, d, B, T):
    """>= 90 % of the robots end without an IK failure, >= a quarter pass through a stance stretch and out of it."""
    assert (ref["ik_fail"] == 0).mean() >= 0.9, ref["ik_fail"]
    stance = zg.is_stance(zg.forward_difference(np.asarray(d["ref_traj"]), 0.01)[:, :T])       # [B][T]
    through = [i for i in range(B) if stance[i].any() and (~stance[i][np.argmax(stance[i]):]).any()]
    assert len(through) >= B / 4, through


def _same(a, b, keys=KEYS + ("ik_fail", "mpc_fail", "hot_try", "hot_hit", "active_lower", "active_upper", "zmp_gains")):
    for k in keys:
        assert np.array_equal(a[k], b[k]), k


@pytest.fixture(scope="module")
def paused_batch(wca):
    B, T = 16, 160
    return _paused(wca.synth.synth_tick_batch(B, T), B, T)


@pytest.mark.gpu
@pytest.mark.parametrize("controller", ["mpc", "reactive"])
@pytest.mark.parametrize("robot", robots.NAMES)
def test_gain_sequence_tick_by_tick(wca, qs, paused_batch, robot, controller):
    """run(1) at a time: the gains of every tick against the two-filter restatement - a standing prefix, a walk, a stop and a restart, and
    explicit velocities straddling the threshold."""
    B, T = 16, 160
    d = paused_batch
    R = robots.ROBOTS[robot]
    vel = zg.forward_difference(np.asarray(d["ref_traj"]), 0.01)
    rng = np.random.default_rng(3)
    straddle = vel.copy()
    for i in range(B):
        for t in rng.choice(T, 20, replace=False):
            u = rng.normal(size=2)
            straddle[i, t] = u / np.linalg.norm(u) * (0.000999 if rng.random() < 0.5 else 0.001001)
    for v, explicit in ((vel, False), (straddle, True)):
        expect = np.stack([zg.gain_sequence(v[i, :T], 0.01, R["k_com"], R["k_zmp"], _sched(robot)) for i in range(B)], axis=1)
        for alg in (0, 4):
            pipe = _pipe(wca, B, T, robot, controller, wca.IkSolver(form=wca.IK_FORM_QPOASES, v_max=VMAX, algorithm=alg))
            assert pipe.info()["zmp_gain_scheduling"] is True
            pipe.upload(d, dcm_vel_traj=v if explicit else None)
            g0 = pipe.download()["zmp_gains"]
            assert np.array_equal(g0, np.tile([_sched(robot)["k_com_stance"], _sched(robot)["k_zmp_stance"]], (B, 1)))
            for t in range(T):
                pipe.run(1)
                err = np.abs(pipe.download()["zmp_gains"] - expect[t]).max()
                assert err <= 1e-13, (alg, t, err)
        assert np.isclose(expect.max(axis=(0, 1)), [R["k_com"], R["k_zmp"]], atol=0.3).all()


@pytest.mark.gpu
@pytest.mark.parametrize("controller", ["mpc", "reactive"])
@pytest.mark.parametrize("alg", [0, 4, 3])
def test_closed_loop_constant_jacobians(wca, qs, paused_batch, controller, alg):
    """The skewed single launch (0) and the in-order forms of algorithms 4 and 3 against the restatement, 160 ticks."""
    from oracle import tick_spec as ts
    B, T = 16, 160
    robot = "iCubGazeboV2_5"
    R = robots.ROBOTS[robot]
    p = ts.TickParams(k_com=R["k_com"], k_zmp=R["k_zmp"])
    d = paused_batch
    ref = _reference(qs, p, d, T, qs.IKParams(v_max=VMAX * np.ones(23)), robot, controller)
    _meaningful(ref, d, B, T)
    pipe = _pipe(wca, B, T, robot, controller, wca.IkSolver(form=wca.IK_FORM_QPOASES, v_max=VMAX, algorithm=alg))
    pipe.upload(d)
    pipe.run(T)
    _close(pipe.download(), ref)
    # (the fixed gains give another run: the gains reach the joints through the desired CoM; the plant follows the controller's ZMP)
    fixed = ts.run_ticks(p, d, T, qs.IKParams(v_max=VMAX * np.ones(23)), dcm_controller=controller, k_dcm=K_DCM[robot])
    assert np.abs(ref["dq_log"] - fixed["dq_log"]).max() > 1e-6


def _walk(wca, B, T, horizon):
    kin = wca.KinModel(wca.synth.icub_like_model())
    kb = wca.synth.synth_walk_kin_batch(B)
    poses = kin.jacobians_host(kb["base"], kb["q"], state=np.zeros((B, 87)))["state"]
    return kin, _paused(wca.synth.synth_walk_batch(B, T, poses, kb, horizon=horizon), B, T, seed=1)


@pytest.mark.gpu
@pytest.mark.parametrize("controller,horizon,handoff", [("mpc", 50, 0), ("mpc", 50, 1), ("mpc", 50, 2),
                                                        ("reactive", 50, 0), ("reactive", 200, 0), ("reactive", 50, 1), ("reactive", 200, 1),
                                                        ("reactive", 50, 2), ("reactive", 200, 2)])
def test_closed_loop_kinematics(wca, qs, controller, horizon, handoff):
    """FUSED (0), DENSE (1) and COMPACT (2) kinematics hand-offs, with logger rows on the FUSED form (columns 13-16: com_des and its velocity)."""
    from oracle import tick_spec as ts
    B, T = 12, 150
    robot = "iCubGazeboV2_5"
    p = ts.TickParams(horizon=horizon)
    kin, d = _walk(wca, B, T, horizon)
    vmax = wca.synth.WALK_VMAX.copy()
    ipar = qs.IKParams(v_max=vmax.copy(), joint_reg_deg=wca.synth.WALK_POSTURE_DEG.copy())
    L = 40 if handoff == 0 else 0
    ref = _reference(qs, p, d, T, ipar, robot, controller, kin_model=wca.synth.icub_like_model(), foot_rect=wca.synth.FOOT_RECT, logger_ticks=L)
    _meaningful(ref, d, B, T)
    ik = wca.IkSolver(form=wca.IK_FORM_QPOASES, v_max=vmax, joint_reg_rad=np.deg2rad(wca.synth.WALK_POSTURE_DEG))
    pipe = _pipe(wca, B, T, robot, controller, ik, kin=kin, kin_handoff=handoff, logger_ticks=L, mpc=wca.MpcSolver(horizon=horizon))
    assert pipe.info()["kin_handoff"] == {0: "fused", 1: "dense", 2: "compact"}[handoff]
    pipe.upload(d)
    pipe.run(T)
    _close(pipe.download(), ref, logger=L > 0)


@pytest.mark.gpu
@pytest.mark.parametrize("controller", ["mpc", "reactive"])
def test_logger_rows_constant_jacobians(wca, qs, paused_batch, controller):
    from oracle import tick_spec as ts
    B, T, L = 16, 160, 60
    robot = "icubGazeboSim"
    R = robots.ROBOTS[robot]
    p = ts.TickParams(k_com=R["k_com"], k_zmp=R["k_zmp"])
    ref = _reference(qs, p, paused_batch, T, qs.IKParams(v_max=VMAX * np.ones(23)), robot, controller, logger_ticks=L)
    _meaningful(ref, paused_batch, B, T)
    pipe = _pipe(wca, B, T, robot, controller, wca.IkSolver(form=wca.IK_FORM_QPOASES, v_max=VMAX), logger_ticks=L)
    pipe.upload(paused_batch)
    pipe.run(29); pipe.run(T - 29)
    _close(pipe.download(), ref, logger=True)


@pytest.mark.gpu
@pytest.mark.parametrize("controller", ["mpc", "reactive"])
@pytest.mark.parametrize("kin_mode", [False, True], ids=["constant_jacobians", "fused_kinematics"])
def test_external_plant(wca, qs, controller, kin_mode):
    """Measured DCM / CoM / ZMP / joints from outside, one tick per call, against run_ticks(external=...)."""
    from oracle import tick_spec as ts
    B, T = 10, 150
    robot = "iCubGenova04"
    R = robots.ROBOTS[robot]
    p = ts.TickParams(k_com=R["k_com"], k_zmp=R["k_zmp"])
    if kin_mode:
        kin, d = _walk(wca, B, T, 50)
        vmax = wca.synth.WALK_VMAX.copy()
        ipar = qs.IKParams(v_max=vmax.copy(), joint_reg_deg=wca.synth.WALK_POSTURE_DEG.copy())
        okw = dict(kin_model=wca.synth.icub_like_model(), foot_rect=wca.synth.FOOT_RECT)
        mk_ik = lambda: wca.IkSolver(form=wca.IK_FORM_QPOASES, v_max=vmax, joint_reg_rad=np.deg2rad(wca.synth.WALK_POSTURE_DEG))
    else:
        kin, d = None, _paused(wca.synth.synth_tick_batch(B, T), B, T, seed=2)
        ipar, okw = qs.IKParams(v_max=VMAX * np.ones(23)), {}
        mk_ik = lambda: wca.IkSolver(form=wca.IK_FORM_QPOASES, v_max=VMAX)
    internal = _reference(qs, p, d, T, ipar, robot, controller, **okw)
    rng = np.random.default_rng(4)
    ext = dict(dcm=internal["dcm_log"] + 1e-4 * rng.normal(size=(T, B, 2)), com=internal["com_log"] + 5e-5 * rng.normal(size=(T, B, 2)),
               zmp=internal["zmp_log"] + 2e-4 * rng.normal(size=(T, B, 2)), q=internal["q_log"] + 1e-3 * rng.normal(size=(T, B, 23)))
    ref = _reference(qs, p, d, T, ipar, robot, controller, external=ext, **okw)
    _meaningful(ref, d, B, T)
    pipe = _pipe(wca, B, T, robot, controller, mk_ik(), kin=kin, external_feedback=True)
    pipe.upload(d)
    for t in range(T):
        pipe.set_feedback_host(ext["dcm"][t], ext["com"][t], ext["zmp"][t], ext["q"][t])
        pipe.run(1)
    out = pipe.download()
    for key in ("u0_log", "dq_log", "q_des"):
        assert np.abs(out[key] - ref[key]).max() <= 1e-9, key
    assert np.array_equal(out["ik_fail"], ref["ik_fail"]) and np.array_equal(out["mpc_fail"], ref["mpc_fail"])
    assert np.abs(out["zmp_gains"] - ref["zmp_gains"][-1]).max() <= 1e-13


@pytest.mark.gpu
@pytest.mark.parametrize("controller", ["mpc", "reactive"])
def test_explicit_dcm_velocity(wca, qs, paused_batch, controller):
    """The planner's DCM velocity omega (ref - zmp_ref) drives the stance flag (and the reactive law); the forward difference passed
    explicitly is what NULL means, bit for bit."""
    from oracle import tick_spec as ts
    B, T = 16, 160
    robot = "iCubGazeboV2_5"
    p = ts.TickParams()
    d = paused_batch
    vel = np.sqrt(p.gravity / p.com_height) * (np.asarray(d["ref_traj"]) - np.asarray(d["zmp_ref"]))
    vel[zg.is_stance(zg.forward_difference(np.asarray(d["ref_traj"]), p.dT))] = 0.0      # the planner stands where the reference does
    ref = _reference(qs, p, d, T, qs.IKParams(v_max=VMAX * np.ones(23)), robot, controller, vel=vel)

    def run(v, tpl=0):
        pipe = _pipe(wca, B, T, robot, controller, wca.IkSolver(form=wca.IK_FORM_QPOASES, v_max=VMAX), tpl=tpl)
        pipe.upload(d, dcm_vel_traj=v)
        pipe.run(T)
        return pipe.download()
    out = run(vel)
    _close(out, ref)
    _same(run(zg.forward_difference(np.asarray(d["ref_traj"]), p.dT)), run(None))
    _same(run(vel, 1), out)


@pytest.mark.gpu
@pytest.mark.parametrize("controller", ["mpc", "reactive"])
def test_ticks_per_launch_shards_splice_and_upload(wca, qs, controller):
    """ticks_per_launch 0, 1 and 7 and a two-shard split give the same bits; a splice mid-run follows the restatement spliced the same
    way; an upload rewinds the smoother."""
    from oracle import tick_spec as ts
    B, T = 16, 160
    robot = "iCubGazeboV2_5"
    full_d = _paused(wca.synth.synth_tick_batch(B, T), B, T)
    mk_ik = lambda: wca.IkSolver(form=wca.IK_FORM_QPOASES, v_max=VMAX)
    outs = []
    for tpl, graph in ((0, False), (1, True), (7, False)):
        pipe = _pipe(wca, B, T, robot, controller, mk_ik(), tpl=tpl)
        pipe.upload(full_d)
        pipe.run(61, use_graph=graph); pipe.run(T - 61, use_graph=graph)
        outs.append(pipe.download())
        if tpl == 7:
            pipe.upload(full_d)        # rewinds: the same run again
            pipe.run(61); pipe.run(T - 61)
            outs.append(pipe.download())
    for o in outs[1:]:
        _same(outs[0], o)
    half = {k: (v[B // 2:] if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == B else v) for k, v in full_d.items()}
    half["first"] = B // 2
    pipe = _pipe(wca, B // 2, T, robot, controller, mk_ik(), first=B // 2)
    pipe.upload(half)
    pipe.run(61); pipe.run(T - 61)
    part = pipe.download()
    for key in ("u0_log", "dq_log"):
        assert np.array_equal(part[key], outs[0][key][:, B // 2:]), key
    for key in ("q_des", "dcm", "com", "ik_fail", "mpc_fail", "zmp_gains"):
        assert np.array_equal(part[key], outs[0][key][B // 2:]), key
    # a splice at tick 40 of stages 50..89 (NULL velocities: the forward difference follows the new stages); the new tail stands still
    p = ts.TickParams()
    tail = np.repeat(np.asarray(full_d["ref_traj"])[:, 50:51], 40, axis=1)
    pipe = _pipe(wca, B, T, robot, controller, mk_ik())
    pipe.upload(full_d)
    pipe.run(40)
    pipe.splice_reference(50, tail)
    pipe.run(T - 40)
    out = pipe.download()
    ref = _reference(qs, p, full_d, T, qs.IKParams(v_max=VMAX * np.ones(23)), robot, controller, splices={40: (50, tail)})
    _close(out, ref)
    # with uploaded velocities the splice has no velocity tail
    pipe = _pipe(wca, B, T, robot, controller, mk_ik())
    pipe.upload(full_d, dcm_vel_traj=zg.forward_difference(np.asarray(full_d["ref_traj"]), p.dT))
    pipe.run(5)
    t_ = np.ascontiguousarray(tail)
    assert wca.capi.lib().wcqp_tick_splice_reference(pipe._h, 50, 40, t_.ctypes.data_as(C.c_void_p), None) == WCQP_E_UNSUPPORTED


@pytest.mark.gpu
def test_refusals_and_info(wca):
    mk = lambda **kw: wca.TickPipeline(8, 30, wca.MpcSolver(), wca.IkSolver(form=wca.IK_FORM_QPOASES, v_max=VMAX), **kw)
    assert mk().info()["zmp_gain_scheduling"] is False
    assert mk(zmp_gain_scheduling=True, **_sched("iCubGenova04")).info()["zmp_gain_scheduling"] is True
    base = mk()
    for kc, kz, T in ((float("nan"), 0.9, 0.1), (6.0, float("inf"), 0.1), (6.0, 0.9, 0.0), (6.0, 0.9, -0.05)):
        prm = wca.capi.TickParams.from_buffer_copy(base.params)
        prm.zmp_gain_scheduling, prm.k_com_stance, prm.k_zmp_stance, prm.zmp_smoothing_time = 1, kc, kz, T
        h = C.c_void_p()
        assert wca.capi.lib().wcqp_tick_create(C.byref(prm), C.byref(h)) == WCQP_E_INVALID and not h
        with pytest.raises(ValueError):
            mk(zmp_gain_scheduling=True, k_com_stance=kc, k_zmp_stance=kz, zmp_smoothing_time=T)


@pytest.mark.gpu
@pytest.mark.parametrize("controller", ["mpc", "reactive"])
def test_off_is_off(wca, paused_batch, controller):
    """A zeroed scheduling block and a handle made without the keywords: the same bits, the fixed gains reported."""
    B, T = 16, 160
    ctl = dict(dcm_controller="reactive", k_dcm=1.2) if controller == "reactive" else {}
    mk = lambda **kw: wca.TickPipeline(B, T, wca.MpcSolver(), wca.IkSolver(form=wca.IK_FORM_QPOASES, v_max=VMAX), log_ticks=T, **ctl, **kw)
    a = mk()
    b = mk(zmp_gain_scheduling=False, k_com_stance=6.0, k_zmp_stance=0.9, zmp_smoothing_time=0.05)
    assert b.params.zmp_gain_scheduling == 0 and not b.info()["zmp_gain_scheduling"]
    outs = []
    for pipe in (a, b):
        pipe.upload(paused_batch)
        pipe.run(T)
        outs.append(pipe.download())
    _same(*outs)
    assert np.array_equal(outs[0]["zmp_gains"], np.tile([9.0, 3.0], (B, 1)))
