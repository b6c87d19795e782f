"""A resident plan on the external-feedback tick (wcqp_tick_params_ext.resident_plan, wcqp_tick_set_desired_from_plan): a streamed
handle that holds a generated plan and stages tick t's stage on the device.  CPU: the ABI, the refusals that need no device, the scenario
(helpers/resident_plan.py) as a fair yardstick.  GPU: the walk against oracle/tick_spec.py on the restated stages, against the per-tick
hand-over of the same plan, under disturbed feedback, through the sensor form, replanned between two ticks, and the forms and refusals."""
import ctypes as C

import numpy as np
import pytest
from walking_controllers_amd.capi import E_INVALID as WCQP_E_INVALID, E_UNSUPPORTED as WCQP_E_UNSUPPORTED

import robots
from helpers import footstep_plan as fp
from helpers import resident_plan as rs
from helpers import streamed_tick as stt
from helpers import unicycle_plan as up
from helpers import zmp_gains as zg

CFGS = list(rs.CONFIGS)
B, MAXT = rs.B, rs.MAXT
SAME = ("u0_log", "dq_log", "q_des", "ik_fail", "mpc_fail", "measured", "feedback_fail")
WINDOW = ("left_traj", "right_traj", "left_twist", "right_twist", "contact")


# ---------------------------------------------------------------------------------------------------------------- CPU

def test_ext_structs_are_closed_and_entry_points_refuse_null(wca):
    """the two new fields live in structs of their own (wcqp_tick_params_ext, wcqp_tick_info_ext), one int32 each, so wcqp_tick_params and
    wcqp_tick_info keep their last fields; the library exports the three new entry points, which refuse NULL arguments"""
    cp = wca.capi
    for cls in (cp.TickParamsExt, cp.TickInfoExt):
        assert [k for k, _ in cls._fields_] == ["resident_plan"] and cls.resident_plan.size == 4
    assert cp.TickParams._fields_[-1][0] == "position_ik" and cp.TickInfo._fields_[-1][0] == "ik_mode"
    for sym in ("wcqp_tick_set_desired_from_plan", "wcqp_tick_create_ext", "wcqp_tick_get_info_ext"):
        assert sym in cp.ABI_SYMBOLS and getattr(cp.lib(), sym)
    assert cp.lib().wcqp_tick_set_desired_from_plan(None, None) == WCQP_E_INVALID
    assert cp.lib().wcqp_tick_get_info_ext(None, None) == WCQP_E_INVALID


def _params(wca, **kw):
    """the wcqp_tick_params of a streamed handle that every check in front of the device passes, with fields replaced"""
    prm = wca.capi.TickParams()
    prm.batch, prm.max_ticks, prm.step_ticks, prm.ds_ticks = 4, 10, 180, 110
    prm.mpc.horizon, prm.mpc.sampling_time, prm.mpc.com_height, prm.mpc.gravity = 50, 0.01, 0.53, 9.81
    prm.ik.dof, prm.use_kinematics, prm.kin_handoff, prm.streamed_trajectories, prm.plant = 23, 1, 0, 1, 1
    for k in range(9):
        prm.neck_additional_rotation[k] = float(k % 4 == 0)
    for k, v in kw.items():
        setattr(prm, k, v)
    return prm


@pytest.mark.parametrize("bad,rc", [(dict(resident_plan=1, streamed_trajectories=0), WCQP_E_UNSUPPORTED),
                                    (dict(resident_plan=1, streamed_trajectories=0, plant=0), WCQP_E_UNSUPPORTED),
                                    (dict(resident_plan=1, streamed_trajectories=0, planned_trajectories=1, plant=0), WCQP_E_UNSUPPORTED),
                                    (dict(resident_plan=1, planned_trajectories=1), WCQP_E_UNSUPPORTED),
                                    (dict(resident_plan=1, streamed_trajectories=0, planned_trajectories=1), WCQP_E_UNSUPPORTED),
                                    (dict(resident_plan=1, logger_ticks=5), WCQP_E_UNSUPPORTED),
                                    (dict(resident_plan=2), WCQP_E_INVALID), (dict(resident_plan=-1), WCQP_E_INVALID)])
def test_create_refuses_before_the_device(wca, bad, rc):
    """resident_plan without streamed_trajectories is UNSUPPORTED, a value other than 0 / 1 INVALID, and every refusal of a streamed handle
    stays - all before anything touches the device (so with or without a GPU)"""
    h = C.c_void_p()
    bad = dict(bad)
    ext = wca.capi.TickParamsExt(bad.pop("resident_plan"))
    assert wca.capi.lib().wcqp_tick_create_ext(C.byref(_params(wca, **bad)), C.byref(ext), C.byref(h)) == rc and not h
    assert wca.capi.lib().wcqp_tick_create_ext(None, C.byref(ext), C.byref(h)) == WCQP_E_INVALID and not h


def test_binding_refuses_bad_arguments(wca):
    mpc, ik = wca.MpcSolver.__new__(wca.MpcSolver), wca.IkSolver.__new__(wca.IkSolver)
    mpc.params = wca.capi.MpcParams(); ik.params = wca.capi.IkParams(); ik.dof = 23
    with pytest.raises(ValueError, match="streamed"):
        wca.TickPipeline(4, 10, mpc, ik, resident_plan=True)
    with pytest.raises(ValueError, match="streamed"):
        wca.TickPipeline(4, 10, mpc, ik, resident_plan=True, planned_trajectories=True, neck_additional_rotation=np.eye(3))
    pipe = object.__new__(wca.TickPipeline)
    pipe.planned, pipe.streamed, pipe.resident, pipe.batch, pipe._h = False, True, False, 13, None
    with pytest.raises(ValueError, match="resident_plan"):
        pipe.upload_footsteps({}, {})
    with pytest.raises(ValueError, match="resident_plan"):
        pipe.replan_footsteps(np.full(13, -1), {}, 5)


def test_the_scenario_is_a_fair_yardstick(wca, qs):
    """The restatement walks the scenario without a failure under both controllers - with the internal plant, fed that run's own states (the
    same run to 1e-12) and under the disturbed feedback - the joints move, every walking robot changes its contact pair at least three
    times and switches its fixed-frame foot, some robots stand, some turn, and some plans end inside the run."""
    fs, plan, stages = rs.scenario(wca)
    flags = stages["contact"].astype(int)
    walking = np.nonzero(fs["n_steps"] > 0)[0]
    assert 0 < len(walking) < B and (fs["n_steps"] == 0).sum() >= 1
    for i in range(B):
        changes = int((np.diff(flags[:, i] & 3) != 0).sum())
        if i in walking:
            assert changes >= 3 and set(flags[:, i] & 4) == {0, 4}, i
        else:
            assert changes == 0, i
    tg = fs["target"][fs["n_steps"][:, None] > np.arange(rs.K)]
    assert (tg[:, 2] > 0).any() and (tg[:, 2] < 0).any() and (tg[:, 2] == 0).any()                       # turns both ways, and a straight walk
    ends = rs.FIRST_DS + fs["n_steps"] * (rs.SS + rs.DS) - rs.DS + rs.FINAL_DS                          # the stage from which the robot stands
    assert ((ends < MAXT) & (fs["n_steps"] > 0)).any() and (ends > MAXT).any()                          # a plan that ends inside the run, one cut by it
    assert MAXT <= 200
    for cfg in CFGS:
        inner = rs.internal(wca, qs, cfg)
        ext, dist = rs.disturbed(wca, qs, cfg)
        for run in (inner, dist):
            assert (run["ik_fail"] == 0).all() and (run["mpc_fail"] == 0).all()
            assert np.abs(run["dq_log"]).max() > 1e-2
        assert np.abs(dist["u0_log"] - inner["u0_log"]).max() > 1e-4
    fed = rs.restate(wca, qs, "mpc", plan, external=stt.external_of(rs.internal(wca, qs, "mpc")))
    for k in rs.KEYS:
        assert np.abs(fed[k] - rs.internal(wca, qs, "mpc")[k]).max() <= 1e-12, k
    assert (fed["ik_fail"] == 0).all() and (fed["mpc_fail"] == 0).all()


# ---------------------------------------------------------------------------------------------------------------- GPU

def _pipe(wca, cfg, batch=B, resident=True):
    controller, gs = rs.CONFIGS[cfg]
    R = robots.ROBOTS[rs.ROBOT]
    ctl = dict(dcm_controller="reactive", k_dcm=rs.K_DCM) if controller == "reactive" else {}
    sch = dict(zmp_gain_scheduling=True, **zg.ZMP_SCHEDULE[rs.ROBOT]) if gs else {}
    ik = wca.IkSolver(form=wca.IK_FORM_QPOASES, neck_weight=R["neck_weight"] * np.eye(3), joint_reg_weights=np.array(R["reg_w"], float),
                      joint_reg_gains=np.array(R["reg_k"], float), joint_reg_rad=np.deg2rad(wca.synth.WALK_POSTURE_DEG),
                      v_max=wca.synth.WALK_VMAX.copy(), k_pos_com=R["k_pos_com"], k_pos_foot=R["k_pos_foot"], k_att_foot=R["k_att_foot"],
                      k_neck=R["k_neck"])
    return wca.TickPipeline(batch, MAXT, wca.MpcSolver(horizon=50), ik, log_ticks=MAXT, k_com=R["k_com"], k_zmp=R["k_zmp"],
                            kin=wca.KinModel(wca.synth.icub_like_model()), external_feedback=True, streamed_trajectories=True,
                            neck_additional_rotation=np.array(R["additional_rotation"]), resident_plan=resident, **ctl, **sch)


def _feed(pipe, ext, t, rows=slice(None)):
    pipe.set_feedback_host(ext["dcm"][t][rows], ext["com"][t][rows], ext["zmp"][t][rows], ext["q"][t][rows] if ext.get("q") is not None else None)


def _walk(pipe, ext, t1=MAXT, t0=0, rows=slice(None)):
    """ticks t0 .. t1 - 1 of the per-tick order: the stage out of the plan, the plain feedback of `ext`, one tick"""
    for t in range(t0, t1):
        pipe.set_desired_from_plan()
        _feed(pipe, ext, t, rows)
        pipe.run(1)


def _stage(stages, t):
    return tuple(stages[k][t] for k in ("left_pose", "right_pose", "left_twist", "right_twist", "contact", "com_height", "com_height_vel"))


def _handed_over(pipe, stages, ext, before=False):
    """the same walk with every stage handed over by set_desired_host (before: behind a set_desired_from_plan it replaces)"""
    for t in range(MAXT):
        if before:
            pipe.set_desired_from_plan()
        pipe.set_desired_host(*_stage(stages, t))
        _feed(pipe, ext, t)
        pipe.run(1)


def _window_stages(w):
    return stt.stages_of(dict(w, com_height_traj=w["com_height"]), MAXT)


def _upload_streamed(pipe, fs, w):
    """wcqp_tick_upload of a streamed handle without a plan, from a plan window"""
    pipe.upload(dict(state0=fs["state0"], q0=fs["q0"], com0=fs["com0"], ref_traj=w["ref_traj"], dcm0=w["ref_traj"][:, 0].copy(), u_init=w["u_init"]),
                dcm_vel_traj=w.get("dcm_vel_traj"))


def _close(out, ref, tol=1e-9, n=MAXT):
    assert np.array_equal(out["ik_fail"], ref["ik_fail"]) and np.array_equal(out["mpc_fail"], ref["mpc_fail"])
    for k in rs.KEYS:
        err = np.abs((out[k][:n] if k.endswith("_log") else out[k]) - ref[k]).max()
        print(k, err)
    for k in rs.KEYS:
        err = np.abs((out[k][:n] if k.endswith("_log") else out[k]) - ref[k]).max()
        assert err <= tol, (k, err)


def _same(a, b, keys=SAME):
    for k in keys:
        assert np.array_equal(a[k], b[k]), k


@pytest.fixture(scope="module")
def plan_run(wca, qs):
    """per configuration: upload_footsteps on a resident-plan handle, then the walk fed the restatement's internal-plant states, staged from
    the plan every tick -> (the handle, its outputs, its whole plan)"""
    cache = {}

    def get(cfg):
        if cfg not in cache:
            fs = rs.scenario(wca)[0]
            pipe = _pipe(wca, cfg)
            pipe.upload_footsteps(fs, fs)
            w = pipe.plan_window()
            _walk(pipe, stt.external_of(rs.internal(wca, qs, cfg)))
            cache[cfg] = (pipe, pipe.download(), w)
        return cache[cfg]
    return get


@pytest.fixture(scope="module")
def handover_run(wca, qs, plan_run):
    """per configuration: a streamed handle WITHOUT a plan fed tick by tick the stages of plan_run's plan_window() through set_desired_host,
    with the same feedback -> its outputs"""
    cache = {}

    def get(cfg):
        if cfg not in cache:
            fs = rs.scenario(wca)[0]
            w = plan_run(cfg)[2]
            pipe = _pipe(wca, cfg, resident=False)
            _upload_streamed(pipe, fs, w)
            _handed_over(pipe, _window_stages(w), stt.external_of(rs.internal(wca, qs, cfg)))
            cache[cfg] = pipe.download()
        return cache[cfg]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", CFGS)
def test_against_the_restatement(wca, qs, plan_run, cfg):
    """(1) upload_footsteps, then per tick set_desired_from_plan, set_feedback_host with the restatement's internal-plant states, run(1):
    u0_log, dq_log and q_des within 1e-9 of run_ticks on the restated stages, equal failure counts.
    Measured on an MI355X: see DESIGN §8.18."""
    pipe, out, w = plan_run(cfg)
    info = pipe.info()
    assert info["resident_plan"] and info["streamed_trajectories"] and not info["planned_trajectories"] and info["plan_generated"]
    assert info["kin_handoff"] == "fused" and info["ticks_per_launch"] == 1 and info["launches_per_tick"] == 1
    plan = rs.scenario(wca)[1]
    assert np.array_equal(w["contact"], plan["contact"])
    for k in ("left_traj", "right_traj", "ref_traj"):
        assert np.abs(w[k] - plan[k]).max() <= 1e-12, k
    ref = rs.internal(wca, qs, cfg)
    _close(out, ref)
    assert (out["ik_fail"] == 0).all() and out["feedback_fail"].sum() == 0 and out["tick"] == MAXT


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", CFGS)
def test_against_the_hand_over(plan_run, handover_run, cfg):
    """(2) the walk staged from the resident plan against the same plan handed over stage by stage through plan_window() and
    set_desired_host on a streamed handle without a plan: within 1e-9 (the measured difference is printed)"""
    a, b = plan_run(cfg)[1], handover_run(cfg)
    for k in rs.KEYS:
        print(k, "difference", np.abs(a[k] - b[k]).max(), "bit for bit" if np.array_equal(a[k], b[k]) else "")
    for k in rs.KEYS:
        assert np.abs(a[k] - b[k]).max() <= 1e-9, k
    assert np.array_equal(a["ik_fail"], b["ik_fail"]) and np.array_equal(a["mpc_fail"], b["mpc_fail"])


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", CFGS)
def test_disturbed_feedback_follows_the_restatement(wca, qs, cfg):
    """(3) an offset DCM, a ZMP that is not the previous command, measured joints off the desired ones: within 1e-9 of the restatement"""
    fs = rs.scenario(wca)[0]
    ext, ref = rs.disturbed(wca, qs, cfg)
    pipe = _pipe(wca, cfg)
    pipe.upload_footsteps(fs, fs)
    _walk(pipe, ext)
    out = pipe.download()
    _close(out, ref)
    assert out["feedback_fail"].sum() == 0 and np.abs(out["dq_log"]).max() > 1e-2
    assert np.abs(out["measured"] - np.concatenate([ext["dcm"][MAXT - 1], ext["com"][MAXT - 1], ext["zmp"][MAXT - 1]], 1)).max() == 0.0


@pytest.mark.gpu
def test_sensor_form(wca, qs):
    """(4) per tick set_desired_from_plan, set_sensor_feedback_host, run(1), across switches of the fixed-frame foot, the robot in the loop
    restated with its recording (test_tick_streamed.py::test_sensor_form_on_moved_feet and its bars): download()["measured"] within 1e-12
    of the restated evaluation on the ticks around every switch, the run within 1e-9 (dq_log 1e-8) of the restatement, no robot stops, and
    a handle fed the recorded values through the plain form on those ticks is bit for bit the sensor-fed one."""
    fs, _, stages = rs.scenario(wca)
    check, ref = rs.sensor_case(wca, qs)
    T = rs.SENSOR_T
    assert (ref["ik_fail"] == 0).all() and (ref["mpc_fail"] == 0).all() and np.abs(ref["dq_log"]).max() > 1e-2
    readings, restated = ref["readings"], ref["measured_log"]
    moved = max(np.abs(stages[f][check[-1]] - stages[f][0]).max() for f in ("left_pose", "right_pose"))
    assert moved > 1e-3 and len(check) >= 10
    a = _pipe(wca, "mpc")
    a.upload_footsteps(fs, fs)
    with pytest.raises(wca.WcqpError, match=r"\(-1\)"):
        a.set_sensor_feedback_host(*readings[0])            # the anchor's stage is not there yet
    measured = {}
    for t in range(T):
        a.set_desired_from_plan()
        a.set_sensor_feedback_host(*readings[t])
        a.run(1)
        if t in check:
            measured[t] = a.download()["measured"]
            err = np.abs(measured[t] - restated[t]).max()
            print("tick", t, "measured error", err)
            assert err <= 1e-12, (t, err)
    oa = a.download()
    assert oa["feedback_fail"].sum() == 0 and (oa["ik_fail"] == 0).all()
    assert np.array_equal(oa["ik_fail"], ref["ik_fail"]) and np.array_equal(oa["mpc_fail"], ref["mpc_fail"])
    for k, tol in (("u0_log", 1e-9), ("dq_log", 1e-8), ("q_des", 1e-9)):
        err = np.abs((oa[k][:T] if k.endswith("_log") else oa[k]) - ref[k]).max()
        print(k, err)
        assert err <= tol, (k, err)
    b = _pipe(wca, "mpc")
    b.upload_footsteps(fs, fs)
    for t in range(T):
        b.set_desired_from_plan()
        m = measured.get(t)
        if m is not None:
            b.set_feedback_host(m[:, 0:2], m[:, 2:4], m[:, 4:6], readings[t][0])       # the plain form, fed what the sensor form evaluated
        else:
            b.set_sensor_feedback_host(*readings[t])
        b.run(1)
    _same(oa, b.download(), ("u0_log", "dq_log", "q_des", "ik_fail", "mpc_fail", "measured"))


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", CFGS)
def test_replan_between_two_ticks(wca, qs, plan_run, cfg):
    """(5) replan_footsteps between ticks REPLAN_K - 1 and REPLAN_K, at merge stages inside a double support for five robots and -1 for the
    others: the run within 1e-9 of the restatement on the stitched plan; the robots with -1 are bit for bit the run without the replan; a
    replan with M_i = t after tick t was staged is INVALID and leaves the run unchanged."""
    fs = rs.scenario(wca)[0]
    rp, plan1, ref = rs.replanned(wca, qs, cfg)
    assert (ref["ik_fail"] == 0).all() and (ref["mpc_fail"] == 0).all()
    keep = np.nonzero(rs.REPLAN_M < 0)[0]
    ext, ext0 = stt.external_of(ref), stt.external_of(rs.internal(wca, qs, cfg))
    for k in ext:                                            # (the oracle runs robot by robot: a robot that keeps its plan keeps its states)
        assert np.array_equal(ext[k][:, keep], ext0[k][:, keep]), k
    pipe = _pipe(wca, cfg)
    pipe.upload_footsteps(fs, fs)
    _walk(pipe, ext, rs.REPLAN_K)
    pipe.replan_footsteps(rs.REPLAN_M, rp, rp["first_ds_ticks"])
    _walk(pipe, ext, rs.REFUSED_T, t0=rs.REPLAN_K)
    t = rs.REFUSED_T
    late = np.full(B, -1, np.int32)
    late[rs.REFUSED_ROBOT] = t
    assert (int(plan1["contact"][rs.REFUSED_ROBOT, t]) & 3) == 3
    one = dict(n_steps=np.where(late >= 0, 1, 0).astype(np.int32), side=np.zeros((B, 1), np.uint8), target=np.full((B, 1, 3), 1e3), first_ds_ticks=5)
    one["target"][rs.REFUSED_ROBOT, 0] = (plan1["left_traj"][rs.REFUSED_ROBOT, t, 0] + 0.01, plan1["left_traj"][rs.REFUSED_ROBOT, t, 1], 0.0)
    pipe.set_desired_from_plan()
    with pytest.raises(wca.WcqpError, match=r"\(-1\)"):
        pipe.replan_footsteps(late, one, 5)                  # stage t is in hand: M = t is one too early
    _feed(pipe, ext, t)
    pipe.run(1)
    _walk(pipe, ext, t0=t + 1)
    out = pipe.download()
    _close(out, ref)
    assert out["feedback_fail"].sum() == 0
    base = plan_run(cfg)[1]
    for k in rs.KEYS:
        ax = 1 if k.endswith("_log") else 0
        assert np.array_equal(np.take(out[k], keep, axis=ax), np.take(base[k], keep, axis=ax)), k
        moved = np.setdiff1d(np.arange(B), keep)
        assert not np.array_equal(np.take(out[k], moved, axis=ax), np.take(base[k], moved, axis=ax)), k
    w = pipe.plan_window()
    assert np.array_equal(w["contact"], plan1["contact"])
    for k in ("left_traj", "right_traj", "ref_traj"):
        assert np.abs(w[k] - plan1[k]).max() <= 1e-9, k


@pytest.mark.gpu
def test_nothing_else_moved(wca, qs, plan_run, handover_run):
    """(6) a resident-plan handle fed only through set_desired_host on every tick is bit for bit a plain streamed handle; and
    set_desired_from_plan followed by set_desired_host with OTHER stages (the CoM 5 mm lower) runs the latter."""
    cfg = "mpc"
    fs = rs.scenario(wca)[0]
    w = plan_run(cfg)[2]
    stages = _window_stages(w)
    ext = stt.external_of(rs.internal(wca, qs, cfg))
    a = _pipe(wca, cfg)
    a.upload_footsteps(fs, fs)
    _handed_over(a, stages, ext)
    _same(a.download(), handover_run(cfg))
    other = dict(stages, com_height=stages["com_height"] - 0.005)
    b = _pipe(wca, cfg)
    b.upload_footsteps(fs, fs)
    _handed_over(b, other, ext, before=True)
    c = _pipe(wca, cfg, resident=False)
    _upload_streamed(c, fs, w)
    _handed_over(c, other, ext)
    ob = b.download()
    _same(ob, c.download())
    assert np.abs(ob["dq_log"] - plan_run(cfg)[1]["dq_log"]).max() > 1e-6


@pytest.mark.gpu
def test_forms(wca, qs, plan_run):
    """(7) everything of a tick on a non-blocking stream, one robot against thirteen, and the classic upload of the first handle's whole
    plan_window() into a resident-plan handle: each bit for bit the walk of plan_run; upload_goal on such a handle yields the restated plan
    of the restated footsteps to 1e-9."""
    cfg = "mpc"
    fs = rs.scenario(wca)[0]
    _, base, w = plan_run(cfg)
    ext = stt.external_of(rs.internal(wca, qs, cfg))
    # a non-blocking stream: the staging kernel and the tick in its order; the host form of the feedback is taken once the stream has drained
    s = wca.capi.stream_create()
    try:
        a = _pipe(wca, cfg)
        a.upload_footsteps(fs, fs)
        for t in range(MAXT):
            a.set_desired_from_plan(stream=s)
            wca.capi.stream_synchronize(s)
            _feed(a, ext, t)
            a.run(1, stream=s)
        _same(a.download(), base)
    finally:
        wca.capi.stream_synchronize(s)
        wca.capi.stream_destroy(s)
    # one robot (a wave with three dead slots and nothing else)
    sub = {k: (v[:1] if isinstance(v, np.ndarray) and v.shape[:1] == (B,) else v) for k, v in fs.items()}
    one = _pipe(wca, cfg, batch=1)
    one.upload_footsteps(sub, sub)
    _walk(one, ext, rows=slice(0, 1))
    o1 = one.download()
    assert fs["n_steps"][0] > 0
    for k in rs.KEYS:
        assert np.array_equal(o1[k], base[k][:, :1] if k.endswith("_log") else base[k][:1]), k
    # the classic upload with the planned arrays
    c = _pipe(wca, cfg)
    c.upload(dict(state0=fs["state0"], q0=fs["q0"], com0=fs["com0"], ref_traj=w["ref_traj"], dcm0=w["ref_traj"][:, 0].copy(), u_init=w["u_init"]),
             com_height_traj=w["com_height"], com_height_vel=w["com_height_vel"], **{k: w[k] for k in WINDOW})
    assert not c.info()["plan_generated"]
    wc = c.plan_window()
    for k in wc:
        assert np.array_equal(wc[k], w[k]), k
    _walk(c, ext)
    _same(c.download(), base)
    # upload_goal
    params = dict(step_ticks=rs.SS + rs.DS, max_steps=rs.K, nominal_width=0.118, min_width=0.10, max_linear_velocity=0.03, max_angular_velocity=0.15,
                  min_step_length=0.005, min_angle_variation=0.01)
    rng = np.random.default_rng(3)
    goals = np.stack([rng.uniform(0.02, 0.05, B), rng.uniform(-0.03, 0.03, B)], 1)
    st = fs["state0"]
    r = up.unicycle_plan(dict(wca.UnicyclePlanner.DEFAULTS, **params), st[:, 24:36], st[:, 36:48], goals, 1)
    sure = np.nonzero(r["margin"] >= 1e-9)[0]                # (a robot decided by less may be decided otherwise on the device)
    assert len(sure) >= B - 1 and (r["n_steps"][sure] > 0).any()
    g = _pipe(wca, cfg)
    got = g.upload_goal(fs, goals, wca.UnicyclePlanner(**params), 1, rs.FIRST_DS, rs.SS, rs.DS, final_ds_ticks=rs.FINAL_DS, lift=fs["lift"],
                        zmp_delta_left=fs["zmp_delta_left"], zmp_delta_right=fs["zmp_delta_right"])
    assert np.array_equal(got["n_steps"][sure], r["n_steps"][sure]) and np.array_equal(got["side"][sure], r["side"][sure])
    gfs = dict(fs, n_steps=r["n_steps"], side=r["side"], target=r["target"])
    gplan = fp.footstep_plan(gfs, st, rs.T, MAXT)
    wg = g.plan_window()
    assert np.array_equal(wg["contact"][sure], gplan["contact"][sure])
    for k in ("left_traj", "right_traj", "left_twist", "right_twist", "ref_traj"):
        err = np.abs(wg[k][sure] - gplan[k][sure]).max()
        print(k, err)
        assert err <= 1e-9, (k, err)
    g.set_desired_from_plan()


@pytest.mark.gpu
def test_refusals_and_order(wca, qs, plan_run):
    """(8) set_desired_from_plan before an upload and once t has reached max_ticks is INVALID, on a handle without resident_plan UNSUPPORTED;
    run(1) without a stage and sensor feedback before the stage are INVALID; upload_footsteps, replan_footsteps and get_plan on a streamed
    handle without resident_plan stay UNSUPPORTED; wcqp_tick_upload of a resident-plan handle without the planned arrays is INVALID."""
    cfg = "mpc"
    lib = wca.capi.lib()
    fs = rs.scenario(wca)[0]
    done, _, w = plan_run(cfg)
    assert lib.wcqp_tick_set_desired_from_plan(done._h, None) == WCQP_E_INVALID          # every tick of the handle has run
    ext = stt.external_of(rs.internal(wca, qs, cfg))
    pipe = _pipe(wca, cfg)
    assert lib.wcqp_tick_set_desired_from_plan(pipe._h, None) == WCQP_E_INVALID          # before an upload
    with pytest.raises(ValueError, match="left_traj"):
        _upload_streamed(pipe, fs, w)                                                       # no planned arrays: the binding ...
    keep = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in dict(ref_traj=w["ref_traj"], state0=fs["state0"], q0=fs["q0"], com0=fs["com0"],
                                                                          dcm0=w["ref_traj"][:, 0], u_init=w["u_init"]).items()}
    ins = wca.capi.TickInputs(**{k: v.ctypes.data for k, v in keep.items()})
    assert lib.wcqp_tick_upload(pipe._h, C.byref(ins)) == WCQP_E_INVALID                    # ... and the library
    assert lib.wcqp_tick_set_desired_from_plan(pipe._h, None) == WCQP_E_INVALID
    pipe.upload_footsteps(fs, fs)
    _feed(pipe, ext, 0)
    with pytest.raises(wca.WcqpError, match=r"\(-1\)"):
        pipe.run(1)                                                                         # feedback, but no stage
    z23 = np.zeros((B, 23)); wr = np.zeros((B, 6)); wr[:, 2] = 150.0
    pipe.upload_footsteps(fs, fs)
    with pytest.raises(wca.WcqpError, match=r"\(-1\)"):
        pipe.set_sensor_feedback_host(fs["q0"], z23, wr, wr)                                # the anchor's stage is not there yet
    pipe.set_desired_from_plan()
    with pytest.raises(wca.WcqpError, match=r"\(-1\)"):
        pipe.run(1)                                                                         # a stage, but no feedback
    pipe.set_desired_from_plan()                                                            # restaged
    _feed(pipe, ext, 0)
    pipe.run(1)
    assert pipe.download()["tick"] == 1
    plain = _pipe(wca, cfg, resident=False)
    assert not plain.info()["resident_plan"]
    for ext in (None, C.byref(wca.capi.TickParamsExt(1))):                                  # wcqp_tick_create is wcqp_tick_create_ext(p, NULL)
        raw, x = C.c_void_p(), wca.capi.TickInfoExt(7)
        rc = lib.wcqp_tick_create(C.byref(plain.params), C.byref(raw)) if ext is None else lib.wcqp_tick_create_ext(C.byref(plain.params), ext, C.byref(raw))
        assert rc == 0 and lib.wcqp_tick_get_info_ext(raw, C.byref(x)) == 0 and x.resident_plan == (0 if ext is None else 1)
        assert lib.wcqp_tick_destroy(raw) == 0
    assert lib.wcqp_tick_set_desired_from_plan(plain._h, None) == WCQP_E_UNSUPPORTED
    ins, st = wca.capi.TickInputs(), wca.capi.TickFootsteps()
    assert lib.wcqp_tick_upload_footsteps(plain._h, C.byref(ins), C.byref(st)) == WCQP_E_UNSUPPORTED
    assert lib.wcqp_tick_get_plan(plain._h, 0, 1, 0, 1, C.byref(wca.capi.TickPlanWindow())) == WCQP_E_UNSUPPORTED
    assert lib.wcqp_tick_replan_footsteps(plain._h, C.byref(wca.capi.TickReplan()), None) == WCQP_E_UNSUPPORTED
    with pytest.raises(ValueError, match="resident_plan"):
        plain.upload_footsteps(fs, fs)
