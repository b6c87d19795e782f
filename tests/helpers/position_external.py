"""The POSITION tick on a streamed handle of the EXTERNAL plant (WCQP_TICK_OPT_POSITION_STREAMED) restated, on the scenario of
helpers/position_tick.py as it stands (13 robots, 70 ticks, the MPC at N = 50 and the reactive law with gain scheduling).

The restatement of one robot: oracle.tick_spec.run_ticks(..., external=ext) on the plan's stages gives the chain on the measured state -
u0_log, and the com_log / zmp_log / zmp_gains the ZMP-CoM law read - the ten lines of LIPM reference and ZMP-CoM law of position_tick.chain
are repeated on those logs for p_star, and position_tick.walk runs the non-linear IK tick by tick.  Everything here is computed once per
process and handed out unchanged.

The feeds (all [T][B13][..], fixed and seeded):
  own        the internal-plant logs of run_ticks over all 13 robots: what a robot that follows the LIPM exactly reports
  disturbed  helpers/resident_plan.disturbed's recipe on them: a 1.5e-3 sinusoid on the DCM, 2e-4 / 1e-3 normal noise on the CoM and the ZMP
  recording  encoders, joint velocities and foot wrenches for the sensor form (sensor_recording), SENSOR_T ticks

Run as a script (tests/test_tick_position_external.py::test_forms does, in a process of its own: torch brings its own HIP runtime and has
to initialise before libwcqp's does) it checks the DEVICE form of the feedback against the host form and prints "position external device
ok"."""
import functools
import os
import sys

import numpy as np

if __name__ == "__main__":
    _ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path[:0] = [_ROOT, os.path.join(_ROOT, "tests")]
    import torch  # noqa: F401  (the GPU runtime first, then libwcqp)

import robots
from helpers import position_tick as pk
from helpers import streamed_tick as stt
from helpers import zmp_gains as zg
from oracle import sensor_spec as sn
from oracle import tick_spec as ts

B13, T, N, H, SEL = pk.B13, pk.T, pk.N, pk.H, pk.SEL
OPT_RESIDENT_PLAN, OPT_POSITION_STREAMED = 1, 2
# The scenario's steps (15 + 10 stages) are too fast for the robot's joint velocity limits: the VELOCITY IK of run_ticks stops every robot
# at tick 11 or 12 with them, and with four times the limits it walks all 70 ticks.  The streamed velocity handle the rejection test compares
# failure counts with gets ten times the limits, so that its ik_fail counts rejections and nothing else.
VELOCITY_VMAX_SCALE = 10.0


def _tick_params():
    R = robots.ROBOTS[pk.ROBOT]
    return ts.TickParams(horizon=N, com_height=H, k_com=R["k_com"], k_zmp=R["k_zmp"])


def _controller(controller):
    return {} if controller == "mpc" else dict(dcm_controller="reactive", k_dcm=pk.K_DCM, zmp_gain_schedule=zg.ZMP_SCHEDULE[pk.ROBOT])


def _ik_params(vmax_scale=1.0):
    from oracle import qp_spec as qs
    sc = pk.scenario()
    ipar = robots.ik_params(qs, pk.ROBOT, v_max=sc["v_max"] * vmax_scale)
    ipar.joint_reg_deg = sc["posture_deg"]
    return ipar


def data_of(plan, rows=slice(None)):
    """what run_ticks takes of the scenario's footsteps and a restated plan (rows: these robots)"""
    fs = pk.scenario()["fs"]
    cut = lambda v: v[rows] if isinstance(v, np.ndarray) and v.shape[:1] == (B13,) else v
    d = {k: cut(v) for k, v in fs.items()}
    ref = plan["ref_traj"][rows]
    return dict(d, ref_traj=ref, dcm_vel_traj=plan["dcm_vel_traj"][rows], dcm0=ref[:, 0].copy(), u_init=plan["zmp_ref"][rows][:, 0].copy())


def run(controller, plan=None, rows=slice(None), external=None, n_ticks=T, vmax_scale=1.0):
    """run_ticks on the stages of `plan` (default: the scenario's) for the robots `rows`"""
    sc = pk.scenario()
    plan = sc["plan"] if plan is None else plan
    p1 = {k: v[rows] for k, v in plan.items() if isinstance(v, np.ndarray) and v.shape[:1] == (B13,)}
    first = 0 if rows == slice(None) else rows.start
    return ts.run_ticks(_tick_params(), dict(data_of(plan, rows), first=first), n_ticks, _ik_params(vmax_scale), kin_model=sc["model"],
                        foot_rect=sc["foot_rect"], stages=stt.stages_of(p1, n_ticks), neck_additional_rotation=pk.ADD_ROT, dcm_vel=p1["dcm_vel_traj"],
                        external=external, **_controller(controller))


@functools.lru_cache(maxsize=None)
def own(controller):
    """the internal-plant run of all 13 robots and its logs as a feed: (external, run)"""
    r = run(controller)
    return stt.external_of(r), r


@functools.lru_cache(maxsize=None)
def disturbed(controller):
    """helpers/resident_plan.disturbed's recipe on this scenario's own logs (the joints ride along: the handle validates them, the IK does
    not read them)"""
    inner = own(controller)[1]
    rng = np.random.default_rng(17)
    tt = np.arange(T)[:, None, None]
    return dict(dcm=inner["dcm_log"] + 1.5e-3 * np.sin(0.05 * tt + rng.uniform(0, 6, size=(1, B13, 2))),
                com=inner["com_log"] + 2e-4 * rng.normal(size=(T, B13, 2)),
                zmp=inner["zmp_log"] + 1e-3 * rng.normal(size=(T, B13, 2)),
                q=inner["q_log"] + 0.004 * rng.normal(size=(T, B13, 23)))


def one(ext, i):
    """robot i's slice of a feed"""
    return {k: np.ascontiguousarray(v[:, i:i + 1]) for k, v in ext.items() if v is not None}


def p_star_of(r, d, n_ticks):
    """The LIPM reference and the ZMP-CoM law of position_tick.chain again, on what run_ticks `r` logged over the data `d`: p_star
    [n_ticks][B][2] (elementwise over the robots: the numbers position_tick.chain forms for one)"""
    tp = _tick_params()
    omega = np.sqrt(tp.gravity / tp.com_height)
    ref = d["ref_traj"]
    c_ref = d["com0"].copy(); v_ref_prev = np.zeros_like(c_ref)
    p_star = d["com0"].copy(); v_star_prev = np.zeros_like(c_ref)
    out = np.zeros((n_ticks,) + c_ref.shape)
    for t in range(n_ticks):
        v_ref = -omega * (c_ref - ref[:, t])
        c_ref = c_ref + 0.5 * tp.dT * (v_ref + v_ref_prev); v_ref_prev = v_ref
        g = r["zmp_gains"][t]
        v_star = g[:, 0:1] * (c_ref - r["com_log"][t]) - g[:, 1:2] * (r["u0_log"][t] - r["zmp_log"][t]) + v_ref
        p_star = p_star + 0.5 * tp.dT * (v_star + v_star_prev); v_star_prev = v_star
        out[t] = p_star
    return out


def _plan_row(plan, i):
    return {k: v[i:i + 1] for k, v in plan.items() if isinstance(v, np.ndarray) and v.shape[:1] == (B13,)}


def restate(controller, i, ext, plan=None, n_ticks=T):
    """The restatement of robot i fed `ext` ([>= n_ticks][B13][..]): run_ticks with external feedback on the plan's stages, p_star_of its
    logs, then position_tick.walk.  -> dict(run=, chain=dict(u0_log, p_star, plan, mpc_fail, measured [n_ticks][6]), walk=)"""
    sc = pk.scenario()
    plan = sc["plan"] if plan is None else plan
    rows = slice(i, i + 1)
    r = run(controller, plan, rows, external=one(ext, i), n_ticks=n_ticks)
    ch = dict(u0_log=r["u0_log"][:, 0], p_star=p_star_of(r, data_of(plan, rows), n_ticks)[:, 0], plan=_plan_row(plan, i), mpc_fail=int(r["mpc_fail"][0]),
              measured=np.concatenate([r["dcm_log"][:, 0], r["com_log"][:, 0], r["zmp_log"][:, 0]], 1))
    return dict(run=r, chain=ch, walk=pk.walk(ch, sc["fs"]["q0"][i], pk.params(), n_ticks=n_ticks))


@functools.lru_cache(maxsize=None)
def reference(controller, feed):
    """the restatement of the robots SEL under a feed: "own" | "disturbed" over T ticks, "sensor" (the recording, the MPC) over SENSOR_T
    -> {robot: restate(...)}"""
    if feed == "sensor":
        return {i: restate(controller, i, sensor_recording()["external"], n_ticks=SENSOR_T) for i in SEL}
    ext = own(controller)[0] if feed == "own" else disturbed(controller)
    return {i: restate(controller, i, ext) for i in SEL}


SENSOR_T = 45        # the sensor form's ticks: past the switch of the fixed-frame foot at tick 35, by when the right foot has taken its step


@functools.lru_cache(maxsize=None)
def commanded():
    """what the POSITION tick commands every one of the 13 robots over SENSOR_T ticks under the own feed, MPC controller: [SENSOR_T][B13][23]
    (the robots SEL: reference("mpc", "own"); the other ten walk here, on the own run's p_star)"""
    sc = pk.scenario()
    ps = p_star_of(own("mpc")[1], data_of(sc["plan"]), SENSOR_T)
    out = np.zeros((SENSOR_T, B13, 23))
    for i in range(B13):
        if i in SEL:
            out[:, i] = reference("mpc", "own")[i]["walk"]["q_log"][:SENSOR_T]
        else:
            w = pk.walk(dict(p_star=ps[:, i], plan=_plan_row(sc["plan"], i)), sc["fs"]["q0"][i], pk.params(), n_ticks=SENSOR_T)
            assert w["ik_fail"] == 0, i
            out[:, i] = w["q_log"]
    return out


@functools.lru_cache(maxsize=None)
def sensor_recording():
    """The sensor form's recording over SENSOR_T ticks, MPC controller, built beforehand: what a robot that tracks its POSITION commands
    reports, plus seeded noise - q_meas[t] = the joints tick t - 1 commanded under the own feed (commanded(); tick 0: q0) + 1e-3 noise,
    dq_meas = 2e-3 noise, and the wrenches of helpers/resident_plan.sensor_case: the feet in contact loaded, each loaded foot's ZMP where
    the previous command is (own("mpc")'s u0_log).
    -> dict(readings=[(q, dq, wl, wr)] per tick, external= the measured state oracle.sensor_spec.sensor_measured evaluates from them)"""
    sc = pk.scenario()
    n = SENSOR_T
    stages = stt.stages_of(sc["plan"], n)
    q_prev = np.concatenate([sc["fs"]["q0"][None], commanded()[:-1]])
    rng = np.random.default_rng(23)
    qn, dqn = 1e-3 * rng.normal(size=(n, B13, 23)), 2e-3 * rng.normal(size=(n, B13, 23))
    wn = rng.normal(size=(n, 2, B13, 6)) * np.array([5.0, 5.0, 2.0, 0.05, 0.05, 0.5])
    u_prev = np.concatenate([data_of(sc["plan"])["u_init"][None], own("mpc")[1]["u0_log"][:n - 1]])
    omega = np.sqrt(_tick_params().gravity / H)
    readings, meas = [], np.zeros((n, B13, 6))
    for t in range(n):
        code = (stages["contact"][t].astype(int) & 3) - 1
        w = []
        for f, pose in enumerate((stages["left_pose"][t], stages["right_pose"][t])):
            loaded = code != 1 - f
            fz = np.where(loaded, np.where(code == 2, 150.0, 300.0) + wn[t, f, :, 2], 0.0)
            R = pose[:, 3:].reshape(B13, 3, 3)
            z = np.einsum("bji,bj->bi", R, np.concatenate([u_prev[t], np.zeros((B13, 1))], 1) - pose[:, :3])      # the command in the sole frame
            wf = wn[t, f].copy()
            wf[:, 2] = fz; wf[:, 3] += z[:, 1] * fz; wf[:, 4] += -z[:, 0] * fz
            w.append(wf)
        r = (q_prev[t] + qn[t], dqn[t], w[0], w[1])
        m, rej = sn.sensor_measured(sc["model"], stages, t, *r, omega)
        assert not rej.any(), ("a rejected reading", t)
        readings.append(r); meas[t] = m
    return dict(readings=readings, external=dict(dcm=meas[:, :, 0:2], com=meas[:, :, 2:4], zmp=meas[:, :, 4:6], q=np.stack([r[0] for r in readings])))


# ---------------------------------------------------------------------------------------------------------------- handles

def ik_solver(wca, vmax_scale=1.0):
    R = robots.ROBOTS[pk.ROBOT]
    return wca.IkSolver(form=wca.IK_FORM_QPOASES, neck_weight=R["neck_weight"] * np.eye(3), joint_reg_weights=np.array(R["reg_w"], float),
                        joint_reg_gains=np.array(R["reg_k"], float), joint_reg_rad=np.deg2rad(wca.synth.WALK_POSTURE_DEG),
                        v_max=wca.synth.WALK_VMAX * vmax_scale, k_pos_com=R["k_pos_com"], k_pos_foot=R["k_pos_foot"], k_att_foot=R["k_att_foot"],
                        k_neck=R["k_neck"])


def pipe(wca, controller, B=B13, resident=False, position=True, max_iter=30):
    """a streamed handle of the EXTERNAL plant on the scenario: the POSITION tick, or (position=False) the velocity tick with the wide
    velocity limits of VELOCITY_VMAX_SCALE"""
    R = robots.ROBOTS[pk.ROBOT]
    mode = dict(ik_mode="position", position_ik=dict(q_reg=pk.scenario()["q_reg"], max_iter=max_iter)) if position else {}
    return wca.TickPipeline(B, T, wca.MpcSolver(horizon=N, com_height=H), ik_solver(wca, 1.0 if position else VELOCITY_VMAX_SCALE), log_ticks=T,
                            k_com=R["k_com"], k_zmp=R["k_zmp"], kin=wca.KinModel(pk.scenario()["model"]), external_feedback=True,
                            streamed_trajectories=True, resident_plan=resident, neck_additional_rotation=pk.ADD_ROT, **pk.controller_kwargs(controller),
                            **mode)


def upload_streamed(p, plan, rows=slice(None)):
    """wcqp_tick_upload of a streamed handle without a plan: the DCM reference, its velocity and the initial state of a restated plan or of
    a plan_window() (whose generated ZMP of stage 0 is u_init)"""
    fs = pk.scenario()["fs"]
    u_init = plan["u_init"] if "u_init" in plan else plan["zmp_ref"][:, 0]
    vel = plan.get("dcm_vel_traj")               # (a window of an MPC handle without scheduling has none, and such a handle reads none)
    p.upload(dict(state0=fs["state0"][rows], q0=fs["q0"][rows], com0=fs["com0"][rows], ref_traj=plan["ref_traj"][rows],
                  dcm0=plan["ref_traj"][rows][:, 0].copy(), u_init=np.ascontiguousarray(u_init[rows])), dcm_vel_traj=None if vel is None else vel[rows])


def window_stages(w):
    """the stages of a plan_window()"""
    return stt.stages_of(dict(w, com_height_traj=w["com_height"]), T)


def stage(stages, t, rows=slice(None)):
    return tuple(np.ascontiguousarray(stages[k][t][rows]) for k in ("left_pose", "right_pose", "left_twist", "right_twist", "contact", "com_height",
                                                                   "com_height_vel"))


def feed(p, ext, t, rows=slice(None)):
    p.set_feedback_host(ext["dcm"][t][rows], ext["com"][t][rows], ext["zmp"][t][rows], ext["q"][t][rows] if ext.get("q") is not None else None)


def handed_over(p, stages, ext, t1=T, t0=0, rows=slice(None)):
    """ticks t0 .. t1 - 1 of the per-tick order: the stage through set_desired_host, the plain feedback of `ext`, one tick"""
    for t in range(t0, t1):
        p.set_desired_host(*stage(stages, t, rows))
        feed(p, ext, t, rows)
        p.run(1)


def from_plan(p, ext, t1=T, t0=0):
    """the same with the stage out of the handle's resident plan"""
    for t in range(t0, t1):
        p.set_desired_from_plan()
        feed(p, ext, t)
        p.run(1)


# ---------------------------------------------------------------------------------------------------------------- the device form, as a script

DEVICE_T = 20        # past the first change of contact pair (tick 10)


def _device_form_main():
    """The reactive handle with gain scheduling over DEVICE_T ticks of the own feed: stages and plain feedback from torch tensors on a
    non-blocking torch stream, with the runs on that stream, against the host forms on the NULL stream - every downloaded array bit for bit."""
    import torch
    import walking_controllers_amd as wca
    c = "reactive_gs"
    dev = torch.device("cuda", 0)
    plan = pk.scenario()["plan"]
    stages = stt.stages_of(plan, DEVICE_T)
    ext = dict(own(c)[0], q=own(c)[1]["q_log"])
    stream = torch.cuda.Stream()          # non-blocking

    def loop(form):
        p = pipe(wca, c)
        upload_streamed(p, plan)
        for t in range(DEVICE_T):
            if form == "host":
                p.set_desired_host(*stage(stages, t))
                feed(p, ext, t)
                p.run(1)
                continue
            with torch.cuda.stream(stream):
                x = [torch.from_numpy(a).to(dev) for a in stage(stages, t)]
                f = [torch.from_numpy(np.ascontiguousarray(ext[k][t])).to(dev) for k in ("dcm", "com", "zmp", "q")]
                stream.synchronize()
                p.set_desired_device(*x, stream=stream.cuda_stream)
                p.set_feedback_device(*(y.data_ptr() for y in f), stream=stream.cuda_stream)
                p.run(1, stream=stream.cuda_stream)
                stream.synchronize()
        return p.download()
    host, device = loop("host"), loop("device")
    assert host["tick"] == DEVICE_T and not host["ik_fail"].any() and not host["feedback_fail"].any()
    assert np.abs(host["q_log"][DEVICE_T - 1] - host["q_log"][0]).max() > 1e-4
    for k in host:
        assert np.array_equal(device[k], host[k]), k
    print("position external device ok")


if __name__ == "__main__":
    _device_form_main()
