"""The scenario of tests/test_tick_resident_plan.py (wcqp_tick_params_ext.resident_plan): 13 robots - three full waves of the
staging kernel and one with three dead slots - on a generated walk of short steps, its restatement (helpers/footstep_plan.py) and the runs
of oracle/tick_spec.py over it, each computed once per process and handed out unchanged."""
import functools

import numpy as np

import robots
from helpers import footstep_plan as fp
from helpers import footstep_replan as fr
from helpers import planned_tick as pt
from helpers import streamed_tick as stt
from helpers import zmp_gains as zg
from oracle import sensor_spec as sn

ROBOT = "iCubGazeboV2_5"
K_DCM = 1.0
# A first double support of 30 stages, steps of 40 + 60.  Shorter ones make the restatement fail, so they were lengthened: with 15 + 10 the
# IK fails on tick 21 of every walking robot (the swing is too fast for the joint velocity limits), and with 30 + 20 up to 30 + 80 the MPC,
# tuned for slow steps, lets the DCM fall behind the reference and the IK fails late in the second swing.  Single supports [30, 70) and
# [130, 170): the plan of a robot of two steps ends at stage 170 + FINAL_DS < MAXT, the third step of the others starts past MAXT
B, MAXT, FIRST_DS, SS, DS, K, FINAL_DS = 13, 190, 30, 40, 60, 4, 15
T = MAXT + 51
STEP, YAW = (0.01, 0.02), (0.02, 0.05)         # how far a swinging foot advances [m] and turns [rad] per step
# robot 0 walks (the one-robot handle of the forms test holds it); 1 and 7 stand; nobody takes one step only (a walking robot changes its pair >= 3 times)
N_STEPS = np.array([4, 0, 4, 2, 3, 3, 4, 0, 2, 4, 3, 2, 4], np.int32)
CONFIGS = {"mpc": ("mpc", False), "reactive_gs": ("reactive", True)}       # the MPC at N = 50; the reactive law with gain scheduling
KEYS = ("u0_log", "dq_log", "q_des")


@functools.lru_cache(maxsize=None)
def _scenario(wca):
    kb = wca.synth.synth_walk_kin_batch(B)
    fs = wca.synth.synth_footstep_walk_batch(B, MAXT, pt.poses_host(wca.synth.icub_like_model(), kb), kb)
    rng = np.random.default_rng(31)
    side = np.tile(np.array([1, 0, 1, 0], np.uint8), (B, 1))
    side[9] = (0, 1, 1, 0); side[5] = (0, 1, 0, 1)          # the left foot first
    target = np.full((B, K, 3), 1e3)                          # (steps a robot does not take are not read)
    st = fs["state0"]
    for i in range(B):
        p = [st[i, 24:26].copy(), st[i, 36:38].copy()]
        yaw = [np.arctan2(st[i, 33], st[i, 27]), np.arctan2(st[i, 45], st[i, 39])]
        turn = 1.0 if i % 3 else -1.0                         # robots turn one way or the other, robot 4 walks straight
        for k in range(int(N_STEPS[i])):
            sw = side[i, k]
            inc = 0.0 if i == 4 else rng.uniform(*YAW) * turn
            yaw[sw] += inc
            p[sw] = p[sw] + rng.uniform(*STEP) * np.array([np.cos(yaw[sw]), np.sin(yaw[sw])])
            target[i, k] = (p[sw][0], p[sw][1], inc)
    fs.update(n_steps=N_STEPS.copy(), side=side, target=target, first_ds_ticks=FIRST_DS, ss_ticks=SS, ds_ticks=DS, final_ds_ticks=FINAL_DS, lift=0.02)
    plan = fp.footstep_plan(fs, fs["state0"], T, MAXT)
    return fs, plan


def scenario(wca):
    """(footsteps, the restated plan, its stages [MAXT][B][..])"""
    fs, plan = _scenario(wca)
    return fs, plan, stt.stages_of(plan, MAXT)


def data_of(fs, plan):
    """what run_ticks takes of a restated plan"""
    return dict(fs, ref_traj=plan["ref_traj"], dcm_vel_traj=plan["dcm_vel_traj"], dcm0=plan["ref_traj"][:, 0].copy(), u_init=plan["zmp_ref"][:, 0].copy())


def ik_params(wca, qs):
    ipar = robots.ik_params(qs, ROBOT, v_max=wca.synth.WALK_VMAX.copy())
    ipar.joint_reg_deg = wca.synth.WALK_POSTURE_DEG.copy()
    return ipar


def restate(wca, qs, cfg, plan, n_ticks=MAXT, rows=None, **kw):
    """run_ticks on a restated plan's stages with the scenario's robot (rows: only these robots)"""
    from oracle import tick_spec as ts
    controller, gs = CONFIGS[cfg]
    R = robots.ROBOTS[ROBOT]
    fs = _scenario(wca)[0]
    d = data_of(fs, plan)
    stages = stt.stages_of(plan, n_ticks)
    vel = plan["dcm_vel_traj"]
    if rows is not None:
        d = {k: (v[rows] if isinstance(v, np.ndarray) and v.shape[:1] == (B,) else v) for k, v in d.items()}
        stages = {k: np.ascontiguousarray(v[:, rows]) for k, v in stages.items()}
        vel = vel[rows]
    return ts.run_ticks(ts.TickParams(horizon=50, k_com=R["k_com"], k_zmp=R["k_zmp"]), d, n_ticks, ik_params(wca, qs), kin_model=wca.synth.icub_like_model(),
                        foot_rect=wca.synth.FOOT_RECT, stages=stages, neck_additional_rotation=R["additional_rotation"], dcm_controller=controller,
                        k_dcm=K_DCM, dcm_vel=vel, zmp_gain_schedule=zg.ZMP_SCHEDULE[ROBOT] if gs else None, **kw)


@functools.lru_cache(maxsize=None)
def internal(wca, qs, cfg):
    """the restatement with the internal plant: what the handles are fed, and what they are compared against"""
    return restate(wca, qs, cfg, _scenario(wca)[1])


@functools.lru_cache(maxsize=None)
def disturbed(wca, qs, cfg):
    """test_tick_streamed.py's _disturbed on this scenario: an offset DCM, a ZMP that is not the previous command, measured joints off the
    desired ones - fixed arrays, seeded - and the restatement fed them: (external, run)"""
    inner = internal(wca, qs, cfg)
    rng = np.random.default_rng(17)
    tt = np.arange(MAXT)[:, None, None]
    ext = dict(dcm=inner["dcm_log"] + 1.5e-3 * np.sin(0.05 * tt + rng.uniform(0, 6, size=(1, B, 2))),
               com=inner["com_log"] + 2e-4 * rng.normal(size=(MAXT, B, 2)),
               zmp=inner["zmp_log"] + 1e-3 * rng.normal(size=(MAXT, B, 2)),
               q=inner["q_log"] + 0.004 * rng.normal(size=(MAXT, B, 23)))
    return ext, restate(wca, qs, cfg, _scenario(wca)[1], external=ext)


SENSOR_T = FIRST_DS + (SS + DS) + 3        # past the switch of the fixed-frame foot at the second step: the first foot has moved by then


@functools.lru_cache(maxsize=None)
def sensor_case(wca, qs):
    """test_tick_streamed.py's robot-in-the-loop recording on this scenario, SENSOR_T ticks: readings a robot that tracks its commands
    reports plus seeded noise - the run's own desired joints and previous velocities, wrenches that load the feet in contact and put each
    loaded foot's ZMP where the previous command is.  -> (the ticks within two of a switch of any robot's fixed-frame foot, the restated run)"""
    stages = scenario(wca)[2]
    side = sn.stage_side(stages["contact"])
    sw = [t for t in range(1, SENSOR_T) if (side[t] != side[t - 1]).any()]
    check = sorted({u for t in sw for u in range(t - 2, t + 3) if 0 <= u < SENSOR_T})
    rng = np.random.default_rng(23)
    qn, dqn = 1e-3 * rng.normal(size=(SENSOR_T, B, 23)), 2e-3 * rng.normal(size=(SENSOR_T, B, 23))
    wn = rng.normal(size=(SENSOR_T, 2, B, 6)) * np.array([5.0, 5.0, 2.0, 0.05, 0.05, 0.5])

    def sensors(t, q_des, dq_prev, u_prev):
        code = (stages["contact"][t].astype(int) & 3) - 1
        w = []
        for f, pose in enumerate((stages["left_pose"][t], stages["right_pose"][t])):
            loaded = code != 1 - f
            fz = np.where(loaded, np.where(code == 2, 150.0, 300.0) + wn[t, f, :, 2], 0.0)
            R = pose[:, 3:].reshape(B, 3, 3)
            z = np.einsum("bji,bj->bi", R, np.concatenate([u_prev, np.zeros((B, 1))], 1) - pose[:, :3])      # the command in the sole frame
            wf = wn[t, f].copy()
            wf[:, 2] = fz; wf[:, 3] += z[:, 1] * fz; wf[:, 4] += -z[:, 0] * fz
            w.append(wf)
        return q_des + qn[t], dq_prev + dqn[t], w[0], w[1]
    return check, restate(wca, qs, "mpc", _scenario(wca)[1], n_ticks=SENSOR_T, sensors=sensors)


# The replan of the GPU test, enqueued between ticks REPLAN_K - 1 and REPLAN_K, during the first swing: robots 0, 2, 3 at stage 80 and
# robot 4 at 90, inside the double support [70, 130); robot 1, which stands, at 95; everybody else keeps their plan.  The new plans'
# first double support is as long as the old one's rest (the new steps start at stage 130 or later).  REFUSED_T: the tick after whose
# staging a replan at that very stage is tried - for robot 9, which keeps its plan and is in the double support [70, 130) there
REPLAN_K, REPLAN_FD, REFUSED_T, REFUSED_ROBOT = 60, 50, 100, 9
REPLAN_M = np.array([80, 95, 80, 80, 90, -1, -1, -1, -1, -1, -1, -1, -1], np.int32)
REPLAN_N = np.array([2, 2, 3, 1, 2, 0, 0, 0, 0, 0, 0, 0, 0], np.int32)


@functools.lru_cache(maxsize=None)
def replanned(wca, qs, cfg):
    """-> (the replan's arguments, the stitched plan, the restatement's run over it: the old DCM reference up to tick REPLAN_K, the
    stitched one from then on)"""
    fs, plan = _scenario(wca)
    sides = np.tile(np.array([0, 1, 0], np.uint8), (B, 1))
    rp = fr.new_steps(plan, REPLAN_M, REPLAN_N, sides, REPLAN_FD, 41)
    plan1 = fr.footstep_replan(plan, fs, REPLAN_M, rp, T, MAXT)
    m0 = int(REPLAN_M[REPLAN_M >= 0].min())
    old = dict(plan1, ref_traj=plan["ref_traj"])            # (the run starts on the old reference; the stages below every M are the old ones anyway)
    run = restate(wca, qs, cfg, old, splices={REPLAN_K: (m0, np.ascontiguousarray(plan1["ref_traj"][:, m0:]))})
    return rp, plan1, run
