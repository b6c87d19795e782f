"""oracle/tick_spec.py::run_ticks against the outputs of the restatements it replaced: the one loop with its patches (the reactive law,
the gain schedule) and its two copies (planned, streamed trajectories), recorded from their last version on a small matrix of cases -
tests/golden/tick_restatement_parent.npz holds the outputs only, the inputs are regenerated here from the seeded generators.  Where they
were recorded the new loop reproduced every key of every case bit for bit; here the bar is the project's restatement-against-restatement
1e-12 (the exact solvers go through LAPACK, whose last bit may differ between machines) and equality for the counters."""
import os

import numpy as np
import pytest

import robots
from helpers import planned_tick as pt
from helpers import streamed_tick as stt
from helpers import zmp_gains as zgh

ROBOT = "iCubGazeboV2_5"
ADD_ROT = robots.ROBOTS[ROBOT]["additional_rotation"]
SCHED = zgh.ZMP_SCHEDULE[ROBOT]
K_DCM = 1.2
FLOAT_KEYS = ("u0_log", "dq_log", "q_des", "dcm", "com", "zmp_gains", "logger", "measured_log")
COUNT_KEYS = ("mpc_fail", "ik_fail", "feedback_fail")


def _feedback(d, T, seed, bad=None):
    """`external` arrays around the uploaded state (no run needed to build them); bad = (site, tick, robot): one non-finite entry"""
    B = d["q0"].shape[0]
    rng = np.random.default_rng(seed)
    ext = dict(dcm=d["dcm0"] + 1e-3 * rng.normal(size=(T, B, 2)), com=d["com0"] + 1e-4 * rng.normal(size=(T, B, 2)),
               zmp=d["u_init"] + 1e-3 * rng.normal(size=(T, B, 2)), q=d["q0"] + 0.005 * rng.normal(size=(T, B, 23)))
    if bad is not None:
        ext[bad[0]][bad[1], bad[2], 1] = np.nan
    return ext


def cases(wca, qs):
    """name -> dict(args = (p, data, T, ik_params), kw = run_ticks' keywords; `loop` / `plan`: which of the replaced restatements recorded
    the case and the planned arrays [B][T][..] it was given - what the test does not read)"""
    from oracle import tick_spec as ts
    S = wca.synth
    model = S.icub_like_model()
    kin = dict(kin_model=model, foot_rect=S.FOOT_RECT)
    p = ts.TickParams()
    ipar_c = qs.IKParams(v_max=0.45 * np.ones(23))
    ipar_k = robots.ik_params(qs, ROBOT, v_max=S.WALK_VMAX.copy())
    ipar_k.joint_reg_deg = S.WALK_POSTURE_DEG.copy()
    out = {}

    def walk(B, T, planned=False):
        kb = S.synth_walk_kin_batch(B)
        poses = pt.poses_host(model, kb)
        if planned:
            return S.synth_planned_walk_batch(B, T, poses, kb, yaw_step=(0.03, 0.08))
        return S.synth_walk_batch(B, T, poses, kb)

    # the loop itself: constant Jacobians with logger rows and a splice; kinematics through a change of contact pair
    B, T = 3, 20
    dc = S.synth_tick_batch(B, T)
    tail = dc["ref_traj"][:, 12:16] + 0.01
    out["plain_logger_splice"] = dict(loop="run_ticks", args=(p, dc, T, ipar_c), kw=dict(logger_ticks=T, splices={8: (12, tail)}))
    dk130 = walk(2, 130)
    codes = np.array([ts.contact_code(t, dk130["phase0"], p) for t in range(130)])
    assert all(len(set(codes[:, i])) >= 2 for i in range(2)), "the run passes through a change of contact pair"
    out["plain_kinematics_contact_change"] = dict(loop="run_ticks", args=(p, dk130, 130, ipar_k), kw=dict(kin))
    # the reactive law: an explicit velocity with logger rows; the forward difference with kinematics
    vel = np.sqrt(p.gravity / p.com_height) * (dc["ref_traj"] - dc["zmp_ref"])
    out["reactive_explicit_velocity_logger"] = dict(loop="reactive", args=(p, dc, T, ipar_c),
                                                    kw=dict(dcm_controller="reactive", k_dcm=K_DCM, dcm_vel=vel, logger_ticks=T))
    dk = walk(2, 16)
    out["reactive_kinematics"] = dict(loop="reactive", args=(p, dk, 16, ipar_k), kw=dict(kin, dcm_controller="reactive", k_dcm=K_DCM))
    # the gain schedule on a paused reference (the gains move), MPC and reactive, forward difference and explicit velocity
    T = 40
    dp = dict(S.synth_tick_batch(B, T))
    dp["ref_traj"], _ = zgh.pause_reference(np.asarray(dp["ref_traj"]), {0: [(0, 6), (20, 12)], 2: [(10, 15)]})
    out["scheduled_paused"] = dict(loop="scheduled", args=(p, dp, T, ipar_c), kw=dict(zmp_gain_schedule=SCHED, logger_ticks=T))
    velp = np.zeros_like(dp["ref_traj"])
    velp[:, :-1] = 0.5 * (dp["ref_traj"][:, 1:] - dp["ref_traj"][:, :-1]) / p.dT          # another velocity than the forward difference
    out["scheduled_reactive_explicit_velocity"] = dict(loop="scheduled", args=(p, dp, T, ipar_c),
                                                       kw=dict(zmp_gain_schedule=SCHED, dcm_controller="reactive", k_dcm=K_DCM, dcm_vel=velp))
    # given stages: the planned loop and the streamed loop, alone and under both patches
    T = 24
    dw = walk(2, T, planned=True)
    st = stt.stages_of(dw, T)
    given = dict(kin, stages=st, neck_additional_rotation=ADD_ROT)
    both = dict(zmp_gain_schedule=SCHED, dcm_controller="reactive", k_dcm=K_DCM, dcm_vel=dw["dcm_vel_traj"])
    out["planned"] = dict(loop="planned", plan=dw, args=(p, dw, T, ipar_k), kw=dict(given))
    out["planned_reactive_scheduled"] = dict(loop="planned", plan=dw, args=(p, dw, T, ipar_k), kw=dict(given, **both))
    tailw = np.ascontiguousarray(dw["ref_traj"][:, 10:20] + 0.002)
    out["streamed_splice"] = dict(loop="streamed", args=(p, dw, T, ipar_k), kw=dict(given, splices={6: (10, tailw)}))
    out["streamed_reactive_scheduled_external"] = dict(loop="streamed", args=(p, dw, T, ipar_k),
                                                       kw=dict(given, external=_feedback(dw, T, 3), **both))
    rng = np.random.default_rng(2)
    noise = 1e-3 * rng.normal(size=(T, 2, 23))
    w = np.zeros((2, 6)); w[:, 2] = 150.0
    out["streamed_sensors"] = dict(loop="streamed", args=(p, dw, T, ipar_k),
                                   kw=dict(given, sensors=lambda t, q_des, dq_prev, u_prev: (q_des + noise[t], dq_prev, w, w)))
    # the rejection rule of `external`: robot 1's DCM is a NaN on tick 4
    out["external_rejected"] = dict(loop="run_ticks", args=(p, dk, 12, ipar_k), kw=dict(kin, external=_feedback(dk, 12, 7, bad=("dcm", 4, 1))))
    return out


@pytest.fixture(scope="module")
def recorded(golden_dir):
    return np.load(os.path.join(golden_dir, "tick_restatement_parent.npz"))


@pytest.fixture(scope="module")
def matrix(wca, qs):
    return cases(wca, qs)


CASE_NAMES = ("plain_logger_splice", "plain_kinematics_contact_change", "reactive_explicit_velocity_logger", "reactive_kinematics",
              "scheduled_paused", "scheduled_reactive_explicit_velocity", "planned", "planned_reactive_scheduled", "streamed_splice",
              "streamed_reactive_scheduled_external", "streamed_sensors", "external_rejected")


def test_the_matrix_is_the_recorded_one(matrix, recorded):
    assert set(matrix) == set(CASE_NAMES) == {k.split("/")[0] for k in recorded.files}


@pytest.mark.parametrize("name", CASE_NAMES)
def test_run_ticks_reproduces_the_replaced_restatements(matrix, recorded, name):
    from oracle import tick_spec as ts
    case = matrix[name]
    out = ts.run_ticks(*case["args"], **case["kw"])
    keys = [k.split("/")[1] for k in recorded.files if k.startswith(name + "/")]
    assert {"u0_log", "dq_log", "q_des", "dcm", "com", "mpc_fail", "ik_fail"} <= set(keys)
    for k in keys:
        want = recorded[name + "/" + k]
        if k in COUNT_KEYS:
            assert np.array_equal(out[k], want), (k, out[k], want)
        else:
            assert k in FLOAT_KEYS and out[k].shape == want.shape
            err = np.abs(out[k] - want).max()
            assert err <= 1e-12, (k, err)
    assert np.abs(out["dq_log"]).max() > 1e-4
    if name == "external_rejected":
        assert list(out["feedback_fail"]) == [0, 1] and list(out["ik_fail"]) == [0, 12 - 4 + 1]
    if name.startswith("scheduled"):
        assert np.ptp(out["zmp_gains"][:, 0, 0]) > 0.5            # the gains really move
