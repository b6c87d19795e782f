"""
ctypes binding of the C ABI declared in include/wcqp.h.

This is host-side plumbing only: every solve goes through libwcqp.so's HIP
kernels.  There is no CPU fallback — if the library is missing the import
fails, and if no GPU is present the solve entry points return WCQP_E_HIP and
`check()` raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("WCQP_LIB_PATH") or os.path.join(_HERE, "libwcqp.so")   # override: diagnostic builds only

VERSION = 400
WCQP_OK = OK = 0
E_INVALID, E_UNSUPPORTED, E_NUMERIC, E_HIP, E_NOMEM = -1, -2, -3, -4, -5
STATUS_SOLVED, STATUS_MAX_ITER, STATUS_INFEASIBLE, STATUS_OUTSIDE_HULL, STATUS_NUMERIC, STATUS_STRUCTURE = range(6)
IK_FORM_QPOASES, IK_FORM_OSQP = 0, 1
IK_ALG_DEFAULT, IK_ALG_SWEEP, IK_ALG_NULLSPACE, IK_ALG_NULLSPACE_MFMA, IK_ALG_NULLSPACE_16L, IK_ALG_BASE_ELIM = 0, 1, 2, 3, 4, 5
IK_JAC_AUTO, IK_JAC_MIXED, IK_JAC_GENERAL = 0, 1, 2
KIN_HANDOFF_NONE, KIN_HANDOFF_FUSED, KIN_HANDOFF_DENSE, KIN_HANDOFF_COMPACT = -1, 0, 1, 2      # (NONE: get_info's answer without kinematics)
HULL_ROWS = 8
MAX_DOF = KIN_MAX_DOF = 32
IK_STATE_LEN = 87

# every symbol include/wcqp.h declares (tests check the library exports all of them)
ABI_SYMBOLS = (
    "wcqp_strerror", "wcqp_version", "wcqp_device_count", "wcqp_stream_create", "wcqp_stream_destroy", "wcqp_stream_synchronize",
    "wcqp_mpc_create", "wcqp_mpc_destroy", "wcqp_mpc_get_condensed", "wcqp_mpc_get_matrices",
    "wcqp_mpc_solve_device", "wcqp_mpc_solve_host",
    "wcqp_ik_create", "wcqp_ik_destroy", "wcqp_ik_set_posture", "wcqp_ik_solve_device", "wcqp_ik_solve_host",
    "wcqp_hull_from_feet_device", "wcqp_hull_from_feet_host",
    "wcqp_kin_create", "wcqp_kin_destroy", "wcqp_kin_jacobians_device", "wcqp_kin_jacobians_host",
    "wcqp_prepare_create", "wcqp_prepare_destroy", "wcqp_prepare_solve_device", "wcqp_prepare_solve_host",
    "wcqp_tick_create", "wcqp_tick_create_ext", "wcqp_tick_create_opts", "wcqp_tick_get_option", "wcqp_tick_get_info_ext", "wcqp_tick_destroy", "wcqp_tick_upload", "wcqp_tick_run", "wcqp_tick_download", "wcqp_tick_splice_reference",
    "wcqp_tick_set_feedback_device", "wcqp_tick_set_feedback_host", "wcqp_tick_get_info",
    "wcqp_tick_set_sensor_feedback_device", "wcqp_tick_set_sensor_feedback_host",
    "wcqp_tick_set_desired_device", "wcqp_tick_set_desired_host", "wcqp_tick_set_desired_from_plan",
    "wcqp_tick_upload_footsteps", "wcqp_tick_upload_footsteps_timed", "wcqp_tick_replan_footsteps_timed", "wcqp_tick_get_plan", "wcqp_tick_replan_footsteps", "wcqp_tick_replan_goals", "wcqp_tick_get_goal_result",
    "wcqp_tick_replan_goals_timed", "wcqp_tick_get_goal_timing", "wcqp_tick_rebase_plan", "wcqp_tick_restart_robots", "wcqp_tick_get_restart_result", "wcqp_tick_recover_robots", "wcqp_tick_get_recover_result", "wcqp_tick_reset_robots", "wcqp_tick_set_swing_profile", "wcqp_tick_get_swing_profile",
    "wcqp_qp_enqueue_steps", "wcqp_qp_plan_create", "wcqp_qp_plan_enqueue", "wcqp_qp_plan_destroy",
    "wcqp_slab_layout_for", "wcqp_qp_step_from_slabs",
    "wcqp_unicycle_create", "wcqp_unicycle_destroy", "wcqp_unicycle_plan_device", "wcqp_unicycle_plan_host",
    "wcqp_unicycle_plan_timed_device", "wcqp_unicycle_plan_timed_host",
)


class WcqpError(RuntimeError):
    pass


class MpcParams(C.Structure):
    _fields_ = [("horizon", C.c_int32), ("sampling_time", C.c_double), ("com_height", C.c_double),
                ("gravity", C.c_double), ("Q", C.c_double * 4), ("R", C.c_double * 4),
                ("convex_hull_tolerance", C.c_double), ("feas_tol", C.c_double)]


class IkParams(C.Structure):
    _fields_ = [("dof", C.c_int32), ("use_com_as_constraint", C.c_int32), ("form", C.c_int32),
                ("max_iter", C.c_int32),
                ("com_weight", C.c_double * 9), ("neck_weight", C.c_double * 9),
                ("joint_reg_weights", C.c_double * MAX_DOF), ("joint_reg_gains", C.c_double * MAX_DOF),
                ("joint_reg_rad", C.c_double * MAX_DOF),
                ("v_min", C.c_double * MAX_DOF), ("v_max", C.c_double * MAX_DOF),
                ("k_pos_com", C.c_double), ("k_pos_foot", C.c_double),
                ("k_att_foot", C.c_double), ("k_neck", C.c_double),
                ("rho", C.c_double), ("tol", C.c_double), ("algorithm", C.c_int32),
                ("jacobian_structure", C.c_int32)]


class QpStep(C.Structure):
    """wcqp_qp_step: the arguments of one wcqp_mpc_solve_device + one wcqp_ik_solve_device call (raw device addresses)."""
    _fields_ = [("x0", C.c_void_p), ("ref", C.c_void_p), ("ref_len", C.c_int32), ("u_prev", C.c_void_p),
                ("hull_A", C.c_void_p), ("hull_b", C.c_void_p), ("hull_nc", C.c_void_p),
                ("u0", C.c_void_p), ("mpc_status", C.c_void_p), ("mpc_active", C.c_void_p), ("mpc_margin", C.c_void_p),
                ("mpc_stream", C.c_void_p),
                ("J_left", C.c_void_p), ("J_right", C.c_void_p), ("J_neck", C.c_void_p), ("J_com", C.c_void_p),
                ("q", C.c_void_p), ("state", C.c_void_p),
                ("dq", C.c_void_p), ("ik_status", C.c_void_p), ("active_lower", C.c_void_p), ("active_upper", C.c_void_p),
                ("foot_err", C.c_void_p), ("iters", C.c_void_p), ("ik_stream", C.c_void_p)]


SLAB_IN = ("x0", "ref", "u_prev", "hull_A", "hull_b", "hull_nc", "J_left", "J_right", "J_neck", "J_com", "q", "state")
SLAB_OUT = ("u0", "mpc_margin", "dq", "mpc_status", "mpc_active", "ik_status", "active_lower", "active_upper", "iters")
SLAB_IN_ARRAYS, SLAB_OUT_ARRAYS = 12, 9
assert (SLAB_IN_ARRAYS, SLAB_OUT_ARRAYS) == (len(SLAB_IN), len(SLAB_OUT))


class SlabLayout(C.Structure):
    """wcqp_slab_layout: where the arrays of one rank's block of robots sit inside its input / output slab (include/wcqp.h)."""
    _fields_ = [("batch", C.c_int32), ("ref_len", C.c_int32), ("in_offset", C.c_int64 * len(SLAB_IN)), ("in_bytes", C.c_int64),
                ("out_offset", C.c_int64 * len(SLAB_OUT)), ("out_bytes", C.c_int64)]

    @classmethod
    def make(cls, batch, ref_len):
        L = cls()
        check(lib().wcqp_slab_layout_for(int(batch), int(ref_len), C.byref(L)), "wcqp_slab_layout_for")
        return L

    def in_shapes(self):
        """name -> (byte offset, numpy dtype, shape) of the input slab's arrays."""
        B, n = self.batch, self.ref_len
        shp = dict(x0=(B, 2), ref=(B, n, 2), u_prev=(B, 2), hull_A=(B, HULL_ROWS, 2), hull_b=(B, HULL_ROWS), hull_nc=(B,), J_left=(B, 6, 29),
                   J_right=(B, 6, 29), J_neck=(B, 3, 29), J_com=(B, 3, 29), q=(B, 23), state=(B, IK_STATE_LEN))
        return {k: (int(self.in_offset[i]), np.int32 if k == "hull_nc" else np.float64, shp[k]) for i, k in enumerate(SLAB_IN)}

    def out_shapes(self):
        B = self.batch
        f64 = dict(u0=(B, 2), mpc_margin=(B,), dq=(B, 23))
        return {k: (int(self.out_offset[i]), np.float64 if k in f64 else (np.int32 if k in ("mpc_status", "ik_status", "iters") else np.uint32), f64.get(k, (B,)))
                for i, k in enumerate(SLAB_OUT)}

    def step(self, in_slab: int, out_slab: int) -> "QpStep":
        """A step record whose pointers point INTO the two slabs (raw device addresses)."""
        r = QpStep()
        check(lib().wcqp_qp_step_from_slabs(C.byref(self), C.c_void_p(in_slab), C.c_void_p(out_slab), C.byref(r)), "wcqp_qp_step_from_slabs")
        return r


def qp_enqueue_steps(mpc, ik, batch, steps):
    """wcqp_qp_enqueue_steps: `steps` is a ctypes array of QpStep (build it once, replay it often); mpc / ik are the
    MpcSolver / IkSolver handles (either may be None when no record uses it)."""
    done = C.c_int32(0)
    check(lib().wcqp_qp_enqueue_steps(mpc._h if mpc is not None else None, ik._h if ik is not None else None, int(batch),
                                      len(steps), steps, C.byref(done)), "wcqp_qp_enqueue_steps")
    return done.value


class _Handle:
    """What the handle classes share: close() calls the wcqp_*_destroy entry point `_destroy` names, once; __del__ closes."""

    def close(self):
        if self._h:
            getattr(lib(), self._destroy)(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:          # (also an object made with __new__ that never got _h)
            pass


PLAN_WAYS_AUTO = -1


class QpPlan(_Handle):
    """wcqp_qp_plan_*: the records of qp_enqueue_steps uploaded once, replayed as ONE launch that walks through them; `ways`
    wavefronts share a robot group (way w takes records w, w + ways, ...: records of different ways need their own outputs);
    ways = 0: a work queue over (record, robot group) units - every record needs outputs of its own.
    Records without an IK part (J_left = None in all of them; ik may be None): an MPC-only plan; without an MPC part (x0 = None; mpc may
    be None): an IK-only plan."""
    _destroy = "wcqp_qp_plan_destroy"

    def __init__(self, mpc, ik, batch, steps, ways=1):
        self._h = C.c_void_p()
        self._keep = (mpc, ik, steps)
        check(lib().wcqp_qp_plan_create(mpc._h if mpc is not None else None, ik._h if ik is not None else None, int(batch), len(steps), steps, int(ways), C.byref(self._h)), "wcqp_qp_plan_create")

    def enqueue(self, stream=0):
        check(lib().wcqp_qp_plan_enqueue(self._h, stream or None), "wcqp_qp_plan_enqueue")


class KinParams(C.Structure):
    _fields_ = [("dof", C.c_int32), ("parent", C.c_int32 * 32),
                ("R0", (C.c_double * 9) * 32), ("p0", (C.c_double * 3) * 32), ("axis", (C.c_double * 3) * 32),
                ("mass", C.c_double * 32), ("com", (C.c_double * 3) * 32),
                ("root_mass", C.c_double), ("root_com", C.c_double * 3),
                ("frame_joint", C.c_int32 * 3), ("frame_R", (C.c_double * 9) * 3), ("frame_p", (C.c_double * 3) * 3)]


class PrepareParams(C.Structure):
    """wcqp_prepare_params: weights, step cap, tolerances and iteration budget of the non-linear IK; q_reg / q_min / q_max are HOST pointers
    the library copies at create."""
    _fields_ = [("w_q", C.c_double), ("w_n", C.c_double), ("step_cap", C.c_double), ("tol_step", C.c_double), ("tol_constraint", C.c_double),
                ("max_iter", C.c_int32), ("q_reg", C.c_void_p), ("q_min", C.c_void_p), ("q_max", C.c_void_p)]


class TickParams(C.Structure):
    _fields_ = [("batch", C.c_int32), ("first", C.c_int32), ("max_ticks", C.c_int32), ("log_ticks", C.c_int32),
                ("step_ticks", C.c_int32), ("ds_ticks", C.c_int32),
                ("k_com", C.c_double), ("k_zmp", C.c_double), ("noise", C.c_double), ("seed", C.c_uint64),
                ("mpc", MpcParams), ("ik", IkParams),
                ("ik_cold_start_only", C.c_int32), ("use_kinematics", C.c_int32), ("kin", KinParams), ("foot_rect", C.c_double * 8),
                ("kin_handoff", C.c_int32), ("ticks_per_launch", C.c_int32), ("logger_ticks", C.c_int32), ("plant", C.c_int32),
                ("dcm_controller", C.c_int32), ("k_dcm", C.c_double),
                ("zmp_gain_scheduling", C.c_int32), ("k_com_stance", C.c_double), ("k_zmp_stance", C.c_double), ("zmp_smoothing_time", C.c_double),
                ("planned_trajectories", C.c_int32), ("neck_additional_rotation", C.c_double * 9),
                ("streamed_trajectories", C.c_int32),
                ("joint_velocity_cut_frequency", C.c_double), ("wrench_cut_frequency", C.c_double), ("com_cut_frequency", C.c_double),
                ("ik_mode", C.c_int32), ("position_ik", PrepareParams)]


class TickParamsExt(C.Structure):
    """wcqp_tick_params_ext: the parameters added since wcqp_tick_params was closed (wcqp_tick_create_ext)."""
    _fields_ = [("resident_plan", C.c_int32)]


class TickOption(C.Structure):
    """wcqp_tick_option: one (key, value) of the option list of wcqp_tick_create_opts - a capability added since both structs were closed."""
    _fields_ = [("key", C.c_int32), ("value", C.c_int32)]


TICK_OPT_RESIDENT_PLAN, TICK_OPT_POSITION_STREAMED = 1, 2
TICK_OPT_PLAN_TIMED = 3        # reported only (TickPipeline.option / info()["plan_timed"]): the plan in place carries per-step timings
TICK_OPT_PLAN_SHIFT = 4        # reported only (TickPipeline.option): the stages rebase_plan has taken since the last upload, summed
TICK_OPT_SWING_PROFILE = 5     # reported only (TickPipeline.option): the plan in force was generated with a non-zero swing profile
TICK_REBASE_AUTO = -1          # rebase_plan: the largest even shift <= the ticks enqueued
TICK_PLANT_INTERNAL, TICK_PLANT_EXTERNAL = 0, 1
TICK_DCM_MPC, TICK_DCM_REACTIVE = 0, 1
TICK_IK_VELOCITY, TICK_IK_POSITION = 0, 1
POSITION_IK_DEFAULTS = dict(q_reg=None, w_q=0.5, w_n=1.0, step_cap=0.3, tol_step=1e-12, tol_constraint=1e-10, max_iter=30, q_min=None, q_max=None)


class TickInfo(C.Structure):
    _fields_ = [("kin_handoff", C.c_int32), ("ticks_per_launch", C.c_int32), ("dcm_controller", C.c_int32), ("launches_per_tick", C.c_int32),
                ("zmp_gain_scheduling", C.c_int32), ("planned_trajectories", C.c_int32), ("streamed_trajectories", C.c_int32),
                ("sensor_filters", C.c_int32), ("plan_generated", C.c_int32), ("plan_record_ms", C.c_double), ("ik_mode", C.c_int32)]


class TickStepTiming(C.Structure):
    """wcqp_tick_step_timing: per-step durations ss_ticks / ds_ticks [B][K] (int32) of the timed footstep calls."""
    _fields_ = [("ss_ticks", C.c_void_p), ("ds_ticks", C.c_void_p)]


class TickSwingProfile(C.Structure):
    """wcqp_tick_swing_profile: the shape of a generated step (wcqp_tick_set_swing_profile, which defines the shaped swing)."""
    _fields_ = [("apex_ratio", C.c_double), ("landing_velocity", C.c_double), ("pitch_delta", C.c_double), ("com_height_delta", C.c_double)]


class TickInfoExt(C.Structure):
    """wcqp_tick_info_ext: what the handle took of wcqp_tick_params_ext (wcqp_tick_get_info_ext)."""
    _fields_ = [("resident_plan", C.c_int32)]


SENSOR_FILTERS = ("joint_velocity", "wrench", "com")      # bit k of wcqp_tick_info.sensor_filters


class TickDesired(C.Structure):
    """wcqp_tick_desired: the desired stage of one tick (streamed trajectories)."""
    _fields_ = [(k, C.c_void_p) for k in ("left_pose", "right_pose", "left_twist", "right_twist", "contact", "com_height", "com_height_vel")]


class TickInputs(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("ref_traj", "hull_tab_A", "hull_tab_b", "hull_tab_nc", "phase0",
                                          "J_left", "J_right", "J_neck", "J_com", "state0", "swing_twist",
                                          "q0", "dcm0", "com0", "u_init", "dcm_vel_traj",
                                          "left_traj", "right_traj", "left_twist", "right_twist", "contact", "com_height_traj", "com_height_vel")]


class TickFootsteps(C.Structure):
    """wcqp_tick_footsteps: the footsteps wcqp_tick_upload_footsteps expands into a planned handle's stages on the device."""
    _fields_ = [("max_steps", C.c_int32), ("n_steps", C.c_void_p), ("side", C.c_void_p), ("target", C.c_void_p),
                ("first_ds_ticks", C.c_int32), ("ss_ticks", C.c_int32), ("ds_ticks", C.c_int32), ("final_ds_ticks", C.c_int32),
                ("lift", C.c_double), ("zmp_delta_left", C.c_double * 2), ("zmp_delta_right", C.c_double * 2)]


class TickReplan(C.Structure):
    """wcqp_tick_replan: per robot the merge stage (-1: the robot keeps its plan) and the footsteps its plan is regenerated from there."""
    _fields_ = [("merge_stage", C.c_void_p), ("max_steps", C.c_int32), ("n_steps", C.c_void_p), ("side", C.c_void_p), ("target", C.c_void_p),
                ("first_ds_ticks", C.c_int32)]


TICK_MERGE_KEEP, TICK_MERGE_AUTO, TICK_SIDE_AUTO = -1, -2, 255
GOAL_KEPT, GOAL_TOO_LATE = -1, -2


class TickGoals(C.Structure):
    """wcqp_tick_goals: per robot the goal, the merge stage (KEEP / AUTO / M_i; NULL: AUTO) and the first swing foot (0 / 1 / SIDE_AUTO; NULL:
    SIDE_AUTO) of wcqp_tick_replan_goals."""
    _fields_ = [("goal", C.c_void_p), ("merge_stage", C.c_void_p), ("first_side", C.c_void_p), ("first_ds_ticks", C.c_int32), ("min_lead_ticks", C.c_int32)]


GOAL_RESULT = (("merge_stage", (), np.int32), ("first_side", (), np.uint8), ("status", (), np.int32), ("n_steps", (), np.int32),
               ("side", ("K",), np.uint8), ("target", ("K", 3), np.float64), ("desired_point", (2,), np.float64), ("unicycle_end", (3,), np.float64))


class TickGoalResult(C.Structure):
    """wcqp_tick_goal_result: what wcqp_tick_get_goal_result fills (GOAL_RESULT: [B] rows; K = the planner's max_steps)."""
    _fields_ = [(k, C.c_void_p) for k, _, _ in GOAL_RESULT]


TICK_RESTART_KEEP, TICK_RESTART_ALWAYS, TICK_RESTART_IF_STOPPED = 0, 1, 2


class TickRestart(C.Structure):
    """wcqp_tick_restart: per robot the mode (TICK_RESTART_*) and the rows a restarted robot starts from - state0 [B][87], q0 [B][dof],
    com0 [B][2], dcm0 / u_init [B][2] or NULL (the standing stage's ZMP)."""
    _fields_ = [(k, C.c_void_p) for k in ("mode", "state0", "q0", "com0", "dcm0", "u_init")]


class TickRestartResult(C.Structure):
    """wcqp_tick_restart_result: what wcqp_tick_get_restart_result fills - restarted [B] (uint8), stopped_ticks [B] (int64), stage (one int32)."""
    _fields_ = [(k, C.c_void_p) for k in ("restarted", "stopped_ticks", "stage")]


RECOVER_KEPT, RECOVER_NOT_STOPPED, RECOVER_NOT_STANDING = -1, -2, -3
RECOVER_ROWS = ("left_d", "right_d", "com_d", "Rd_neck", "q_guess", "dcm0", "u_init")


class TickRecover(C.Structure):
    """wcqp_tick_recover: per robot the mode (TICK_RESTART_*) and the targets of its posture IK - left_d / right_d [B][12] (both NULL: the
    soles of the plan's record S), com_d [B][3], Rd_neck [B][9], q_guess [B][dof], dcm0 / u_init [B][2], each or NULL."""
    _fields_ = [(k, C.c_void_p) for k in ("mode",) + RECOVER_ROWS]


class TickRecoverResult(C.Structure):
    """wcqp_tick_recover_result: what wcqp_tick_get_recover_result fills - restarted [B] (uint8), stopped_ticks [B] (int64), status and
    iters [B] (int32), residual [B][2], stage (one int32)."""
    _fields_ = [(k, C.c_void_p) for k in ("restarted", "stopped_ticks", "status", "iters", "residual", "stage")]


UNICYCLE_DONE, UNICYCLE_TRUNCATED, UNICYCLE_STUCK, UNICYCLE_INVALID_INPUT = range(4)


class UnicycleParams(C.Structure):
    """wcqp_unicycle_params: the unicycle planner's parameters (plannerParams.ini keys in include/wcqp.h; angles in radians)."""
    _fields_ = [("dT", C.c_double), ("reference_position", C.c_double * 2), ("unicycle_gain", C.c_double), ("slow_when_turning_gain", C.c_double),
                ("max_linear_velocity", C.c_double), ("max_angular_velocity", C.c_double), ("max_step_length", C.c_double),
                ("min_step_length", C.c_double), ("min_width", C.c_double), ("nominal_width", C.c_double),
                ("max_angle_variation", C.c_double), ("min_angle_variation", C.c_double), ("step_ticks", C.c_int32), ("max_steps", C.c_int32)]


class UnicycleInputs(C.Structure):
    """wcqp_unicycle_inputs: left0 / right0 [B][12], goal [B][2], first_side [B] (uint8)."""
    _fields_ = [(k, C.c_void_p) for k in ("left0", "right0", "goal", "first_side")]


class UnicycleOutputs(C.Structure):
    """wcqp_unicycle_outputs: n_steps [B], side [B][K], target [B][K][3], status [B], desired_point [B][2], unicycle_end [B][3]."""
    _fields_ = [(k, C.c_void_p) for k in ("n_steps", "side", "target", "status", "desired_point", "unicycle_end")]


class UnicycleTiming(C.Structure):
    """wcqp_unicycle_timing: the candidates' range and nominal duration in ticks, the two weights of a candidate's score and the
    double-support / single-support ratio of wcqp_unicycle_plan_timed_*."""
    _fields_ = [("min_step_ticks", C.c_int32), ("max_step_ticks", C.c_int32), ("nominal_step_ticks", C.c_int32),
                ("time_weight", C.c_double), ("position_weight", C.c_double), ("switch_over_swing_ratio", C.c_double)]


PLAN_WINDOW = (("left_traj", (12,), np.float64), ("right_traj", (12,), np.float64), ("left_twist", (6,), np.float64), ("right_twist", (6,), np.float64),
               ("contact", (), np.uint8), ("com_height", (), np.float64), ("com_height_vel", (), np.float64),
               ("ref_traj", (2,), np.float64), ("dcm_vel_traj", (2,), np.float64),
               ("hull_A", (HULL_ROWS, 2), np.float64), ("hull_b", (HULL_ROWS,), np.float64), ("hull_nc", (), np.int32))


class TickPlanWindow(C.Structure):
    """wcqp_tick_plan_window: what wcqp_tick_get_plan fills (PLAN_WINDOW: the [n][m] arrays; u_init [n][2])."""
    _fields_ = [(k, C.c_void_p) for k, _, _ in PLAN_WINDOW] + [("u_init", C.c_void_p)]


class TickOutputs(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("u0_log", "dq_log", "q_des", "dcm", "com", "mpc_fail", "ik_fail", "hot_try", "hot_hit", "tick", "logger", "active_lower", "active_upper", "zmp_gains",
                                          "measured", "feedback_fail", "q_log", "ik_iters")]


# every by-value struct and every integer macro of include/wcqp.h, by header name (tests check layout and values against the header)
ABI_STRUCTS = {
    "wcqp_mpc_params": MpcParams, "wcqp_ik_params": IkParams, "wcqp_qp_step": QpStep, "wcqp_slab_layout": SlabLayout, "wcqp_kin_params": KinParams,
    "wcqp_prepare_params": PrepareParams, "wcqp_tick_params": TickParams, "wcqp_tick_params_ext": TickParamsExt, "wcqp_tick_option": TickOption,
    "wcqp_tick_inputs": TickInputs, "wcqp_tick_outputs": TickOutputs, "wcqp_tick_info": TickInfo, "wcqp_tick_info_ext": TickInfoExt,
    "wcqp_tick_desired": TickDesired, "wcqp_tick_footsteps": TickFootsteps, "wcqp_tick_replan": TickReplan, "wcqp_tick_plan_window": TickPlanWindow,
    "wcqp_tick_goals": TickGoals, "wcqp_tick_goal_result": TickGoalResult, "wcqp_tick_step_timing": TickStepTiming,
    "wcqp_tick_swing_profile": TickSwingProfile, "wcqp_tick_restart": TickRestart, "wcqp_tick_restart_result": TickRestartResult,
    "wcqp_tick_recover": TickRecover, "wcqp_tick_recover_result": TickRecoverResult,
    "wcqp_unicycle_params": UnicycleParams, "wcqp_unicycle_inputs": UnicycleInputs, "wcqp_unicycle_outputs": UnicycleOutputs,
    "wcqp_unicycle_timing": UnicycleTiming,
}
ABI_CONSTANTS = {"WCQP_" + k: globals()[k] for k in (
    "VERSION OK E_INVALID E_UNSUPPORTED E_NUMERIC E_HIP E_NOMEM "
    "STATUS_SOLVED STATUS_MAX_ITER STATUS_INFEASIBLE STATUS_OUTSIDE_HULL STATUS_NUMERIC STATUS_STRUCTURE HULL_ROWS MAX_DOF IK_STATE_LEN "
    "IK_FORM_QPOASES IK_FORM_OSQP IK_ALG_DEFAULT IK_ALG_SWEEP IK_ALG_NULLSPACE IK_ALG_NULLSPACE_MFMA IK_ALG_NULLSPACE_16L IK_ALG_BASE_ELIM "
    "IK_JAC_AUTO IK_JAC_MIXED IK_JAC_GENERAL PLAN_WAYS_AUTO SLAB_IN_ARRAYS SLAB_OUT_ARRAYS KIN_MAX_DOF "
    "KIN_HANDOFF_FUSED KIN_HANDOFF_DENSE KIN_HANDOFF_COMPACT TICK_PLANT_INTERNAL TICK_PLANT_EXTERNAL TICK_DCM_MPC TICK_DCM_REACTIVE "
    "TICK_IK_VELOCITY TICK_IK_POSITION TICK_OPT_RESIDENT_PLAN TICK_OPT_POSITION_STREAMED TICK_OPT_PLAN_TIMED TICK_OPT_PLAN_SHIFT TICK_OPT_SWING_PROFILE TICK_REBASE_AUTO UNICYCLE_DONE UNICYCLE_TRUNCATED UNICYCLE_STUCK UNICYCLE_INVALID_INPUT "
    "TICK_MERGE_KEEP TICK_MERGE_AUTO TICK_SIDE_AUTO GOAL_KEPT GOAL_TOO_LATE TICK_RESTART_KEEP TICK_RESTART_ALWAYS TICK_RESTART_IF_STOPPED "
    "RECOVER_KEPT RECOVER_NOT_STOPPED RECOVER_NOT_STANDING").split()}

_lib: Optional[C.CDLL] = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise WcqpError(f"{LIB_PATH} is missing: build it with __graft_entry__.build() "
                            "(make -C walking-controllers_amd/csrc); there is no fallback path")
        L = C.CDLL(LIB_PATH)
        dp, ip, up, vp = C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p
        L.wcqp_strerror.restype = C.c_char_p
        L.wcqp_strerror.argtypes = [C.c_int]
        L.wcqp_stream_create.argtypes = [C.POINTER(C.c_void_p)]
        L.wcqp_stream_destroy.argtypes = [C.c_void_p]
        L.wcqp_stream_synchronize.argtypes = [C.c_void_p]
        L.wcqp_mpc_create.argtypes = [C.POINTER(MpcParams), C.POINTER(C.c_void_p)]
        L.wcqp_mpc_destroy.argtypes = [C.c_void_p]
        L.wcqp_mpc_get_condensed.argtypes = [C.c_void_p, dp, dp, dp, dp]
        L.wcqp_mpc_get_matrices.argtypes = [C.c_void_p, dp, dp, dp]
        mpc_args = [C.c_void_p, C.c_int32, dp, dp, C.c_int32, dp, dp, dp, ip, dp, ip, up, dp]
        L.wcqp_mpc_solve_device.argtypes = mpc_args + [vp]
        L.wcqp_mpc_solve_host.argtypes = mpc_args
        L.wcqp_ik_create.argtypes = [C.POINTER(IkParams), C.POINTER(C.c_void_p)]
        L.wcqp_ik_destroy.argtypes = [C.c_void_p]
        L.wcqp_ik_set_posture.argtypes = [C.c_void_p, C.c_void_p]
        ik_args = [C.c_void_p, C.c_int32, dp, dp, dp, dp, dp, dp, dp, ip, up, up, dp, ip]
        L.wcqp_ik_solve_device.argtypes = ik_args + [vp]
        L.wcqp_ik_solve_host.argtypes = ik_args
        L.wcqp_hull_from_feet_device.argtypes = [C.c_int32] + [C.c_void_p] * 8
        L.wcqp_hull_from_feet_host.argtypes = [C.c_int32] + [C.c_void_p] * 7
        L.wcqp_kin_create.argtypes = [C.POINTER(KinParams), C.POINTER(C.c_void_p)]
        L.wcqp_kin_destroy.argtypes = [C.c_void_p]
        L.wcqp_kin_jacobians_device.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 8
        L.wcqp_kin_jacobians_host.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 7
        L.wcqp_prepare_create.argtypes = [C.c_void_p, C.POINTER(PrepareParams), C.POINTER(C.c_void_p)]
        L.wcqp_prepare_destroy.argtypes = [C.c_void_p]
        L.wcqp_prepare_solve_device.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 12
        L.wcqp_prepare_solve_host.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 11
        L.wcqp_tick_create.argtypes = [C.POINTER(TickParams), C.POINTER(C.c_void_p)]
        L.wcqp_tick_create_ext.argtypes = [C.POINTER(TickParams), C.POINTER(TickParamsExt), C.POINTER(C.c_void_p)]
        L.wcqp_tick_create_opts.argtypes = [C.POINTER(TickParams), C.POINTER(TickOption), C.c_int32, C.POINTER(C.c_void_p)]
        L.wcqp_tick_get_option.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
        L.wcqp_tick_get_info_ext.argtypes = [C.c_void_p, C.POINTER(TickInfoExt)]
        L.wcqp_tick_destroy.argtypes = [C.c_void_p]
        L.wcqp_tick_upload.argtypes = [C.c_void_p, C.POINTER(TickInputs)]
        L.wcqp_tick_run.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
        L.wcqp_tick_download.argtypes = [C.c_void_p, C.POINTER(TickOutputs)]
        L.wcqp_tick_splice_reference.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        L.wcqp_tick_set_feedback_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.wcqp_tick_set_feedback_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.wcqp_tick_set_sensor_feedback_device.argtypes = [C.c_void_p] * 6
        L.wcqp_tick_set_sensor_feedback_host.argtypes = [C.c_void_p] * 5
        L.wcqp_tick_set_desired_device.argtypes = [C.c_void_p, C.POINTER(TickDesired), C.c_void_p]
        L.wcqp_tick_set_desired_host.argtypes = [C.c_void_p, C.POINTER(TickDesired)]
        L.wcqp_tick_set_desired_from_plan.argtypes = [C.c_void_p, C.c_void_p]
        L.wcqp_tick_get_info.argtypes = [C.c_void_p, C.POINTER(TickInfo)]
        L.wcqp_tick_upload_footsteps.argtypes = [C.c_void_p, C.POINTER(TickInputs), C.POINTER(TickFootsteps)]
        L.wcqp_tick_upload_footsteps_timed.argtypes = [C.c_void_p, C.POINTER(TickInputs), C.POINTER(TickFootsteps), C.POINTER(TickStepTiming)]
        L.wcqp_tick_replan_footsteps_timed.argtypes = [C.c_void_p, C.POINTER(TickReplan), C.POINTER(TickStepTiming), C.c_void_p]
        L.wcqp_tick_get_plan.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(TickPlanWindow)]
        L.wcqp_tick_replan_footsteps.argtypes = [C.c_void_p, C.POINTER(TickReplan), C.c_void_p]
        L.wcqp_tick_replan_goals.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(TickGoals), C.c_void_p]
        L.wcqp_tick_rebase_plan.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        L.wcqp_tick_restart_robots.argtypes = [C.c_void_p, C.POINTER(TickRestart), C.c_void_p]
        L.wcqp_tick_reset_robots.argtypes = [C.c_void_p, C.POINTER(TickRestart), C.c_void_p]
        L.wcqp_tick_get_restart_result.argtypes = [C.c_void_p, C.POINTER(TickRestartResult)]
        L.wcqp_tick_recover_robots.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(TickRecover), C.c_void_p]
        L.wcqp_tick_get_recover_result.argtypes = [C.c_void_p, C.POINTER(TickRecoverResult)]
        L.wcqp_tick_set_swing_profile.argtypes = [C.c_void_p, C.POINTER(TickSwingProfile)]
        L.wcqp_tick_get_swing_profile.argtypes = [C.c_void_p, C.POINTER(TickSwingProfile)]
        L.wcqp_tick_get_goal_result.argtypes = [C.c_void_p, C.POINTER(TickGoalResult)]
        L.wcqp_tick_replan_goals_timed.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(UnicycleTiming), C.POINTER(TickGoals), C.c_void_p]
        L.wcqp_tick_get_goal_timing.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.wcqp_unicycle_create.argtypes = [C.POINTER(UnicycleParams), C.POINTER(C.c_void_p)]
        L.wcqp_unicycle_destroy.argtypes = [C.c_void_p]
        L.wcqp_unicycle_plan_device.argtypes = [C.c_void_p, C.c_int32, C.POINTER(UnicycleInputs), C.POINTER(UnicycleOutputs), C.c_void_p]
        L.wcqp_unicycle_plan_host.argtypes = [C.c_void_p, C.c_int32, C.POINTER(UnicycleInputs), C.POINTER(UnicycleOutputs)]
        L.wcqp_unicycle_plan_timed_device.argtypes = [C.c_void_p, C.POINTER(UnicycleTiming), C.c_int32, C.POINTER(UnicycleInputs), C.POINTER(UnicycleOutputs),
                                                      C.c_void_p, C.c_void_p, C.c_void_p]
        L.wcqp_unicycle_plan_timed_host.argtypes = [C.c_void_p, C.POINTER(UnicycleTiming), C.c_int32, C.POINTER(UnicycleInputs), C.POINTER(UnicycleOutputs),
                                                    C.c_void_p, C.c_void_p]
        L.wcqp_qp_enqueue_steps.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(QpStep), C.POINTER(C.c_int32)]
        L.wcqp_qp_plan_create.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(QpStep), C.c_int32, C.POINTER(C.c_void_p)]
        L.wcqp_qp_plan_enqueue.argtypes = [C.c_void_p, C.c_void_p]
        L.wcqp_qp_plan_destroy.argtypes = [C.c_void_p]
        L.wcqp_slab_layout_for.argtypes = [C.c_int32, C.c_int32, C.POINTER(SlabLayout)]
        L.wcqp_qp_step_from_slabs.argtypes = [C.POINTER(SlabLayout), C.c_void_p, C.c_void_p, C.POINTER(QpStep)]
        _lib = L
    return _lib


def check(rc: int, what: str = "wcqp call") -> None:
    if rc != WCQP_OK:
        raise WcqpError(f"{what} failed: {lib().wcqp_strerror(rc).decode()} ({rc})")


def _p(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f64(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64)


# --------------------------------------------------------------------------------------
class MpcSolver(_Handle):
    """Handle over wcqp_mpc_* — the batched stand-in for WalkingController + MPCSolver."""
    _destroy = "wcqp_mpc_destroy"

    def __init__(self, horizon=50, sampling_time=0.01, com_height=0.53, gravity=9.81,
                 Q=None, R=None, convex_hull_tolerance=0.05, feas_tol=0.0):
        Q = 7500.0 * np.eye(2) if Q is None else np.asarray(Q, float)
        R = 9.0e6 * np.eye(2) if R is None else np.asarray(R, float)
        self.params = MpcParams(horizon, sampling_time, com_height, gravity,
                                (C.c_double * 4)(*Q.reshape(-1)), (C.c_double * 4)(*R.reshape(-1)),
                                convex_hull_tolerance, feas_tol)
        self.N = int(horizon)
        self._h = C.c_void_p()
        check(lib().wcqp_mpc_create(C.byref(self.params), C.byref(self._h)), "wcqp_mpc_create")

    def condensed(self):
        Gr = np.zeros((self.N + 1, 2, 2)); Gx = np.zeros((2, 2)); Gu = np.zeros((2, 2)); S0 = np.zeros((2, 2))
        check(lib().wcqp_mpc_get_condensed(self._h, _p(Gr), _p(Gx), _p(Gu), _p(S0)))
        return Gr, Gx, Gu, S0

    def matrices(self):
        n, nx, nu = 4 * self.N + 2, 2 * self.N + 2, 2 * self.N
        P = np.zeros((n, n)); A = np.zeros((nx, n)); G = np.zeros((nu, 2))
        check(lib().wcqp_mpc_get_matrices(self._h, _p(P), _p(A), _p(G)))
        return P, A, G

    def solve_host(self, x0, ref, u_prev, hull_A, hull_b, hull_nc):
        x0, ref, u_prev, hull_A, hull_b = map(_f64, (x0, ref, u_prev, hull_A, hull_b))
        hull_nc = np.ascontiguousarray(hull_nc, dtype=np.int32)
        B = x0.shape[0]
        ref_len = ref.shape[1]
        u0 = np.zeros((B, 2)); status = np.zeros(B, np.int32)
        active = np.zeros(B, np.uint32); margin = np.zeros(B)
        check(lib().wcqp_mpc_solve_host(self._h, B, _p(x0), _p(ref), ref_len, _p(u_prev), _p(hull_A), _p(hull_b),
                                        _p(hull_nc), _p(u0), _p(status), _p(active), _p(margin)),
              "wcqp_mpc_solve_host")
        return dict(u0=u0, status=status, active=active, margin=margin)

    def solve_device(self, batch, x0, ref, ref_len, u_prev, hull_A, hull_b, hull_nc,
                     u0, status, active=0, margin=0, stream=0):
        """All arguments are raw device addresses (ints), e.g. torch.Tensor.data_ptr()."""
        check(lib().wcqp_mpc_solve_device(self._h, batch, x0, ref, ref_len, u_prev, hull_A, hull_b, hull_nc,
                                          u0, status, active or None, margin or None, stream or None),
              "wcqp_mpc_solve_device")


class IkSolver(_Handle):
    """Handle over wcqp_ik_* — the batched stand-in for WalkingQPIK_{osqp,qpOASES}."""
    _destroy = "wcqp_ik_destroy"

    def __init__(self, form=IK_FORM_QPOASES, dof=23, use_com_as_constraint=True,
                 com_weight=None, neck_weight=None, joint_reg_weights=None, joint_reg_gains=None,
                 joint_reg_rad=None, v_min=None, v_max=None,
                 k_pos_com=1.0, k_pos_foot=4.0, k_att_foot=2.0, k_neck=1.0,
                 rho=0.0, tol=0.0, max_iter=0, algorithm=0, jacobian_structure=0):
        from .synth import ICUB_JOINT_REG_DEG
        com_weight = 100.0 * np.eye(3) if com_weight is None else np.asarray(com_weight, float)
        neck_weight = 5.0 * np.eye(3) if neck_weight is None else np.asarray(neck_weight, float)
        if joint_reg_weights is None:
            joint_reg_weights = np.array([1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2] + [1] * 12, float)
        joint_reg_gains = 5.0 * np.ones(dof) if joint_reg_gains is None else joint_reg_gains
        joint_reg_rad = np.deg2rad(ICUB_JOINT_REG_DEG) if joint_reg_rad is None else joint_reg_rad
        v_max = np.ones(dof) if v_max is None else np.broadcast_to(np.asarray(v_max, float), (dof,))
        v_min = -v_max if v_min is None else np.broadcast_to(np.asarray(v_min, float), (dof,))

        def pad(a):
            out = np.zeros(MAX_DOF)
            out[:dof] = np.asarray(a, float)[:dof]
            return (C.c_double * MAX_DOF)(*out)

        self.params = IkParams(dof, int(bool(use_com_as_constraint)), int(form), int(max_iter),
                               (C.c_double * 9)(*com_weight.reshape(-1)), (C.c_double * 9)(*neck_weight.reshape(-1)),
                               pad(joint_reg_weights), pad(joint_reg_gains), pad(joint_reg_rad),
                               pad(v_min), pad(v_max), k_pos_com, k_pos_foot, k_att_foot, k_neck, rho, tol, int(algorithm),
                               int(jacobian_structure))
        self.dof = dof
        self._h = C.c_void_p()
        check(lib().wcqp_ik_create(C.byref(self.params), C.byref(self._h)), "wcqp_ik_create")

    def set_posture(self, joint_reg_rad):
        """WalkingQPIK::setDesiredJointPosition: a new regularisation posture (rad) for every later solve."""
        a = _f64(np.asarray(joint_reg_rad, float).reshape(self.dof))
        check(lib().wcqp_ik_set_posture(self._h, _p(a)), "wcqp_ik_set_posture")

    def solve_host(self, J_left, J_right, J_neck, J_com, q, state, want_foot_err=True):
        J_left, J_right, J_neck, J_com, q, state = map(_f64, (J_left, J_right, J_neck, J_com, q, state))
        B = q.shape[0]
        dq = np.zeros((B, self.dof)); status = np.zeros(B, np.int32)
        lo = np.zeros(B, np.uint32); up = np.zeros(B, np.uint32)
        ferr = np.zeros((B, 12)) if want_foot_err else None
        iters = np.zeros(B, np.int32)
        check(lib().wcqp_ik_solve_host(self._h, B, _p(J_left), _p(J_right), _p(J_neck), _p(J_com), _p(q), _p(state),
                                       _p(dq), _p(status), _p(lo), _p(up), _p(ferr), _p(iters)),
              "wcqp_ik_solve_host")
        return dict(dq=dq, status=status, active_lower=lo, active_upper=up, foot_err=ferr, iters=iters)

    def solve_device(self, batch, J_left, J_right, J_neck, J_com, q, state, dq, status,
                     active_lower=0, active_upper=0, foot_err=0, iters=0, stream=0):
        """All arguments are raw device addresses (ints)."""
        check(lib().wcqp_ik_solve_device(self._h, batch, J_left, J_right, J_neck, J_com, q, state, dq, status,
                                         active_lower or None, active_upper or None, foot_err or None,
                                         iters or None, stream or None),
              "wcqp_ik_solve_device")


def hull_from_feet_host(foot_rect, left_T, right_T, contact):
    """Batch analogue of WalkingController::setConvexHullConstraint: foot poses -> hull rows."""
    foot_rect, left_T, right_T = _f64(foot_rect).reshape(8), _f64(left_T), _f64(right_T)
    contact = np.ascontiguousarray(contact, dtype=np.uint8)
    B = contact.shape[0]
    A = np.zeros((B, HULL_ROWS, 2)); b = np.zeros((B, HULL_ROWS)); nc = np.zeros(B, np.int32)
    check(lib().wcqp_hull_from_feet_host(B, _p(foot_rect), _p(left_T), _p(right_T), _p(contact), _p(A), _p(b), _p(nc)),
          "wcqp_hull_from_feet_host")
    return A, b, nc


class KinModel(_Handle):
    """Handle over wcqp_kin_* - batched forward kinematics + MIXED free-floating Jacobians.
    `model` is a table as returned by `synth.icub_like_model()`."""
    _destroy = "wcqp_kin_destroy"

    def __init__(self, model: dict):
        n = int(model["dof"])
        p = KinParams()
        p.dof = n
        for j in range(n):
            p.parent[j] = int(model["parent"][j])
            for k in range(9):
                p.R0[j][k] = float(np.asarray(model["R0"][j]).reshape(9)[k])
            for k in range(3):
                p.p0[j][k] = float(model["p0"][j][k]); p.axis[j][k] = float(model["axis"][j][k]); p.com[j][k] = float(model["com"][j][k])
            p.mass[j] = float(model["mass"][j])
        p.root_mass = float(model["root_mass"])
        for k in range(3):
            p.root_com[k] = float(model["root_com"][k])
        for f in range(3):
            p.frame_joint[f] = int(model["frame_joint"][f])
            for k in range(9):
                p.frame_R[f][k] = float(np.asarray(model["frame_R"][f]).reshape(9)[k])
            for k in range(3):
                p.frame_p[f][k] = float(model["frame_p"][f][k])
        self.params, self.dof = p, n
        self._h = C.c_void_p()
        check(lib().wcqp_kin_create(C.byref(p), C.byref(self._h)), "wcqp_kin_create")

    def jacobians_host(self, base, q, state=None):
        base, q = _f64(base), _f64(q)
        B, nc = q.shape[0], 6 + self.dof
        JL = np.zeros((B, 6, nc)); JR = np.zeros((B, 6, nc)); JN = np.zeros((B, 3, nc)); JC = np.zeros((B, 3, nc))
        st = None if state is None else _f64(state).copy()
        check(lib().wcqp_kin_jacobians_host(self._h, B, _p(base), _p(q), _p(JL), _p(JR), _p(JN), _p(JC), _p(st)), "wcqp_kin_jacobians_host")
        return dict(J_left=JL, J_right=JR, J_neck=JN, J_com=JC, state=st)

    def jacobians_device(self, batch, base, q, J_left, J_right, J_neck, J_com, state=0, stream=0):
        check(lib().wcqp_kin_jacobians_device(self._h, int(batch), base, q, J_left, J_right, J_neck, J_com, state or None, stream or None),
              "wcqp_kin_jacobians_device")


class PrepareSolver(_Handle):
    """Handle over wcqp_prepare_* - the batched non-linear IK that gives every robot the posture its walk starts from
    (WalkingModule::prepareRobot -> WalkingIK::computeIK; include/wcqp.h states the problem and the iteration).  kin: a KinModel;
    q_reg: the regularisation posture [dof] in rad; q_min / q_max: joint limits [dof] or None (both).  Defaults follow the reference:
    w_q = 0.5 (joint_regularization_weight), w_n = 1.0 (0: no neck target)."""
    _destroy = "wcqp_prepare_destroy"

    def __init__(self, kin: "KinModel", q_reg, w_q=0.5, w_n=1.0, step_cap=0.3, tol_step=1e-12, tol_constraint=1e-10, max_iter=100,
                 q_min=None, q_max=None):
        self.dof = kin.dof
        q_reg = _f64(np.asarray(q_reg, float).reshape(self.dof))
        lim = [None if x is None else _f64(np.asarray(x, float).reshape(self.dof)) for x in (q_min, q_max)]
        self.params = PrepareParams(float(w_q), float(w_n), float(step_cap), float(tol_step), float(tol_constraint), int(max_iter),
                                    q_reg.ctypes.data, *(None if x is None else x.ctypes.data for x in lim))
        self._h = C.c_void_p()
        check(lib().wcqp_prepare_create(kin._h, C.byref(self.params), C.byref(self._h)), "wcqp_prepare_create")

    def solve_host(self, left_d, right_d, com_d, q_guess, Rd_neck=None) -> dict:
        """left_d / right_d [B][12] desired sole poses (p 3 | R 9 row-major; the left one is the anchor), com_d [B][3], q_guess [B][dof],
        Rd_neck [B][9] or None (no neck target).  -> q, base [B][12], state [B][87] (ready to be state0), status, iters, residual [B][2]."""
        left_d, right_d, com_d, q_guess = map(_f64, (left_d, right_d, com_d, q_guess))
        neck = None if Rd_neck is None else _f64(Rd_neck).reshape(-1, 9)
        B = q_guess.shape[0]
        assert left_d.shape == (B, 12) and right_d.shape == (B, 12) and com_d.shape == (B, 3) and q_guess.shape == (B, self.dof) and \
            (neck is None or neck.shape == (B, 9)), (left_d.shape, right_d.shape, com_d.shape, q_guess.shape)
        o = dict(q=np.zeros((B, self.dof)), base=np.zeros((B, 12)), state=np.zeros((B, IK_STATE_LEN)), status=np.full(B, -1, np.int32),
                 iters=np.zeros(B, np.int32), residual=np.zeros((B, 2)))
        check(lib().wcqp_prepare_solve_host(self._h, B, _p(left_d), _p(right_d), _p(com_d), _p(neck), _p(q_guess), _p(o["q"]), _p(o["base"]),
                                            _p(o["state"]), _p(o["status"]), _p(o["iters"]), _p(o["residual"])), "wcqp_prepare_solve_host")
        return o

    def solve_device(self, batch, left_d, right_d, com_d, q_guess, q, status, Rd_neck=0, base=0, state=0, iters=0, residual=0, stream=0):
        """All array arguments are raw device addresses (ints); enqueue only."""
        check(lib().wcqp_prepare_solve_device(self._h, int(batch), left_d, right_d, com_d, Rd_neck or None, q_guess, q, base or None,
                                              state or None, status, iters or None, residual or None, stream or None), "wcqp_prepare_solve_device")


class UnicyclePlanner(_Handle):
    """Handle over wcqp_unicycle_* - footsteps from per-robot goals, the reference's setGoal (include/wcqp.h states the planner).  Defaults
    follow plannerParams.ini where it has the key (angles in radians here); the two saturations are this build's own.  step_ticks: unicycle
    samples per step, ss_ticks + ds_ticks of the walk the footsteps are for; max_steps: K, the row length of side / target.  timing (a
    dict over TIMING_DEFAULTS, kept as `planner.timing`): what the timed form - plan_host / plan_device with `timing=` - chooses every
    step's duration by; that form does not read step_ticks."""
    _destroy = "wcqp_unicycle_destroy"
    DEFAULTS = dict(dT=0.01, reference_position=(0.1, 0.0), unicycle_gain=10.0, slow_when_turning_gain=5.0, max_linear_velocity=0.1,
                    max_angular_velocity=0.5, max_step_length=0.20, min_step_length=0.05, min_width=0.14, nominal_width=0.16,
                    max_angle_variation=np.deg2rad(10.0), min_angle_variation=np.deg2rad(8.0), step_ticks=90, max_steps=8)

    # the reference's plannerParams.ini through dT = 0.01: minStepDuration 0.8, maxStepDuration 1.0, nominalDuration 0.9 [s], timeWeight 2.5,
    # positionWeight 1.0, switchOverSwingRatio 0.7
    TIMING_DEFAULTS = dict(min_step_ticks=80, max_step_ticks=100, nominal_step_ticks=90, time_weight=2.5, position_weight=1.0,
                           switch_over_swing_ratio=0.7)

    def __init__(self, timing=None, **params):
        unknown = set(params) - set(self.DEFAULTS)
        if unknown:
            raise TypeError("unknown unicycle parameter(s): " + ", ".join(sorted(unknown)))
        p = dict(self.DEFAULTS, **params)
        self.values = p
        self.timing = None if timing is None else self.timing_values(timing)      # what plan_host(..., timing=planner.timing) takes
        self.max_steps, self.step_ticks = int(p["max_steps"]), int(p["step_ticks"])
        scalars = [float(p[k]) for k, _ in UnicycleParams._fields_[2:12]]
        self.params = UnicycleParams(float(p["dT"]), (C.c_double * 2)(*map(float, p["reference_position"])), *scalars, self.step_ticks, self.max_steps)
        self._h = C.c_void_p()
        check(lib().wcqp_unicycle_create(C.byref(self.params), C.byref(self._h)), "wcqp_unicycle_create")

    @classmethod
    def from_ini_values(cls, values: dict, **params):
        """From the VALUES of a plannerParams.ini (a dict keyed as the file: unicycleGain, referencePosition, slowWhenTurningGain,
        maxStepLength, minStepLength, minWidth, nominalWidth, maxAngleVariation / minAngleVariation in DEGREES); `params` adds or
        overrides (dT, the saturations, step_ticks, max_steps).  The step timings of the file - minStepDuration, maxStepDuration,
        nominalDuration in SECONDS (ticks of dT here), timeWeight, positionWeight, switchOverSwingRatio - end up in `planner.timing`,
        what plan_host(..., timing=planner.timing) takes; None when the file has none of them."""
        key = dict(unicycleGain="unicycle_gain", referencePosition="reference_position", slowWhenTurningGain="slow_when_turning_gain",
                   maxStepLength="max_step_length", minStepLength="min_step_length", minWidth="min_width", nominalWidth="nominal_width")
        p = {v: values[k] for k, v in key.items() if k in values}
        for k, v in (("maxAngleVariation", "max_angle_variation"), ("minAngleVariation", "min_angle_variation")):
            if k in values:
                p[v] = float(np.deg2rad(values[k]))
        p.update(params)
        # the step timings, in seconds there and in ticks of dT here; held as planner.timing when the file has any of them
        dT = float(p.get("dT", cls.DEFAULTS["dT"]))
        tm = {v: int(round(float(values[k]) / dT)) for k, v in (("minStepDuration", "min_step_ticks"), ("maxStepDuration", "max_step_ticks"),
                                                                 ("nominalDuration", "nominal_step_ticks")) if k in values}
        tm.update({v: float(values[k]) for k, v in (("timeWeight", "time_weight"), ("positionWeight", "position_weight"),
                                                    ("switchOverSwingRatio", "switch_over_swing_ratio")) if k in values})
        return cls(timing=tm or None, **p)

    @classmethod
    def timing_values(cls, timing: dict) -> dict:
        """`timing` over TIMING_DEFAULTS (the keys of wcqp_unicycle_timing); an unknown key is a TypeError"""
        unknown = set(timing) - set(cls.TIMING_DEFAULTS)
        if unknown:
            raise TypeError("unknown timing parameter(s): " + ", ".join(sorted(unknown)))
        return dict(cls.TIMING_DEFAULTS, **timing)

    def _timing_struct(self, timing: dict) -> "UnicycleTiming":
        t = self.timing_values(timing)
        return UnicycleTiming(int(t["min_step_ticks"]), int(t["max_step_ticks"]), int(t["nominal_step_ticks"]), float(t["time_weight"]),
                              float(t["position_weight"]), float(t["switch_over_swing_ratio"]))

    def plan_host(self, left0, right0, goals, first_side, timing: Optional[dict] = None) -> dict:
        """left0 / right0 [B][12] sole poses (p 3 | R 9 row-major: the desired-foot entries of state0), goals [B][2] in the unicycle's frame,
        first_side [B] or a scalar (0: the left foot swings first, 1: the right).  -> n_steps [B], side [B][K], target [B][K][3] - what
        upload_footsteps / replan_footsteps take -, status [B] (UNICYCLE_*), desired_point [B][2], unicycle_end [B][3].
        timing: a dict of wcqp_unicycle_timing's fields (over TIMING_DEFAULTS; planner.timing holds an ini file's) - the planner then
        chooses every step's duration (wcqp_unicycle_plan_timed_host; step_ticks is not read) and ss_ticks, ds_ticks [B][K] come back too."""
        left0, right0, goals = _f64(left0), _f64(right0), _f64(goals)
        B = goals.shape[0] if goals.ndim else -1
        fs = np.asarray(first_side)
        if fs.ndim == 0:
            fs = np.full(max(B, 0), fs)
        if fs.size and (fs.min() < 0 or fs.max() > 1):
            raise ValueError("first_side is 0 (left) or 1 (right)")
        fs = np.ascontiguousarray(fs, dtype=np.uint8)
        if not (goals.shape == (B, 2) and left0.shape == (B, 12) and right0.shape == (B, 12) and fs.shape == (B,)):
            raise ValueError("shapes: left0 %s right0 %s goals %s first_side %s" % (left0.shape, right0.shape, goals.shape, fs.shape))
        K = self.max_steps
        o = dict(n_steps=np.zeros(B, np.int32), side=np.zeros((B, K), np.uint8), target=np.zeros((B, K, 3)), status=np.full(B, -1, np.int32),
                 desired_point=np.zeros((B, 2)), unicycle_end=np.zeros((B, 3)))
        tm = None if timing is None else self._timing_struct(timing)
        dur = {} if tm is None else dict(ss_ticks=np.zeros((B, K), np.int32), ds_ticks=np.zeros((B, K), np.int32))
        if B == 0:
            return dict(o, **dur)
        ins = UnicycleInputs(_p(left0), _p(right0), _p(goals), _p(fs))
        outs = UnicycleOutputs(**{k: (v.ctypes.data if v.size else None) for k, v in o.items()})
        if tm is None:
            check(lib().wcqp_unicycle_plan_host(self._h, B, C.byref(ins), C.byref(outs)), "wcqp_unicycle_plan_host")
        else:
            check(lib().wcqp_unicycle_plan_timed_host(self._h, C.byref(tm), B, C.byref(ins), C.byref(outs), *(v.ctypes.data if v.size else None for v in dur.values())),
                  "wcqp_unicycle_plan_timed_host")
        return dict(o, **dur)

    def plan_device(self, batch, left0, right0, goals, first_side, n_steps, side, target, status, desired_point=0, unicycle_end=0, stream=0,
                    timing: Optional[dict] = None, ss_ticks=0, ds_ticks=0):
        """All array arguments are raw device addresses (ints); enqueue only.  With `timing` (plan_host's) the timed form fills ss_ticks and
        ds_ticks [B][K] (int32) too."""
        ins = UnicycleInputs(left0, right0, goals, first_side)
        outs = UnicycleOutputs(n_steps, side or None, target or None, status, desired_point or None, unicycle_end or None)
        if timing is None:
            check(lib().wcqp_unicycle_plan_device(self._h, int(batch), C.byref(ins), C.byref(outs), stream or None), "wcqp_unicycle_plan_device")
        else:
            tm = self._timing_struct(timing)
            check(lib().wcqp_unicycle_plan_timed_device(self._h, C.byref(tm), int(batch), C.byref(ins), C.byref(outs), ss_ticks or None, ds_ticks or None,
                                                        stream or None), "wcqp_unicycle_plan_timed_device")


class TickPipeline(_Handle):
    """Handle over wcqp_tick_* — the device-resident MPC -> glue -> IK tick (configs 4/5)."""
    _destroy = "wcqp_tick_destroy"

    def __init__(self, batch, max_ticks, mpc: MpcSolver, ik: IkSolver, first=0, log_ticks=0,
                 step_ticks=180, ds_ticks=110, k_com=9.0, k_zmp=3.0, noise=1e-4, seed=99,
                 kin: "Optional[KinModel]" = None, foot_rect=None, ik_hot_start: bool = True, kin_handoff: int = 0,
                 ticks_per_launch: int = 0, logger_ticks: int = 0, external_feedback: bool = False,
                 dcm_controller: str = "mpc", k_dcm: Optional[float] = None, zmp_gain_scheduling: bool = False,
                 k_com_stance: Optional[float] = None, k_zmp_stance: Optional[float] = None, zmp_smoothing_time: Optional[float] = None,
                 planned_trajectories: bool = False, neck_additional_rotation=None, streamed_trajectories: bool = False,
                 sensor_filters: Optional[dict] = None, ik_mode: str = "velocity", position_ik: Optional[dict] = None,
                 resident_plan: bool = False):
        """kin: a KinModel -> per-tick kinematics (Jacobians, actual poses and hull rows rebuilt every tick from the
        integrated joint state with the base anchored at the stance foot; upload() then ignores J_* / hull_tab_*).
        dcm_controller: "mpc" (the DCM-MPC, the reference's use_mpc 1) or "reactive" (WalkingDCMReactiveController, the
        reference's default use_mpc 0), which needs k_dcm (kDCM of the robot's dcmReactiveControllerParams.ini).
        zmp_gain_scheduling: the reference's useGainScheduling 1 (zmpControllerParams.ini) - k_com / k_zmp are then the walking gains
        and k_com_stance, k_zmp_stance and zmp_smoothing_time (kCoM_stance, kZMP_stance, smoothingTime) are needed.
        planned_trajectories: every tick follows the planner's feet, twists, contact flags and CoM height (upload(left_traj=...)) instead of
        the synthetic gait; needs kin (the FUSED hand-off) and neck_additional_rotation (additional_rotation of qpInverseKinematics.ini, 3 x 3).
        streamed_trajectories (with external_feedback): every tick takes its desired stage from the set_desired_host / set_desired_device call
        in front of it - per tick set_desired -> set_sensor_feedback (or set_feedback) -> run(1); needs kin and neck_additional_rotation too.
        sensor_filters: dict(joint_velocity=, wrench=, com=) - cut frequencies in Hz of the low-pass filters set_sensor_feedback_* applies
        (joint_velocity_cut_frequency / wrench_cut_frequency of robotControl.ini, cut_frequency of forwardKinematics.ini); a missing key or
        0 leaves that filter off.  Needs external_feedback and kin.
        ik_mode: "velocity" (the Jacobian QP-IK whose joint velocities are integrated, the reference's use_QP-IK 1) or "position" (the
        reference's use_QP-IK 0: the non-linear IK of PrepareSolver every tick, hot-started at the previous tick's joints - a mode of a
        planned handle, or of a streamed one: with external_feedback and streamed_trajectories the tick runs its chain on the measured
        state and the non-linear IK on the live stage, per tick set_desired -> set_feedback / set_sensor_feedback -> run(1)).  position_ik: dict(q_reg=..., w_q=0.5, w_n=1.0, step_cap=0.3, tol_step=1e-12, tol_constraint=1e-10, max_iter=30,
        q_min=None, q_max=None) - the problem's parameters, max_iter the budget PER TICK; q_reg [dof] in rad is required.  `ik` then only
        supplies dof.  download() of such a handle returns q_log [log_ticks][B][dof] and ik_iters [B], and no dq_log.
        resident_plan (with streamed_trajectories): the handle also holds a plan, as a planned handle does - upload_footsteps, upload_goal,
        upload(left_traj=...), replan_footsteps, replan_goal and plan_window work on it - and set_desired_from_plan() stages tick t's stage
        out of it on the device: per tick set_desired_from_plan -> set_sensor_feedback (or set_feedback) -> run(1)."""
        self.resident = bool(resident_plan)
        if self.resident and not streamed_trajectories:
            raise ValueError("resident_plan is a capability of a streamed handle (streamed_trajectories=True, external_feedback=True)")
        if ik_mode not in ("velocity", "position"):
            raise ValueError(f"ik_mode must be 'velocity' or 'position', not {ik_mode!r}")
        self.position = ik_mode == "position"
        if not self.position and position_ik is not None:
            raise ValueError("position_ik was given to a handle created without ik_mode='position'")
        pik = dict(POSITION_IK_DEFAULTS)
        if self.position:
            unknown = set(position_ik or {}) - set(pik)
            if unknown:
                raise ValueError(f"position_ik: unknown key(s) {sorted(unknown)} (known: {', '.join(pik)})")
            pik.update(position_ik or {})
            if pik["q_reg"] is None:
                raise ValueError("ik_mode='position' needs position_ik['q_reg'], the regularisation posture [dof] in rad")
            if not planned_trajectories and not streamed_trajectories:
                raise ValueError("ik_mode='position' is a mode of a planned handle (planned_trajectories=True) or of a streamed one "
                                 "(streamed_trajectories=True, external_feedback=True)")
        cuts = dict.fromkeys(SENSOR_FILTERS, 0.0)
        for k, v in (sensor_filters or {}).items():
            if k not in cuts:
                raise ValueError(f"sensor_filters: unknown key {k!r} (one of {', '.join(SENSOR_FILTERS)})")
            v = float(v)
            if not np.isfinite(v) or v < 0.0:
                raise ValueError(f"sensor_filters[{k!r}] must be a finite cut frequency >= 0 Hz, not {v!r}")
            cuts[k] = v
        if dcm_controller not in ("mpc", "reactive"):
            raise ValueError(f"dcm_controller must be 'mpc' or 'reactive', not {dcm_controller!r}")
        self.reactive = dcm_controller == "reactive"
        if self.reactive and k_dcm is None:
            raise ValueError("the reactive DCM controller needs k_dcm")
        self.gain_sched = bool(zmp_gain_scheduling)
        if self.gain_sched and (k_com_stance is None or k_zmp_stance is None or zmp_smoothing_time is None):
            raise ValueError("ZMP gain scheduling needs k_com_stance, k_zmp_stance and zmp_smoothing_time")
        if self.gain_sched and not (np.isfinite(k_com_stance) and np.isfinite(k_zmp_stance) and np.isfinite(zmp_smoothing_time) and zmp_smoothing_time > 0):
            raise ValueError("ZMP gain scheduling needs finite stance gains and a finite zmp_smoothing_time > 0 (wcqp_tick_create: WCQP_E_INVALID)")
        self.planned = bool(planned_trajectories)
        if self.planned and streamed_trajectories:
            raise ValueError("streamed_trajectories and planned_trajectories exclude each other")
        if self.planned and neck_additional_rotation is None:
            raise ValueError("planned trajectories need neck_additional_rotation (additional_rotation of qpInverseKinematics.ini)")
        if self.planned and kin is None:
            raise ValueError("planned trajectories need per-tick kinematics (kin=KinModel(...)): with constant Jacobians the feet never move")
        self.streamed = bool(streamed_trajectories)
        if self.streamed and not external_feedback:
            raise ValueError("streamed trajectories are a mode of the external plant (external_feedback=True)")
        if self.streamed and neck_additional_rotation is None:
            raise ValueError("streamed trajectories need neck_additional_rotation (additional_rotation of qpInverseKinematics.ini)")
        if self.streamed and kin is None:
            raise ValueError("streamed trajectories need per-tick kinematics (kin=KinModel(...)): with constant Jacobians the feet never move")
        neck = np.asarray(neck_additional_rotation if (self.planned or self.streamed) else np.eye(3), float).reshape(-1)
        if neck.shape != (9,) or not np.all(np.isfinite(neck)):
            raise ValueError("neck_additional_rotation must be a finite 3 x 3 matrix")
        self.batch, self.max_ticks, self.log_ticks, self.dof = batch, max_ticks, log_ticks, ik.dof
        self.external = bool(external_feedback)
        self.logger_ticks = int(logger_ticks)
        self.use_kin = kin is not None
        if foot_rect is None:
            from .synth import FOOT_RECT
            foot_rect = FOOT_RECT
        self.params = TickParams(batch, first, max_ticks, log_ticks, step_ticks, ds_ticks, k_com, k_zmp, noise, seed,
                                 mpc.params, ik.params, int(not ik_hot_start), int(self.use_kin), kin.params if kin is not None else KinParams(),
                                 (C.c_double * 8)(*np.asarray(foot_rect, float).reshape(8)), int(kin_handoff), int(ticks_per_launch), int(logger_ticks),
                                 int(bool(external_feedback)), TICK_DCM_REACTIVE if self.reactive else TICK_DCM_MPC,
                                 float(k_dcm) if k_dcm is not None else 0.0, int(self.gain_sched),
                                 float(k_com_stance) if self.gain_sched else 0.0, float(k_zmp_stance) if self.gain_sched else 0.0,
                                 float(zmp_smoothing_time) if self.gain_sched else 0.0, int(self.planned), (C.c_double * 9)(*neck),
                                 int(self.streamed), *(cuts[k] for k in SENSOR_FILTERS))
        if self.position:
            # (the library copies the three arrays at create)
            arr = [None if pik[k] is None else _f64(np.asarray(pik[k], float).reshape(ik.dof)) for k in ("q_reg", "q_min", "q_max")]
            self.params.ik_mode = TICK_IK_POSITION
            self.params.position_ik = PrepareParams(float(pik["w_q"]), float(pik["w_n"]), float(pik["step_cap"]), float(pik["tol_step"]),
                                                    float(pik["tol_constraint"]), int(pik["max_iter"]), *(None if a is None else a.ctypes.data for a in arr))
        # the capabilities that travel as options (wcqp_tick_create_opts): a resident plan, POSITION on a streamed handle
        opts = {TICK_OPT_RESIDENT_PLAN: int(self.resident), TICK_OPT_POSITION_STREAMED: int(self.position and self.streamed)}
        self.options = (TickOption * len(opts))(*(TickOption(k, v) for k, v in opts.items()))
        self._h = C.c_void_p()
        check(lib().wcqp_tick_create_opts(C.byref(self.params), self.options, len(opts), C.byref(self._h)), "wcqp_tick_create_opts")
        self._keep = None

    def option(self, key: int) -> int:
        """The value the handle took of option `key` (TICK_OPT_*; wcqp_tick_get_option)."""
        v = C.c_int32(-1)
        check(lib().wcqp_tick_get_option(self._h, int(key), C.byref(v)), "wcqp_tick_get_option")
        return int(v.value)

    def _holds_plan(self) -> bool:
        """the handle holds a plan: a planned one, or a streamed one with resident_plan"""
        return self.planned or getattr(self, "resident", False)

    def upload(self, data: dict, dcm_vel_traj=None, left_traj=None, right_traj=None, left_twist=None, right_twist=None, contact=None,
               com_height_traj=None, com_height_vel=None):
        """dcm_vel_traj: [B][max_ticks + N + 1][2], the planner's DCM velocity for the reactive controller and for ZMP gain scheduling
        (None: the forward difference of ref_traj); MPC handles without scheduling ignore it.  A reactive handle takes data without hull
        tables.
        Planned handles: left_traj / right_traj [B][T][12] (sole position, row-major rotation), left_twist / right_twist [B][T][6], contact
        [B][T] (bit 0 left, bit 1 right in contact, bit 2 left is the fixed frame), com_height_traj / com_height_vel [B][T] or None,
        T = max_ticks + N + 1; data then needs no phase0 / swing_twist."""
        plan = dict(left_traj=left_traj, right_traj=right_traj, left_twist=left_twist, right_twist=right_twist, contact=contact)
        holds = self._holds_plan()
        if holds and any(v is None for v in plan.values()):
            raise ValueError("the upload of a handle that holds a plan needs " + ", ".join(k for k, v in plan.items() if v is None))
        if not holds and any(v is not None for v in list(plan.values()) + [com_height_traj, com_height_vel]):
            raise ValueError("planned trajectories were given to a handle created without planned_trajectories=True (or resident_plan=True)")
        nogait = self.planned or getattr(self, "streamed", False)      # (no synthetic gait: phase0 / swing_twist are optional)
        f64 = ("ref_traj", "state0", "q0", "dcm0", "com0", "u_init") + (() if nogait else ("swing_twist",))
        f64 += () if self.use_kin else ("J_left", "J_right", "J_neck", "J_com")
        if not self.use_kin and (not self.reactive or "hull_tab_A" in data):
            f64 += ("hull_tab_A", "hull_tab_b")
        keep = {k: _f64(data[k]) for k in f64}
        if "hull_tab_A" in keep:
            keep["hull_tab_nc"] = np.ascontiguousarray(data["hull_tab_nc"], dtype=np.int32)
        if not nogait or "phase0" in data:
            keep["phase0"] = np.ascontiguousarray(data["phase0"], dtype=np.int32)
        assert keep["ref_traj"].shape == (self.batch, self.max_ticks + self.params.mpc.horizon + 1, 2), keep["ref_traj"].shape
        if dcm_vel_traj is not None:
            keep["dcm_vel_traj"] = _f64(dcm_vel_traj)
            assert keep["dcm_vel_traj"].shape == keep["ref_traj"].shape, keep["dcm_vel_traj"].shape
        if holds:
            T = keep["ref_traj"].shape[1]
            for k, w in (("left_traj", 12), ("right_traj", 12), ("left_twist", 6), ("right_twist", 6)):
                keep[k] = _f64(plan[k])
                assert keep[k].shape == (self.batch, T, w), (k, keep[k].shape)
            keep["contact"] = np.ascontiguousarray(contact, dtype=np.uint8)
            assert keep["contact"].shape == (self.batch, T), keep["contact"].shape
            for k, v in (("com_height_traj", com_height_traj), ("com_height_vel", com_height_vel)):
                if v is not None:
                    keep[k] = _f64(v)
                    assert keep[k].shape == (self.batch, T), (k, keep[k].shape)
        ins = TickInputs(**{k: (keep[k].ctypes.data if k in keep else None) for k, _ in TickInputs._fields_})
        check(lib().wcqp_tick_upload(self._h, C.byref(ins)), "wcqp_tick_upload")

    def upload_footsteps(self, data: dict, footsteps: dict):
        """A planned handle's upload with the stages generated on the device (wcqp_tick_upload_footsteps, which defines the plan).
        data: state0, q0, com0 and optionally dcm0 / u_init (missing or None: the generated DCM reference and ZMP of stage 0).
        footsteps: n_steps [B], side [B][K] (0 left, 1 right), target [B][K][3] (x, y, yaw increment), first_ds_ticks, ss_ticks, ds_ticks,
        final_ds_ticks (0 or missing: ds_ticks), lift, zmp_delta_left, zmp_delta_right - what synth.synth_footstep_walk_batch returns.
        ss_ticks / ds_ticks as [B][K] arrays instead of two numbers: every step carries its own durations (wcqp_tick_upload_footsteps_timed;
        final_ds_ticks 0 or missing: each robot's own last ds) - what synth.synth_timed_footstep_walk_batch and a timed plan_host return."""
        if not self._holds_plan():
            raise ValueError("footsteps were given to a handle created without planned_trajectories=True (or resident_plan=True)")
        keep = {k: _f64(data[k]) for k in ("state0", "q0", "com0")}
        for k in ("dcm0", "u_init"):
            if data.get(k) is not None:
                keep[k] = _f64(data[k])
        n_steps = np.ascontiguousarray(footsteps["n_steps"], dtype=np.int32)
        side = np.ascontiguousarray(footsteps["side"], dtype=np.uint8)
        target = _f64(footsteps["target"])
        assert n_steps.shape == (self.batch,) and side.ndim == 2 and side.shape[0] == self.batch and target.shape == side.shape + (3,), \
            (n_steps.shape, side.shape, target.shape)
        dur = self._step_durations(footsteps, side.shape)
        fs = TickFootsteps(side.shape[1], n_steps.ctypes.data, side.ctypes.data if side.size else None, target.ctypes.data if target.size else None,
                           int(footsteps["first_ds_ticks"]), 0 if dur else int(footsteps["ss_ticks"]), 0 if dur else int(footsteps["ds_ticks"]),
                           int(footsteps.get("final_ds_ticks", 0)),
                           float(footsteps["lift"]), (C.c_double * 2)(*footsteps["zmp_delta_left"]), (C.c_double * 2)(*footsteps["zmp_delta_right"]))
        ins = TickInputs(**{k: (keep[k].ctypes.data if k in keep else None) for k, _ in TickInputs._fields_})
        if dur:
            tm = TickStepTiming(*(a.ctypes.data if a.size else None for a in dur))
            check(lib().wcqp_tick_upload_footsteps_timed(self._h, C.byref(ins), C.byref(fs), C.byref(tm)), "wcqp_tick_upload_footsteps_timed")
        else:
            check(lib().wcqp_tick_upload_footsteps(self._h, C.byref(ins), C.byref(fs)), "wcqp_tick_upload_footsteps")

    @staticmethod
    def _step_durations(footsteps: dict, shape):
        """(ss_ticks, ds_ticks) as int32 [B][K] arrays when `footsteps` carries per-step durations, else None"""
        ss, ds = footsteps.get("ss_ticks"), footsteps.get("ds_ticks")
        if ss is None or ds is None or (np.ndim(ss) == 0 and np.ndim(ds) == 0):
            return None
        ss, ds = np.ascontiguousarray(ss, dtype=np.int32), np.ascontiguousarray(ds, dtype=np.int32)
        if ss.shape != tuple(shape) or ds.shape != tuple(shape):
            raise ValueError("per-step ss_ticks %s / ds_ticks %s next to side %s" % (ss.shape, ds.shape, tuple(shape)))
        return ss, ds

    def replan_footsteps(self, merge_stage, footsteps: dict, first_ds_ticks: int, stream: Optional[int] = None):
        """A new goal for a generated walk that is running (wcqp_tick_replan_footsteps, which defines the replanned plan): robot i's plan is
        regenerated from stage merge_stage[i] on (-1: the robot keeps its plan) from footsteps n_steps [B], side [B][K'], target [B][K'][3],
        behind first_ds_ticks stages of double support; timings, lift and ZMP deltas stay those of upload_footsteps.  On a timed plan
        `footsteps` also carries the new steps' ss_ticks / ds_ticks [B][K'] (wcqp_tick_replan_footsteps_timed).  Enqueue-only on
        `stream`, behind the ticks already enqueued there; the arrays are copied before the call returns."""
        if not self._holds_plan():
            raise ValueError("footsteps were given to a handle created without planned_trajectories=True (or resident_plan=True)")
        merge = np.ascontiguousarray(merge_stage, dtype=np.int32)
        n_steps = np.ascontiguousarray(footsteps["n_steps"], dtype=np.int32)
        side = np.ascontiguousarray(footsteps["side"], dtype=np.uint8)
        target = _f64(footsteps["target"])
        assert merge.shape == (self.batch,) and n_steps.shape == (self.batch,) and side.ndim == 2 and side.shape[0] == self.batch and \
            target.shape == side.shape + (3,), (merge.shape, n_steps.shape, side.shape, target.shape)
        rp = TickReplan(merge.ctypes.data, side.shape[1], n_steps.ctypes.data, side.ctypes.data if side.size else None,
                        target.ctypes.data if target.size else None, int(first_ds_ticks))
        dur = self._step_durations(footsteps, side.shape)
        if dur:
            tm = TickStepTiming(*(a.ctypes.data if a.size else None for a in dur))
            check(lib().wcqp_tick_replan_footsteps_timed(self._h, C.byref(rp), C.byref(tm), stream or None), "wcqp_tick_replan_footsteps_timed")
        else:
            check(lib().wcqp_tick_replan_footsteps(self._h, C.byref(rp), stream or None), "wcqp_tick_replan_footsteps")

    def rebase_plan(self, shift: Optional[int] = None, stream: Optional[int] = None) -> int:
        """Moves the generated plan `shift` stages towards 0 on the device (wcqp_tick_rebase_plan, which defines the rebased plan): stage
        `shift` becomes stage 0, the tick index goes down by it, the robots' state stays, and run() has `shift` more ticks of room.
        shift None: the largest even shift <= the ticks enqueued.  Merge stages given afterwards are stages of the rebased plan; the
        logs are indexed by the rewound tick index, so download() first where the rows so far matter.  Enqueue-only on `stream`.
        Returns the shift taken."""
        before = self.option(TICK_OPT_PLAN_SHIFT)
        check(lib().wcqp_tick_rebase_plan(self._h, TICK_REBASE_AUTO if shift is None else int(shift), stream or None), "wcqp_tick_rebase_plan")
        return self.option(TICK_OPT_PLAN_SHIFT) - before

    def restart_robots(self, mode, data: dict, stream: Optional[int] = None):
        """Stopped robots restarted per robot, on the device (wcqp_tick_restart_robots, which defines the restarted robot): mode [B] of
        TICK_RESTART_KEEP / TICK_RESTART_ALWAYS / TICK_RESTART_IF_STOPPED (the device decides: ik_fail > 0); data: state0 [B][87], q0 [B][dof],
        com0 [B][2] and optionally dcm0 / u_init [B][2] (missing or None: the standing stage's ZMP).  A restarted robot has the state of an
        upload and stands, from the stage the next tick reads, on the soles of state0; replan_footsteps / replan_goals send it walking
        again.  Rows of KEEP robots are not read.  Enqueue-only on `stream`; the arrays are copied before the call returns.
        The rows can come from the batched start posture: p = PrepareSolver(...).solve_host(left_d, right_d, com_d, q_guess) gives
        restart_robots(mode, dict(state0=p["state"], q0=p["q"], com0=com_d[:, :2]))."""
        if not self._holds_plan():
            raise ValueError("restart_robots on a handle created without planned_trajectories=True (or resident_plan=True)")
        rs, _rows = self._restart_rows(mode, data)
        check(lib().wcqp_tick_restart_robots(self._h, C.byref(rs), stream or None), "wcqp_tick_restart_robots")

    def _restart_rows(self, mode, data: dict):
        """wcqp_tick_restart from mode [B] and data (state0, q0, com0, optionally dcm0 / u_init), with the arrays it points into."""
        m = np.ascontiguousarray(mode, dtype=np.uint8)
        keep = {k: _f64(data[k]) for k in ("state0", "q0", "com0")}
        for k in ("dcm0", "u_init"):
            if data.get(k) is not None:
                keep[k] = _f64(data[k])
        assert m.shape == (self.batch,) and keep["state0"].shape == (self.batch, IK_STATE_LEN) and keep["q0"].ndim == 2 and \
            keep["q0"].shape[0] == self.batch and all(keep[k].shape == (self.batch, 2) for k in keep if k not in ("state0", "q0")), \
            (m.shape, {k: v.shape for k, v in keep.items()})
        rs = TickRestart(m.ctypes.data, *(keep[k].ctypes.data if k in keep else None for k in ("state0", "q0", "com0", "dcm0", "u_init")))
        return rs, (m, keep)

    def reset_robots(self, mode, data: dict, stream: Optional[int] = None):
        """Robots of a sensor-fed fleet reset per robot, on the device (wcqp_tick_reset_robots, which defines the reset robot): a streamed
        EXTERNAL handle, with or without resident_plan.  mode and data as restart_robots takes them.  A reset robot has the controller state
        of an upload from the call's rows, measured joints q0, no rejected reading, no stage in hand, filters that start at its next
        accepted reading and - on a resident plan - stands from the stage the next tick reads.  The call comes first in that tick's
        sequence: reset_robots -> set_desired* -> set_*feedback* -> run(1).  Enqueue-only on `stream`; restart_result() reports it."""
        rs, _rows = self._restart_rows(mode, data)
        check(lib().wcqp_tick_reset_robots(self._h, C.byref(rs), stream or None), "wcqp_tick_reset_robots")

    def restart_result(self) -> dict:
        """What the last restart_robots call did (wcqp_tick_get_restart_result; waits for that call only): restarted [B] (bool),
        stopped_ticks [B] (the robot's ik_fail just before; 0 if it was not restarted) and stage, the stage S it restarted at."""
        out = dict(restarted=np.zeros(self.batch, np.uint8), stopped_ticks=np.zeros(self.batch, np.int64), stage=np.zeros(1, np.int32))
        res = TickRestartResult(**{k: v.ctypes.data for k, v in out.items()})
        check(lib().wcqp_tick_get_restart_result(self._h, C.byref(res)), "wcqp_tick_get_restart_result")
        return dict(restarted=out["restarted"].astype(bool), stopped_ticks=out["stopped_ticks"], stage=int(out["stage"][0]))

    def recover_robots(self, mode, prepare, left_d=None, right_d=None, com_d=None, Rd_neck=None, q_guess=None, dcm0=None, u_init=None,
                       stream: Optional[int] = None):
        """Stopped robots stood up on the device, posture IK and restart in one enqueue-only call (wcqp_tick_recover_robots, which defines
        the recovered robot): mode [B] as for restart_robots; prepare: a PrepareSolver on the handle's kinematic model.  Per listed robot the
        device decides whether it goes on (IF_STOPPED: ik_fail > 0), solves the start posture of those that do - towards left_d / right_d
        [B][12] (both None: the soles of the plan's next stage, which must be a double support), com_d [B][3] (None: the standing ZMP of the
        soles at the plan's CoM height), Rd_neck [B][9] (None: no neck target), from q_guess [B][dof] (None: the joints the robot stopped at) -
        and restarts exactly those whose IK ended SOLVED, with dcm0 / u_init [B][2] as restart_robots takes them.  Rows of KEEP robots are
        not read; the arrays are copied before the call returns."""
        if not self._holds_plan():
            raise ValueError("recover_robots on a handle created without planned_trajectories=True (or resident_plan=True)")
        if not isinstance(prepare, PrepareSolver):
            raise TypeError("recover_robots needs a PrepareSolver")
        m = np.ascontiguousarray(mode, dtype=np.uint8)
        given = dict(left_d=left_d, right_d=right_d, com_d=com_d, Rd_neck=Rd_neck, q_guess=q_guess, dcm0=dcm0, u_init=u_init)
        keep = {k: _f64(v) for k, v in given.items() if v is not None}
        width = dict(left_d=12, right_d=12, com_d=3, Rd_neck=9, dcm0=2, u_init=2)
        assert m.shape == (self.batch,) and all(v.ndim == 2 and v.shape[0] == self.batch and v.shape[1] == width.get(k, v.shape[1])
                                                for k, v in keep.items()), (m.shape, {k: v.shape for k, v in keep.items()})
        rv = TickRecover(m.ctypes.data, *(keep[k].ctypes.data if k in keep else None for k in RECOVER_ROWS))
        check(lib().wcqp_tick_recover_robots(self._h, prepare._h, C.byref(rv), stream or None), "wcqp_tick_recover_robots")

    def recover_result(self) -> dict:
        """What the last recover_robots call did (wcqp_tick_get_recover_result; waits for that call only): restarted [B] (bool),
        stopped_ticks [B], status [B] (the STATUS_* of the robot's IK, or RECOVER_KEPT / RECOVER_NOT_STOPPED / RECOVER_NOT_STANDING), iters [B],
        residual [B][2] and stage."""
        out = dict(restarted=np.zeros(self.batch, np.uint8), stopped_ticks=np.zeros(self.batch, np.int64), status=np.zeros(self.batch, np.int32),
                   iters=np.zeros(self.batch, np.int32), residual=np.zeros((self.batch, 2)), stage=np.zeros(1, np.int32))
        res = TickRecoverResult(**{k: v.ctypes.data for k, v in out.items()})
        check(lib().wcqp_tick_get_recover_result(self._h, C.byref(res)), "wcqp_tick_get_recover_result")
        return dict(out, restarted=out["restarted"].astype(bool), stage=int(out["stage"][0]))

    def set_swing_profile(self, apex_ratio: float = 0.0, landing_velocity: float = 0.0, pitch_delta: float = 0.0, com_height_delta: float = 0.0):
        """The shape of the steps the NEXT upload_footsteps / upload_goal generates (wcqp_tick_set_swing_profile, which defines the shaped
        swing): apex_ratio (footApexTime; 0: the symmetric quartic), landing_velocity [m/s, <= 0], pitch_delta [rad] and com_height_delta
        [m] - synth.shipped_swing_profile() holds plannerParams.ini's.  Host only; a running plan keeps the profile it was uploaded with,
        through every replan.  All zero: the plain plan, bit for bit."""
        p = TickSwingProfile(float(apex_ratio), float(landing_velocity), float(pitch_delta), float(com_height_delta))
        check(lib().wcqp_tick_set_swing_profile(self._h, C.byref(p)), "wcqp_tick_set_swing_profile")

    def swing_profile(self) -> dict:
        """The swing profile of the plan in force (wcqp_tick_get_swing_profile) - not the one set_swing_profile left for the next upload."""
        p = TickSwingProfile()
        check(lib().wcqp_tick_get_swing_profile(self._h, C.byref(p)), "wcqp_tick_get_swing_profile")
        return {k: float(getattr(p, k)) for k, _ in TickSwingProfile._fields_}

    def upload_goal(self, data: dict, goals, planner: "UnicyclePlanner", first_side, first_ds_ticks: int, ss_ticks: int = 0, ds_ticks: int = 0,
                    final_ds_ticks: int = 0, lift: float = 0.02, zmp_delta_left=(0.03, -0.005), zmp_delta_right=(0.03, 0.005),
                    timing: Optional[dict] = None) -> dict:
        """"Robot i, go there" from standing: plans footsteps on the device from the desired soles of data["state0"] (entries 24..47) towards
        goals [B][2] (UnicyclePlanner.plan_host), then upload_footsteps with them.  planner.step_ticks is the path samples per step: callers
        create it with ss_ticks + ds_ticks.  With `timing` (plan_host's) the planner chooses every step's durations and the plan is a
        timed one: ss_ticks / ds_ticks are not read.  Returns the planner's output dict (status says how each robot's planning ended)."""
        if not self._holds_plan():
            raise ValueError("a goal was given to a handle created without planned_trajectories=True (or resident_plan=True)")
        st = _f64(data["state0"])
        plan = planner.plan_host(st[:, 24:36], st[:, 36:48], goals, first_side, timing=timing)
        if timing is not None:
            ss_ticks, ds_ticks = plan["ss_ticks"], plan["ds_ticks"]
        self.upload_footsteps(data, dict(n_steps=plan["n_steps"], side=plan["side"], target=plan["target"], first_ds_ticks=first_ds_ticks,
                                         ss_ticks=ss_ticks, ds_ticks=ds_ticks, final_ds_ticks=final_ds_ticks, lift=lift,
                                         zmp_delta_left=zmp_delta_left, zmp_delta_right=zmp_delta_right))
        return plan

    def replan_goal(self, merge_stage, goals, planner: "UnicyclePlanner", first_side, first_ds_ticks: int, stream: Optional[int] = None,
                    timing: Optional[dict] = None) -> dict:
        """A new goal for a generated walk that is running: for every robot with merge_stage[i] >= 1 plans footsteps from the two desired
        soles of its plan's record merge_stage[i] towards goals[i], then replan_footsteps.  The soles are read through plan_window, one
        one-stage window per distinct merge stage - it synchronises.  Rows of robots with merge_stage -1 are not read.  Returns the planner's
        output dict over the whole batch: rows of robots that keep their plan are zero, with status -1.  With `timing`, on a timed plan, the
        planner chooses the new steps' durations (ss_ticks, ds_ticks in the output too)."""
        if not self._holds_plan():
            raise ValueError("a goal was given to a handle created without planned_trajectories=True (or resident_plan=True)")
        merge = np.ascontiguousarray(merge_stage, dtype=np.int32)
        goals = _f64(goals)
        fs = np.asarray(first_side)
        fs = np.full(self.batch, fs) if fs.ndim == 0 else fs
        if not (merge.shape == (self.batch,) and goals.shape == (self.batch, 2) and fs.shape == (self.batch,)):
            raise ValueError("shapes: merge_stage %s goals %s first_side %s" % (merge.shape, goals.shape, fs.shape))
        K = planner.max_steps
        out = dict(n_steps=np.zeros(self.batch, np.int32), side=np.zeros((self.batch, K), np.uint8), target=np.zeros((self.batch, K, 3)),
                   status=np.full(self.batch, -1, np.int32), desired_point=np.zeros((self.batch, 2)), unicycle_end=np.zeros((self.batch, 3)))
        if timing is not None:
            out.update(ss_ticks=np.zeros((self.batch, K), np.int32), ds_ticks=np.zeros((self.batch, K), np.int32))
        sel = np.nonzero(merge >= 1)[0]
        if sel.size:
            left0, right0 = np.zeros((sel.size, 12)), np.zeros((sel.size, 12))
            lo, n = int(sel.min()), int(sel.max() - sel.min() + 1)
            for M in np.unique(merge[sel]):
                w = self.plan_window(lo, n, int(M), 1, keys=("left_traj", "right_traj"))
                rows = merge[sel] == M
                left0[rows] = w["left_traj"][sel[rows] - lo, 0]; right0[rows] = w["right_traj"][sel[rows] - lo, 0]
            plan = planner.plan_host(left0, right0, goals[sel], fs[sel], timing=timing)
            for k in out:
                out[k][sel] = plan[k]
        self.replan_footsteps(merge, out, first_ds_ticks, stream=stream)
        return out

    def replan_goals(self, goals, planner: "UnicyclePlanner", first_ds_ticks: int, merge_stage=None, first_side=None, min_lead_ticks: int = 20,
                     stream: Optional[int] = None, timing: Optional[dict] = None) -> None:
        """"Robot i, go there" for a generated walk that is running, on the device and enqueue-only (wcqp_tick_replan_goals, which states the
        rules): goals [B][2]; merge_stage [B] of TICK_MERGE_KEEP / TICK_MERGE_AUTO / M_i >= 1 (None: AUTO for all - the first merge point of
        the robot's plan at least min_lead_ticks ahead); first_side [B] or a scalar of 0 / 1 / TICK_SIDE_AUTO (None: AUTO for all - the feet
        keep alternating).  The footsteps are planned and the plan regenerated on `stream` behind the ticks already enqueued; nothing is
        waited for and nothing returned - goal_result() reads what was decided.  A goal row of a robot that keeps its plan is not read.
        timing: on a timed plan, the dict plan_host / replan_goal take - the timed planner chooses every new step's durations on the device
        (wcqp_tick_replan_goals_timed) and goal_result() returns them too.  Without it the untimed call is made, which a timed plan refuses."""
        if not self._holds_plan():
            raise ValueError("a goal was given to a handle created without planned_trajectories=True (or resident_plan=True)")
        goals = _f64(goals)
        merge = None if merge_stage is None else np.ascontiguousarray(merge_stage, dtype=np.int32)
        fs = None if first_side is None else np.asarray(first_side)
        if fs is not None:
            fs = np.full(self.batch, fs) if fs.ndim == 0 else fs
            if ((fs < 0) | ((fs > 1) & (fs != TICK_SIDE_AUTO))).any():
                raise ValueError("first_side is 0 (left), 1 (right) or TICK_SIDE_AUTO")
            fs = np.ascontiguousarray(fs, dtype=np.uint8)
        if goals.shape != (self.batch, 2) or (merge is not None and merge.shape != (self.batch,)) or (fs is not None and fs.shape != (self.batch,)):
            raise ValueError("shapes: goals %s merge_stage %s first_side %s" % (goals.shape, None if merge is None else merge.shape, None if fs is None else fs.shape))
        if int(min_lead_ticks) < 0 or int(first_ds_ticks) < 1:
            raise ValueError("min_lead_ticks >= 0 and first_ds_ticks >= 1")
        g = TickGoals(goals.ctypes.data, None if merge is None else merge.ctypes.data, None if fs is None else fs.ctypes.data, int(first_ds_ticks), int(min_lead_ticks))
        if timing is not None:
            tm = planner._timing_struct(timing)
            check(lib().wcqp_tick_replan_goals_timed(self._h, planner._h, C.byref(tm), C.byref(g), stream or None), "wcqp_tick_replan_goals_timed")
        else:
            check(lib().wcqp_tick_replan_goals(self._h, planner._h, C.byref(g), stream or None), "wcqp_tick_replan_goals")
        self._goal_K = planner.max_steps
        self._goal_timed = timing is not None

    def goal_result(self) -> dict:
        """What the last replan_goals call decided and planned (wcqp_tick_get_goal_result; waits for that call only): per robot the
        merge_stage and first_side TAKEN, status (UNICYCLE_*, or GOAL_KEPT / GOAL_TOO_LATE with every other row zero), n_steps, side [B][K],
        target [B][K][3], desired_point [B][2], unicycle_end [B][3]; after a call with `timing` also ss_ticks, ds_ticks [B][K]
        (wcqp_tick_get_goal_timing)."""
        K = getattr(self, "_goal_K", None)
        if K is None:
            raise ValueError("goal_result() before any replan_goals()")
        out = {k: np.zeros((self.batch,) + tuple(K if d == "K" else d for d in shp), dt) for k, shp, dt in GOAL_RESULT}
        res = TickGoalResult(**{k: (v.ctypes.data if v.size else None) for k, v in out.items()})
        check(lib().wcqp_tick_get_goal_result(self._h, C.byref(res)), "wcqp_tick_get_goal_result")
        if getattr(self, "_goal_timed", False):
            dur = dict(ss_ticks=np.zeros((self.batch, K), np.int32), ds_ticks=np.zeros((self.batch, K), np.int32))
            check(lib().wcqp_tick_get_goal_timing(self._h, *(v.ctypes.data if v.size else None for v in dur.values())), "wcqp_tick_get_goal_timing")
            out.update(dur)
        return out

    def plan_window(self, robot0: int = 0, n: Optional[int] = None, stage0: int = 0, m: Optional[int] = None, keys=None) -> dict:
        """The plan a planned handle holds (wcqp_tick_get_plan): n robots from robot0, m stages from stage0 (None: to the end) - left_traj,
        right_traj, left_twist, right_twist, contact, com_height, com_height_vel, ref_traj, the support-polygon rows in force per stage
        (hull_A, hull_b, hull_nc), dcm_vel_traj where the handle keeps it (reactive controller, gain scheduling) and, after
        upload_footsteps, u_init [n][2], the generated ZMP of stage 0.  keys: only these arrays (None: all the handle offers)."""
        T = self.max_ticks + self.params.mpc.horizon + 1
        n = self.batch - robot0 if n is None else n
        m = T - stage0 if m is None else m
        out = {k: np.zeros((max(n, 0), max(m, 0)) + shp, dt) for k, shp, dt in PLAN_WINDOW if k != "dcm_vel_traj" or self.reactive or self.gain_sched}
        if self.info()["plan_generated"]:
            out["u_init"] = np.zeros((max(n, 0), 2))
        if keys is not None:
            out = {k: out[k] for k in keys}
        win = TickPlanWindow(**{k: v.ctypes.data for k, v in out.items()})
        check(lib().wcqp_tick_get_plan(self._h, int(robot0), int(n), int(stage0), int(m), C.byref(win)), "wcqp_tick_get_plan")
        return out

    def info(self) -> dict:
        """The form the handle took (wcqp_tick_get_info): kin_handoff ("fused", "compact", "dense" or None without kinematics),
        ticks_per_launch, dcm_controller ("mpc" / "reactive"), launches_per_tick, zmp_gain_scheduling (bool), planned_trajectories (bool),
        streamed_trajectories (bool), sensor_filters (the mask: bit 0 joint velocity, bit 1 wrench, bit 2 CoM), plan_generated (bool: the plan
        in place came from upload_footsteps), plan_record_ms (the device time of that upload's record pass) and ik_mode ("velocity" /
        "position"), resident_plan (bool) and plan_timed (bool: the plan in place carries per-step timings)."""
        i, x = TickInfo(), TickInfoExt()
        check(lib().wcqp_tick_get_info_ext(self._h, C.byref(x)), "wcqp_tick_get_info_ext")
        check(lib().wcqp_tick_get_info(self._h, C.byref(i)), "wcqp_tick_get_info")
        return dict(kin_handoff={KIN_HANDOFF_NONE: None, KIN_HANDOFF_FUSED: "fused", KIN_HANDOFF_DENSE: "dense",
                                 KIN_HANDOFF_COMPACT: "compact"}[i.kin_handoff],
                    ticks_per_launch=int(i.ticks_per_launch), dcm_controller="reactive" if i.dcm_controller == TICK_DCM_REACTIVE else "mpc",
                    launches_per_tick=int(i.launches_per_tick), zmp_gain_scheduling=bool(i.zmp_gain_scheduling),
                    planned_trajectories=bool(i.planned_trajectories), streamed_trajectories=bool(i.streamed_trajectories),
                    sensor_filters=int(i.sensor_filters), plan_generated=bool(i.plan_generated), plan_record_ms=float(i.plan_record_ms),
                    ik_mode="position" if i.ik_mode == TICK_IK_POSITION else "velocity", resident_plan=bool(x.resident_plan),
                    plan_timed=bool(self.option(TICK_OPT_PLAN_TIMED)))

    def run(self, n_ticks: int, use_graph: bool = True, stream: int = 0):
        check(lib().wcqp_tick_run(self._h, int(n_ticks), int(bool(use_graph)), stream or None), "wcqp_tick_run")

    def set_feedback_device(self, dcm_meas: int, com_meas: int, zmp_meas: int, q_meas: int = 0, stream: int = 0):
        """External feedback (plant = EXTERNAL): raw DEVICE addresses of the measured DCM / CoM / ZMP [B][2] and, optionally, joint positions
        [B][dof] the next tick is to use; enqueue only."""
        check(lib().wcqp_tick_set_feedback_device(self._h, dcm_meas, com_meas, zmp_meas, q_meas or None, stream or None), "wcqp_tick_set_feedback_device")

    def set_feedback_host(self, dcm_meas, com_meas, zmp_meas, q_meas=None):
        """External feedback from host arrays ([B][2] each, q_meas [B][dof] or None): in place when the call returns (the run may name any stream)."""
        a = [_f64(x) for x in (dcm_meas, com_meas, zmp_meas)]
        q = None if q_meas is None else _f64(q_meas)
        assert all(x.shape == (self.batch, 2) for x in a) and (q is None or q.shape == (self.batch, self.dof))
        check(lib().wcqp_tick_set_feedback_host(self._h, _p(a[0]), _p(a[1]), _p(a[2]), _p(q)), "wcqp_tick_set_feedback_host")

    def _sensor_arrays(self, q_meas, dq_meas, wrench_left, wrench_right):
        """the four sensor arrays as contiguous float64, or ValueError - non-finite values pass (the device rejects that robot)"""
        B, D = self.batch, self.dof
        out = []
        for name, x, shape in (("q_meas", q_meas, (B, D)), ("dq_meas", dq_meas, (B, D)), ("wrench_left", wrench_left, (B, 6)),
                               ("wrench_right", wrench_right, (B, 6))):
            a = np.asarray(x)
            if a.dtype != np.float64:
                raise ValueError(f"{name} must be float64, not {a.dtype}")
            if a.shape != shape:
                raise ValueError(f"{name} must have shape {shape}, not {a.shape}")
            out.append(np.ascontiguousarray(a))
        return out

    def set_sensor_feedback_host(self, q_meas, dq_meas, wrench_left, wrench_right):
        """Sensor feedback (plant = EXTERNAL with kinematics, wcqp_tick_set_sensor_feedback_host): measured joint positions / velocities
        [B][dof] and the two sole wrenches [B][6] (fx fy fz tx ty tz in the sole frame) of the next tick; the device evaluates CoM, DCM and
        ZMP from them.  In place when the call returns (the run may name any stream).  Shapes and dtypes are checked here, before any device
        call; a robot with a non-finite value is rejected on the device (download()["feedback_fail"])."""
        a = self._sensor_arrays(q_meas, dq_meas, wrench_left, wrench_right)
        check(lib().wcqp_tick_set_sensor_feedback_host(self._h, *(_p(x) for x in a)), "wcqp_tick_set_sensor_feedback_host")

    def set_sensor_feedback_device(self, q_meas, dq_meas, wrench_left, wrench_right, stream: int = 0):
        """The same from DEVICE memory: raw addresses, or float64 torch tensors of the shapes above on the GPU (checked here); enqueue only."""
        shapes = ((self.batch, self.dof), (self.batch, self.dof), (self.batch, 6), (self.batch, 6))
        ptrs = []
        for name, x, shape in zip(("q_meas", "dq_meas", "wrench_left", "wrench_right"), (q_meas, dq_meas, wrench_left, wrench_right), shapes):
            if hasattr(x, "data_ptr"):
                import torch
                if x.dtype != torch.float64 or tuple(x.shape) != shape or not x.is_contiguous() or not x.is_cuda:
                    raise ValueError(f"{name} must be a contiguous float64 device tensor of shape {shape}")
                ptrs.append(x.data_ptr())
            else:
                ptrs.append(int(x))
        check(lib().wcqp_tick_set_sensor_feedback_device(self._h, *[p or None for p in ptrs], stream or None), "wcqp_tick_set_sensor_feedback_device")

    _DESIRED = (("left_pose", 12), ("right_pose", 12), ("left_twist", 6), ("right_twist", 6))

    def set_desired_host(self, left_pose, right_pose, left_twist, right_twist, contact, com_height=None, com_height_vel=None):
        """Streamed trajectories (wcqp_tick_set_desired_host): the desired stage of the next tick - sole poses [B][12] (p 3 | R 9 row-major),
        twists [B][6], contact [B] uint8 (bit 0 left, bit 1 right in contact, bit 2 left is the fixed frame), CoM height / velocity [B] or
        None (state0[68], 0).  Shapes and dtypes are checked here; an invalid stage (no foot in contact, a fixed-frame foot in the air, a
        non-finite value) is refused by the library with the handle unchanged.  In place when the call returns."""
        B = self.batch
        keep = []
        for (name, w), x in zip(self._DESIRED, (left_pose, right_pose, left_twist, right_twist)):
            a = np.asarray(x)
            if a.dtype != np.float64 or a.shape != (B, w):
                raise ValueError(f"{name} must be float64 of shape {(B, w)}, not {a.dtype} {a.shape}")
            keep.append(np.ascontiguousarray(a))
        c = np.asarray(contact)
        if c.dtype != np.uint8 or c.shape != (B,):
            raise ValueError(f"contact must be uint8 of shape {(B,)}, not {c.dtype} {c.shape}")
        keep.append(np.ascontiguousarray(c))
        for name, x in (("com_height", com_height), ("com_height_vel", com_height_vel)):
            if x is None:
                keep.append(None)
                continue
            a = np.asarray(x)
            if a.dtype != np.float64 or a.shape != (B,):
                raise ValueError(f"{name} must be float64 of shape {(B,)}, not {a.dtype} {a.shape}")
            keep.append(np.ascontiguousarray(a))
        des = TickDesired(*[None if a is None else a.ctypes.data for a in keep])
        check(lib().wcqp_tick_set_desired_host(self._h, C.byref(des)), "wcqp_tick_set_desired_host")

    def set_desired_from_plan(self, stream: Optional[int] = None):
        """A resident plan (wcqp_tick_set_desired_from_plan): stage t of the plan the handle holds becomes the desired stage of the next
        tick, for every robot - one kernel on `stream`, enqueue only; t is read on the device.  It takes set_desired_*'s place in the
        per-tick order; a set_desired_* call after it replaces the stage."""
        check(lib().wcqp_tick_set_desired_from_plan(self._h, stream or None), "wcqp_tick_set_desired_from_plan")

    def set_desired_device(self, left_pose, right_pose, left_twist, right_twist, contact, com_height=None, com_height_vel=None, stream: int = 0):
        """The same from DEVICE memory: raw addresses, or contiguous torch tensors on the GPU of the shapes above (float64; contact uint8),
        checked here; enqueue only.  A robot with an invalid stage is rejected on the device (download()["feedback_fail"])."""
        B = self.batch
        spec = tuple((n, (B, w), "float64") for n, w in self._DESIRED) + (("contact", (B,), "uint8"), ("com_height", (B,), "float64"),
                                                                           ("com_height_vel", (B,), "float64"))
        ptrs = []
        for (name, shape, dt), x in zip(spec, (left_pose, right_pose, left_twist, right_twist, contact, com_height, com_height_vel)):
            if x is None or (isinstance(x, int) and x == 0):
                if name not in ("com_height", "com_height_vel"):
                    raise ValueError(f"{name} is required")
                ptrs.append(None)
            elif hasattr(x, "data_ptr"):
                import torch
                if x.dtype != getattr(torch, dt) or tuple(x.shape) != shape or not x.is_contiguous() or not x.is_cuda:
                    raise ValueError(f"{name} must be a contiguous {dt} device tensor of shape {shape}")
                ptrs.append(x.data_ptr())
            else:
                ptrs.append(int(x))
        des = TickDesired(*ptrs)
        check(lib().wcqp_tick_set_desired_device(self._h, C.byref(des), stream or None), "wcqp_tick_set_desired_device")

    def splice_reference(self, from_tick: int, ref_tail, stream: int = 0):
        """Trajectory merge: stages [from_tick, from_tick + n) of every instance's DCM reference <- ref_tail[B][n][2]."""
        tail = _f64(ref_tail)
        assert tail.ndim == 3 and tail.shape[0] == self.batch and tail.shape[2] == 2, tail.shape
        # (the library stages the host rows before it returns: `tail` may go out of scope at once, whatever `stream` is still doing)
        check(lib().wcqp_tick_splice_reference(self._h, int(from_tick), tail.shape[1], _p(tail), stream or None), "wcqp_tick_splice_reference")

    def download(self):
        B, L, D = self.batch, self.log_ticks, self.dof
        o = dict(u0_log=np.zeros((L, B, 2)), dq_log=np.zeros((L, B, D)), q_des=np.zeros((B, D)), dcm=np.zeros((B, 2)),
                 com=np.zeros((B, 2)), mpc_fail=np.zeros(B, np.int64), ik_fail=np.zeros(B, np.int64),
                 hot_try=np.zeros(B, np.int64), hot_hit=np.zeros(B, np.int64), tick=np.zeros(1, np.int32),
                 active_lower=np.zeros(B, np.uint32), active_upper=np.zeros(B, np.uint32), zmp_gains=np.zeros((B, 2)))
        if getattr(self, "position", False):
            # a POSITION handle forms no velocity: the joints every tick commanded, and the iterations spent
            del o["dq_log"]
            o["q_log"] = np.zeros((L, B, D)); o["ik_iters"] = np.zeros(B, np.int64)
        if self.logger_ticks > 0:
            o["logger"] = np.zeros((self.logger_ticks, B, 53))
        if getattr(self, "external", False):
            o["measured"] = np.zeros((B, 6)); o["feedback_fail"] = np.zeros(B, np.int64)
        outs = TickOutputs(**{k: (o[k].ctypes.data if k in o else None) for k, _ in TickOutputs._fields_})
        check(lib().wcqp_tick_download(self._h, C.byref(outs)), "wcqp_tick_download")
        o["tick"] = int(o["tick"][0])
        return o


def source_hash() -> str:
    """sha256 over the kernel sources (csrc/*.hip, *.h, *.inc, *.cpp): what a measurement that is kept in the repository
    (profiles/traffic.json) is stamped with, so that it is not quoted for kernels that have changed since."""
    import glob
    import hashlib
    h = hashlib.sha256()
    files = sorted(glob.glob(os.path.join(_HERE, "csrc", "*.hip")) + glob.glob(os.path.join(_HERE, "csrc", "*.h")) + glob.glob(os.path.join(_HERE, "csrc", "*.inc")) +
                   glob.glob(os.path.join(_HERE, "csrc", "*.cpp")))
    for f in files:
        h.update(os.path.basename(f).encode() + b"\0")
        h.update(open(f, "rb").read())
    return h.hexdigest()


def device_count() -> int:
    return int(lib().wcqp_device_count())


def stream_create() -> int:
    """A HIP stream (raw handle as an int) from the library's own runtime - for callers without torch."""
    s = C.c_void_p()
    check(lib().wcqp_stream_create(C.byref(s)), "wcqp_stream_create")
    return s.value


def stream_destroy(stream: int) -> None:
    check(lib().wcqp_stream_destroy(C.c_void_p(stream)), "wcqp_stream_destroy")


def stream_synchronize(stream: int = 0) -> None:
    check(lib().wcqp_stream_synchronize(C.c_void_p(stream) if stream else None), "wcqp_stream_synchronize")
