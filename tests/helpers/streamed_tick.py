"""Scenario builders for given stages (oracle/tick_spec.py::run_ticks(stages=...), wcqp_tick_params.streamed_trajectories): the
stage-major arrays [T][B][..] out of a planned upload [B][T][..], a replanned walk out of two, and a run's own plant or measured states as
the `external` dict of the next run."""
import numpy as np

STAGE_KEYS = (("left_traj", "left_pose"), ("right_traj", "right_pose"), ("left_twist", "left_twist"), ("right_twist", "right_twist"),
              ("contact", "contact"), ("com_height_traj", "com_height"), ("com_height_vel", "com_height_vel"))


def stages_of(plan, T):
    """planned arrays [B][>= T][..] -> per-tick arrays [T][B][..] (contiguous, one stage per tick)"""
    out = {}
    for src, dst in STAGE_KEYS:
        if plan.get(src) is not None:
            out[dst] = np.ascontiguousarray(np.swapaxes(np.asarray(plan[src])[:, :T], 0, 1))
    return out


def concat_stages(a, b, k):
    """stages of `a` for ticks < k, of `b` from tick k on"""
    return {key: np.ascontiguousarray(np.concatenate([a[key][:k], b[key][k:]])) for key in a}


def external_of(run):
    """the plant states an internal run returned, as the `external` dict of the next run (q: None - the desired joints)"""
    return dict(dcm=run["dcm_log"], com=run["com_log"], zmp=run["zmp_log"])


def external_of_sensors(run):
    """the measured states and joints a run with `sensors` evaluated, as the `external` dict of the next run"""
    m = run["measured_log"]
    return dict(dcm=m[:, :, 0:2], com=m[:, :, 2:4], zmp=m[:, :, 4:6], q=np.stack([r[0] for r in run["readings"]]))
