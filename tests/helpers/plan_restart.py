"""The plan wcqp_tick_restart_robots leaves behind (include/wcqp.h states THE RESTARTED ROBOT), restated in plain numpy on the dicts
TickPipeline.plan_window returns - and on any dict of per-stage arrays [B][T][...], helpers/footstep_plan.py's plans among them: a
restarted robot keeps its stages below S and stands from S on, on the soles of its state0 row."""
import numpy as np

NOT_STAGED = ("u_init", "change", "a")      # entries of a window or a restated plan that are not [B][T][...]
HULL = ("hull_A", "hull_b", "hull_nc")      # the rows in force per stage: the tests hold them to the classic rule (oracle/hull_spec.py)
STANDING_FLAGS = 7                          # both feet in contact, the left one the fixed frame


def zmp_point(sole, delta):
    """a foot's ZMP point p_xy + R_2x2 delta of a sole (p 3 | R 9 row-major), each operation rounded on its own"""
    return np.array([sole[0] + (sole[3] * delta[0] + sole[4] * delta[1]), sole[1] + (sole[6] * delta[0] + sole[7] * delta[1])])


def standing_zmp(state0_row, delta_left, delta_right):
    """the ZMP - and DCM reference - of the standing stage: the midpoint of the two feet's points"""
    return 0.5 * (zmp_point(state0_row[24:36], delta_left) + zmp_point(state0_row[36:48], delta_right))


def restart(w, robots, S, state0, delta_left, delta_right):
    """w: the plan in force; robots: those that restart; S: the stage the next tick reads; state0 [B][87].  Returns the plan with every
    stage >= S of those robots the standing stage (the hull rows, where `w` has them, are left out: they are not the restatement's to build)."""
    S = int(S)
    out = {k: np.array(v, copy=True) for k, v in w.items() if k not in HULL}
    dl, dr = np.asarray(delta_left, float), np.asarray(delta_right, float)
    for i in robots:
        st = np.asarray(state0[i], float)
        mid = standing_zmp(st, dl, dr)
        for k, v in out.items():
            if k in NOT_STAGED:
                continue
            if k == "left_traj":
                v[i, S:] = st[24:36]
            elif k == "right_traj":
                v[i, S:] = st[36:48]
            elif k == "contact":
                v[i, S:] = STANDING_FLAGS
            elif k in ("com_height", "com_height_traj"):
                v[i, S:] = st[68]
            elif k in ("ref_traj", "zmp_ref"):
                v[i, S:] = mid
            elif k in ("left_twist", "right_twist", "com_height_vel", "dcm_vel_traj"):
                v[i, S:] = 0.0
            else:
                raise KeyError(k)
    return out
