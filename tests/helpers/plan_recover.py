"""wcqp_tick_recover_robots (include/wcqp.h states THE RECOVERED ROBOT) restated: the targets a recover call takes from the plan, in plain
numpy on the dicts TickPipeline.plan_window returns (and on helpers/footstep_plan.py's plans), and THE HOST COMPOSITION the call equals
bit for bit - the yardstick of tests/test_tick_recover.py: download() -> targets -> PrepareSolver.solve_host from the robots' own joints
-> restart_robots for the robots that went on and whose IK ended SOLVED."""
import numpy as np

from helpers import plan_restart as prs

KEEP, ALWAYS, IF_STOPPED = 0, 1, 2
SOLVED = 0
KEPT, NOT_STOPPED, NOT_STANDING = -1, -2, -3


def _height(w):
    return w["com_height"] if "com_height" in w else w["com_height_traj"]


def standing(w, S):
    """[B] bool: stage S has both feet on the ground (bits 0 and 1 of its flags) - a double support or a standing stage"""
    return (np.asarray(w["contact"])[:, int(S)] & 3) == 3


def standing_com(left_d, right_d, height, delta_left, delta_right):
    """com_d [B][3] a recover call derives: x, y the standing ZMP of the soles (helpers/plan_restart.standing_zmp: the midpoint of the two
    feet's ZMP points, each operation rounded on its own), z the given height"""
    B = len(left_d)
    out = np.zeros((B, 3))
    for i in range(B):
        row = np.concatenate([np.zeros(24), left_d[i], right_d[i]])
        out[i, :2] = prs.standing_zmp(row, np.asarray(delta_left, float), np.asarray(delta_right, float))
        out[i, 2] = height[i]
    return out


def targets(w, S, delta_left, delta_right):
    """What a recover call with every target NULL reads from stage S of the plan `w`: left_d, right_d [B][12] (the soles of the stage),
    com_d [B][3] (their standing ZMP at the stage's CoM height) and standing [B] (false: the call reports NOT_STANDING)"""
    S = int(S)
    left, right = np.array(w["left_traj"][:, S], float), np.array(w["right_traj"][:, S], float)
    return dict(left_d=left, right_d=right, com_d=standing_com(left, right, _height(w)[:, S], delta_left, delta_right), standing=standing(w, S))


def compose(pipe, prepare, mode, delta_left, delta_right, left_d=None, right_d=None, com_d=None, Rd_neck=None, q_guess=None, dcm0=None,
            u_init=None):
    """THE HOST COMPOSITION of recover_robots(mode, prepare, ...) on `pipe`, with the synchronisations the call removes.  Returns what
    recover_result() returns for that call."""
    assert (left_d is None) == (right_d is None)
    mode = np.asarray(mode, np.uint8)
    out = pipe.download()
    S, B = int(out["tick"]), len(mode)
    listed = mode != KEEP
    go = listed & ((mode == ALWAYS) | (out["ik_fail"] > 0))
    status = np.where(listed, np.where(go, SOLVED, NOT_STOPPED), KEPT).astype(np.int32)
    w = pipe.plan_window() if left_d is None or com_d is None else None
    if left_d is None:
        t = targets(w, S, delta_left, delta_right)
        left_d, right_d = t["left_d"], t["right_d"]
        status[go & ~t["standing"]] = NOT_STANDING
        go = go & t["standing"]
    if com_d is None:
        rows = np.where(listed[:, None], left_d, 0.0), np.where(listed[:, None], right_d, 0.0)        # (a KEPT robot's rows may hold NaN)
        com_d = standing_com(rows[0], rows[1], _height(w)[:, S], delta_left, delta_right)
    guess = out["q_des"] if q_guess is None else q_guess
    # (the rows of the robots that do not go on are solved too and dropped: a robot's result depends on no other row)
    p = prepare.solve_host(left_d, right_d, com_d, guess, Rd_neck=Rd_neck)
    ran = go[:, None]
    status = np.where(go, p["status"], status).astype(np.int32)
    restart = go & (p["status"] == SOLVED)
    rows = dict(state0=np.where(restart[:, None], p["state"], np.nan), q0=np.where(restart[:, None], p["q"], np.nan),
                com0=np.where(restart[:, None], p["state"][:, 66:68], np.nan), dcm0=dcm0, u_init=u_init)
    pipe.restart_robots(np.where(restart, ALWAYS, KEEP).astype(np.uint8), rows)
    res = pipe.restart_result()
    assert res["stage"] == S and np.array_equal(res["restarted"], restart)
    return dict(restarted=restart, stopped_ticks=np.where(restart, out["ik_fail"], 0).astype(np.int64), status=status,
                iters=np.where(go, p["iters"], 0).astype(np.int32), residual=np.where(ran, p["residual"], 0.0), stage=S)
