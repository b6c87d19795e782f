"""The record pass of wcqp_tick_upload_footsteps and wcqp_tick_upload_footsteps_timed past robot 65534, in a process of its own
(tests/test_tick_footsteps_timed.py runs this under a time limit): the robots lie on grid.y, 65535 at most per launch, so robot 65535 is
robot 0 of a second launch whose per-robot rows - the footsteps, the tables and, timed, the duration rows and the start table - the host
advances (plan_gen.hip).

B = 65536 robots, the smallest batch with such a robot, on the smallest handle there is: max_ticks = 1 and an MPC horizon of 1, three
stages per robot.  K = 1, n_steps alternating 0 and 1; every robot stands somewhere else (its feet, its target and its CoM shifted by its
own offset), so rows read from another robot show.  One untimed upload (ss = ds = first_ds = 1) and one timed upload whose durations are
(1, 1) but (1, 2) for robot 65534 and (2, 1) for robot 65535, which is then still on one foot at stage 2.  Robots 0, 65533, 65534 and 65535
are read back (wcqp_tick_get_plan) and compared with helpers/footstep_plan.py and helpers/footstep_plan_timed.py restated for those four
robots alone - contact flags, the fixed frame and hull_nc exact, everything else within 1e-9, the bar of the tests at small batches - and
bit for bit with what a handle of just those four robots generates.  Prints a JSON line with the gaps and the seconds it took."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import walking_controllers_amd as wca  # noqa: E402
from helpers import footstep_plan as fp  # noqa: E402
from helpers import footstep_plan_timed as ft  # noqa: E402
from helpers import planned_tick as pt  # noqa: E402

B, MAXT, N_MPC, SEEDS = 65536, 1, 1, 8
T = MAXT + N_MPC + 1
ROWS = [0, 65533, 65534, 65535]
TOL = 1e-9
WINDOW = (("left_traj", "left_traj"), ("right_traj", "right_traj"), ("left_twist", "left_twist"), ("right_twist", "right_twist"),
          ("com_height", "com_height_traj"), ("com_height_vel", "com_height_vel"), ("ref_traj", "ref_traj"))


def scenario():
    """SEEDS robots of the walk tests repeated over the batch, each copy shifted along x by its own offset; one short step for the odd robots"""
    S = wca.synth
    kb = S.synth_walk_kin_batch(SEEDS)
    fs = S.synth_footstep_walk_batch(SEEDS, MAXT, pt.poses_host(S.icub_like_model(), kb), kb, horizon=N_MPC, n_steps=1)
    rep = lambda a: np.ascontiguousarray(np.tile(a, (B // SEEDS,) + (1,) * (a.ndim - 1)))
    shift = 1e-4 * np.arange(B)
    state0, target, com0 = rep(fs["state0"]), rep(fs["target"]), rep(fs["com0"])
    for col in (0, 12, 24, 36, 66):                       # the actual and the desired soles and the CoM: x
        state0[:, col] += shift
    target[:, 0, 0] += shift
    com0[:, 0] += shift
    n_steps = (np.arange(B) % 2).astype(np.int32)
    data = dict(state0=state0, q0=rep(fs["q0"]), com0=com0)
    steps = dict(n_steps=n_steps, side=rep(fs["side"]), target=target, first_ds_ticks=1, ss_ticks=1, ds_ticks=1, final_ds_ticks=0,
                 lift=fs["lift"], zmp_delta_left=fs["zmp_delta_left"], zmp_delta_right=fs["zmp_delta_right"])
    ss, ds = np.ones((B, 1), np.int32), np.ones((B, 1), np.int32)
    ds[65534], ss[65535] = 2, 2
    return data, steps, dict(steps, ss_ticks=ss, ds_ticks=ds)


def pipe(batch):
    S = wca.synth
    ik = wca.IkSolver(form=wca.IK_FORM_QPOASES, v_max=S.WALK_VMAX, joint_reg_rad=np.deg2rad(S.WALK_POSTURE_DEG))
    return wca.TickPipeline(batch, MAXT, wca.MpcSolver(horizon=N_MPC), ik, kin=wca.KinModel(S.icub_like_model()), planned_trajectories=True,
                            neck_additional_rotation=np.eye(3))


def rows_of(d):
    return {k: (np.ascontiguousarray(v[ROWS]) if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == B else v) for k, v in d.items()}


def main():
    from oracle import hull_spec as hs
    t_start = time.perf_counter()
    data, untimed, timed = scenario()
    big, small = pipe(B), pipe(len(ROWS))
    out = {"batch": B, "stages": T}
    t_made = time.perf_counter()
    for name, steps in (("untimed", untimed), ("timed", timed)):
        big.upload_footsteps(data, steps)
        assert big.info()["plan_timed"] is (name == "timed")
        w = {}
        for i in ROWS:
            for k, v in big.plan_window(robot0=i, n=1).items():
                w.setdefault(k, []).append(v[0])
        w = {k: np.stack(v) for k, v in w.items()}
        d4, s4 = rows_of(data), rows_of(steps)
        plan = (ft.footstep_plan_timed if name == "timed" else fp.footstep_plan)(s4, d4["state0"], T, MAXT)
        # the four robots on a handle of their own: the same kernels, no second launch - bit for bit
        small.upload_footsteps(d4, s4)
        ws = small.plan_window()
        assert set(ws) == set(w)
        for k in ws:
            assert np.array_equal(w[k], ws[k]), (name, k)
        gap = {}
        for j in range(len(ROWS)):
            assert np.array_equal(w["contact"][j], plan["contact"][j]), (name, ROWS[j], w["contact"][j], plan["contact"][j])
            for k, kr in WINDOW:
                gap[k] = max(gap.get(k, 0.0), float(np.abs(w[k][j] - plan[kr][j]).max()))
            pair = plan["contact"][j] & 3
            c = 0
            for t in range(T):
                if 0 < t <= MAXT and pair[t] != pair[t - 1]:
                    c = t
                A, b, nc = hs.hull_from_feet(wca.synth.FOOT_RECT, plan["left_traj"][j, c], plan["right_traj"][j, c], int(pair[c]))
                assert w["hull_nc"][j, t] == nc, (name, ROWS[j], t)
                gap["hull"] = max(gap.get("hull", 0.0), float(np.abs(w["hull_A"][j, t] - A).max()), float(np.abs(w["hull_b"][j, t, :nc] - b[:nc]).max()))
        gap["u_init"] = float(np.abs(w["u_init"] - plan["zmp_ref"][:, 0]).max())
        out[name] = gap
        assert max(gap.values()) <= TOL, (name, gap)
        # what the scenario claims: the stepping robots differ from the standing ones, and each stands at its own offset
        assert (w["contact"][1] & 3)[1] != 3 and (w["contact"][0] & 3).tolist() == [3, 3, 3] and (w["contact"][2] & 3).tolist() == [3, 3, 3]
        assert len({float(x) for x in w["left_traj"][:, 0, 0]}) == len(ROWS)
        if name == "timed":
            assert (w["contact"][3] & 3)[2] != 3 and (w["contact"][1] & 3)[2] == 3
    out["seconds"] = {"handles": t_made - t_start, "all": time.perf_counter() - t_start}
    print(json.dumps(out))
    print("footstep second slab ok")


if __name__ == "__main__":
    main()
