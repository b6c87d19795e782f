"""THE RESET ROBOT of wcqp_tick_reset_robots (include/wcqp.h), restated for tests/test_tick_reset*.py on the scenario of
helpers/resident_plan.py: which robots are reset and where, the rows they are reset to, the plan the call leaves (helpers/plan_restart.py:
a reset robot's plan is THE RESTARTED ROBOT's), the fresh twin a reset robot must equal from stage S on, the fixed feeds both are given,
the per-robot filter reset on helpers/sensor_filters.py, and the run of oracle/tick_spec.py from the reset rows with the robot in the loop."""
import functools

import numpy as np

import robots as robots_
from helpers import plan_restart as prs
from helpers import resident_plan as rs
from helpers import sensor_filters as sf
from helpers import streamed_tick as stt
from helpers import zmp_gains as zg

ROBOTS = (0, 3, 5, 12)        # a walker in a full wave, two wave-mates of the next, and the robot alone in the last wave
STAGES = (41, 64)             # odd and inside the first swing; even, the first stage of a 64-stage tile
B, MAXT, T = rs.B, rs.MAXT, rs.T
KEPT = tuple(i for i in range(B) if i not in ROBOTS)
FILTERS = dict(joint_velocity=10, wrench=10, com=10)
KEEP, ALWAYS, IF_STOPPED = 0, 1, 2
STATE = ("q_des", "ik_fail", "mpc_fail", "feedback_fail", "measured")
LOGS = ("u0_log", "dq_log")


def mode(listed=ROBOTS, how=ALWAYS):
    m = np.full(B, KEEP, np.uint8)
    m[list(listed)] = how
    return m


def zmp_point(sole, delta):
    """p_xy + R_2x2 delta of a sole (p 3 | R 9 row-major): product, product, their sum, then the sum with p - each rounded on its own"""
    out = []
    for ax in range(2):
        r = float(sole[3 + 3 * ax]) * float(delta[0]) + float(sole[4 + 3 * ax]) * float(delta[1])
        out.append(float(sole[ax]) + r)
    return np.array(out)


def standing_zmp(state0_row, delta_left, delta_right):
    """the standing ZMP of the two soles of a state0 row: the midpoint of the two feet's points (what dcm0 / u_init NULL stand for)"""
    zl, zr = zmp_point(state0_row[24:36], delta_left), zmp_point(state0_row[36:48], delta_right)
    return 0.5 * (zl + zr)


def rows(fs, explicit=False, listed=ROBOTS, nan_kept=True):
    """The call's rows: the scenario's own state0 / q0 / com0 of the listed robots - the simulator put them back where they started -
    and NaN in every kept robot's rows (they are never read).  explicit: dcm0 / u_init rows a few millimetres off the standing ZMP, each
    robot its own; else they are absent (NULL)."""
    on = np.isin(np.arange(B), listed)[:, None]
    out = {k: np.where(on, fs[k], np.nan if nan_kept else fs[k]) for k in ("state0", "q0", "com0")}
    if explicit:
        out.update(start_rows(fs, True, listed, nan_kept))
    return out


def start_rows(fs, explicit, listed=ROBOTS, nan_kept=False):
    """dcm0 / u_init [B][2] the reset robots start from: the explicit rows, or what NULL stands for"""
    on = np.isin(np.arange(B), listed)[:, None]
    zmp = np.array([standing_zmp(fs["state0"][i], fs["zmp_delta_left"], fs["zmp_delta_right"]) for i in range(B)])
    if not explicit:
        return dict(dcm0=zmp, u_init=zmp.copy())
    off = 1e-3 * (1.0 + np.arange(B)[:, None] % 4)
    fill = np.nan if nan_kept else zmp
    return dict(dcm0=np.where(on, zmp + off * np.array([1.0, -0.5]), fill), u_init=np.where(on, zmp - off * np.array([0.5, 0.25]), fill))


def reset_plan(w, S, fs, listed=ROBOTS):
    """the plan in force after the call: helpers/plan_restart.restart on the window / plan `w`"""
    return prs.restart(w, listed, S, fs["state0"], fs["zmp_delta_left"], fs["zmp_delta_right"])


def twin_upload(w_after, S, fs, explicit):
    """what the fresh twin is uploaded with: (data, window [S, T)) - the reset's rows for every robot (the kept ones are not compared)"""
    wb = {k: np.ascontiguousarray(v[:, S:]) for k, v in w_after.items() if k != "u_init"}
    d = dict(state0=fs["state0"], q0=fs["q0"], com0=fs["com0"], **start_rows(fs, explicit))
    return d, wb


def plain_feed(fs, n, seed=5):
    """a fixed seeded feed of the plain form, n ticks: the measured state near the start posture (a robot that was put back and stands)"""
    rng = np.random.default_rng(seed)
    z = start_rows(fs, False)["dcm0"]
    return dict(dcm=z + 1.5e-3 * rng.normal(size=(n, B, 2)), com=fs["com0"] + 2e-4 * rng.normal(size=(n, B, 2)),
                zmp=z + 1e-3 * rng.normal(size=(n, B, 2)), q=fs["q0"] + 0.004 * rng.normal(size=(n, B, 23)))


def sensor_feed(fs, n, seed=6):
    """... and of the sensor form: joints near q0, small velocities, both feet loaded with 150 N, each foot's ZMP near its sole origin"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        w = rng.normal(size=(2, B, 6)) * np.array([5.0, 5.0, 2.0, 0.05, 0.05, 0.5])
        w[:, :, 2] += 150.0
        out.append((fs["q0"] + 1e-3 * rng.normal(size=(B, 23)), 2e-3 * rng.normal(size=(B, 23)), w[0], w[1]))
    return out


def bad_force(reading, listed):
    """the reading with zero normal force on both feet of the listed robots: rejected (fz_l + fz_r < 0.1)"""
    q, dq, wl, wr = (np.array(x, copy=True) for x in reading)
    wl[list(listed), 2] = 0.0; wr[list(listed), 2] = 0.0
    return q, dq, wl, wr


class ResetFilters(sf.SensorFilters):
    """helpers/sensor_filters.py with the per-robot reset: reset(i, com0) puts robot i's CoM position filter at com0, its velocity filter
    at 0 and marks the robot fresh - its joint-velocity and wrench filters start AT its next accepted reading, a rejected one leaves it
    fresh.  step() is SensorFilters.step with `first` decided per robot."""

    def __init__(self, B, Ts, com0, **cuts):
        super().__init__(B, Ts, com0, **cuts)
        self.fresh = np.zeros(B, bool)

    def reset(self, i, com0):
        self.com.u[i] = self.com.y[i] = np.asarray(com0, float)[:2]
        self.vel.u[i] = self.vel.y[i] = 0.0
        self.dq.u[i] = self.dq.y[i] = 0.0
        self.w.u[i] = self.w.y[i] = 0.0
        self.fresh[i] = True

    def step(self, model, soles, side, q, dq, wl, wr, omega):
        from oracle import sensor_spec as sn
        q, dq, wl, wr = (np.asarray(x, float) for x in (q, dq, wl, wr))
        meas, rej = np.full((self.B, 6), np.nan), np.zeros(self.B, bool)
        w_raw = np.concatenate([wl[:, sf.W_IDX], wr[:, sf.W_IDX]], 1)
        for i in range(self.B):
            first = (not self.started) or bool(self.fresh[i])
            if not all(np.all(np.isfinite(x[i])) for x in (q, dq, wl, wr)):
                rej[i] = True
                continue
            dq_f = dq[i].copy() if first else self.dq.peek(dq[i], i)
            w_f = w_raw[i].copy() if first else self.w.peek(w_raw[i], i)
            wl_f, wr_f = wl[i].copy(), wr[i].copy()
            wl_f[list(sf.W_IDX)], wr_f[list(sf.W_IDX)] = w_f[:3], w_f[3:]
            r = sn.evaluate(model, q[i], dq_f, wl_f, wr_f, soles[i], side[i], omega)
            if r["rejected"]:
                rej[i] = True
                continue
            self.dq.commit(dq[i], dq_f, i); self.w.commit(w_raw[i], w_f, i)
            com_f, vel_f = self.com.step(r["com"], i), self.vel.step(r["v_com"][:2], i)
            meas[i] = np.concatenate([com_f + vel_f / omega, com_f, r["zmp"]])
            self.fresh[i] = False
        self.started = True
        return meas, rej


def loop_sensors(stages, n, nb, seed=23):
    """helpers/resident_plan.sensor_case's robot in the loop (a closure over that function's own stages and batch, which it does not hand
    out; that file is an existing yardstick and stays as it is) on `stages` [n][nb][..]: readings a robot that tracks its commands reports
    plus seeded noise, wrenches that load the feet in contact and put each loaded foot's ZMP where the previous command is"""
    rng = np.random.default_rng(seed)
    qn, dqn = 1e-3 * rng.normal(size=(n, nb, 23)), 2e-3 * rng.normal(size=(n, nb, 23))
    wn = rng.normal(size=(n, 2, nb, 6)) * np.array([5.0, 5.0, 2.0, 0.05, 0.05, 0.5])

    def sensors(t, q_des, dq_prev, u_prev):
        code = (stages["contact"][t].astype(int) & 3) - 1
        w = []
        for f, pose in enumerate((stages["left_pose"][t], stages["right_pose"][t])):
            loaded = code != 1 - f
            fz = np.where(loaded, np.where(code == 2, 150.0, 300.0) + wn[t, f, :, 2], 0.0)
            R = pose[:, 3:].reshape(nb, 3, 3)
            z = np.einsum("bji,bj->bi", R, np.concatenate([u_prev, np.zeros((nb, 1))], 1) - pose[:, :3])
            wf = wn[t, f].copy()
            wf[:, 2] = fz; wf[:, 3] += z[:, 1] * fz; wf[:, 4] += -z[:, 0] * fz
            w.append(wf)
        return q_des + qn[t], dq_prev + dqn[t], w[0], w[1]
    return sensors


@functools.lru_cache(maxsize=None)
def restated(wca, qs, cfg, S, listed=ROBOTS):
    """oracle/tick_spec.run_ticks for the listed robots alone, started from the reset rows (NULL dcm0 / u_init) on the window [S, T) of
    the scenario's restated plan after the call, MAXT - S ticks, fed the robot-in-the-loop sensors from there.  The run holds `readings`,
    what a handle is fed to reproduce it."""
    from oracle import tick_spec as ts
    controller, gs = rs.CONFIGS[cfg]
    R = robots_.ROBOTS[rs.ROBOT]
    fs, plan, _ = rs.scenario(wca)
    r = list(listed)
    after = reset_plan(plan, S, fs, listed)
    win = {k: v[r][:, S:] for k, v in after.items() if k not in prs.NOT_STAGED}
    n = MAXT - S
    stages = stt.stages_of(win, n)
    start = start_rows(fs, False)
    d = dict(fs, ref_traj=win["ref_traj"], dcm_vel_traj=win["dcm_vel_traj"])
    d = {k: (v[r] if isinstance(v, np.ndarray) and v.shape[:1] == (B,) else v) for k, v in d.items()}
    d.update(ref_traj=win["ref_traj"], dcm_vel_traj=win["dcm_vel_traj"], dcm0=start["dcm0"][r], u_init=start["u_init"][r])
    return ts.run_ticks(ts.TickParams(horizon=50, k_com=R["k_com"], k_zmp=R["k_zmp"]), d, n, rs.ik_params(wca, qs), kin_model=wca.synth.icub_like_model(),
                        foot_rect=wca.synth.FOOT_RECT, stages=stages, neck_additional_rotation=R["additional_rotation"], dcm_controller=controller,
                        k_dcm=rs.K_DCM, dcm_vel=win["dcm_vel_traj"], zmp_gain_schedule=zg.ZMP_SCHEDULE[rs.ROBOT] if gs else None,
                        sensors=loop_sensors(stages, n, len(r)))
