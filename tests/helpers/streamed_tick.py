"""CPU restatement of the closed-loop tick with streamed trajectories (wcqp_tick_params.streamed_trajectories): the loop of
planned_tick.run_ticks_planned with the plant replaced the way oracle/tick_spec.py::run_ticks(external=...) replaces it - tick t reads its
measured DCM, CoM, ZMP and (optionally) joint positions from `external` = dict(dcm, com, zmp [T][B][2], q [T][B][23] or absent) - and
the desired stage of tick t read from per-tick arrays, `stages`:

  left_pose, right_pose [T][B][12]   left_twist, right_twist [T][B][6]   contact [T][B] uint8
  com_height, com_height_vel [T][B] or absent (state0[68], 0)

(stage-major: what the caller hands over tick by tick; stages_of turns the planned arrays [B][T][..] into it, and concatenating two
walks' stages along the first axis is a replanned walk).  Run WITHOUT `external` it is the internal plant, and then also returns the plant
state at the start of every tick (dcm_log, com_log, zmp_log, q_log), as run_ticks does: feeding those back as `external` reproduces the run.

Built from the pieces the other restatements are built from: planned_tick.neck_orientation, tick_spec's qs / ks / hs / disturbance, the
solve called as tick_spec.qs.mpc_exact and the gains read as p.k_com / p.k_zmp at the time of use in the order `for t: for i`, so that
reactive_tick.reactive_solve and zmp_gains.scheduled_gains apply unchanged; sensor_feedback.evaluate gives the measured state of the sensor
form (sensor_measured).  splices {t: (from, tail [B][n][2])}: the DCM reference's merge, as run_ticks applies it."""
import numpy as np

from oracle import tick_spec

from . import planned_tick as pt
from . import sensor_feedback as sf

qs, ks, hs = tick_spec.qs, tick_spec.ks, tick_spec.hs
IDENT = sf.IDENT
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


def stage_side(flags):
    """0: the left sole is the fixed frame"""
    return np.where(np.asarray(flags).astype(np.int64) & 4, 0, 1)


def run_ticks_streamed(p, data, stages, n_ticks, ik_params, kin_model, foot_rect, add_rot, external=None, splices=None, ik_form="qpoases",
                       sensors=None):
    """sensors(t, q_des, dq_prev, u_prev) -> (q_meas, dq_meas, wrench_left, wrench_right): a robot in the loop - tick t's measured state is
    what the sensor form evaluates from these readings (sensor_measured), which may depend on what the run did up to tick t - 1.  The run
    then also returns the readings (`readings`, a list of the four arrays per tick) and what was evaluated (`measured_log` [T][B][6]):
    fed back as fixed arrays - external_of_sensors - they reproduce the run."""
    B = data["q0"].shape[0]
    N = p.horizon
    data = dict(data)
    data["ref_traj"] = np.array(data["ref_traj"], float, copy=True)
    mp = qs.MPCParams(horizon=N, sampling_time=p.dT, com_height=p.com_height, gravity=p.gravity)
    c = qs.mpc_constants(mp)
    omega = np.sqrt(p.gravity / p.com_height)
    inst = np.arange(B, dtype=np.uint64) + np.uint64(data.get("first", 0))
    dcm = data["dcm0"].copy(); com = data["com0"].copy(); zmp_meas = data["u_init"].copy()
    u_prev = data["u_init"].copy()
    c_ref = data["com0"].copy(); v_ref_prev = np.zeros((B, 2))
    p_star = data["com0"].copy(); v_star_prev = np.zeros((B, 2))
    q_des = data["q0"].copy(); dq_prev = np.zeros((B, 23))
    u0_log = np.zeros((n_ticks, B, 2)); dq_log = np.zeros((n_ticks, B, 23))
    dcm_log = np.zeros((n_ticks, B, 2)); com_log = np.zeros((n_ticks, B, 2)); zmp_log = np.zeros((n_ticks, B, 2)); q_log = np.zeros((n_ticks, B, 23))
    mpc_fail = np.zeros(B, np.int64); ik_fail = np.zeros(B, np.int64)
    state_now = data["state0"].copy()
    hull_cur = [None] * B; hull_code = -np.ones(B, np.int64)
    J_now = [None] * B
    h_traj = stages.get("com_height"); h_vel = stages.get("com_height_vel")
    readings, measured_log = [], np.zeros((n_ticks, B, 6))
    assert external is None or sensors is None
    for t in range(n_ticks):
        if splices and t in splices:
            frm, tail = splices[t]
            assert frm >= t
            data["ref_traj"][:, frm:frm + tail.shape[1]] = tail
        flags = np.asarray(stages["contact"])[t].astype(np.int64)
        code = (flags & 3) - 1
        if external is not None:
            dcm = np.array(external["dcm"][t], float); com = np.array(external["com"][t], float); zmp_meas = np.array(external["zmp"][t], float)
        q_ik = np.array(external["q"][t], float) if (external is not None and external.get("q") is not None) else q_des
        if sensors is not None:
            r = [np.array(x, float) for x in sensors(t, q_des.copy(), dq_prev.copy(), u_prev.copy())]
            m, rej = sensor_measured(kin_model, stages, t, *r, omega)
            assert not rej.any(), ("a rejected reading", t)
            dcm, com, zmp_meas, q_ik = m[:, 0:2].copy(), m[:, 2:4].copy(), m[:, 4:6].copy(), r[0]
            readings.append(r); measured_log[t] = m
        dcm_log[t] = dcm; com_log[t] = com; zmp_log[t] = zmp_meas; q_log[t] = q_des
        for i in range(B):
            s = state_now[i]
            s[24:36] = stages["left_pose"][t, i]; s[36:48] = stages["right_pose"][t, i]
            s[57:66] = pt.neck_orientation(s[27:36], s[39:48], add_rot).reshape(9)
            side = 0 if flags[i] & 4 else 1
            base = sf.anchored_base(kin_model, q_des[i], s[36:48] if side else s[24:36], side)
            K = ks.jacobians(kin_model, base, q_des[i])
            J_now[i] = K
            s[0:3] = K["p_left"]; s[3:12] = K["R_left"].reshape(9); s[12:15] = K["p_right"]; s[15:24] = K["R_right"].reshape(9)
            s[48:57] = K["R_neck"].reshape(9); s[66:69] = K["com"]
            if int(code[i]) != hull_code[i]:
                k = int(code[i])
                hull_cur[i] = hs.hull_from_feet(foot_rect, s[24:36], s[36:48], {0: 1, 1: 2, 2: 3}[k])
                hull_code[i] = k
        r_t = data["ref_traj"][:, t, :]
        v_ref = -omega * (c_ref - r_t)
        c_ref = c_ref + 0.5 * p.dT * (v_ref + v_ref_prev); v_ref_prev = v_ref
        u0 = np.zeros((B, 2))
        for i in range(B):
            hA, hb, nc = hull_cur[i]
            try:
                u0[i] = tick_spec.qs.mpc_exact(c, dcm[i], data["ref_traj"][i, t:t + N + 1], u_prev[i], hA, hb, nc)["u0"]
            except qs.QPOracleError:
                u0[i] = u_prev[i]; mpc_fail[i] += 1
        v_star = p.k_com * (c_ref - com) - p.k_zmp * (u0 - zmp_meas) + v_ref
        p_star = p_star + 0.5 * p.dT * (v_star + v_star_prev); v_star_prev = v_star
        dq = np.zeros((B, 23))
        for i in range(B):
            s = state_now[i].copy()
            s[69:71] = p_star[i]
            s[71] = h_traj[t, i] if h_traj is not None else data["state0"][i][68]
            s[72:74] = v_star[i]
            s[74] = h_vel[t, i] if h_vel is not None else 0.0
            s[75:81] = stages["left_twist"][t, i]; s[81:87] = stages["right_twist"][t, i]
            one = dict(q=q_ik[i:i + 1], state=s[None, :], **{n: J_now[i][n][None] for n in ("J_left", "J_right", "J_neck", "J_com")})
            if ik_fail[i] > 0:
                ik_fail[i] += 1
                continue
            try:
                dq[i] = qs.ik_exact(ik_params, qs.ik_inputs_from_batch(one, 0), ik_form)["dq"]
            except qs.QPOracleError:
                ik_fail[i] += 1
        q_des = q_des + 0.5 * p.dT * (dq + dq_prev); dq_prev = dq
        w = np.stack([tick_spec.disturbance(p.seed, inst, t, 0), tick_spec.disturbance(p.seed, inst, t, 1)], 1)
        com = com + p.dT * (-omega * (com - dcm))
        dcm = c.a * dcm + c.b * u0 + p.noise * w
        zmp_meas = u0.copy(); u_prev = u0.copy()
        u0_log[t] = u0; dq_log[t] = dq
    return dict(u0_log=u0_log, dq_log=dq_log, q_des=q_des, dcm=dcm, com=com, mpc_fail=mpc_fail, ik_fail=ik_fail,
                dcm_log=dcm_log, com_log=com_log, zmp_log=zmp_log, q_log=q_log, readings=readings, measured_log=measured_log)


def external_of(run):
    """the plant states an internal run returned, as the `external` dict of the next run (q: None - the desired joints)"""
    return dict(dcm=run["dcm_log"], com=run["com_log"], zmp=run["zmp_log"])


def external_of_sensors(run):
    """the measured states and joints a run with `sensors` evaluated, as the `external` dict of the next run"""
    m = run["measured_log"]
    return dict(dcm=m[:, :, 0:2], com=m[:, :, 2:4], zmp=m[:, :, 4:6], q=np.stack([r[0] for r in run["readings"]]))


def sensor_measured(model, stages, t, q, dq, wl, wr, omega):
    """What the sensor form evaluates on tick t of a streamed handle: measured [B][6] (dcm, com, zmp xy; NaN where rejected), rejected [B] -
    sensor_feedback.evaluate with the stage's fixed-frame side and that sole's desired pose."""
    B = len(q)
    side = stage_side(stages["contact"][t])
    meas = np.full((B, 6), np.nan)
    rej = np.zeros(B, bool)
    for i in range(B):
        sole = (stages["right_pose"] if side[i] else stages["left_pose"])[t, i]
        r = sf.evaluate(model, q[i], dq[i], wl[i], wr[i], sole, side[i], omega)
        rej[i] = r["rejected"]
        if not rej[i]:
            meas[i] = np.concatenate([r["dcm"], r["com"], r["zmp"]])
    return meas, rej
