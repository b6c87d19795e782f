"""Planned walks generated on the device from per-robot footstep lists (wcqp_tick_upload_footsteps / wcqp_tick_get_plan).
CPU: the numpy restatement of the plan (helpers/footstep_plan.py) against synth_planned_walk_batch, the ABI.  GPU: the generated plan
against the restatement, its own properties, the classic upload fed the same plan, the closed loop against oracle/tick_spec.py."""
import ctypes as C

import numpy as np
import pytest
from walking_controllers_amd.capi import E_INVALID as WCQP_E_INVALID, E_UNSUPPORTED as WCQP_E_UNSUPPORTED

import robots
from helpers import footstep_plan as fp
from helpers import planned_tick as pt
from helpers import streamed_tick as stt
from helpers import zmp_gains as zg

K_DCM = {"iCubGazeboV2_5": 1.0, "iCubGenova04": 1.0, "icubGazeboSim": 1.5}
KEYS = ("u0_log", "dq_log", "q_des", "dcm", "com")
SAME = KEYS + ("ik_fail", "mpc_fail", "hot_try", "hot_hit", "active_lower", "active_upper", "zmp_gains")
PLAN = ("left_traj", "right_traj", "left_twist", "right_twist", "contact", "com_height_traj", "com_height_vel")
WALK_T = 880
# the small scenario: 13 robots (not a multiple of the 4 robots per wave of the tick, nor of the 32 per block of the DCM pass), T = 186 stages
# (no multiple of the 64-stage tile of the record pass nor of the 32-stage tile of the DCM pass); steps of 30 + 20 stages behind 20
B13, MAXT, FIRST_DS, SS, DS, K = 13, 135, 20, 30, 20, 4


def _walk_inputs(wca, B):
    model = wca.synth.icub_like_model()
    kb = wca.synth.synth_walk_kin_batch(B)
    return model, kb, pt.poses_host(model, kb)


def _ik_params(wca, qs, robot):
    ipar = robots.ik_params(qs, robot, v_max=wca.synth.WALK_VMAX.copy())
    ipar.joint_reg_deg = wca.synth.WALK_POSTURE_DEG.copy()
    return ipar


def _pipe(wca, B, T, robot="iCubGazeboV2_5", controller="mpc", gs=False, horizon=50, planned=True, tpl=0, first=0):
    R = robots.ROBOTS[robot]
    ctl = dict(dcm_controller="reactive", k_dcm=K_DCM[robot]) if controller == "reactive" else {}
    sch = dict(zmp_gain_scheduling=True, **zg.ZMP_SCHEDULE[robot]) if gs else {}
    pl = dict(planned_trajectories=True, neck_additional_rotation=np.array(R["additional_rotation"])) if planned else {}
    ik = wca.IkSolver(form=wca.IK_FORM_QPOASES, neck_weight=R["neck_weight"] * np.eye(3), joint_reg_weights=np.array(R["reg_w"], float),
                      joint_reg_gains=np.array(R["reg_k"], float), joint_reg_rad=np.deg2rad(wca.synth.WALK_POSTURE_DEG),
                      v_max=wca.synth.WALK_VMAX.copy(), k_pos_com=R["k_pos_com"], k_pos_foot=R["k_pos_foot"], k_att_foot=R["k_att_foot"],
                      k_neck=R["k_neck"])
    return wca.TickPipeline(B, T, wca.MpcSolver(horizon=horizon), ik, first=first, log_ticks=T, k_com=R["k_com"], k_zmp=R["k_zmp"],
                            kin=wca.KinModel(wca.synth.icub_like_model()), ticks_per_launch=tpl, **ctl, **sch, **pl)


def _same(a, b):
    for k in SAME:
        assert np.array_equal(a[k], b[k]), k


def _classic_upload(pipe, d, w):
    """wcqp_tick_upload with the arrays of a plan window (plan_window() of another handle, or the restatement's)"""
    e = dict(d, ref_traj=w["ref_traj"])
    pipe.upload(e, dcm_vel_traj=w.get("dcm_vel_traj"), left_traj=w["left_traj"], right_traj=w["right_traj"], left_twist=w["left_twist"],
                right_twist=w["right_twist"], contact=w["contact"], com_height_traj=w.get("com_height", w.get("com_height_traj")),
                com_height_vel=w["com_height_vel"])


@pytest.fixture(scope="module")
def small(wca):
    """13 robots: 0 steps, K steps, the same foot twice in a row, yaw increments of both signs, plans that end inside T, a plan cut
    mid-swing by T (4 steps: the last swing is stages 170..199 of 186) and changes of contact pair after max_ticks (stages 150, 170)."""
    _, kb, poses = _walk_inputs(wca, B13)
    fs = wca.synth.synth_footstep_walk_batch(B13, MAXT, poses, kb)
    rng = np.random.default_rng(5)
    n_steps = np.array([0, 4, 4, 2, 1, 3, 4, 0, 2, 4, 3, 1, 4], np.int32)
    side = np.tile(np.array([1, 0, 1, 0], np.uint8), (B13, 1))
    side[2] = (1, 1, 0, 0); side[5] = (0, 0, 0, 1); side[9] = (0, 1, 1, 0)
    target = np.zeros((B13, K, 3))
    st = fs["state0"]
    for i in range(B13):
        p = [st[i, 24:26].copy(), st[i, 36:38].copy()]
        yaw = [np.arctan2(st[i, 33], st[i, 27]), np.arctan2(st[i, 45], st[i, 39])]
        for k in range(K):
            sw = side[i, k]
            inc = rng.uniform(0.02, 0.06) * (1.0 if (i + k) % 3 else -1.0)
            yaw[sw] += inc
            p[sw] = p[sw] + rng.uniform(0.015, 0.03) * np.array([np.cos(yaw[sw]), np.sin(yaw[sw])])
            target[i, k] = (p[sw][0], p[sw][1], inc)
    target[n_steps[:, None] <= np.arange(K)[None, :]] = 1e3        # (steps a robot does not take are not read)
    fs.update(n_steps=n_steps, side=side, target=target, first_ds_ticks=FIRST_DS, ss_ticks=SS, ds_ticks=DS, final_ds_ticks=0, lift=0.02)
    T = MAXT + 51
    plan = fp.footstep_plan(fs, fs["state0"], T, MAXT)
    assert {int(n) for n in n_steps} == {0, 1, 2, 3, 4} and (target[:, :, 2][n_steps[:, None] > np.arange(K)] > 0).any() and (target[..., 2] < 0).any()
    return fs, plan, T


# ---------------------------------------------------------------------------------------------------------------- CPU

def test_restatement_reproduces_the_planned_walk(wca):
    """The restatement fed synth_footstep_walk_batch reproduces synth_planned_walk_batch: feet, twists, contact and - on the stages < T - the
    DCM reference, its velocity and the ZMP plan to 1e-12.  (The two recursions start from different terminal conditions - xi = zmp at the
    first standing stage here, at the last stage of the generator's extended plan there - 720 stages or more past T: the two differ by
    less than 1e-4 there, and the backward recursion damps that by exp(-omega dT) = 0.958 per stage, to below 1e-17 at T.)"""
    B, T_ticks = 3, WALK_T
    _, kb, poses = _walk_inputs(wca, B)
    kw = dict(yaw_step=(0.03, 0.08))
    d = wca.synth.synth_planned_walk_batch(B, T_ticks, poses, kb, **kw)
    fs = wca.synth.synth_footstep_walk_batch(B, T_ticks, poses, kb, **kw)
    T = T_ticks + 51
    assert fs["final_ds_ticks"] == (T + 4 * 180) - (110 + 3 * 180 + 70)
    assert np.array_equal(fs["state0"], d["state0"]) and np.array_equal(fs["q0"], d["q0"]) and np.array_equal(fs["com0"], d["com0"])
    plan = fp.footstep_plan(fs, fs["state0"], T, T_ticks)
    assert np.array_equal(plan["contact"], d["contact"])
    for k in ("left_traj", "right_traj", "left_twist", "right_twist", "ref_traj", "dcm_vel_traj", "zmp_ref"):
        err = np.abs(plan[k] - d[k]).max()
        print(k, err)
        assert err <= 1e-12, (k, err)
    assert np.exp(-np.sqrt(9.81 / 0.53) * 0.01 * 720) * 1e-4 < 1e-17


# ---------------------------------------------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def generated(wca, small):
    """the small scenario generated on a reactive handle with gain scheduling (keeps dcm_vel), horizon 50: (handle, its whole plan)"""
    fs, plan, T = small
    pipe = _pipe(wca, B13, MAXT, controller="reactive", gs=True)
    pipe.upload_footsteps(fs, fs)
    return pipe, pipe.plan_window()


@pytest.mark.gpu
def test_generated_plan_matches_the_restatement(wca, small, generated):
    from oracle import hull_spec as hs
    fs, plan, T = small
    _, w = generated
    assert w["contact"].shape == (B13, T) and np.array_equal(w["contact"], plan["contact"])
    for k, kr in (("left_traj", "left_traj"), ("right_traj", "right_traj"), ("left_twist", "left_twist"), ("right_twist", "right_twist"),
                  ("com_height", "com_height_traj"), ("com_height_vel", "com_height_vel"), ("ref_traj", "ref_traj"), ("dcm_vel_traj", "dcm_vel_traj")):
        err = np.abs(w[k] - plan[kr]).max()
        print(k, err)
        assert err <= 1e-12, (k, err)
    assert np.abs(w["u_init"] - plan["zmp_ref"][:, 0]).max() <= 1e-12
    # hull rows: at every stage the rows of the last change of contact pair a tick can reach, built from THAT stage's feet
    changes = set()
    for i in range(B13):
        c = int(plan["change"][i])
        changes.add(c > 0)
        A, b, nc = hs.hull_from_feet(wca.synth.FOOT_RECT, plan["left_traj"][i, c], plan["right_traj"][i, c], int(plan["contact"][i, c]) & 3)
        for t in (c, T - 1):
            assert w["hull_nc"][i, t] == nc
            assert np.abs(w["hull_A"][i, t] - A).max() < 1e-12 and np.abs(w["hull_b"][i, t, :nc] - b[:nc]).max() < 1e-12 and (w["hull_b"][i, t, nc:] == 1e30).all()
        if c > 0:       # ... and the stage before still names the set before
            assert not (np.array_equal(w["hull_A"][i, c - 1], w["hull_A"][i, c]) and np.array_equal(w["hull_b"][i, c - 1], w["hull_b"][i, c]))
    assert changes == {False, True}
    # a contact change after max_ticks changes no rows
    i = 1
    assert (plan["contact"][i, 150] & 3) != (plan["contact"][i, 149] & 3) and np.array_equal(w["hull_A"][i, 149], w["hull_A"][i, 150])


@pytest.mark.gpu
def test_generated_plan_properties(wca, small, generated):
    """Properties of the downloaded plan alone."""
    fs, _, T = small
    _, w = generated
    dT, omega = 0.01, np.sqrt(9.81 / 0.53)
    a = np.exp(omega * dT)
    xi = w["ref_traj"]
    zmp = xi - w["dcm_vel_traj"] / omega
    res = np.abs(xi[:, 1:] - a * xi[:, :-1] - (1.0 - a) * zmp[:, :-1]).max()
    print("recursion residual", res)
    assert res <= 1e-12
    for i in range(B13):
        n = int(fs["n_steps"][i])
        s_end = FIRST_DS + n * (SS + DS) if n else FIRST_DS
        if s_end < T:
            assert np.array_equal(w["dcm_vel_traj"][i, s_end:], np.zeros((T - s_end, 2))), i
            assert np.all(xi[i, s_end:] == xi[i, s_end])
    for f, (tr, tw) in enumerate(((w["left_traj"], w["left_twist"]), (w["right_traj"], w["right_twist"]))):
        # the tolerances of test_generator_is_self_consistent (trapezoid: O(dT^2))
        dp = (tr[:, 1:, :3] - tr[:, :-1, :3]) / dT
        err = np.abs(dp - 0.5 * (tw[:, 1:, :3] + tw[:, :-1, :3])).max()
        print("twist vs difference", err)
        assert err < 2e-3
        yaw = np.unwrap(np.arctan2(tr[..., 6], tr[..., 3]), axis=1)
        assert np.abs((yaw[:, 1:] - yaw[:, :-1]) / dT - 0.5 * (tw[:, 1:, 5] + tw[:, :-1, 5])).max() < 2e-2
        moving = np.abs(tw).max(-1) > 0
        assert not np.any(moving & (w["contact"] & (1 << f) > 0)), "a foot in contact does not move"
        Rm = tr[..., 3:].reshape(B13, T, 3, 3)
        assert np.abs(np.einsum("btij,btkj->btik", Rm, Rm) - np.eye(3)).max() <= 1e-14
    c = w["contact"]
    assert np.all(c & 3) and np.all(np.where(c & 4, c & 1, c & 2))


@pytest.mark.gpu
@pytest.mark.parametrize("controller,horizon,gs", [("mpc", 50, False), ("reactive", 200, True)])
def test_classic_upload_of_the_generated_plan_is_identical(wca, small, controller, horizon, gs):
    """Handle A takes upload_footsteps, handle B wcqp_tick_upload with A's whole plan_window(): the plans are equal bit for bit, hull rows
    included, and so is every output after the run."""
    fs, _, _ = small
    a = _pipe(wca, B13, MAXT, controller=controller, gs=gs, horizon=horizon)
    a.upload_footsteps(fs, fs)
    wa = a.plan_window()
    b = _pipe(wca, B13, MAXT, controller=controller, gs=gs, horizon=horizon)
    d = dict(fs, dcm0=wa["ref_traj"][:, 0].copy(), u_init=wa["u_init"])
    _classic_upload(b, d, wa)
    wb = b.plan_window()
    assert ("dcm_vel_traj" in wa) == (controller == "reactive") and "u_init" not in wb
    for k in wb:
        assert np.array_equal(wa[k], wb[k]), k
    a.run(MAXT); b.run(MAXT)
    _same(a.download(), b.download())


@pytest.mark.gpu
def test_plan_window_of_a_classic_upload(wca, small):
    """plan_window() on a classically uploaded handle returns the uploaded arrays bit for bit (a sub-window with robot0 > 0, stage0 > 0)."""
    fs, plan, T = small
    pipe = _pipe(wca, B13, MAXT, controller="reactive")
    d = dict(fs, dcm0=plan["ref_traj"][:, 0].copy(), u_init=plan["zmp_ref"][:, 0].copy())
    _classic_upload(pipe, d, plan)
    r0, n, s0, m = 3, 7, 11, 150
    w = pipe.plan_window(r0, n, s0, m)
    for k, kr in (("left_traj", "left_traj"), ("right_traj", "right_traj"), ("left_twist", "left_twist"), ("right_twist", "right_twist"),
                  ("contact", "contact"), ("com_height", "com_height_traj"), ("com_height_vel", "com_height_vel"), ("ref_traj", "ref_traj"),
                  ("dcm_vel_traj", "dcm_vel_traj")):
        assert np.array_equal(w[k], plan[kr][r0:r0 + n, s0:s0 + m]), k
    lib = wca.capi.lib()
    win = wca.capi.TickPlanWindow()
    for bad in ((-1, 2, 0, 5), (0, B13 + 1, 0, 5), (12, 2, 0, 5), (0, 2, T - 4, 5), (0, 2, -1, 5), (0, 0, 0, 5), (0, 2, 0, 0)):
        assert lib.wcqp_tick_get_plan(pipe._h, *bad, C.byref(win)) == WCQP_E_INVALID, bad
    u0 = np.zeros((B13, 2))
    assert lib.wcqp_tick_get_plan(pipe._h, 0, B13, 0, 1, C.byref(wca.capi.TickPlanWindow(u_init=u0.ctypes.data))) == WCQP_E_UNSUPPORTED
    mpc = _pipe(wca, B13, MAXT)
    mpc.upload_footsteps(fs, fs)
    v = np.zeros((B13, 1, 2))
    assert lib.wcqp_tick_get_plan(mpc._h, 0, B13, 0, 1, C.byref(wca.capi.TickPlanWindow(dcm_vel_traj=v.ctypes.data))) == WCQP_E_UNSUPPORTED


@pytest.fixture(scope="module")
def turning_walk(wca):
    """the 4-step turning walk of test_tick_planned.py as footsteps, and its restatement"""
    _, kb, poses = _walk_inputs(wca, 3)
    fs = wca.synth.synth_footstep_walk_batch(3, WALK_T, poses, kb, yaw_step=(0.03, 0.08))
    plan = fp.footstep_plan(fs, fs["state0"], WALK_T + 51, WALK_T)
    return fs, plan


@pytest.mark.gpu
@pytest.mark.parametrize("controller", ["mpc", "reactive"])
@pytest.mark.parametrize("robot", robots.NAMES)
def test_closed_loop_against_the_restatement(wca, qs, turning_walk, robot, controller):
    """upload_footsteps, run: the device against oracle/tick_spec.py on the restatement's stages to 1e-9; dcm0 / u_init NULL equals the
    generated stage-0 values passed explicitly, bit for bit."""
    from oracle import tick_spec as ts
    fs, plan = turning_walk
    T = WALK_T
    R = robots.ROBOTS[robot]
    pipe = _pipe(wca, 3, T, robot, controller)
    pipe.upload_footsteps(fs, fs)
    w = pipe.plan_window(stage0=0, m=1)
    pipe.run(T)
    out = pipe.download()
    d = dict(fs, ref_traj=plan["ref_traj"], dcm_vel_traj=plan["dcm_vel_traj"], dcm0=plan["ref_traj"][:, 0].copy(), u_init=plan["zmp_ref"][:, 0].copy())
    ref = ts.run_ticks(ts.TickParams(horizon=50, k_com=R["k_com"], k_zmp=R["k_zmp"]), d, T, _ik_params(wca, qs, robot),
                       kin_model=wca.synth.icub_like_model(), foot_rect=wca.synth.FOOT_RECT, stages=stt.stages_of(plan, T),
                       neck_additional_rotation=R["additional_rotation"], dcm_controller=controller, k_dcm=K_DCM[robot], dcm_vel=plan["dcm_vel_traj"])
    assert (ref["ik_fail"] == 0).all()
    for k in KEYS:
        err = np.abs(out[k] - ref[k]).max()
        print(k, err)
        assert err <= 1e-9, (k, err)
    assert np.array_equal(out["mpc_fail"], ref["mpc_fail"]) and np.array_equal(out["ik_fail"], ref["ik_fail"])
    explicit = _pipe(wca, 3, T, robot, controller)
    explicit.upload_footsteps(dict(fs, dcm0=w["ref_traj"][:, 0].copy(), u_init=w["u_init"]), fs)
    explicit.run(T)
    _same(out, explicit.download())


@pytest.mark.gpu
def test_launch_forms_agree(wca, small):
    """ticks_per_launch 0 / 1 / 7 agree bit for bit; two shards (first) agree with the whole batch; a second upload_footsteps with another
    plan gives what a fresh handle gives."""
    fs, _, _ = small
    outs, pipes = [], []
    for tpl in (0, 1, 7):
        pipe = _pipe(wca, B13, MAXT, tpl=tpl)
        pipe.upload_footsteps(fs, fs)
        pipe.run(MAXT)
        outs.append(pipe.download()); pipes.append(pipe)
    _same(outs[0], outs[1]); _same(outs[0], outs[2])
    parts = []
    for lo, hi in ((0, 5), (5, B13)):
        sub = {k: (v[lo:hi] if isinstance(v, np.ndarray) and v.shape[:1] == (B13,) else v) for k, v in fs.items()}
        pipe = _pipe(wca, hi - lo, MAXT, first=lo)
        pipe.upload_footsteps(sub, sub)
        pipe.run(MAXT)
        parts.append(pipe.download())
    for k in ("q_des", "dcm", "com"):
        assert np.array_equal(np.concatenate([p_[k] for p_ in parts]), outs[0][k]), k
    for k in ("u0_log", "dq_log"):
        assert np.array_equal(np.concatenate([p_[k] for p_ in parts], axis=1), outs[0][k]), k
    # another plan into a used handle: fewer steps, other timings
    other = dict(fs, n_steps=np.minimum(fs["n_steps"], 2), first_ds_ticks=15, ss_ticks=33, ds_ticks=12, final_ds_ticks=40, lift=0.03)
    pipes[0].upload_footsteps(other, other)
    pipes[0].run(MAXT)
    fresh = _pipe(wca, B13, MAXT)
    fresh.upload_footsteps(other, other)
    fresh.run(MAXT)
    _same(pipes[0].download(), fresh.download())
    wa, wb = pipes[0].plan_window(), fresh.plan_window()
    for k in wa:
        assert np.array_equal(wa[k], wb[k]), k


@pytest.mark.gpu
def test_refusals(wca, small):
    fs, _, _ = small
    _, kb, poses = _walk_inputs(wca, B13)
    plain = _pipe(wca, B13, MAXT, planned=False)
    ins, st = wca.capi.TickInputs(), wca.capi.TickFootsteps()
    assert wca.capi.lib().wcqp_tick_upload_footsteps(plain._h, C.byref(ins), C.byref(st)) == WCQP_E_UNSUPPORTED
    assert wca.capi.lib().wcqp_tick_get_plan(plain._h, 0, 1, 0, 1, C.byref(wca.capi.TickPlanWindow())) == WCQP_E_UNSUPPORTED
    pipe = _pipe(wca, B13, MAXT)
    pipe.upload_footsteps(fs, fs)
    pipe.run(60)

    def arr(key, idx, val):
        e = dict(fs); e[key] = np.array(fs[key], copy=True); e[key][idx] = val
        return e
    bad = [arr("n_steps", 3, K + 1), arr("n_steps", 0, -1), arr("side", (1, 2), 2), arr("target", (1, 3, 0), np.nan), arr("target", (6, 0, 2), np.inf),
           arr("state0", (4, 30), np.nan), arr("state0", (4, 68), np.inf), arr("q0", (2, 5), np.nan), arr("com0", (0, 1), np.nan),
           dict(fs, dcm0=np.full((B13, 2), np.nan)), dict(fs, u_init=np.full((B13, 2), np.inf)), dict(fs, lift=np.nan),
           dict(fs, zmp_delta_left=(np.nan, 0.0)), dict(fs, zmp_delta_right=(0.0, np.inf)), dict(fs, first_ds_ticks=0), dict(fs, ss_ticks=0),
           dict(fs, ds_ticks=0), dict(fs, final_ds_ticks=-1)]
    for e in bad:
        with pytest.raises(wca.WcqpError, match="invalid|INVALID"):
            pipe.upload_footsteps(e, e)
    # NULL required pointers
    lib = wca.capi.lib()
    n_steps, side, target = np.ascontiguousarray(fs["n_steps"]), np.ascontiguousarray(fs["side"]), np.ascontiguousarray(fs["target"])
    base = dict(state0=fs["state0"].ctypes.data, q0=fs["q0"].ctypes.data, com0=fs["com0"].ctypes.data)
    sbase = dict(max_steps=K, n_steps=n_steps.ctypes.data, side=side.ctypes.data, target=target.ctypes.data, first_ds_ticks=FIRST_DS, ss_ticks=SS,
                 ds_ticks=DS, lift=0.02)
    for drop in ("state0", "q0", "com0"):
        ins = wca.capi.TickInputs(**{k: v for k, v in base.items() if k != drop})
        assert lib.wcqp_tick_upload_footsteps(pipe._h, C.byref(ins), C.byref(wca.capi.TickFootsteps(**sbase))) == WCQP_E_INVALID, drop
    for drop in ("n_steps", "side", "target"):
        st = wca.capi.TickFootsteps(**{k: v for k, v in sbase.items() if k != drop})
        assert lib.wcqp_tick_upload_footsteps(pipe._h, C.byref(wca.capi.TickInputs(**base)), C.byref(st)) == WCQP_E_INVALID, drop
    assert lib.wcqp_tick_upload_footsteps(pipe._h, C.byref(wca.capi.TickInputs(**base)), None) == WCQP_E_INVALID
    # the checks ran before the handle changed: the previous upload runs on, as on a fresh handle
    pipe.run(MAXT - 60)
    fresh = _pipe(wca, B13, MAXT)
    fresh.upload_footsteps(fs, fs)
    fresh.run(MAXT)
    _same(pipe.download(), fresh.download())
