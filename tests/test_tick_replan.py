"""A running generated walk replanned from new footsteps at a merge stage (wcqp_tick_replan_footsteps).  CPU: the ABI, the
numpy restatement (helpers/footstep_replan.py) and its own properties, the refusals that need no device.  GPU: the replanned plan against
the restatement, the run against the classic upload of the stitched plan and against oracle/tick_spec.py, launch forms, streams, refusals."""
import ctypes as C

import numpy as np
import pytest
from walking_controllers_amd.capi import E_INVALID as WCQP_E_INVALID, E_UNSUPPORTED as WCQP_E_UNSUPPORTED

import robots
from helpers import footstep_plan as fp
from helpers import footstep_replan as fr
from helpers import planned_tick as pt
from helpers import streamed_tick as stt
from helpers import zmp_gains as zg

K_DCM = {"iCubGazeboV2_5": 1.0, "iCubGenova04": 1.0, "icubGazeboSim": 1.5}
KEYS = ("u0_log", "dq_log", "q_des", "dcm", "com")
SAME = KEYS + ("ik_fail", "mpc_fail", "hot_try", "hot_hit", "active_lower", "active_upper", "zmp_gains")
WINDOW = (("left_traj", "left_traj"), ("right_traj", "right_traj"), ("left_twist", "left_twist"), ("right_twist", "right_twist"),
          ("com_height", "com_height_traj"), ("com_height_vel", "com_height_vel"), ("ref_traj", "ref_traj"), ("dcm_vel_traj", "dcm_vel_traj"))
B13, MAXT, T = fr.B13, fr.MAXT, fr.MAXT + 51


def _pipe(wca, B, Tt, robot="iCubGazeboV2_5", controller="mpc", gs=False, horizon=50, planned=True, tpl=0):
    R = robots.ROBOTS[robot]
    ctl = dict(dcm_controller="reactive", k_dcm=K_DCM[robot]) if controller == "reactive" else {}
    sch = dict(zmp_gain_scheduling=True, **zg.ZMP_SCHEDULE[robot]) if gs else {}
    pl = dict(planned_trajectories=True, neck_additional_rotation=np.array(R["additional_rotation"])) if planned else {}
    ik = wca.IkSolver(form=wca.IK_FORM_QPOASES, neck_weight=R["neck_weight"] * np.eye(3), joint_reg_weights=np.array(R["reg_w"], float),
                      joint_reg_gains=np.array(R["reg_k"], float), joint_reg_rad=np.deg2rad(wca.synth.WALK_POSTURE_DEG),
                      v_max=wca.synth.WALK_VMAX.copy(), k_pos_com=R["k_pos_com"], k_pos_foot=R["k_pos_foot"], k_att_foot=R["k_att_foot"],
                      k_neck=R["k_neck"])
    return wca.TickPipeline(B, Tt, wca.MpcSolver(horizon=horizon), ik, log_ticks=Tt, k_com=R["k_com"], k_zmp=R["k_zmp"],
                            kin=wca.KinModel(wca.synth.icub_like_model()), ticks_per_launch=tpl, **ctl, **sch, **pl)


def _same(a, b):
    for k in SAME:
        assert np.array_equal(a[k], b[k]), k


def _same_window(wa, wb, keys=None):
    for k in (keys or wb):
        assert np.array_equal(wa[k], wb[k]), k


def _classic_upload(pipe, d, w):
    e = dict(d, ref_traj=w["ref_traj"])
    pipe.upload(e, dcm_vel_traj=w.get("dcm_vel_traj"), left_traj=w["left_traj"], right_traj=w["right_traj"], left_twist=w["left_twist"],
                right_twist=w["right_twist"], contact=w["contact"], com_height_traj=w.get("com_height", w.get("com_height_traj")),
                com_height_vel=w["com_height_vel"])


def _walk(pipe, fs, reps, ks, **run_kw):
    """upload_footsteps, then run up to each k of `ks` and enqueue the replan that belongs to it, then the rest"""
    pipe.upload_footsteps(fs, fs)
    done = 0
    for k, (M, rp, _) in zip(ks, reps):
        if k > done:
            pipe.run(k - done, **run_kw)
            done = k
        pipe.replan_footsteps(M, rp, rp["first_ds_ticks"], stream=run_kw.get("stream"))
    pipe.run(MAXT - done, **run_kw)


@pytest.fixture(scope="module")
def small(wca):
    fs = fr.small_footsteps(wca, pt)
    plan0, rep1, rep2 = fr.small_replans(fs)
    return fs, plan0, rep1, rep2


# ---------------------------------------------------------------------------------------------------------------- CPU

def test_replan_refuses_a_null_handle(wca):
    """the library exports the entry point, which refuses NULL arguments"""
    lib = wca.capi.lib()
    assert "wcqp_tick_replan_footsteps" in wca.capi.ABI_SYMBOLS and lib.wcqp_tick_replan_footsteps
    assert lib.wcqp_tick_replan_footsteps(None, C.byref(wca.capi.TickReplan()), None) == WCQP_E_INVALID


def test_binding_refusals_without_a_device(wca):
    """What TickPipeline.replan_footsteps refuses before it reaches the library: a handle without planned trajectories, arrays of the wrong shape."""
    pipe = object.__new__(wca.TickPipeline)
    pipe.planned, pipe.batch, pipe._h = False, 3, None
    rp = dict(n_steps=np.zeros(3, np.int32), side=np.zeros((3, 2), np.uint8), target=np.zeros((3, 2, 3)))
    with pytest.raises(ValueError):
        pipe.replan_footsteps(np.full(3, -1), rp, 5)
    pipe.planned = True
    for bad in (dict(rp, n_steps=np.zeros(4, np.int32)), dict(rp, target=np.zeros((3, 2, 2))), dict(rp, side=np.zeros((2, 2), np.uint8))):
        with pytest.raises(AssertionError):
            pipe.replan_footsteps(np.full(3, -1), bad, 5)
    with pytest.raises(AssertionError):
        pipe.replan_footsteps(np.full(4, -1), rp, 5)
    pipe._h = None      # (nothing to destroy)


def test_restatement_properties(small):
    """The stitched plan alone: the recursion residual over it, ref[M] unchanged to 1e-12 (first_ds >= 10 at dT = 0.01), stages below M and
    robots that keep their plan untouched, feet continuous across M, both feet in contact through the first double support."""
    fs, plan0, (M1, rp1, plan1), (M2, rp2, plan2) = small
    omega = np.sqrt(9.81 / 0.53)
    a = np.exp(omega * 0.01)
    assert fr.FD1 >= 10
    for before, M, rp, after in ((plan0, M1, rp1, plan1), (plan1, M2, rp2, plan2)):
        xi, zmp = after["ref_traj"], after["zmp_ref"]
        res = np.abs(xi[:, 1:] - a * xi[:, :-1] - (1.0 - a) * zmp[:, :-1]).max()
        print("recursion residual", res)
        assert res <= 1e-12
        assert np.abs(after["dcm_vel_traj"] - omega * (xi - zmp)).max() <= 1e-12
        for i in range(B13):
            m = int(M[i])
            if m < 0:
                for k in fr.PLAN_KEYS:
                    assert np.array_equal(after[k][i], before[k][i]), (k, i)
                continue
            for k in fr.PLAN_KEYS:
                assert np.array_equal(after[k][i, :m], before[k][i, :m]), (k, i)
            if rp["first_ds_ticks"] >= 10:
                err = np.abs(after["ref_traj"][i, m] - before["ref_traj"][i, m]).max()
                assert err <= 1e-12, (i, err)
            fd = rp["first_ds_ticks"]
            assert np.all(after["contact"][i, m:min(m + fd, T)] & 3 == 3)
            assert np.all(after["contact"][i, m:min(m + fd, T)] & 4 == before["contact"][i, m - 1] & 4)
            for k in ("left_traj", "right_traj"):
                assert np.array_equal(after[k][i, m], before[k][i, m]), (k, i)
        c = after["contact"]
        assert np.all(c & 3) and np.all(np.where(c & 4, c & 1, c & 2))
    # the scenario covers what it claims: a plan cut mid-swing by T, changes of pair past max_ticks, a stop, a foot twice in a row, both yaw signs
    assert (plan1["contact"][7, T - 1] & 3) != 3 and (plan1["contact"][7, 142] & 3) != (plan1["contact"][7, 141] & 3)
    assert rp1["n_steps"][6] == 0 and tuple(rp1["side"][2][:2]) == (0, 0)
    taken = rp1["target"][:, :, 2][(M1[:, None] >= 0) & (rp1["n_steps"][:, None] > np.arange(4)[None, :])]
    assert (taken > 0).any() and (taken < 0).any()


def test_replan_with_the_old_steps_reproduces_the_old_plan(small):
    """M at the first stage of a double support, first_ds = ds, the old remaining steps: the old plan to 1e-12, and the solved `a` is the old
    ramp's start point - the previous stance foot's ZMP point."""
    fs, plan0, _, _ = small
    per = fr.SS + fr.DS
    M = np.full(B13, -1, np.int32); n_new = np.zeros(B13, np.int32)
    side = np.zeros((B13, fr.K), np.uint8); target = np.full((B13, fr.K, 3), 1e3)
    for i in range(B13):
        n = int(fs["n_steps"][i])
        if n < 2:
            continue
        done = 1 + i % (n - 1)                       # steps landed at the merge stage, one at least and not the last
        M[i] = fr.FIRST_DS + (done - 1) * per + fr.SS
        n_new[i] = n - done
        side[i, :n - done] = fs["side"][i, done:n]; target[i, :n - done] = fs["target"][i, done:n]
    assert (M >= 0).sum() >= 8
    rp = dict(n_steps=n_new, side=side, target=target, first_ds_ticks=fr.DS)
    again = fr.footstep_replan(plan0, fs, M, rp, T, MAXT)
    for k in fr.PLAN_KEYS:
        err = np.abs(again[k].astype(float) - plan0[k].astype(float)).max()
        print(k, err)
        assert err <= 1e-12, (k, err)
    assert np.array_equal(again["contact"], plan0["contact"]) and np.array_equal(again["change"], plan0["change"])
    for i in np.nonzero(M >= 0)[0]:
        # the old ramp starts at the ZMP the single support before it held: zmp_ref of stage M - 1
        assert np.abs(again["a"][i] - plan0["zmp_ref"][i, M[i] - 1]).max() <= 1e-10, i


# ---------------------------------------------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def replanned(wca, small):
    """the small scenario on a reactive handle with gain scheduling (keeps dcm_vel): the windows before, after the first and after the second replan"""
    fs, plan0, (M1, rp1, _), (M2, rp2, _) = small
    pipe = _pipe(wca, B13, MAXT, controller="reactive", gs=True)
    pipe.upload_footsteps(fs, fs)
    w0 = pipe.plan_window()
    pipe.replan_footsteps(M1, rp1, rp1["first_ds_ticks"])
    w1 = pipe.plan_window()
    pipe.replan_footsteps(M2, rp2, rp2["first_ds_ticks"])
    return w0, w1, pipe.plan_window()


def _window_matches_the_restatement(wca, before, M, plan, w):
    """the window `w` read after a replan at stages M of the plan read as `before`, against the restatement's stitched `plan`"""
    from oracle import hull_spec as hs
    assert np.array_equal(w["contact"], plan["contact"])
    for k, kr in WINDOW:
        err = np.abs(w[k] - plan[kr]).max()
        print(k, err)
        assert err <= 1e-12, (k, err)
    assert np.array_equal(w["u_init"], before["u_init"])
    for i in range(B13):
        m = T if M[i] < 0 else int(M[i])
        for k in w:
            if k != "u_init":
                assert np.array_equal(w[k][i, :m], before[k][i, :m]), (k, i)
        # the rows in force at every stage: those of the last change of pair <= min(stage, max_ticks), built from THAT stage's feet
        pair = plan["contact"][i] & 3
        c = 0
        for t in range(T):
            if 0 < t <= MAXT and pair[t] != pair[t - 1]:
                c = t
            if t == c or t == T - 1 or t == m:
                A, b, nc = hs.hull_from_feet(wca.synth.FOOT_RECT, plan["left_traj"][i, c], plan["right_traj"][i, c], int(pair[c]))
                assert w["hull_nc"][i, t] == nc, (i, t)
                assert np.abs(w["hull_A"][i, t] - A).max() < 1e-12 and np.abs(w["hull_b"][i, t, :nc] - b[:nc]).max() < 1e-12, (i, t)


@pytest.mark.gpu
def test_replanned_plan_matches_the_restatement(wca, small, replanned):
    """(5) plan_window() of the whole replanned plan against the restatement to 1e-12, hull rows by the classic rule on the stitched plan;
    stages below M_i and robots with -1 bit-identical to the window read before the call."""
    fs, plan0, (M1, rp1, plan1), (M2, rp2, plan2) = small
    w0, w1, w2 = replanned
    for before, M, plan, w in ((w0, M1, plan1, w1), (w1, M2, plan2, w2)):
        _window_matches_the_restatement(wca, before, M, plan, w)


@pytest.mark.gpu
def test_replan_into_a_growing_block(wca, small):
    """The first replan of the small scenario in two calls on one non-blocking stream, the second right behind the first: robot 1 alone,
    then every other robot the scenario replans.  The second call needs a larger block of device memory than the first left behind, while
    the first one's kernels may still be reading it: more robots and tiles, and lists of up to 4 steps where the first call handed over
    robot 1's two (the block's rows are padded to 256 bytes, so at 13 robots it is the wider lists and footprint tables that make it grow:
    13 x 2 x 24 -> 768 and 13 x 3 x 224 -> 8960 bytes, then 13 x 4 x 24 -> 1280 and 13 x 5 x 224 -> 14592).  plan_window() against the
    restatement of the same two calls by the comparison of test_replanned_plan_matches_the_restatement, robots neither call names
    bit-identical to the window read before."""
    fs, plan0, (M1, rp1, plan1), _ = small
    one = 1
    Ma = np.full(B13, -1, np.int32); Ma[one] = M1[one]
    Mb = M1.copy(); Mb[one] = -1
    Ka = int(rp1["n_steps"][one])
    assert Ka < rp1["side"].shape[1] and (Mb >= 0).sum() > 1
    rpa = dict(rp1, n_steps=np.where(Ma >= 0, rp1["n_steps"], 0).astype(np.int32), side=np.ascontiguousarray(rp1["side"][:, :Ka]),
               target=np.ascontiguousarray(rp1["target"][:, :Ka]))
    # CPU first: the restatement of the two calls is that of the one
    plan = fr.footstep_replan(fr.footstep_replan(plan0, fs, Ma, rpa, T, MAXT), fs, Mb, rp1, T, MAXT)
    for k in fr.PLAN_KEYS:
        assert np.array_equal(plan[k], plan1[k]), k
    s = wca.capi.stream_create()
    try:
        pipe = _pipe(wca, B13, MAXT, controller="reactive", gs=True)
        pipe.upload_footsteps(fs, fs)
        w0 = pipe.plan_window()
        pipe.replan_footsteps(Ma, rpa, rpa["first_ds_ticks"], stream=s)
        pipe.replan_footsteps(Mb, rp1, rp1["first_ds_ticks"], stream=s)
        wca.capi.stream_synchronize(s)
        w = pipe.plan_window()
    finally:
        wca.capi.stream_destroy(s)
    _window_matches_the_restatement(wca, w0, M1, plan, w)


@pytest.mark.gpu
@pytest.mark.parametrize("controller,horizon,gs,ks", [("mpc", 50, False, (0, 50)), ("reactive", 200, True, (50, 100))])
def test_run_replan_run_equals_the_classic_upload_of_the_stitched_plan(wca, small, controller, horizon, gs, ks):
    """(6) run(k1), replan, run(k2 - k1), replan, run(rest) on handle A; handle B takes A's final plan_window() through wcqp_tick_upload and
    runs in one go: q_des, dq_log, u0_log, every counter and the plan (hull rows per stage included) are equal bit for bit.
    The reactive controller reads stage t alone, so its replans sit exactly at the boundary M_i = ticks enqueued (robot 2: M = 50 = k1;
    robots 9 and 11: M = 100 = k2).  The MPC of tick t reads ref_traj[t .. t + N]: a one-go run on the stitched plan is the same computation
    only if no window of a tick already run reaches a merge stage, k - 1 + N < min M_i - so its first replan precedes tick 0 and its second
    (min M = 100) follows tick 49.  (At the boundary the ticks M - N .. M - 1 of handle A have seen the OLD stages >= M, as the reference's
    controller has before a merge; the launch-form test holds that case to the other forms.)"""
    fs, _, rep1, rep2 = small
    if controller == "mpc":
        assert all(k == 0 or k - 1 + horizon < int(M[M >= 0].min()) for k, (M, _, _) in zip(ks, (rep1, rep2)))
    else:
        assert ks[0] in rep1[0] and ks[1] in rep2[0]
    a = _pipe(wca, B13, MAXT, controller=controller, gs=gs, horizon=horizon)
    _walk(a, fs, (rep1, rep2), ks)
    wa = a.plan_window()
    b = _pipe(wca, B13, MAXT, controller=controller, gs=gs, horizon=horizon)
    _classic_upload(b, dict(fs, dcm0=wa["ref_traj"][:, 0].copy(), u_init=wa["u_init"]), wa)
    _same_window(wa, b.plan_window())
    b.run(MAXT)
    _same(a.download(), b.download())


@pytest.mark.gpu
@pytest.mark.parametrize("controller", ["mpc", "reactive"])
@pytest.mark.parametrize("robot", robots.NAMES)
def test_closed_loop_against_the_restatement(wca, qs, small, robot, controller):
    """(7) three robots of the small scenario, replanned before tick 0 and run: the device against oracle/tick_spec.py on the stitched stages
    to 1e-9, no robot stopped."""
    from oracle import tick_spec as ts
    fs, _, (M1, rp1, plan1), _ = small
    sel = [4, 5, 7]      # (M = 128 standing, M = 65 just past a tile edge with two steps, M = 100 with three steps cut by T)
    sub = {k: (v[sel] if isinstance(v, np.ndarray) and v.shape[:1] == (B13,) else v) for k, v in fs.items()}
    rp = {k: (v[sel] if isinstance(v, np.ndarray) else v) for k, v in rp1.items()}
    plan = {k: v[sel] for k, v in plan1.items()}
    R = robots.ROBOTS[robot]
    pipe = _pipe(wca, 3, MAXT, robot, controller)
    pipe.upload_footsteps(sub, sub)
    pipe.replan_footsteps(M1[sel], rp, rp["first_ds_ticks"])
    pipe.run(MAXT)
    out = pipe.download()
    ipar = robots.ik_params(qs, robot, v_max=wca.synth.WALK_VMAX.copy())
    ipar.joint_reg_deg = wca.synth.WALK_POSTURE_DEG.copy()
    d = dict(sub, ref_traj=plan["ref_traj"], dcm_vel_traj=plan["dcm_vel_traj"], dcm0=plan["ref_traj"][:, 0].copy(), u_init=plan["zmp_ref"][:, 0].copy())
    ref = ts.run_ticks(ts.TickParams(horizon=50, k_com=R["k_com"], k_zmp=R["k_zmp"]), d, MAXT, ipar, kin_model=wca.synth.icub_like_model(),
                       foot_rect=wca.synth.FOOT_RECT, stages=stt.stages_of(plan, MAXT), neck_additional_rotation=R["additional_rotation"],
                       dcm_controller=controller, k_dcm=K_DCM[robot], dcm_vel=plan["dcm_vel_traj"])
    assert (ref["ik_fail"] == 0).all() and (out["ik_fail"] == 0).all()
    for k in KEYS:
        err = np.abs(out[k] - ref[k]).max()
        print(k, err)
        assert err <= 1e-9, (k, err)
    assert np.array_equal(out["mpc_fail"], ref["mpc_fail"])


@pytest.fixture(scope="module")
def forms(wca, small):
    """(8) the MPC walk with both replans at the boundary region (k1 = 48 <= M = 50, k2 = 96 <= M = 100; 48 and 96 ticks are whole graph
    replays of 8) in every launch form: one launch per call, a launch per tick with and without graphs, 7 ticks per launch"""
    fs, _, rep1, rep2 = small
    outs = []
    for tpl, graph in ((0, True), (1, True), (1, False), (7, True)):
        pipe = _pipe(wca, B13, MAXT, tpl=tpl)
        _walk(pipe, fs, (rep1, rep2), (48, 96), use_graph=graph)
        outs.append((pipe.download(), pipe.plan_window()))
    return outs


@pytest.mark.gpu
def test_launch_forms_agree(forms):
    for out, w in forms[1:]:
        _same(forms[0][0], out)
        _same_window(forms[0][1], w)


@pytest.mark.gpu
def test_replan_on_a_stream_copies_its_arrays_at_the_call(wca, small, forms):
    """(9) everything enqueued on one non-blocking stream, the host arrays overwritten as soon as each replan call returns: the same result"""
    fs, _, rep1, rep2 = small
    s = wca.capi.stream_create()
    try:
        pipe = _pipe(wca, B13, MAXT)
        pipe.upload_footsteps(fs, fs)
        done = 0
        for k, (M, rp, _) in zip((48, 96), (rep1, rep2)):
            pipe.run(k - done, stream=s)
            done = k
            M = M.copy(); rp = {key: (v.copy() if isinstance(v, np.ndarray) else v) for key, v in rp.items()}
            pipe.replan_footsteps(M, rp, rp["first_ds_ticks"], stream=s)
            M[:] = 3; rp["n_steps"][:] = 1; rp["side"][:] = 1; rp["target"][:] = 7.0
        pipe.run(MAXT - done, stream=s)
        wca.capi.stream_synchronize(s)
        _same(forms[0][0], pipe.download())
        _same_window(forms[0][1], pipe.plan_window())
    finally:
        wca.capi.stream_destroy(s)


@pytest.mark.gpu
def test_refusals(wca, small):
    """(10) every refusal; after each one plan_window() is what it was, and the run that follows all of them equals that of a handle that
    never saw the calls."""
    fs, plan0, (M1, rp1, _), _ = small
    lib = wca.capi.lib()

    def call(pipe, M, rp, fd=None, drop=()):
        M = np.ascontiguousarray(M, np.int32); n = np.ascontiguousarray(rp["n_steps"], np.int32)
        side = np.ascontiguousarray(rp["side"], np.uint8); tg = np.ascontiguousarray(rp["target"], float)
        f = dict(merge_stage=M.ctypes.data, max_steps=side.shape[1], n_steps=n.ctypes.data, side=side.ctypes.data, target=tg.ctypes.data,
                 first_ds_ticks=rp["first_ds_ticks"] if fd is None else fd)
        return lib.wcqp_tick_replan_footsteps(pipe._h, C.byref(wca.capi.TickReplan(**{k: v for k, v in f.items() if k not in drop})), None)

    plain = _pipe(wca, B13, MAXT, planned=False)
    assert call(plain, M1, rp1) == WCQP_E_UNSUPPORTED
    fresh = _pipe(wca, B13, MAXT)
    assert call(fresh, M1, rp1) == WCQP_E_INVALID                      # not uploaded
    classic = _pipe(wca, B13, MAXT)
    _classic_upload(classic, dict(fs, dcm0=plan0["ref_traj"][:, 0].copy(), u_init=plan0["zmp_ref"][:, 0].copy()), plan0)
    assert call(classic, M1, rp1) == WCQP_E_UNSUPPORTED               # a plan that was not generated

    pipe, twin = _pipe(wca, B13, MAXT), _pipe(wca, B13, MAXT)
    for p_ in (pipe, twin):
        p_.upload_footsteps(fs, fs)
        p_.run(52)
        p_.replan_footsteps(M1 * (M1 != 50) - (M1 == 50), rp1, rp1["first_ds_ticks"])      # (robot 2's M = 50 < 52 ticks: it keeps its plan here)
    w_ref = twin.plan_window()

    def arr(key, idx, val):
        e = dict(rp1); e[key] = np.array(rp1[key], copy=True); e[key][idx] = val
        return e

    def merge(i, m):
        M = np.full(B13, -1, np.int32); M[i] = m
        return M
    later = merge(0, 120)
    bad = [(later, rp1, None, ("merge_stage",)), (later, rp1, None, ("n_steps",)), (later, rp1, None, ("side",)), (later, rp1, None, ("target",)),
           (later, rp1, 0, ()), (later, rp1, -3, ()),
           (merge(3, 120), arr("n_steps", 3, 5), None, ()), (merge(3, 120), arr("n_steps", 3, -1), None, ()),
           (merge(3, 120), arr("side", (3, 1), 2), None, ()), (merge(3, 120), arr("target", (3, 2, 0), np.nan), None, ()),
           (merge(3, 120), arr("target", (3, 0, 2), np.inf), None, ()),
           (merge(0, 0), rp1, None, ()), (merge(0, -2), rp1, None, ()), (merge(0, 51), rp1, None, ()),      # 51 < the 52 ticks enqueued
           (merge(0, T), rp1, None, ()), (merge(0, T + 40), rp1, None, ()),
           (merge(1, 59), rp1, None, ()),                                  # below robot 1's previous merge stage (60)
           (merge(1, 80), rp1, None, ()),                                  # robot 1's new plan: 60 + 12 .. 102 is a single support
           (merge(2, 75), rp1, None, ())]                                  # robot 2 kept its plan: 70 .. 100 is a single support
    for M, rp, fd, drop in bad:
        assert call(pipe, M, rp, fd, drop) == WCQP_E_INVALID, (M, fd, drop)
        _same_window(pipe.plan_window(), w_ref)
    assert lib.wcqp_tick_replan_footsteps(pipe._h, None, None) == WCQP_E_INVALID
    # (a robot that keeps its plan: none of its rows is read - its n_steps may hold anything)
    ok = arr("n_steps", 0, 99)
    assert call(pipe, merge(3, 120), ok) == 0 and call(twin, merge(3, 120), rp1) == 0
    pipe.run(MAXT - 52); twin.run(MAXT - 52)
    _same(pipe.download(), twin.download())
    _same_window(pipe.plan_window(), twin.plan_window())
