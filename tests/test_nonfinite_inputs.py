"""
Non-finite inputs (include/wcqp.h, "Non-finite inputs"): a NaN or an Inf in one robot's inputs never comes back WCQP_STATUS_SOLVED, never
reaches a documented output, and what the robot reports does not depend on its neighbours - who do not notice it, bit for bit.

The MPC case is the one that was wrong: with a NaN in x0 / ref / u_prev every comparison of the hull rows is false for that robot, so when
no wave-mate violated a hull row the wave's early-out handed the robot back SOLVED with u0 = NaN, and when one did, INFEASIBLE.

Neighbours come from synth_mpc_batch / synth_ik_batch: for the MPC the poisoned wave is composed once of robots strictly inside their
hulls (the early-out is taken) and once with robots whose optimum sits on a hull row (the enumeration is taken); the tests assert that the
clean run really has both kinds, so that neither path is skipped silently.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOLVED, NUMERIC, STRUCTURE = 0, 4, 5
POISON = (float("nan"), float("inf"), float("-inf"))
MK = ("x0", "ref", "u_prev", "hull_A", "hull_b", "hull_nc")
IKK = ("J_left", "J_right", "J_neck", "J_com", "q", "state")
N = 50


def _mpc_pools(wca):
    """a pool of synthetic robots, split by what the clean solve does with them: strictly inside (no active row) / on a hull row"""
    pool = wca.synth.synth_mpc_batch(16384, seed=21, uprev_sigma=0.04, horizon=N)
    out = wca.MpcSolver(horizon=N).solve_host(*(pool[k] for k in MK))
    ok = (out["status"] == SOLVED) & (pool["hull_nc"] >= 3) & (pool["hull_nc"] < 8)
    inside, onrow = np.flatnonzero(ok & (out["active"] == 0)), np.flatnonzero(ok & (out["active"] != 0))
    assert len(inside) >= 4096 and len(onrow) >= 64, (len(inside), len(onrow))
    return pool, inside, onrow


def _compose(pool, inside, onrow, B, kind, victim):
    """B robots from the pool: all strictly inside their hulls, or (kind 'enumeration') with a robot on a hull row next to the victim and in
    every second group; the reference window is padded by 4 stages the horizon never reads"""
    idx = inside[:B].copy()
    if kind == "enumeration":
        g0 = victim // 4 * 4
        mates = [i for i in range(g0, min(g0 + 4, B)) if i != victim]
        for n, i in enumerate(mates[:2]):
            idx[i] = onrow[n]
        for g in range(0, B, 8):
            if g // 4 != victim // 4:
                idx[g] = onrow[2 + (g // 8) % 32]
    b = {k: np.array(pool[k][idx], copy=True) for k in MK}
    b["ref"] = np.concatenate([b["ref"], np.repeat(b["ref"][:, -1:, :], 4, axis=1)], axis=1)
    return b


def _placements(B):
    groups = sorted({0, (B // 4) // 2, (B - 1) // 4})
    return [g * 4 + p for g in groups for p in range(4) if g * 4 + p < B]


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 5, 777, 4096])
def test_mpc_poisoned_robot_is_numeric_wherever_it_sits_and_whatever_its_neighbours_do(wca, B):
    pool, inside, onrow = _mpc_pools(wca)
    mpc = wca.MpcSolver(horizon=N)
    sites = [("x0", (0,)), ("x0", (1,)), ("u_prev", (0,)), ("ref", (0, 0)), ("ref", (17, 1)), ("ref", (N, 0)), ("hull_A", (0, 0)), ("hull_A", (1, 1)),
             ("hull_b", (0,)), ("hull_b", (2,))]
    ignored = [("ref", (N + 1, 0)), ("ref", (N + 4, 1)), ("hull_A", "nc"), ("hull_b", "nc")]
    n_checked = 0
    for kind in ("early_out", "enumeration"):
        for victim in _placements(B):
            b = _compose(pool, inside, onrow, B, kind, victim)
            clean = mpc.solve_host(*(b[k] for k in MK))
            g0 = victim // 4 * 4
            wave = np.arange(g0, min(g0 + 4, B))
            assert (clean["status"] == SOLVED).all()
            if B >= 5 and kind == "early_out":
                assert (clean["active"][wave] == 0).all()                    # nobody violates a row: the early-out is taken
            mates = wave[wave != victim]
            if B >= 5 and kind == "enumeration" and len(mates):      # (B = 5: the robot of the ragged group is alone in its wave - its dead slots shadow it)
                assert (clean["active"][mates] != 0).any() and (clean["active"][wave] == 0).any()      # both kinds in the poisoned wave
            others = np.arange(B) != victim
            for n_site, (key, where) in enumerate(sites):
                for val in (POISON if n_site < 4 else (POISON[(n_site + victim) % 3],)):
                    p = {k: b[k].copy() for k in MK}
                    p[key][(victim,) + where] = val
                    got = mpc.solve_host(*(p[k] for k in MK))
                    tag = (B, kind, victim, key, where, val)
                    assert got["status"][victim] == NUMERIC, (tag, got["status"][victim], got["u0"][victim])
                    assert (got["u0"][victim] == 0.0).all() and got["active"][victim] == 0 and got["margin"][victim] == -np.inf, tag
                    for k in ("u0", "status", "active", "margin"):
                        assert np.array_equal(got[k][others], clean[k][others]), (tag, k)
                    assert np.isfinite(got["u0"]).all(), tag
                    n_checked += 1
            nc = int(b["hull_nc"][victim])
            for key, where in ignored:
                w = (nc,) + ((1,) if key == "hull_A" else ()) if where == "nc" else where
                p = {k: b[k].copy() for k in MK}
                p[key][(victim,) + w] = POISON[victim % 3]
                got = mpc.solve_host(*(p[k] for k in MK))
                for k in ("u0", "status", "active", "margin"):
                    assert np.array_equal(got[k], clean[k]), (B, kind, victim, key, w, k)              # never looked at: nothing changes
    assert n_checked >= 2 * len(_placements(B)) * len(sites)


def _ik_solver(wca, alg, form, structure=None):
    kw = dict(form=form, v_max=0.4, algorithm=alg)
    if structure is not None:
        kw["jacobian_structure"] = structure
    return wca.IkSolver(**kw)


# joint columns of the four Jacobians, q, and entries of every block of the pose block: actual and desired foot poses, neck rotations, CoM,
# desired CoM and its velocity, the desired twists
IK_SITES = [("J_left", (0, 6)), ("J_left", (5, 28)), ("J_right", (2, 13)), ("J_neck", (1, 20)), ("J_com", (0, 9)), ("q", (0,)), ("q", (22,)),
            ("state", (1,)), ("state", (7,)), ("state", (13,)), ("state", (25,)), ("state", (40,)), ("state", (50,)), ("state", (60,)), ("state", (67,)),
            ("state", (70,)), ("state", (73,)), ("state", (75,)), ("state", (79,)), ("state", (84,))]


def _ik_site_is_read(form, key, where, state_row):
    """The OSQP form's zero-twist rule (WalkingQPInverseKinematics_osqp.cpp:286-306; oracle/qp_spec.py: ik_task_rhs): a foot whose desired
    twist has twist[0] == twist[1] == 0 gets no pose correction, so that foot's actual and desired pose blocks are not read at all."""
    if form != "osqp" or key != "state":
        return True
    k = where[0]
    left_pose, right_pose = (0 <= k < 12) or (24 <= k < 36), (12 <= k < 24) or (36 <= k < 48)
    if left_pose:
        return not (state_row[75] == state_row[76] == 0.0)
    if right_pose:
        return not (state_row[81] == state_row[82] == 0.0)
    return True


def _ik_pools(wca, ik):
    """a pool of synthetic robots split by what the clean solve does with them: no joint-velocity bound active / some bound active (the
    kernels skip the active-set walk when no robot of the wave needs it: the IK's counterpart of the MPC's early-out)"""
    pool = wca.synth.synth_ik_batch(16384, seed=33)
    out = ik.solve_host(*(pool[k] for k in IKK), want_foot_err=False)
    act = out["active_lower"] | out["active_upper"]
    ok = out["status"] == SOLVED
    return pool, np.flatnonzero(ok & (act == 0)), np.flatnonzero(ok & (act != 0))


def _ik_compose(pool, free, bound, B, kind, victim):
    idx = free[:B].copy()
    if kind == "walk_taken":
        g0 = victim // 4 * 4
        mates = [i for i in range(g0, min(g0 + 4, B)) if i != victim]
        for n, i in enumerate(mates[:2]):
            idx[i] = bound[n]
        for g in range(0, B, 8):
            if g // 4 != victim // 4:
                idx[g] = bound[2 + (g // 8) % 32]
    return {k: np.array(pool[k][idx], copy=True) for k in IKK}


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["qpoases", "osqp"])
@pytest.mark.parametrize("alg", [0, 5, 4, 3])
def test_ik_poisoned_robot_is_numeric_and_its_neighbours_are_untouched(wca, alg, form):
    """Every site with all three poison values at batches 1, 5 and 777, one value per site (rotating) at 4096; the poisoned robot at each
    position of the first, a middle and the last (ragged) group; neighbours without an active bound (no robot of the wave needs the
    active-set walk) and with one (the wave takes it) - the OSQP form has no bounds, so only the first kind exists there."""
    fcode = wca.IK_FORM_QPOASES if form == "qpoases" else wca.IK_FORM_OSQP
    ik = _ik_solver(wca, alg, fcode)
    max_iter = int(ik.params.max_iter) or 100            # (0 -> 100: include/wcqp.h)
    pool, free, bound = _ik_pools(wca, ik)
    assert len(free) >= 4096, len(free)
    kinds = ("walk_skipped", "walk_taken") if form == "qpoases" else ("walk_skipped",)
    if form == "qpoases":
        assert len(bound) >= 64, len(bound)
    else:
        assert len(bound) == 0                               # joint-limit rows are zero rows: never active
    n_unread = n_read_pose = 0
    for B in (1, 5, 777, 4096):
        for kind in kinds:
            for n_v, victim in enumerate(_placements(B)):
                b = _ik_compose(pool, free, bound, B, kind, victim)
                clean = ik.solve_host(*(b[k] for k in IKK), want_foot_err=False)
                act = clean["active_lower"] | clean["active_upper"]
                g0 = victim // 4 * 4
                wave = np.arange(g0, min(g0 + 4, B))
                mates = wave[wave != victim]
                assert (clean["status"] == SOLVED).all()
                if kind == "walk_skipped":
                    assert (act[wave] == 0).all()
                elif len(mates):
                    assert (act[mates] != 0).any() and (act[wave] == 0).any()       # both kinds in the poisoned wave
                others = np.arange(B) != victim
                for n_site, (key, where) in enumerate(IK_SITES):
                    for val in (POISON if B <= 777 else (POISON[(n_site + n_v) % 3],)):
                        p = {k: b[k].copy() for k in IKK}
                        p[key][(victim,) + where] = val
                        got = ik.solve_host(*(p[k] for k in IKK), want_foot_err=False)
                        tag = (alg, form, B, kind, victim, key, where, val)
                        if not _ik_site_is_read(form, key, where, b["state"][victim]):
                            n_unread += 1
                            for k in ("dq", "status", "active_lower", "active_upper", "iters"):
                                assert np.array_equal(got[k], clean[k]), (tag, k)          # never looked at: nothing changes
                            continue
                        n_read_pose += key == "state" and where[0] < 48
                        assert got["status"][victim] == NUMERIC, (tag, got["status"][victim], got["dq"][victim])
                        assert (got["dq"][victim] == 0.0).all() and got["active_lower"][victim] == 0 and got["active_upper"][victim] == 0, tag
                        assert 0 <= got["iters"][victim] <= max_iter, tag
                        assert np.isfinite(got["dq"]).all(), tag
                        for k in ("dq", "status", "active_lower", "active_upper", "iters"):
                            assert np.array_equal(got[k][others], clean[k][others]), (tag, k)
    # both sides of the zero-twist rule were met (OSQP), and nothing was taken for unread otherwise
    assert n_read_pose > 0 and (n_unread > 0 if form == "osqp" else n_unread == 0), (n_read_pose, n_unread)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["qpoases", "osqp"])
def test_ik_non_finite_base_block_keeps_its_documented_meaning(wca, form):
    """STRUCTURE under WCQP_IK_JAC_MIXED; under AUTO the general kernel re-solves the robot, which then ends NUMERIC - dq = 0 either way"""
    fcode = wca.IK_FORM_QPOASES if form == "qpoases" else wca.IK_FORM_OSQP
    B = 37
    b = wca.synth.synth_ik_batch(B, seed=34)
    for structure, want in ((wca.IK_JAC_MIXED, STRUCTURE), (wca.IK_JAC_AUTO, NUMERIC)):
        ik = _ik_solver(wca, 0, fcode, structure)
        clean = ik.solve_host(*(b[k] for k in IKK), want_foot_err=False)
        for victim, (key, where), val in ((0, ("J_left", (0, 0)), POISON[0]), (18, ("J_com", (1, 4)), POISON[1]), (36, ("J_right", (4, 2)), POISON[2]),
                                         (35, ("J_neck", (2, 5)), POISON[0])):
            p = {k: b[k].copy() for k in IKK}
            p[key][(victim,) + where] = val
            got = ik.solve_host(*(p[k] for k in IKK), want_foot_err=False)
            tag = (form, structure, victim, key, val)
            assert got["status"][victim] == want, (tag, got["status"][victim])
            assert (got["dq"][victim] == 0.0).all() and got["active_lower"][victim] == 0 and got["active_upper"][victim] == 0, tag
            others = np.arange(B) != victim
            for k in ("dq", "status", "active_lower", "active_upper"):
                assert np.array_equal(got[k][others], clean[k][others]), (tag, k)


@pytest.mark.gpu
def test_poisoned_records_through_one_launch_routes():
    """single calls, wcqp_qp_enqueue_steps (qp_pair_kernel), a plan with ways = 2 and the work-queue plan, the poisoned record in the middle
    of 7: tests/helpers/nonfinite_check.py, in a process of its own (torch device buffers)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "nonfinite_check.py")], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0 and "nonfinite ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


K_DCM = 1.1          # kDCM of the reactive controller (tests/test_tick_reactive.py)


@pytest.mark.gpu
@pytest.mark.parametrize("site", ["dcm", "com", "zmp", "q"])
@pytest.mark.parametrize("controller", ["mpc", "reactive"])
@pytest.mark.parametrize("kin_mode", [False, True], ids=["constant_jacobians", "fused_kinematics"])
def test_tick_external_feedback_with_a_non_finite_value_stops_that_robot_only(wca, qs, kin_mode, controller, site):
    """EXTERNAL plant, constant Jacobians and fused kinematics, both DCM controllers.  A NaN at tick k (and, another robot, an Inf two
    ticks later) in one robot's feedback: the robot is rejected by the rule of the sensor form - it keeps the measured state of the tick
    before, feedback_fail counts the rejection, ik_fail counts it and every tick the robot runs stopped (the counter the stop rule of the
    IK uses, test_a_robot_whose_ik_fails_is_stopped_like_the_oracle: a stopped robot is a stopped robot, whatever stopped it), dq = 0 from
    tick k on and nothing non-finite is in its state.  Every other robot is bit-identical to the clean run over all ticks, and the whole
    run matches the restatement (oracle/tick_spec.py, with either DCM controller) at the tolerances of the
    existing external-feedback tests (u0, q_des 1e-9; dq 1e-8)."""
    from oracle import tick_spec as ts
    B, T, k_nan, k_inf, r_nan, r_inf = 10, 24, 5, 7, 6, 1
    p = ts.TickParams()
    if kin_mode:
        kin = wca.KinModel(wca.synth.icub_like_model())
        kb = wca.synth.synth_walk_kin_batch(B)
        poses = kin.jacobians_host(kb["base"], kb["q"], state=np.zeros((B, 87)))["state"]
        d = wca.synth.synth_walk_batch(B, T, poses, kb)
        vmax = wca.synth.WALK_VMAX.copy()
        ipar = qs.IKParams(v_max=vmax, joint_reg_deg=wca.synth.WALK_POSTURE_DEG.copy())
        okw = dict(kin_model=wca.synth.icub_like_model(), foot_rect=wca.synth.FOOT_RECT)
        mk_ik = lambda: wca.IkSolver(form=wca.IK_FORM_QPOASES, v_max=vmax, joint_reg_rad=np.deg2rad(wca.synth.WALK_POSTURE_DEG))
    else:
        kin, d = None, wca.synth.synth_tick_batch(B, T)
        ipar, okw = qs.IKParams(v_max=0.45 * np.ones(23)), {}
        mk_ik = lambda: wca.IkSolver(form=wca.IK_FORM_QPOASES, v_max=0.45)
    ckw = dict(dcm_controller="reactive", k_dcm=K_DCM) if controller == "reactive" else {}
    spec = lambda **kw: ts.run_ticks(p, d, T, ipar, dcm_controller=controller, k_dcm=K_DCM, **okw, **kw)
    internal = spec()
    rng = np.random.default_rng(4)
    ext = dict(dcm=internal["dcm_log"] + 1e-3 * rng.normal(size=(T, B, 2)), com=internal["com_log"] + 5e-4 * rng.normal(size=(T, B, 2)),
               zmp=internal["zmp_log"] + 2e-3 * rng.normal(size=(T, B, 2)), q=internal["q_log"] + 0.01 * rng.normal(size=(T, B, 23)))
    bad = {k: v.copy() for k, v in ext.items()}
    bad[site][k_nan, r_nan, 1] = np.nan
    bad[site][k_inf, r_inf, 0] = -np.inf

    def run(e):
        pipe = wca.TickPipeline(B, T, wca.MpcSolver(), mk_ik(), log_ticks=T, kin=kin, external_feedback=True, **ckw)
        pipe.upload(d)
        for t in range(T):
            pipe.set_feedback_host(e["dcm"][t], e["com"][t], e["zmp"][t], e["q"][t])
            pipe.run(1)
        return pipe.download()
    clean, got = run(ext), run(bad)
    assert (clean["feedback_fail"] == 0).all() and clean["ik_fail"].sum() == 0
    want_ff = np.zeros(B, np.int64); want_ff[r_nan] = 1; want_ff[r_inf] = 1
    want_if = np.zeros(B, np.int64); want_if[r_nan] = 1 + (T - k_nan); want_if[r_inf] = 1 + (T - k_inf)
    assert np.array_equal(got["feedback_fail"], want_ff) and np.array_equal(got["ik_fail"], want_if), (got["feedback_fail"], got["ik_fail"])
    assert (got["dq_log"][k_nan:, r_nan] == 0.0).all() and (got["dq_log"][k_inf:, r_inf] == 0.0).all()
    assert np.array_equal(got["dq_log"][:k_nan, r_nan], clean["dq_log"][:k_nan, r_nan])
    for k in ("u0_log", "dq_log", "q_des", "dcm", "com", "measured"):
        assert np.isfinite(got[k]).all(), k
    others = np.ones(B, bool); others[[r_nan, r_inf]] = False
    for k in ("u0_log", "dq_log"):
        assert np.array_equal(got[k][:, others], clean[k][:, others]), k
    for k in ("q_des", "mpc_fail", "ik_fail"):
        assert np.array_equal(got[k][others], clean[k][others]), k
    ref = spec(external=bad)
    assert np.array_equal(ref["feedback_fail"], want_ff) and np.array_equal(ref["ik_fail"], want_if)
    assert np.abs(got["u0_log"] - ref["u0_log"]).max() <= 1e-9 and np.abs(got["dq_log"] - ref["dq_log"]).max() <= 1e-8
    assert np.abs(got["q_des"] - ref["q_des"]).max() <= 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("controller", ["mpc", "reactive"])
def test_tick_upload_and_splice_refuse_non_finite_values(wca, controller):
    """The internal plant (and every other handle): a NaN or an Inf in one robot's uploaded DCM (the MPC's x0), CoM, command, joints or
    reference trajectory is refused by wcqp_tick_upload with WCQP_E_INVALID before anything of the handle changes - the handle keeps the
    upload it had and runs it to the same bits - and wcqp_tick_splice_reference refuses a non-finite tail the same way."""
    B, T = 9, 12
    d = wca.synth.synth_tick_batch(B, T)
    ckw = dict(dcm_controller="reactive", k_dcm=K_DCM) if controller == "reactive" else {}
    mk = lambda: wca.TickPipeline(B, T, wca.MpcSolver(), wca.IkSolver(form=wca.IK_FORM_QPOASES, v_max=0.45), log_ticks=T, **ckw)
    ref_pipe = mk(); ref_pipe.upload(d); ref_pipe.run(T)
    want = ref_pipe.download()
    pipe = mk(); pipe.upload(d)
    n = 0
    for key, where in (("dcm0", (4, 1)), ("com0", (0, 0)), ("u_init", (8, 1)), ("q0", (3, 22)), ("ref_traj", (5, 0, 1)), ("ref_traj", (8, T + 50, 0))):
        for val in POISON:
            p = dict(d); p[key] = np.array(d[key], copy=True); p[key][where] = val
            with pytest.raises(wca.WcqpError, match=r"\(-1\)"):
                pipe.upload(p)
            n += 1
    tail = np.array(d["ref_traj"][:, 6:10], copy=True); tail[2, 1, 0] = np.inf
    with pytest.raises(wca.WcqpError, match=r"\(-1\)"):
        pipe.splice_reference(6, tail)
    pipe.run(T)                                   # still the first upload, untouched
    got = pipe.download()
    assert n == 18
    for k in ("u0_log", "dq_log", "q_des", "dcm", "com", "ik_fail", "mpc_fail"):
        assert np.array_equal(got[k], want[k]), k
