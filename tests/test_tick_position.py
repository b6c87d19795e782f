"""The POSITION mode of the closed-loop tick: the non-linear IK every tick (wcqp_tick_params.ik_mode = WCQP_TICK_IK_POSITION).
CPU: the restatement (helpers/position_tick.py) walks three robots of the scenario - every tick SOLVED within the budget, independent of the
start, certified optima at four ticks, a cut joint limit respected - the ABI, and the refusals of wcqp_tick_create that need no device.
GPU: the kernel against the restatement for both controllers, the chain against the velocity handle's, the soles against the plan by the
stand-alone kinematics, the launch forms, limits, robots that are not solved beside robots that are, a replan."""
import ctypes as C

import numpy as np
import pytest
from walking_controllers_amd.capi import E_INVALID as WCQP_E_INVALID, E_UNSUPPORTED as WCQP_E_UNSUPPORTED

import robots
import trees
from helpers import footstep_replan as fr
from helpers import position_tick as pk
from helpers import prepare_spec as ps

B13, T = pk.B13, pk.T
CHAIN_KEYS = ("u0_log", "dcm", "com", "zmp_gains")


def _ik(wca):
    R = robots.ROBOTS[pk.ROBOT]
    return wca.IkSolver(form=wca.IK_FORM_QPOASES, neck_weight=R["neck_weight"] * np.eye(3), joint_reg_weights=np.array(R["reg_w"], float),
                        joint_reg_gains=np.array(R["reg_k"], float), joint_reg_rad=np.deg2rad(wca.synth.WALK_POSTURE_DEG),
                        v_max=wca.synth.WALK_VMAX.copy(), k_pos_com=R["k_pos_com"], k_pos_foot=R["k_pos_foot"], k_att_foot=R["k_att_foot"], k_neck=R["k_neck"])


def _pipe(wca, controller="mpc", position=True, tpl=0, B=B13, max_iter=30, tree="icub", **pik):
    """tree: the scenario's tree (helpers/position_tick.tree_of); the velocity IK's parameters of _ik are in the iCub numbering - a POSITION
    handle on another tree takes only its dof from them"""
    assert position or tree == "icub"
    R = robots.ROBOTS[pk.ROBOT]
    mode = dict(ik_mode="position", position_ik=dict(q_reg=pk.scenario(tree)["q_reg"], max_iter=max_iter, **pik)) if position else {}
    return wca.TickPipeline(B, T, wca.MpcSolver(horizon=pk.N, com_height=pk.H), _ik(wca), log_ticks=T, k_com=R["k_com"], k_zmp=R["k_zmp"],
                            kin=wca.KinModel(pk.scenario(tree)["model"]), planned_trajectories=True, neck_additional_rotation=pk.ADD_ROT,
                            ticks_per_launch=tpl, **pk.controller_kwargs(controller), **mode)


def _run(pipe, fs=None, calls=(T,), **run_kw):
    fs = pk.scenario()["fs"] if fs is None else fs
    pipe.upload_footsteps(fs, fs)
    for n in calls:
        pipe.run(n, **run_kw)
    return pipe.download()


def _same(a, b, rows=None):
    assert set(a) == set(b)
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if rows is not None and x.ndim >= 1 and B13 in x.shape:
            ax = x.shape.index(B13)
            x, y = np.take(x, rows, ax), np.take(y, rows, ax)
        assert np.array_equal(x, y), k


# ---------------------------------------------------------------------------------------------------------------- CPU

def test_restatement_walk_is_solved_on_every_tick():
    """three robots, 70 ticks, no limits: every robot-tick SOLVED within the budget of 30 iterations, the joints move far less than the
    step cap from tick to tick"""
    for i, r in pk.reference("mpc").items():
        w = r["walk"]
        move = np.abs(np.diff(w["q_log"], axis=0)).max()
        print(i, "iters", w["iters"].min(), w["iters"].max(), "largest move per tick", move)
        assert (w["status"] == ps.SOLVED).all() and w["ik_fail"] == 0
        assert (w["iters"] >= 1).all() and (w["iters"] <= 30).all()
        assert move < 0.3
        assert r["chain"]["mpc_fail"] == 0


def test_restatement_walk_does_not_depend_on_its_start():
    """every tick's joints are the optimum of that tick's problem: a walk whose start is perturbed by 1e-3 rad agrees to 1e-11 on every tick"""
    rng = np.random.default_rng(11)
    sc = pk.scenario()
    for i, r in pk.reference("mpc").items():
        w2 = pk.walk(r["chain"], sc["fs"]["q0"][i] + rng.uniform(-1e-3, 1e-3, 23), pk.params())
        err = np.abs(w2["q_log"] - r["walk"]["q_log"]).max()
        print(i, err)
        assert (w2["status"] == ps.SOLVED).all() and err <= 1e-11


@pytest.mark.parametrize("t", [0, 20, 35, 69])
def test_restatement_ticks_pass_the_certificate(t):
    """the certificate of prepare_spec at tick 0, mid-swing (20), the switch of the support foot (35) and the last tick, with the thresholds
    of tests/test_prepare.py: constraints to 1e-10, stationarity to 1e-9, multiplier signs, every joint inside"""
    for i, r in pk.reference("mpc").items():
        ch = r["chain"]
        c = ps.certificate(pk.sc_model(), r["walk"]["q_log"][t], pk.targets(ch["plan"], ch["p_star"], t), pk.params())
        print(i, t, c)
        assert c["constraint"] <= 1e-10 and c["stationarity"] <= 1e-9 and c["mult_ok"] and c["inside"]


def test_restatement_respects_the_joint_17_cut():
    """joint 17's upper limit a quarter of its range below its maximum (each robot's own range: helpers/position_tick.py says why): the joint
    stays inside exactly, the cut is active on at least 5 ticks of every robot, every tick is SOLVED within the budget"""
    for i, w in pk.reference_cut().items():
        lo, hi = pk.cut_limits(i)
        on = int((w["q_log"][:, pk.CUT_JOINT] == hi[pk.CUT_JOINT]).sum())
        print(i, "iters", w["iters"].max(), "ticks on the cut", on, "q0 outside", bool(pk.scenario()["fs"]["q0"][i][pk.CUT_JOINT] > hi[pk.CUT_JOINT]))
        assert (w["status"] == ps.SOLVED).all() and (w["iters"] <= 30).all()
        assert (w["q_log"] <= hi).all() and (w["q_log"] >= lo).all()
        assert on >= 5
        assert all(pk.CUT_JOINT in (a or {}) for a, q in zip(w["active"], w["q_log"]) if q[pk.CUT_JOINT] == hi[pk.CUT_JOINT])


def test_abi_layout_and_symbols(wca):
    """the mode's fields ARE the last ones of their structs (test_abi_host.py compares every offset and size with the header); position_ik is
    a whole wcqp_prepare_params; the version stays 400; the entry points a POSITION handle uses are exported"""
    cp = wca.capi
    assert [k for k, _ in cp.TickParams._fields_][-2:] == ["ik_mode", "position_ik"]
    assert [k for k, _ in cp.TickOutputs._fields_][-2:] == ["q_log", "ik_iters"] and cp.TickInfo._fields_[-1][0] == "ik_mode"
    assert cp.TickParams.position_ik.size == C.sizeof(cp.PrepareParams)
    assert cp.VERSION == 400
    lib = cp.lib()
    for sym in ("wcqp_tick_create", "wcqp_tick_run", "wcqp_tick_download", "wcqp_tick_get_info", "wcqp_tick_upload_footsteps",
                "wcqp_tick_replan_footsteps", "wcqp_tick_get_plan"):
        assert sym in cp.ABI_SYMBOLS and getattr(lib, sym)


def _params(wca, **kw):
    """the wcqp_tick_params of a valid POSITION handle of three robots, with fields replaced; -> (params, what it points to)"""
    cp = wca.capi
    pipe = object.__new__(wca.TickPipeline)          # (the constructor would create the handle: only its parameter block is wanted)
    R = robots.ROBOTS[pk.ROBOT]
    q_reg = np.ascontiguousarray(pk.scenario()["q_reg"])
    p = cp.TickParams(3, 0, T, T, 180, 110, R["k_com"], R["k_zmp"], 1e-4, 99, wca.MpcSolver(horizon=pk.N, com_height=pk.H).params, _ik(wca).params, 0, 1,
                      wca.KinModel(pk.scenario()["model"]).params, (C.c_double * 8)(*np.asarray(wca.synth.FOOT_RECT, float).reshape(8)))
    p.planned_trajectories = 1
    p.neck_additional_rotation = (C.c_double * 9)(*np.eye(3).reshape(9))
    p.ik_mode = cp.TICK_IK_POSITION
    p.position_ik = cp.PrepareParams(0.5, 1.0, 0.3, 1e-12, 1e-10, 30, q_reg.ctypes.data, None, None)
    keep = [q_reg, pipe]
    for k, v in kw.items():
        if k.startswith("pik_"):
            if isinstance(v, np.ndarray):
                keep.append(v)
                v = v.ctypes.data
            setattr(p.position_ik, k[4:], v)
        elif k == "ik_algorithm":
            p.ik.algorithm = v
        else:
            setattr(p, k, v)
    return p, keep


def test_create_refusals_need_no_device(wca):
    """every refusal of wcqp_tick_create the mode adds, answered before anything touches the device (this test runs without one): an
    unknown mode and every position_ik value wcqp_prepare_create refuses are WCQP_E_INVALID; POSITION without planned trajectories, with
    the EXTERNAL plant, streamed stages, logger rows or another IK algorithm is WCQP_E_UNSUPPORTED"""
    lib = wca.capi.lib()

    def create(**kw):
        p, keep = _params(wca, **kw)
        h = C.c_void_p()
        rc = lib.wcqp_tick_create(C.byref(p), C.byref(h))
        if rc == 0:
            lib.wcqp_tick_destroy(h)
        return rc

    assert create(ik_mode=2) == WCQP_E_INVALID and create(ik_mode=-1) == WCQP_E_INVALID
    for bad in (np.nan, np.inf, -1.0):
        for k in ("w_q", "w_n", "step_cap", "tol_step", "tol_constraint"):
            assert create(**{"pik_" + k: bad}) == WCQP_E_INVALID, (k, bad)
    assert create(pik_w_q=0.0) == WCQP_E_INVALID and create(pik_step_cap=0.0) == WCQP_E_INVALID
    assert create(pik_max_iter=0) == WCQP_E_INVALID and create(pik_max_iter=-3) == WCQP_E_INVALID
    assert create(pik_q_reg=None) == WCQP_E_INVALID
    nan_reg = pk.scenario()["q_reg"].copy(); nan_reg[22] = np.nan
    assert create(pik_q_reg=nan_reg) == WCQP_E_INVALID
    lo, hi = -np.ones(23), np.ones(23)
    assert create(pik_q_min=lo) == WCQP_E_INVALID and create(pik_q_max=hi) == WCQP_E_INVALID
    crossed = hi.copy(); crossed[7] = -2.0
    assert create(pik_q_min=lo, pik_q_max=crossed) == WCQP_E_INVALID
    nan_lim = hi.copy(); nan_lim[3] = np.nan
    assert create(pik_q_min=lo, pik_q_max=nan_lim) == WCQP_E_INVALID
    assert create(planned_trajectories=0) == WCQP_E_UNSUPPORTED
    assert create(plant=1) == WCQP_E_UNSUPPORTED
    assert create(planned_trajectories=0, plant=1, streamed_trajectories=1) == WCQP_E_UNSUPPORTED
    assert create(streamed_trajectories=1) == WCQP_E_UNSUPPORTED
    assert create(logger_ticks=4) == WCQP_E_UNSUPPORTED
    assert create(ik_algorithm=wca.IK_ALG_NULLSPACE_16L) == WCQP_E_UNSUPPORTED
    # the refusals of planned trajectories apply unchanged: another hand-off, no kinematics
    assert create(kin_handoff=wca.KIN_HANDOFF_DENSE) == WCQP_E_UNSUPPORTED and create(use_kinematics=0) == WCQP_E_UNSUPPORTED


def test_binding_refusals(wca):
    """what TickPipeline refuses before it reaches the library"""
    mk = lambda **kw: wca.TickPipeline(3, T, wca.MpcSolver(horizon=pk.N), _ik(wca), kin=wca.KinModel(pk.scenario()["model"]), **kw)
    pl = dict(planned_trajectories=True, neck_additional_rotation=np.eye(3))
    with pytest.raises(ValueError):
        mk(ik_mode="positions", **pl)
    with pytest.raises(ValueError):
        mk(ik_mode="position", position_ik=dict(w_q=0.5), **pl)                                  # no q_reg
    with pytest.raises(ValueError):
        mk(ik_mode="position", position_ik=dict(q_reg=np.zeros(23), tolerance=1e-4), **pl)       # an unknown key
    with pytest.raises(ValueError):
        mk(ik_mode="position", position_ik=dict(q_reg=np.zeros(23)))                             # not a planned handle
    with pytest.raises(ValueError):
        mk(position_ik=dict(q_reg=np.zeros(23)), **pl)                                           # parameters without the mode


# ---------------------------------------------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def device(wca):
    """the scenario on the device, once per controller: one launch for the 70 ticks"""
    out = {}
    for c in pk.CONTROLLERS:
        pipe = _pipe(wca, c)
        out[c] = _run(pipe)
        out[c + "/info"] = pipe.info()
        pipe.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("controller", pk.CONTROLLERS)
def test_parity_with_the_restatement(device, controller):
    """(1) q_log of robots 0, 5 and 12 to 1e-9 on every tick; u0_log, dcm, com and zmp_gains to 1e-9; tick == T, no failure of either
    solver, between T and 30 T iterations per robot"""
    _parity(device[controller], device[controller + "/info"], controller, pk.reference(controller))


@pytest.mark.gpu
def test_parity_with_the_restatement_on_a_regauged_tree_numbered_legs_first(wca):
    """the same check, MPC controller, on icub_gauged_legs_first (tests/trees.py): the same robot with general R0, axes and frame rotations
    and the torso's subtree across the two slots of the 16-lane walk; the restatement walks the same table (two of its three robots)."""
    tree = "icub_gauged_legs_first"
    assert trees.check_claims(tree)["handoff"] == "fused"
    pipe = _pipe(wca, "mpc", tree=tree)
    o = _run(pipe, fs=pk.scenario(tree)["fs"])
    info = pipe.info()
    pipe.close()
    _parity(o, info, "mpc", pk.reference("mpc", tree, sel=pk.SEL[1:]))        # a robot of the second wave and the last one


def _parity(o, info, controller, reference):
    assert info["ik_mode"] == "position" and "dq_log" not in o
    assert o["tick"] == T and not o["ik_fail"].any() and not o["mpc_fail"].any()
    assert (o["ik_iters"] >= T).all() and (o["ik_iters"] <= 30 * T).all()
    assert not o["hot_try"].any() and not o["hot_hit"].any()
    for i, r in reference.items():
        assert (r["walk"]["status"] == ps.SOLVED).all()
        err = np.abs(o["q_log"][:, i] - r["walk"]["q_log"]).max()
        print(controller, i, "q_log", err, "iters", int(o["ik_iters"][i]), "restatement", int(r["walk"]["iters"].sum()))
        assert err <= 1e-9
        assert np.abs(o["q_des"][i] - r["walk"]["q_log"][-1]).max() <= 1e-9
        for k in CHAIN_KEYS:
            got = o[k][:, i] if k == "u0_log" else o[k][i]
            e = np.abs(got - r["chain"][k]).max()
            print(controller, i, k, e)
            assert e <= 1e-9, (k, e)


@pytest.mark.gpu
@pytest.mark.parametrize("controller", pk.CONTROLLERS)
def test_chain_does_not_notice_the_mode(wca, device, controller):
    """(2) a velocity handle on the same plan: u0_log, dcm, com and zmp_gains agree to 1e-12 (not bit for bit: the chain's functions are
    inlined into another kernel, where contraction may differ)"""
    v = _run(_pipe(wca, controller, position=False))
    assert v["tick"] == T
    for k in CHAIN_KEYS:
        err = np.abs(v[k] - device[controller][k]).max()
        print(controller, k, err)
        assert err <= 1e-12, (k, err)


@pytest.mark.gpu
def test_soles_sit_on_the_plan(wca, device):
    """(3) knows no restatement: at q_log[t] with the left sole anchored on stage t's pose, the stand-alone kinematics put the right sole on
    stage t's pose and the CoM at stage t's height, to 1e-9 - all 13 robots, every tick"""
    pipe = _pipe(wca, "mpc")
    fs = pk.scenario()["fs"]
    pipe.upload_footsteps(fs, fs)
    w = pipe.plan_window(stage0=0, m=T)
    pipe.close()
    kin = wca.KinModel(pk.scenario()["model"])
    q = device["mpc"]["q_log"]                                   # [T][B][23]
    qf = np.ascontiguousarray(q.reshape(T * B13, 23))
    ident = np.tile(np.concatenate([np.zeros(3), np.eye(3).reshape(9)]), (T * B13, 1))
    k0 = kin.jacobians_host(ident, qf, state=np.zeros((T * B13, 87)))["state"]      # the soles in the base frame
    left = np.swapaxes(w["left_traj"], 0, 1).reshape(T * B13, 12)
    pL, RL = k0[:, 0:3], k0[:, 3:12].reshape(-1, 3, 3)
    Rb = left[:, 3:12].reshape(-1, 3, 3) @ np.swapaxes(RL, 1, 2)
    base = np.concatenate([left[:, :3] - np.einsum("bij,bj->bi", Rb, pL), Rb.reshape(-1, 9)], axis=1)
    k = kin.jacobians_host(np.ascontiguousarray(base), qf, state=np.zeros((T * B13, 87)))["state"]
    right = np.swapaxes(w["right_traj"], 0, 1).reshape(T * B13, 12)
    height = np.swapaxes(w["com_height"], 0, 1).reshape(T * B13)
    e_left = np.abs(k[:, 0:12] - left).max()
    e_right = np.abs(k[:, 12:24] - right).max()
    e_h = np.abs(k[:, 68] - height).max()
    print("left sole", e_left, "right sole", e_right, "CoM height", e_h)
    assert e_left <= 1e-9 and e_right <= 1e-9 and e_h <= 1e-9


@pytest.mark.gpu
def test_launch_forms_agree(wca, device):
    """(4) ticks_per_launch 0, 1 and 7; run(70) against run(30), run(40); use_graph on and off; a non-blocking stream: every downloaded
    array bit for bit"""
    base = device["mpc"]
    for tpl in (1, 7):
        for graph in (True, False):
            _same(base, _run(_pipe(wca, "mpc", tpl=tpl), use_graph=graph))
    _same(base, _run(_pipe(wca, "mpc"), calls=(30, 40)))
    _same(base, _run(_pipe(wca, "mpc", tpl=1), calls=(30, 40), use_graph=True))
    s = wca.capi.stream_create()
    try:
        for tpl in (0, 1):
            pipe = _pipe(wca, "mpc", tpl=tpl)
            fs = pk.scenario()["fs"]
            pipe.upload_footsteps(fs, fs)
            pipe.run(30, stream=s); pipe.run(40, stream=s)
            wca.capi.stream_synchronize(s)
            _same(base, pipe.download())
    finally:
        wca.capi.stream_destroy(s)


@pytest.mark.gpu
def test_limits(wca):
    """(5) the joint-17 cut, a handle per robot of the restatement (the cut is that robot's own; the other twelve robots walk under it or
    are stopped by it): q_log against the restatement to 1e-9, every robot inside the cut with <=, the active limits of the last tick
    the restatement's"""
    for i, w in pk.reference_cut().items():
        lo, hi = pk.cut_limits(i)
        o = _run(_pipe(wca, "mpc", q_min=lo, q_max=hi))
        assert o["tick"] == T and o["ik_fail"][i] == 0
        assert (o["q_log"] <= hi).all() and (o["q_log"] >= lo).all() and (o["q_des"] <= hi).all()
        assert np.isfinite(o["q_log"]).all()
        err = np.abs(o["q_log"][:, i] - w["q_log"]).max()
        print(i, err, "ticks on the cut", int((o["q_log"][:, i, pk.CUT_JOINT] == hi[pk.CUT_JOINT]).sum()))
        assert err <= 1e-9
        assert o["active_upper"][i] == pk.mask_of(w["active"][-1], 1) and o["active_lower"][i] == pk.mask_of(w["active"][-1], -1)


@pytest.mark.gpu
def test_not_solved_in_mixed_batches(wca, device):
    """(6) robot 5 with a CoM height of 0.9 m it cannot reach: ik_fail == T, q_des its (clipped) q0, while the robots of its wave are bit
    for bit those of the healthy batch; then two iterations per tick, which stop every robot at tick 0.  No output is non-finite."""
    fs = pk.scenario()["fs"]
    high = dict(fs, state0=fs["state0"].copy())
    high["state0"][5, 68] = 0.9
    o = _run(_pipe(wca, "mpc"), fs=high)
    print("ik_fail", o["ik_fail"], "iters", o["ik_iters"])
    assert o["tick"] == T and o["ik_fail"][5] == T and np.array_equal(o["q_des"][5], fs["q0"][5])
    assert np.array_equal(o["q_log"][:, 5], np.tile(fs["q0"][5], (T, 1))) and o["ik_iters"][5] <= 30
    rest = [i for i in range(B13) if i != 5]
    assert not o["ik_fail"][rest].any()
    _same(o, device["mpc"], rows=[4, 6, 7])
    _same(o, device["mpc"], rows=rest)
    s = _run(_pipe(wca, "mpc", max_iter=2), fs=high)
    assert s["tick"] == T and (s["ik_fail"] == T).all() and np.array_equal(s["q_des"], fs["q0"]) and (s["ik_iters"][rest] == 2).all() and 1 <= s["ik_iters"][5] <= 2
    for out in (o, s):
        for k, v in out.items():
            assert np.isfinite(np.asarray(v, float)).all(), k
    # the chain keeps running for a stopped robot: the healthy rows' chain is the healthy batch's, stopped or not
    for k in CHAIN_KEYS:
        x, y = s[k], device["mpc"][k]
        ax = x.shape.index(B13)
        assert np.array_equal(np.take(x, rest, ax), np.take(y, rest, ax)), k


@pytest.mark.gpu
def test_replan(wca, device):
    """(7) upload_footsteps, run(30), replan_footsteps at stage 30 - inside the double support [25, 35) - run(40), on the reactive handle
    with gain scheduling (its chain reads stage t alone, so a one-go restatement on the stitched plan is the same computation): robot 0's
    q_log against the restatement on the stitched plan of helpers/footstep_replan.py to 1e-9; a robot with merge stage -1 equals its
    un-replanned run bit for bit."""
    sc = pk.scenario()
    fs, plan0 = sc["fs"], sc["plan"]
    M = np.full(B13, -1, np.int32); M[[0, 3, 6]] = 30
    n_new = np.where(M >= 0, 2, 0).astype(np.int32)
    sides = np.tile(np.array([0, 1], np.uint8), (B13, 1))
    assert np.all(plan0["contact"][M >= 0, 30] & 3 == 3)
    rp = fr.new_steps(plan0, M, n_new, sides, 8, 31)
    stitched = fr.footstep_replan(plan0, fs, M, rp, T + pk.N + 1, T, com_height=pk.H)
    pipe = _pipe(wca, "reactive_gs")
    pipe.upload_footsteps(fs, fs)
    pipe.run(30)
    pipe.replan_footsteps(M, rp, rp["first_ds_ticks"])
    pipe.run(40)
    o = pipe.download()
    assert o["tick"] == T and not o["ik_fail"].any()
    ch = pk.chain("reactive_gs", 0, plan=stitched)
    w = pk.walk(ch, fs["q0"][0], pk.params())
    err = np.abs(o["q_log"][:, 0] - w["q_log"]).max()
    moved = np.abs(o["q_log"][:, 0] - device["reactive_gs"]["q_log"][:, 0]).max()
    print("robot 0 against the stitched restatement", err, "against its un-replanned walk", moved)
    assert (w["status"] == ps.SOLVED).all() and err <= 1e-9 and moved > 1e-4
    _same(o, device["reactive_gs"], rows=[i for i in range(B13) if M[i] < 0])
