"""Footsteps planned on the device from per-robot goals (wcqp_unicycle_*).  CPU: properties of the numpy restatement
(helpers/unicycle_plan.py), its decision margins, the closed loop on its plans, the ABI and the refusals that need no device.  GPU: the
kernel against the restatement, batch sizes, a stuck robot and a NaN goal next to healthy robots, the two forms, a fuzz batch, and
upload_goal / replan_goal end to end against oracle/tick_spec.py."""
import ctypes as C

import numpy as np
import pytest
from walking_controllers_amd.capi import E_INVALID as WCQP_E_INVALID, E_UNSUPPORTED as WCQP_E_UNSUPPORTED, E_HIP as WCQP_E_HIP

import robots
from helpers import footstep_plan as fp
from helpers import footstep_replan as fr
from helpers import planned_tick as pt
from helpers import streamed_tick as stt
from helpers import unicycle_plan as up
from helpers import zmp_gains as zg

OUT = ("n_steps", "side", "target", "status", "desired_point", "unicycle_end")
MARGIN = 1e-9           # a robot the restatement decided by less may be decided otherwise by the device: it is left out of a comparison
# the scenario of the GPU tests: 13 robots (a wave with dead lanes), K = 8 steps of D = 25 samples.  The thresholds are set for steps of
# 0.25 s: the unicycle advances 0.05 m per step at most, a foot twice that
SCEN = dict(step_ticks=25, max_steps=8, max_linear_velocity=0.2, max_angular_velocity=1.0, min_step_length=0.01, min_angle_variation=0.02)
FUZZ_SEED, FUZZ_B = 7, 256
# the walk of the closed-loop tests: the walk tests' robot (feet 0.114 .. 0.123 m apart), steps of 30 + 20 stages behind 20
FIRST_DS, SS, DS, K_WALK, MAXT = 20, 30, 20, 6, 400
WALK = dict(step_ticks=SS + DS, max_steps=K_WALK, nominal_width=0.118, min_width=0.10, max_linear_velocity=0.03, max_angular_velocity=0.15,
            min_step_length=0.005, min_angle_variation=0.01)
GOALS0 = np.array([[0.04, 0.0], [0.03, 0.03], [0.05, -0.01]])      # straight, a turn, and the robot that is replanned
M_REPLAN, FD_REPLAN, GOAL1 = FIRST_DS + (SS + DS) + SS + 5, 15, (0.02, 0.02)    # stage 105: five stages into the double support behind step 2
K_DCM = 1.0
KEYS = ("u0_log", "dq_log", "q_des", "dcm", "com")


def _params(wca, **kw):
    return dict(wca.UnicyclePlanner.DEFAULTS, **kw)


def _replay(p, g, r, i):
    """the feet of robot i walked through the steps of plan r: per step (swing side, its three constraint margins against the stance foot)"""
    feet = [(g["left0"][i, 0], g["left0"][i, 1], np.arctan2(g["left0"][i, 6], g["left0"][i, 3])),
            (g["right0"][i, 0], g["right0"][i, 1], np.arctan2(g["right0"][i, 6], g["right0"][i, 3]))]
    rows = []
    for k in range(int(r["n_steps"][i])):
        sw = int(r["side"][i, k])
        st = feet[1 - sw]
        c, yaw = r["target"][i, k, :2], feet[sw][2] + r["target"][i, k, 2]
        d = c - np.array(st[:2])
        rlon = np.cos(st[2]) * d[0] + np.sin(st[2]) * d[1]
        rlat = np.cos(st[2]) * d[1] - np.sin(st[2]) * d[0]
        rows.append((sw, p["max_step_length"] - np.hypot(rlon, rlat), (1.0 if sw == 0 else -1.0) * rlat - p["min_width"],
                     p["max_angle_variation"] - abs(up.wrap(yaw - st[2]))))
        feet[sw] = (c[0], c[1], yaw)
    return rows, feet


@pytest.fixture(scope="module")
def scen(wca):
    """the 13 scenario robots and their restated plan"""
    g = wca.synth.synth_goal_batch(13)
    p = _params(wca, **SCEN)
    return g, p, up.unicycle_plan(p, g["left0"], g["right0"], g["goals"], g["first_side"])


@pytest.fixture(scope="module")
def fuzz(wca):
    """256 robots heading anywhere with goals from the disc of 1 m, and their restated plan"""
    g = wca.synth.synth_goal_batch(FUZZ_B, seed=FUZZ_SEED, cases=False, radius=1.0)
    p = _params(wca, **SCEN)
    return g, p, up.unicycle_plan(p, g["left0"], g["right0"], g["goals"], g["first_side"])


@pytest.fixture(scope="module")
def walk3(wca, qs):
    """Three robots of the walk tests sent to GOALS0, robot 2 sent on to GOAL1 at stage M_REPLAN: the restated footsteps, the plans
    (before and after the replan) and oracle/tick_spec.py's run over each - reactive controller, gain scheduling."""
    from oracle import tick_spec as ts
    robot = "iCubGazeboV2_5"
    R = robots.ROBOTS[robot]
    model = wca.synth.icub_like_model()
    kb = wca.synth.synth_walk_kin_batch(3)
    fs = wca.synth.synth_footstep_walk_batch(3, MAXT, pt.poses_host(model, kb), kb)
    st = fs["state0"]
    p = _params(wca, **WALK)
    T = MAXT + 51
    r0 = up.unicycle_plan(p, st[:, 24:36], st[:, 36:48], GOALS0, 1)
    fs.update(n_steps=r0["n_steps"], side=r0["side"], target=r0["target"], first_ds_ticks=FIRST_DS, ss_ticks=SS, ds_ticks=DS, final_ds_ticks=0, lift=0.02)
    plan0 = fp.footstep_plan(fs, st, T, MAXT)
    M = np.array([-1, -1, M_REPLAN], np.int32)
    r1 = up.unicycle_plan(p, plan0["left_traj"][2:, M_REPLAN], plan0["right_traj"][2:, M_REPLAN], np.array([GOAL1]), 1)
    rp = dict(n_steps=np.zeros(3, np.int32), side=np.zeros((3, K_WALK), np.uint8), target=np.zeros((3, K_WALK, 3)), first_ds_ticks=FD_REPLAN)
    for k in ("n_steps", "side", "target"):
        rp[k][2] = r1[k][0]
    plan1 = fr.footstep_replan(plan0, fs, M, rp, T, MAXT)
    ipar = robots.ik_params(qs, robot, v_max=wca.synth.WALK_VMAX.copy())
    ipar.joint_reg_deg = wca.synth.WALK_POSTURE_DEG.copy()

    def run(plan):
        d = dict(fs, ref_traj=plan["ref_traj"], dcm_vel_traj=plan["dcm_vel_traj"], dcm0=plan["ref_traj"][:, 0].copy(), u_init=plan0["zmp_ref"][:, 0].copy())
        return ts.run_ticks(ts.TickParams(horizon=50, k_com=R["k_com"], k_zmp=R["k_zmp"]), d, MAXT, ipar, kin_model=model, foot_rect=wca.synth.FOOT_RECT,
                            stages=stt.stages_of(plan, MAXT), neck_additional_rotation=R["additional_rotation"], dcm_controller="reactive",
                            k_dcm=K_DCM, dcm_vel=plan["dcm_vel_traj"], zmp_gain_schedule=zg.ZMP_SCHEDULE[robot])
    return dict(fs=fs, p=p, r0=r0, r1=r1, M=M, rp=rp, plan0=plan0, plan1=plan1, ref0=run(plan0), ref1=run(plan1), robot=robot)


# ---------------------------------------------------------------------------------------------------------------- CPU

def test_restatement_steps_satisfy_the_constraints(scen, fuzz):
    """every step taken satisfies the three constraints against its stance foot (replayed from the outputs alone), sides alternate from
    first_side, rows of steps not taken are zero; the cases end as they are meant to"""
    for g, p, r in (scen, fuzz):
        for i in range(len(r["n_steps"])):
            rows, _ = _replay(p, g, r, i)
            n = int(r["n_steps"][i])
            assert [sw for sw, *_ in rows] == [(int(g["first_side"][i]) + k) % 2 for k in range(n)], i
            assert all(min(m[1:]) >= -1e-12 for m in rows), (i, rows)
            assert not r["side"][i, n:].any() and not r["target"][i, n:].any()
            assert (r["status"][i] == up.TRUNCATED) == (n == p["max_steps"])
    g, p, r = scen
    case = {c: i for i, c in enumerate(g["case"])}
    assert r["n_steps"][case["origin"]] == 0 and r["status"][case["origin"]] == up.DONE
    assert r["n_steps"][case["below_a_step"]] == 0 and r["status"][case["below_a_step"]] == up.DONE
    u = r["unicycle_end"][case["origin"]]                 # (goal (0, 0): the desired point is the reference point)
    assert np.abs(r["desired_point"][case["origin"]] - (u[:2] + 0.1 * np.array([np.cos(u[2]), np.sin(u[2])]))).max() <= 1e-15
    for c in ("far", "far_turn"):
        assert r["n_steps"][case[c]] == p["max_steps"] and r["status"][case[c]] == up.TRUNCATED
    for c in ("straight", "turn_left", "turn_right", "behind"):
        assert 0 < r["n_steps"][case[c]] < p["max_steps"] and r["status"][case[c]] == up.DONE, c
    assert (r["target"][..., 2] > 1e-3).any() and (r["target"][..., 2] < -1e-3).any()


def test_done_robots_end_aligned(wca, scen):
    """A DONE robot's feet end nominal_width apart and parallel, its reference point within min_step_length of the desired point.  The
    unicycle still moves by up to the arrival thresholds between the last two footprints (the definition has no terminal step), so the
    1e-9 holds where the thresholds are below it - asserted here at thresholds of 1e-10 with steps to spare, every scenario robot DONE -
    and at the scenario's own thresholds the feet are aligned to within twice those (the last footprint lies between the rejected candidate
    and the footprint it was compared with, each pair less than a threshold apart), asserted too."""
    g, ps, rs = scen
    tight = _params(wca, step_ticks=50, max_steps=48, max_linear_velocity=0.2, max_angular_velocity=1.0, min_step_length=1e-10, min_angle_variation=1e-10)
    rt = up.unicycle_plan(tight, g["left0"], g["right0"], g["goals"], g["first_side"])
    assert (rt["status"] == up.DONE).all(), rt["status"]
    for p, r, tol_w, tol_a in ((tight, rt, 1e-9, 1e-9), (ps, rs, 2 * ps["min_step_length"], 2 * ps["min_angle_variation"])):
        for i in np.nonzero(r["status"] == up.DONE)[0]:
            f, u = r["feet"][i], r["unicycle_end"][i]
            width = np.hypot(*(f[0, :2] - f[1, :2]))
            y = u[:2] + np.array([np.cos(u[2]) * 0.1, np.sin(u[2]) * 0.1])
            print(i, width - p["nominal_width"], up.wrap(f[0, 2] - f[1, 2]), np.hypot(*(y - r["desired_point"][i])))
            assert abs(width - p["nominal_width"]) <= tol_w and abs(up.wrap(f[0, 2] - f[1, 2])) <= tol_a, i
            assert np.hypot(*(y - r["desired_point"][i])) <= p["min_step_length"], i


def test_a_small_K_truncates(wca, scen):
    g, p, r8 = scen
    r = up.unicycle_plan(dict(p, max_steps=2), g["left0"], g["right0"], g["goals"], g["first_side"])
    for i in range(13):
        if r8["n_steps"][i] > 2:
            assert r["status"][i] == up.TRUNCATED and r["n_steps"][i] == 2
            assert np.array_equal(r["target"][i], r8["target"][i, :2]) and np.array_equal(r["side"][i], r8["side"][i, :2])
        else:
            assert r["status"][i] == r8["status"][i] and r["n_steps"][i] == r8["n_steps"][i]
    assert (r["status"] == up.TRUNCATED).sum() >= 8


def test_mirrored_inputs_give_mirrored_footsteps(scen, fuzz):
    """y -> -y with the sides swapped (d_y = 0): the same steps, mirrored"""
    def mirror(pose):
        yaw = np.arctan2(pose[:, 6], pose[:, 3])
        out = np.zeros_like(pose)
        out[:, 0], out[:, 1], out[:, 2] = pose[:, 0], -pose[:, 1], pose[:, 2]
        c, s = np.cos(-yaw), np.sin(-yaw)
        out[:, 3], out[:, 4], out[:, 6], out[:, 7], out[:, 11] = c, -s, s, c, 1.0
        return out
    for g, p, r in (scen, fuzz):
        m = up.unicycle_plan(p, mirror(g["right0"]), mirror(g["left0"]), g["goals"] * np.array([1.0, -1.0]), 1 - g["first_side"])
        ok = np.minimum(r["margin"], m["margin"]) >= MARGIN
        assert ok.mean() >= 0.98
        assert np.array_equal(m["n_steps"][ok], r["n_steps"][ok]) and np.array_equal(m["status"][ok], r["status"][ok])
        taken = (np.arange(p["max_steps"])[None, :] < r["n_steps"][:, None]) & ok[:, None]
        assert np.array_equal(m["side"][taken], 1 - r["side"][taken])
        err = np.abs(m["target"][taken] - r["target"][taken] * np.array([1.0, -1.0, -1.0])).max()
        print("mirror", err)
        assert err <= 1e-12


def test_decision_margins_stay_inside_the_caps(scen, fuzz):
    """the restatement alone, for the committed seeds: no scenario robot and at most 2 % of the fuzz batch is decided by less than 1e-9"""
    print("scenario", np.sort(scen[2]["margin"])[:3], "fuzz", np.sort(fuzz[2]["margin"])[:5])
    assert (scen[2]["margin"] >= MARGIN).all()
    assert (fuzz[2]["margin"] < MARGIN).mean() <= 0.02
    assert set(np.unique(fuzz[2]["status"])) >= {up.DONE, up.TRUNCATED}


def test_closed_loop_on_the_planned_footsteps(walk3):
    """(straight, turn, replanned) footstep_plan on the planned footsteps and oracle/tick_spec.py walk the whole plan - every robot
    stands before max_ticks - with no IK or MPC failure, before and after robot 2 is sent on at stage 105"""
    w = walk3
    assert (w["r0"]["status"] == up.DONE).all() and (w["r0"]["n_steps"] >= 3).all() and w["r1"]["status"][0] == up.DONE and w["r1"]["n_steps"][0] >= 2
    assert (w["r0"]["margin"] >= MARGIN).all() and w["r1"]["margin"][0] >= MARGIN
    assert abs(w["r0"]["target"][1, :, 2]).max() > 0.05                       # (the turn turns)
    assert FIRST_DS + int(w["r0"]["n_steps"].max()) * (SS + DS) < MAXT and M_REPLAN + FD_REPLAN + int(w["r1"]["n_steps"][0]) * (SS + DS) < MAXT
    assert (w["plan0"]["contact"][2, M_REPLAN] & 3) == 3
    for ref in (w["ref0"], w["ref1"]):
        assert (ref["ik_fail"] == 0).all() and (ref["mpc_fail"] == 0).all()
    for k in KEYS:                                                            # (the replan changed robot 2's walk, and only that)
        ax = 1 if k in ("u0_log", "dq_log") else 0
        assert np.array_equal(np.take(w["ref0"][k], [0, 1], axis=ax), np.take(w["ref1"][k], [0, 1], axis=ax)), k
    assert not np.array_equal(w["ref0"]["q_des"][2], w["ref1"]["q_des"][2])


def test_create_refusals(wca):
    lib = wca.capi.lib()

    def create(out=True, **kw):
        v = _params(wca, **kw)
        p = wca.capi.UnicycleParams(v["dT"], (C.c_double * 2)(*v["reference_position"]), *(v[k] for k, _ in wca.capi.UnicycleParams._fields_[2:]))
        h = C.c_void_p()
        rc = lib.wcqp_unicycle_create(C.byref(p), C.byref(h) if out else None)
        if rc == 0:
            assert lib.wcqp_unicycle_destroy(h) == 0
        return rc
    assert create() == 0 and create(slow_when_turning_gain=0.0) == 0 and create(max_steps=0) == 0 and create(min_width=0.16) == 0
    assert create(reference_position=(-0.1, 0.02)) == 0
    assert create(out=False) == WCQP_E_INVALID and lib.wcqp_unicycle_create(None, C.byref(C.c_void_p())) == WCQP_E_INVALID
    positive = ("dT", "unicycle_gain", "max_linear_velocity", "max_angular_velocity", "max_step_length", "min_step_length", "min_width",
                "nominal_width", "max_angle_variation", "min_angle_variation")
    for k in positive:
        for bad in (np.nan, np.inf, 0.0, -1.0):
            assert create(**{k: bad}) == WCQP_E_INVALID, (k, bad)
    for bad in (np.nan, np.inf, -1.0):
        assert create(slow_when_turning_gain=bad) == WCQP_E_INVALID
    for bad in ((np.nan, 0.0), (0.1, np.inf), (0.0, 0.0)):
        assert create(reference_position=bad) == WCQP_E_INVALID, bad
    assert create(min_width=0.17) == WCQP_E_INVALID and create(min_step_length=0.2) == WCQP_E_INVALID and create(min_step_length=0.3) == WCQP_E_INVALID
    assert create(step_ticks=0) == WCQP_E_INVALID and create(max_steps=-1) == WCQP_E_INVALID
    assert lib.wcqp_unicycle_destroy(None) == WCQP_E_INVALID


def test_plan_refusals_without_a_device(wca, scen):
    """what both forms refuse before they look for a device, and what the host form finds in its arrays"""
    lib = wca.capi.lib()
    g = scen[0]
    pl = wca.UnicyclePlanner(**SCEN)
    B, K = 13, SCEN["max_steps"]
    o = dict(n_steps=np.full(B, 77, np.int32), side=np.full((B, K), 9, np.uint8), target=np.full((B, K, 3), 5.0), status=np.full(B, 77, np.int32),
             desired_point=np.full((B, 2), 5.0), unicycle_end=np.full((B, 3), 5.0))
    base_in = dict(left0=g["left0"], right0=g["right0"], goal=g["goals"], first_side=g["first_side"])

    def structs(drop=(), **kw):
        a = {k: np.ascontiguousarray(v) for k, v in dict(base_in, **kw).items()}
        return a, wca.capi.UnicycleInputs(**{k: v.ctypes.data for k, v in a.items() if k not in drop}), \
            wca.capi.UnicycleOutputs(**{k: v.ctypes.data for k, v in o.items() if k not in drop})

    def host(batch=B, **kw):
        """the host form's code"""
        _keep, ins, outs = structs(**kw)
        return lib.wcqp_unicycle_plan_host(pl._h, batch, C.byref(ins), C.byref(outs))

    def both(batch=B, drop=()):
        """the codes of both forms - only for calls the device form refuses before it launches: the arrays are HOST memory, and with a
        device present it would launch on them"""
        _keep, ins, outs = structs(drop=drop)
        return lib.wcqp_unicycle_plan_host(pl._h, batch, C.byref(ins), C.byref(outs)), lib.wcqp_unicycle_plan_device(pl._h, batch, C.byref(ins), C.byref(outs), None)

    def arr(key, idx, val):
        a = np.array(base_in[key], copy=True); a[idx] = val
        return {key: a}
    for drop in ("left0", "right0", "goal", "first_side", "n_steps", "side", "target", "status"):
        assert both(drop=(drop,)) == (WCQP_E_INVALID, WCQP_E_INVALID), drop
    assert both(batch=-1) == (WCQP_E_INVALID, WCQP_E_INVALID) and both(batch=0) == (0, 0)
    # the 4 GB rule: target rows of 24 K = 192 bytes, so 2^32 / 192 = 22369621 robots pass and one more does not
    assert both(batch=22369622) == (WCQP_E_UNSUPPORTED, WCQP_E_UNSUPPORTED)
    ins, outs = wca.capi.UnicycleInputs(), wca.capi.UnicycleOutputs()
    assert lib.wcqp_unicycle_plan_host(None, B, C.byref(ins), C.byref(outs)) == WCQP_E_INVALID
    assert lib.wcqp_unicycle_plan_host(pl._h, B, None, C.byref(outs)) == WCQP_E_INVALID and lib.wcqp_unicycle_plan_host(pl._h, B, C.byref(ins), None) == WCQP_E_INVALID
    assert lib.wcqp_unicycle_plan_device(pl._h, B, None, C.byref(outs), None) == WCQP_E_INVALID
    # the host form reads its arrays first: a non-finite entry that is read, a side above 1 - of any robot - and nothing is written
    for bad in (arr("goal", (12, 1), np.nan), arr("goal", (0, 0), np.inf), arr("left0", (3, 0), np.nan), arr("left0", (3, 6), np.inf),
                arr("right0", (5, 1), -np.inf), arr("right0", (7, 3), np.nan), arr("first_side", 4, 2)):
        assert host(**bad) == WCQP_E_INVALID
    assert (o["n_steps"] == 77).all() and (o["status"] == 77).all() and (o["side"] == 9).all() and (o["target"] == 5.0).all()
    # entries that are not read may hold anything: the sole's z, the rest of the rotation
    junk = np.array(g["left0"], copy=True); junk[:, [2, 4, 5, 7, 8, 9, 10, 11]] = np.nan
    rc = host(left0=junk)
    if wca.device_count() == 0:
        assert rc == WCQP_E_HIP and host() == WCQP_E_HIP          # no device: an error, never a plan from somewhere else
    else:
        assert rc == 0


def test_binding_refusals(wca, scen):
    g = scen[0]
    with pytest.raises(TypeError):
        wca.UnicyclePlanner(step_length=0.1)
    with pytest.raises(wca.WcqpError, match="invalid|INVALID"):
        wca.UnicyclePlanner(min_width=0.2)
    pl = wca.UnicyclePlanner(**SCEN)
    with pytest.raises(ValueError):
        pl.plan_host(g["left0"], g["right0"], g["goals"], np.full(13, 2))
    for bad in ((g["left0"][:12], g["right0"], g["goals"], g["first_side"]), (g["left0"], g["right0"][:, :11], g["goals"], g["first_side"]),
                (g["left0"], g["right0"], g["goals"][:, :1], g["first_side"]), (g["left0"], g["right0"], g["goals"], g["first_side"][:5])):
        with pytest.raises(ValueError):
            pl.plan_host(*bad)
    pipe = object.__new__(wca.TickPipeline)
    pipe.planned, pipe.batch, pipe._h = False, 13, None
    with pytest.raises(ValueError):
        pipe.upload_goal(dict(state0=np.zeros((13, 87))), g["goals"], pl, 1, 20, 30, 20)
    with pytest.raises(ValueError):
        pipe.replan_goal(np.full(13, -1), g["goals"], pl, 1, 10)
    pipe.planned = True
    for bad in ((np.full(12, -1), g["goals"], 1), (np.full(13, -1), g["goals"][:12], 1), (np.full(13, -1), g["goals"], np.zeros(12))):
        with pytest.raises(ValueError):
            pipe.replan_goal(bad[0], bad[1], pl, bad[2], 10)
    vals = wca.UnicyclePlanner.from_ini_values(dict(unicycleGain=10.0, referencePosition=(0.1, 0.0), slowWhenTurningGain=5.0, maxStepLength=0.2,
                                                    minStepLength=0.05, minWidth=0.14, nominalWidth=0.16, maxAngleVariation=10.0, minAngleVariation=8.0),
                                               step_ticks=90).values
    assert vals == dict(wca.UnicyclePlanner.DEFAULTS, step_ticks=90)


# ---------------------------------------------------------------------------------------------------------------- GPU

def _device(wca, pl, g, B=None, stream=0, overwrite=False):
    """wcqp_unicycle_plan_device on device arrays -> the outputs as numpy arrays (prefilled with junk: every row is written).  The arrays
    come from the HIP runtime libwcqp itself is linked against, reached through the library's own handle: one runtime in the process."""
    L = wca.capi.lib()
    L.hipMalloc.argtypes, L.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p]
    L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    B = len(g["goals"]) if B is None else B
    K = pl.max_steps
    host = {k: np.ascontiguousarray(g[k][:B]) for k in ("left0", "right0", "goals", "first_side")}
    host.update(n_steps=np.full(B, 77, np.int32), side=np.full((B, K), 9, np.uint8), target=np.full((B, K, 3), np.nan), status=np.full(B, 77, np.int32),
                desired_point=np.full((B, 2), np.nan), unicycle_end=np.full((B, 3), np.nan))
    assert host["first_side"].dtype == np.uint8 and host["goals"].dtype == np.float64
    ptr = {}
    try:
        for k, v in host.items():
            ptr[k] = C.c_void_p()
            assert L.hipMalloc(C.byref(ptr[k]), max(v.nbytes, 8)) == 0
            assert L.hipMemcpy(ptr[k], v.ctypes.data, v.nbytes, 1) == 0
        ins = wca.capi.UnicycleInputs(ptr["left0"], ptr["right0"], ptr["goals"], ptr["first_side"])
        outs = wca.capi.UnicycleOutputs(**{k: ptr[k] for k in OUT})
        wca.capi.check(L.wcqp_unicycle_plan_device(pl._h, B, C.byref(ins), C.byref(outs), stream or None))
        if overwrite:          # the two structs are read at the call
            C.memset(C.byref(ins), 0, C.sizeof(ins)); C.memset(C.byref(outs), 0, C.sizeof(outs))
        wca.capi.stream_synchronize(stream)
        for k in OUT:
            assert L.hipMemcpy(host[k].ctypes.data, ptr[k], host[k].nbytes, 2) == 0
    finally:
        for v in ptr.values():
            L.hipFree(v)
    return {k: host[k] for k in OUT}


def _against_the_restatement(dev, r, rows=None):
    """decisions equal, numbers to 1e-9 - on `rows` (default: all)"""
    rows = np.arange(len(r["n_steps"])) if rows is None else rows
    for k in ("n_steps", "side", "status"):
        assert np.array_equal(dev[k][rows], r[k][rows]), k
    for k in ("target", "desired_point", "unicycle_end"):
        err = np.abs(dev[k][rows] - r[k][rows]).max()
        print(k, err)
        assert err <= 1e-9, (k, err)


def _same_rows(a, b, rows):
    for k in OUT:
        assert np.array_equal(a[k][rows], b[k][rows]), k


@pytest.fixture(scope="module")
def scen_dev(wca, scen):
    return _device(wca, wca.UnicyclePlanner(**SCEN), scen[0])


@pytest.mark.gpu
def test_scenario_matches_the_restatement(scen, scen_dev):
    """13 robots, K = 8, D = 25: n_steps, side and status equal, target, desired_point and unicycle_end to 1e-9 (the gap printed: both
    sides do the same RK4 in binary64)"""
    _against_the_restatement(scen_dev, scen[2])
    assert all(np.isfinite(scen_dev[k]).all() for k in OUT)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [70, 1])
def test_other_batch_sizes_are_bit_identical(wca, scen, scen_dev, B):
    """a full wave plus six lanes, and one robot: the first 13 rows equal the 13-robot run bit for bit; rows of steps not taken are zero"""
    g = wca.synth.synth_goal_batch(B)
    assert np.array_equal(g["goals"][:13], scen[0]["goals"][:B]) and np.array_equal(g["left0"][:13], scen[0]["left0"][:B])
    d = _device(wca, wca.UnicyclePlanner(**SCEN), g)
    _same_rows(d, scen_dev, np.arange(min(B, 13)))
    idle = np.arange(SCEN["max_steps"])[None, :] >= d["n_steps"][:, None]
    assert not d["side"][idle].any() and not d["target"][idle].any()
    assert all(np.isfinite(d[k]).all() for k in OUT) and (d["status"] <= up.STUCK).all() and (d["n_steps"] <= SCEN["max_steps"]).all()


@pytest.mark.gpu
def test_a_stuck_robot_next_to_healthy_ones(wca, scen):
    """K = 3, min_width just under nominal_width and a saturated turn of 8 rad/s: the turning robots find no candidate wide enough and
    end STUCK; the others equal the batch in which the stuck ones stand still (goal 0, 0), bit for bit"""
    g = scen[0]
    par = dict(SCEN, max_steps=3, max_angular_velocity=8.0, min_width=0.1599)
    r = up.unicycle_plan(_params(wca, **par), g["left0"], g["right0"], g["goals"], g["first_side"])
    stuck = r["status"] == up.STUCK
    assert 3 <= stuck.sum() <= 9 and (r["status"][~stuck] != up.STUCK).all() and (r["margin"] >= MARGIN).all()
    pl = wca.UnicyclePlanner(**par)
    d = _device(wca, pl, g)
    _against_the_restatement(d, r)
    assert (d["n_steps"][stuck] == 0).all() and not d["target"][stuck].any()
    calm = dict(g, goals=np.where(stuck[:, None], 0.0, g["goals"]))
    _same_rows(d, _device(wca, pl, calm), np.nonzero(~stuck)[0])


@pytest.mark.gpu
def test_a_nan_goal_on_the_device_form(wca, scen, scen_dev):
    """robots with a NaN goal, an Inf sole and a first_side of 2: INVALID_INPUT with zero steps and zero rows; the wave's other robots are
    bit-identical and nothing stored is non-finite"""
    g = {k: np.array(v, copy=True) for k, v in scen[0].items() if k != "case"}
    g["goals"][4, 1] = np.nan; g["left0"][9, 6] = np.inf; g["first_side"][11] = 2
    bad = np.array([4, 9, 11])
    d = _device(wca, wca.UnicyclePlanner(**SCEN), g)
    assert (d["status"][bad] == up.INVALID_INPUT).all() and (d["n_steps"][bad] == 0).all()
    for k in ("side", "target", "desired_point", "unicycle_end"):
        assert not d[k][bad].any(), k
    _same_rows(d, scen_dev, np.setdiff1d(np.arange(13), bad))
    assert all(np.isfinite(d[k]).all() for k in OUT)


@pytest.mark.gpu
def test_forms_agree(wca, scen, scen_dev):
    """the host form, and the device form on a non-blocking stream with the host structs overwritten as soon as the call returns: bit for bit"""
    g = scen[0]
    pl = wca.UnicyclePlanner(**SCEN)
    h = pl.plan_host(g["left0"], g["right0"], g["goals"], g["first_side"])
    _same_rows(h, scen_dev, np.arange(13))
    s = wca.capi.stream_create()
    try:
        _same_rows(_device(wca, pl, g, stream=s, overwrite=True), scen_dev, np.arange(13))
    finally:
        wca.capi.stream_destroy(s)
    with pytest.raises(wca.WcqpError, match="invalid|INVALID"):
        pl.plan_host(g["left0"], g["right0"], np.where(np.arange(13)[:, None] == 6, np.nan, g["goals"]), g["first_side"])
    assert pl.plan_host(g["left0"][:0], g["right0"][:0], g["goals"][:0], g["first_side"][:0])["n_steps"].shape == (0,)


@pytest.mark.gpu
def test_fuzz_against_the_restatement(wca, fuzz):
    """256 robots, goals from the disc of 1 m, any heading: robots the restatement decided by 1e-9 or more agree with it, and those are
    at least 98 % of the batch"""
    g, p, r = fuzz
    d = _device(wca, wca.UnicyclePlanner(**SCEN), g)
    keep = r["margin"] >= MARGIN
    print("left out", int((~keep).sum()), "of", FUZZ_B)
    assert (~keep).mean() <= 0.02
    _against_the_restatement(d, r, np.nonzero(keep)[0])
    assert all(np.isfinite(d[k]).all() for k in OUT)


def _pipe(wca, B, robot):
    R = robots.ROBOTS[robot]
    ik = wca.IkSolver(form=wca.IK_FORM_QPOASES, neck_weight=R["neck_weight"] * np.eye(3), joint_reg_weights=np.array(R["reg_w"], float),
                      joint_reg_gains=np.array(R["reg_k"], float), joint_reg_rad=np.deg2rad(wca.synth.WALK_POSTURE_DEG),
                      v_max=wca.synth.WALK_VMAX.copy(), k_pos_com=R["k_pos_com"], k_pos_foot=R["k_pos_foot"], k_att_foot=R["k_att_foot"],
                      k_neck=R["k_neck"])
    return wca.TickPipeline(B, MAXT, wca.MpcSolver(horizon=50), ik, log_ticks=MAXT, k_com=R["k_com"], k_zmp=R["k_zmp"],
                            kin=wca.KinModel(wca.synth.icub_like_model()), dcm_controller="reactive", k_dcm=K_DCM, zmp_gain_scheduling=True,
                            **zg.ZMP_SCHEDULE[robot], planned_trajectories=True, neck_additional_rotation=np.array(R["additional_rotation"]))


def _run_against(out, ref):
    assert (ref["ik_fail"] == 0).all() and (out["ik_fail"] == 0).all()
    for k in KEYS:
        err = np.abs(out[k] - ref[k]).max()
        print(k, err)
        assert err <= 1e-9, (k, err)
    assert np.array_equal(out["mpc_fail"], ref["mpc_fail"])


@pytest.mark.gpu
def test_upload_goal_and_replan_goal_end_to_end(wca, walk3):
    """upload_goal and the whole plan on a reactive handle with gain scheduling against oracle/tick_spec.py on the restated plan to 1e-9;
    then, on a second handle, replan_goal for robot 2 at stage 105 (-1 for the others), run on, against the restatement on the stitched
    plan; the robots with -1 are bit-identical to the run without the replan."""
    w = walk3
    fs = w["fs"]
    pl = wca.UnicyclePlanner(**WALK)
    kw = dict(lift=fs["lift"], zmp_delta_left=fs["zmp_delta_left"], zmp_delta_right=fs["zmp_delta_right"])
    a = _pipe(wca, 3, w["robot"])
    got = a.upload_goal(fs, GOALS0, pl, 1, FIRST_DS, SS, DS, **kw)
    _against_the_restatement(got, w["r0"])
    a.run(MAXT)
    out_a = a.download()
    _run_against(out_a, w["ref0"])
    b = _pipe(wca, 3, w["robot"])
    b.upload_goal(fs, GOALS0, pl, 1, FIRST_DS, SS, DS, **kw)
    b.run(M_REPLAN)
    goals1 = np.array([[9.0, 9.0], [np.nan, 0.0], GOAL1])                     # (rows of robots that keep their plan are not read)
    got = b.replan_goal(w["M"], goals1, pl, 1, FD_REPLAN)
    assert (got["status"][:2] == -1).all() and not got["target"][:2].any()
    _against_the_restatement(got, dict(w["r1"], **{k: np.concatenate([got[k][:2], w["r1"][k]]) for k in OUT}), np.array([2]))
    b.run(MAXT - M_REPLAN)
    out_b = b.download()
    _run_against(out_b, w["ref1"])
    for k in KEYS:
        ax = 1 if k in ("u0_log", "dq_log") else 0
        assert np.array_equal(np.take(out_a[k], [0, 1], axis=ax), np.take(out_b[k], [0, 1], axis=ax)), k
    win = b.plan_window()
    for k, kr in (("left_traj", "left_traj"), ("right_traj", "right_traj"), ("ref_traj", "ref_traj"), ("dcm_vel_traj", "dcm_vel_traj")):
        err = np.abs(win[k] - w["plan1"][kr]).max()
        print(k, err)
        assert err <= 1e-9, (k, err)
    assert np.array_equal(win["contact"], w["plan1"]["contact"])
