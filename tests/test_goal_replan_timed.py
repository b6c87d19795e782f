"""wcqp_tick_replan_goals_timed on the device: running TIMED walks sent on to new goals, enqueue-only - footsteps and their
durations planned by goal_plan_timed_kernel -, against the host composition TickPipeline.replan_goal(timing=) on a twin handle, against
the restatement (helpers/goal_replan_timed.py) and against oracle/tick_spec.py on the restated stitched plan; a batch with a tail whose
second call meets durations the first one still owes; owed durations deciding a later footstep replan; TOO_LATE and all-KEEP calls;
refusals; a resident plan on a streamed handle; a POSITION handle."""
import ctypes as C

import numpy as np
import pytest
from walking_controllers_amd.capi import E_INVALID as WCQP_E_INVALID, E_UNSUPPORTED as WCQP_E_UNSUPPORTED

from helpers import goal_merge_timed as gmt
from helpers import goal_replan as gr
from helpers import goal_replan_timed as gt
from helpers import position_tick as pk
from helpers import resident_plan as rs
from helpers import unicycle_plan_timed as ut

KEYS, MAXT = gr.KEYS, gt.MAXT
WINDOW = ("left_traj", "right_traj", "ref_traj", "dcm_vel_traj")
NUMBERS = ("target", "desired_point", "unicycle_end")
TOL = 1e-9          # the bar DESIGN §8.13, §8.17 and §8.21 use for chained device arithmetic

FAILED = []           # what _close found above its bar: every comparison of a test is printed before the test asserts that this is empty


def _rows(x, rows, k):
    return np.take(x, rows, axis=1 if k in ("u0_log", "dq_log") else 0)


def _close(what, a, b, keys, rows, tol=TOL):
    """|a - b| <= tol on `rows` of every key - printed, and noted in FAILED where it does not hold; returns whether all were bit-identical"""
    same = True
    for k in keys:
        x, y = (_rows(a[k], rows, k), _rows(b[k], rows, k)) if k in KEYS else (a[k][rows], b[k][rows])
        d = np.abs(x - y)
        err = d.max() if d.size else 0.0
        same = same and np.array_equal(x, y)
        print(what, k, err, "" if err <= tol else "at %s" % (np.unravel_index(np.argmax(d), d.shape),))
        if err > tol:
            FAILED.append((what, k, err))
    return same


def _decisions(a, b, rows):
    for k in ("n_steps", "side", "status", "ss_ticks", "ds_ticks"):
        assert np.array_equal(a[k][rows], b[k][rows]), k


def _result_matches(res, c, rows):
    """goal_result() against a restated call: what was taken, the decisions and durations, the numbers"""
    assert np.array_equal(res["merge_stage"], np.where(c["M"] >= 1, c["M"], 0)) and np.array_equal(res["first_side"][c["sel"]], c["fside"][c["sel"]])
    assert np.array_equal(res["status"][c["decided"] != 0], c["decided"][c["decided"] != 0])
    off = np.nonzero(c["decided"] != 0)[0]
    for k in ("first_side", "n_steps", "side", "ss_ticks", "ds_ticks") + NUMBERS:
        assert not res[k][off].any(), k
    _decisions(res, c["r"], rows)
    _close("result against the restatement", res, c["r"], NUMBERS, rows)


def _windows(a, b, c, rows):
    """the plans of twin handles against each other and against the restated plan"""
    wa, wb = a.plan_window(), b.plan_window()
    same = _close("plan A against B", wa, wb, WINDOW, rows)
    assert np.array_equal(wa["contact"][rows], wb["contact"][rows])
    _close("plan B against the restatement", wb, c["plan"], WINDOW, rows)
    assert np.array_equal(wb["contact"][rows], c["plan"]["contact"][rows])
    return same


def _against_oracle(out, ref, rows):
    print("ik_fail of the oracle", ref["ik_fail"].tolist(), "of the device", out["ik_fail"][rows].tolist())
    assert (ref["ik_fail"] == 0).all() and (out["ik_fail"][rows] == 0).all()
    _close("against the oracle", {k: _rows(out[k], rows, k) for k in KEYS}, ref, KEYS, np.arange(len(rows)))
    assert np.array_equal(out["mpc_fail"][rows], ref["mpc_fail"])


def _upload(pipe_, sc, planner):
    fs = sc["fs"]
    return pipe_.upload_goal(fs, sc["goals0"], planner, 1, gt.FIRST_DS, lift=fs["lift"], zmp_delta_left=fs["zmp_delta_left"],
                             zmp_delta_right=fs["zmp_delta_right"], timing=sc["timing"])


def _same_windows(w0, w1):
    for k in w0:
        assert np.array_equal(w0[k], w1[k]), k


def _timing_rows(wca, h, B, K):
    ss, ds = np.full((B, K), 77, np.int32), np.full((B, K), 77, np.int32)
    rc = wca.capi.lib().wcqp_tick_get_goal_timing(h._h, ss.ctypes.data, ds.ctypes.data)
    return rc, ss, ds


# ---------------------------------------------------------------------------------------------------------------- the walk scenario

@pytest.mark.gpu
def test_walk_scenario(wca, qs):
    """Three robots sent to GOALS0 by the timed planner on a reactive handle with gain scheduling and fused kinematics.  After run(90)
    handle B calls replan_goals(timing=) for robot 2 with AUTO, SIDE_AUTO and a lead of 10 (rows 0 and 1 KEEP, a NaN goal among them):
    goal_result() gives the restatement's merge stage and side.  Twin A calls replan_goal(timing=) with that stage and side.  n_steps, side,
    status, ss_ticks, ds_ticks, merge_stage and first_side equal the restatement's; target, desired_point, unicycle_end and plan_window()'s
    feet, ref_traj and dcm_vel_traj within 1e-9, contact equal; below the merge stage robot 2's plan is bit for bit what it was; after the
    run the logs of A and B within 1e-9 of each other and of oracle/tick_spec.py on the restated stitched plan; robots 0 and 1 bit-identical
    to a handle that was never replanned.  Bit-identity of A and B is printed, not asserted."""
    sc = gt.walk_scenario(wca)
    c = sc["c1"]
    ref1 = gt.oracle_runs(wca, qs)[0]
    del FAILED[:]
    pl = wca.UnicyclePlanner(**gt.WALK)
    a, b, n = (gr.pipe(wca, 3) for _ in range(3))
    for h in (a, b, n):
        _upload(h, sc, pl)
    assert b.info()["plan_timed"] is True and b.info()["kin_handoff"] == "fused"
    n.run(MAXT)
    a.run(sc["t1"]); b.run(sc["t1"])
    w_before = b.plan_window()
    assert b.replan_goals(sc["goals1"], pl, gt.FD, merge_stage=sc["merge1"], min_lead_ticks=sc["lead1"], timing=sc["timing"]) is None
    res = b.goal_result()
    M2 = int(c["M"][2])
    assert res["merge_stage"].tolist() == [0, 0, M2] and res["first_side"].tolist() == [0, 0, int(c["fside"][2])]
    assert res["status"].tolist() == [gt.KEPT, gt.KEPT, 0] and set(res) == {k for k, _, _ in wca.capi.GOAL_RESULT} | {"ss_ticks", "ds_ticks"}
    _result_matches(res, c, np.array([2]))
    got = a.replan_goal(np.array([-1, -1, M2], np.int32), sc["goals1"], pl, res["first_side"], gt.FD, timing=sc["timing"])
    every = np.arange(3)
    _decisions(res, got, every)
    same = _close("result A against B", got, res, NUMBERS, every)
    same = _windows(a, b, c, every) and same
    w_after = b.plan_window()
    for k in w_before:
        assert np.array_equal(w_before[k][:, :M2], w_after[k][:, :M2]) and np.array_equal(w_before[k][:2], w_after[k][:2]), k
    a.run(MAXT - sc["t1"]); b.run(MAXT - sc["t1"])
    oa, ob, on = a.download(), b.download(), n.download()
    same = _close("logs A against B", oa, ob, KEYS, every) and same
    print("A and B bit-identical:", same)
    _against_oracle(oa, ref1, every)
    _against_oracle(ob, ref1, every)
    for k in KEYS:
        assert np.array_equal(_rows(ob[k], [0, 1], k), _rows(on[k], [0, 1], k)), k
    assert not np.array_equal(ob["q_des"][2], on["q_des"][2])
    assert not FAILED, FAILED


# ---------------------------------------------------------------------------------------------------------------- the batch scenario

def _two_calls(sc, pl, b, rows=slice(None)):
    """the batch scenario's two replan_goals(timing=) calls on handle b, no goal_result() in between"""
    b.run(gt.T1)
    b.replan_goals(sc["goals1"][rows], pl, gt.FD, merge_stage=sc["merge1"][rows], first_side=sc["side1"][rows], min_lead_ticks=gt.LEAD1, timing=sc["timing"])
    b.run(gt.T2 - gt.T1)
    b.replan_goals(sc["goals2"][rows], pl, gt.FD, merge_stage=sc["merge2"][rows], min_lead_ticks=gt.LEAD2, timing=sc["timing"])


@pytest.mark.gpu
def test_batch_scenario(wca, qs):
    """70 robots, a full wave and a tail, on plans whose durations differ per robot and per step: KEEP, AUTO and explicit stages, sides 0,
    1 and AUTO after 90 ticks, and a second call after 160 with no goal_result() in between - its AUTO reads durations the first call
    still owes.  Twin A is fed through replan_goal(timing=), call by call, with the restatement's merge stages and sides.  The comparisons
    of the walk scenario over every robot whose restated decision margins are >= 1e-9 (at most 2 % may be left out): goal_result() of the
    second call against A's and the restatement's, both plans, the logs of A and B; robots kept in both calls bit-identical to a handle
    never replanned; oracle/tick_spec.py walks robots 0 to 3.  wcqp_tick_get_goal_timing equals goal_result()'s rows, and every row is a
    valid split: min <= ss + ds <= max, ds = min(max(floor(m rho + 0.5), 1), m - 1).  The batch of 1 - robot 0 alone - against row 0
    within 1e-9."""
    sc = gt.batch_scenario(wca)
    c1, c2 = sc["c1"], sc["c2"]
    ref2 = gt.oracle_runs(wca, qs)[1]
    B, K, tm = sc["B"], gt.K_WALK, sc["timing"]
    del FAILED[:]
    left_out = gr.left_out(sc)
    print("left out", int(left_out.sum()), "of", B)
    assert left_out.mean() <= 0.02
    rows = np.nonzero(~left_out)[0]
    pl = wca.UnicyclePlanner(**gt.WALK)
    a, b, n = (gr.pipe(wca, B) for _ in range(3))
    for h in (a, b, n):
        _upload(h, sc, pl)
    n.run(MAXT)
    _two_calls(sc, pl, b)
    res2 = b.goal_result()
    rc, ss, ds = _timing_rows(wca, b, B, K)
    assert rc == 0 and np.array_equal(ss, res2["ss_ticks"]) and np.array_equal(ds, res2["ds_ticks"])
    taken = np.arange(K)[None, :] < res2["n_steps"][:, None]
    m = ss + ds
    assert not ss[~taken].any() and not ds[~taken].any() and taken.sum() >= 100
    assert (m[taken] >= tm["min_step_ticks"]).all() and (m[taken] <= tm["max_step_ticks"]).all()
    assert [(int(x), int(y)) for x, y in zip(ss[taken], ds[taken])] == [ut.durations(int(v), tm["switch_over_swing_ratio"]) for v in m[taken]]
    a.run(gt.T1)
    got1 = a.replan_goal(c1["M"], sc["goals1"], pl, c1["fside"], gt.FD, timing=tm)
    _close("plan A after the first call against the restatement", a.plan_window(), c1["plan"], WINDOW, rows)
    a.run(gt.T2 - gt.T1)
    got2 = a.replan_goal(c2["M"], sc["goals2"], pl, c2["fside"], gt.FD, timing=tm)
    _decisions(got1, c1["r"], rows)
    _result_matches(res2, c2, rows)
    _decisions(res2, got2, rows)
    same = _close("result A against B", got2, res2, NUMBERS, rows)
    same = _windows(a, b, c2, rows) and same
    a.run(MAXT - gt.T2); b.run(MAXT - gt.T2)
    oa, ob, on = a.download(), b.download(), n.download()
    same = _close("logs A against B", oa, ob, KEYS, rows) and same
    print("A and B bit-identical:", same)
    assert np.array_equal(oa["ik_fail"][rows], ob["ik_fail"][rows]) and np.array_equal(oa["mpc_fail"][rows], ob["mpc_fail"][rows])
    _against_oracle(ob, ref2, gt.ORACLE_ROWS)
    kept = np.nonzero((c1["M"] < 0) & (c2["M"] < 0))[0]
    assert kept.size >= 3
    for k in KEYS:
        assert np.array_equal(_rows(ob[k], kept, k), _rows(on[k], kept, k)), k
    # robot 0 alone: its first call is all-KEEP (nothing enqueued), its second AUTO
    one = gt.batch_scenario(wca, 1)
    s = gr.pipe(wca, 1)
    _upload(s, one, pl)
    _two_calls(sc, pl, s, rows=slice(0, 1))
    r1 = s.goal_result()
    s.run(MAXT - gt.T2)
    o1, w1, wb = s.download(), s.plan_window(), b.plan_window(0, 1)
    assert r1["merge_stage"][0] == res2["merge_stage"][0] >= gt.T2 + gt.LEAD2 and r1["first_side"][0] == res2["first_side"][0]
    _decisions(r1, res2, [0])
    same1 = _close("one robot against row 0", r1, res2, NUMBERS, [0])
    same1 = _close("one robot's plan against row 0", w1, wb, WINDOW, [0]) and same1
    same1 = _close("one robot's logs against row 0", o1, ob, KEYS, [0]) and same1
    print("the batch of 1 and row 0 bit-identical:", same1)
    assert not FAILED, FAILED


# ---------------------------------------------------------------------------------------------------------------- owed durations

@pytest.mark.gpu
def test_owed_durations_decide_a_later_footstep_replan(wca):
    """After a timed goal call and no goal_result(), robot 2's durations exist on the device only.  replan_footsteps (timed) at an explicit
    stage inside a single support of the DEVICE-CHOSEN timeline - a stage the nominal timeline has in a double support - is refused with
    the plan unchanged; at the first stage of the double support that follows it is accepted, and the walk goes on to its end."""
    sc = gt.walk_scenario(wca)
    c = sc["c1"]
    tm = sc["timing"]
    x, y = gt.single_support_probe(c["force"], 2, tm["nominal_step_ticks"], tm["switch_over_swing_ratio"], sc["t1"])
    O, fo, ss, ds = gt.timeline(c["force"], 2)
    nss, nds = ut.durations(tm["nominal_step_ticks"], tm["switch_over_swing_ratio"])
    assert gmt.in_single_support(O, fo, ss, ds, x) and not gmt.in_single_support(O, fo, ss, ds, y) and y > x >= sc["t1"]
    assert gmt.merge_allowed(O, fo, [nss] * len(ss), [nds] * len(ss), x, sc["t1"], gt.T)      # (the nominal timeline would let x through)
    pl = wca.UnicyclePlanner(**gt.WALK)
    h = gr.pipe(wca, 3)
    _upload(h, sc, pl)
    h.run(sc["t1"])
    h.replan_goals(sc["goals1"], pl, gt.FD, merge_stage=sc["merge1"], min_lead_ticks=sc["lead1"], timing=tm)
    K = gt.K_WALK
    stop = dict(n_steps=np.zeros(3, np.int32), side=np.zeros((3, K), np.uint8), target=np.zeros((3, K, 3)), ss_ticks=np.zeros((3, K), np.int32),
                ds_ticks=np.zeros((3, K), np.int32))
    with pytest.raises(wca.WcqpError, match="invalid|INVALID"):
        h.replan_footsteps(np.array([-1, -1, x], np.int32), stop, gt.FD)
    w1 = h.plan_window()
    with pytest.raises(wca.WcqpError, match="invalid|INVALID"):
        h.replan_footsteps(np.array([-1, -1, x], np.int32), stop, gt.FD)
    _same_windows(w1, h.plan_window())
    del FAILED[:]
    _close("the plan behind the refused calls against the restatement", w1, c["plan"], WINDOW, np.arange(3))
    assert np.array_equal(w1["contact"], c["plan"]["contact"]) and not FAILED, FAILED
    h.replan_footsteps(np.array([-1, -1, y], np.int32), stop, gt.FD)
    w2 = h.plan_window()
    for k in w1:
        assert np.array_equal(w1[k][:, :y], w2[k][:, :y]) and np.array_equal(w1[k][:2], w2[k][:2]), k
    assert not np.array_equal(w1["ref_traj"][2], w2["ref_traj"][2]) and (w2["contact"][2, y:] & 3 == 3).all()
    h.run(MAXT - sc["t1"])
    o = h.download()
    assert o["tick"] == MAXT and not o["ik_fail"][:2].any()


# ---------------------------------------------------------------------------------------------------------------- other ends, other handles

@pytest.mark.gpu
def test_too_late_and_all_keep(wca):
    """an all-KEEP call and a call whose every AUTO robot is TOO_LATE (a lead past the plan's T stages) return WCQP_OK with nothing enqueued:
    the plan is bit-identical, the result rows and the timing rows are zero; a TOO_LATE robot next to one that replans at an explicit stage
    keeps its rows bit for bit"""
    sc = gt.walk_scenario(wca)
    tm = sc["timing"]
    pl = wca.UnicyclePlanner(**gt.WALK)
    h = gr.pipe(wca, 3)
    _upload(h, sc, pl)
    w0 = h.plan_window()
    goals = np.tile(np.array(gt.GOAL1), (3, 1))
    for kw, status in ((dict(merge_stage=np.full(3, gt.KEEP, np.int32)), gt.KEPT), (dict(min_lead_ticks=gt.T), gt.TOO_LATE)):
        h.replan_goals(goals, pl, gt.FD, timing=tm, **kw)
        r = h.goal_result()
        assert "ss_ticks" in r and (r["status"] == status).all() and not any(r[k].any() for k in r if k != "status")
        rc, ss, ds = _timing_rows(wca, h, 3, gt.K_WALK)
        assert rc == 0 and not ss.any() and not ds.any()
    _same_windows(w0, h.plan_window())
    O, fo, ss0, ds0 = gt.timeline(sc["force0"], 1)
    M = gmt.merge_points(O, fo, ss0, ds0)[0][0] + 3            # three stages into robot 1's first inner double support
    h.replan_goals(goals, pl, gt.FD, merge_stage=np.array([gt.AUTO, M, gt.KEEP], np.int32), min_lead_ticks=gt.T, timing=tm)
    r = h.goal_result()
    assert r["status"].tolist()[::2] == [gt.TOO_LATE, gt.KEPT] and r["status"][1] >= 0 and r["merge_stage"].tolist() == [0, M, 0]
    assert r["first_side"][1] == (0 if sc["plan0"]["contact"][1, M - 1] & 4 else 1)
    assert r["n_steps"][1] >= 1 and (r["ss_ticks"][1, :r["n_steps"][1]] >= 1).all() and not r["ss_ticks"][[0, 2]].any() and not r["ds_ticks"][[0, 2]].any()
    w2 = h.plan_window()
    for k in w0:
        assert np.array_equal(w0[k][[0, 2]], w2[k][[0, 2]]) and np.array_equal(w0[k][1, :M], w2[k][1, :M]), k
    assert not np.array_equal(w0["ref_traj"][1], w2["ref_traj"][1])
    h.run(MAXT)
    assert h.download()["tick"] == MAXT


@pytest.mark.gpu
def test_refusals_leave_the_handle_as_it_was(wca):
    """on an uploaded timed handle: NULL tm, planner, struct and goal; a tm with min_step_ticks = 1 and one with min > nominal; a non-finite
    goal of a robot that replans; a side of 7; a negative lead; first_ds_ticks = 0; a merge stage of -3, of 0, a consumed one, T, and one
    inside a single support of the timed plan in force (which the nominal timeline has in a double support) - each WCQP_E_INVALID, the plan
    bit-identical afterwards, and the next good call works.  An untimed plan is UNSUPPORTED, a handle not uploaded INVALID;
    wcqp_tick_get_goal_timing is INVALID before any goal call and after an untimed call on an untimed handle."""
    sc = gt.walk_scenario(wca)
    timing = sc["timing"]
    L = wca.capi.lib()
    pl = wca.UnicyclePlanner(**gt.WALK)
    tm = pl._timing_struct(timing)
    h = gr.pipe(wca, 3)
    goals = np.tile(np.array(gt.GOAL1), (3, 1))
    g_ok = wca.capi.TickGoals(goals.ctypes.data, None, None, gt.FD, 20)

    def call(handle=h, planner=pl._h, t=tm, g=g_ok):
        return L.wcqp_tick_replan_goals_timed(handle._h, planner, None if t is None else C.byref(t), None if g is None else C.byref(g), None)
    assert call() == WCQP_E_INVALID                                            # not uploaded
    _upload(h, sc, pl)
    h.run(40)
    w0 = h.plan_window()
    assert _timing_rows(wca, h, 3, gt.K_WALK)[0] == WCQP_E_INVALID              # before any goal call
    assert call(planner=None) == WCQP_E_INVALID and call(t=None) == WCQP_E_INVALID and call(g=None) == WCQP_E_INVALID
    assert call(g=wca.capi.TickGoals(None, None, None, gt.FD, 20)) == WCQP_E_INVALID
    assert call(t=pl._timing_struct(dict(timing, min_step_ticks=1))) == WCQP_E_INVALID
    assert call(t=pl._timing_struct(dict(timing, min_step_ticks=timing["nominal_step_ticks"] + 1))) == WCQP_E_INVALID
    bad_side = np.array([0, 7, 1], np.uint8)
    assert call(g=wca.capi.TickGoals(goals.ctypes.data, None, bad_side.ctypes.data, gt.FD, 20)) == WCQP_E_INVALID
    assert call(g=wca.capi.TickGoals(goals.ctypes.data, None, None, gt.FD, -1)) == WCQP_E_INVALID
    assert call(g=wca.capi.TickGoals(goals.ctypes.data, None, None, 0, 20)) == WCQP_E_INVALID
    with pytest.raises(wca.WcqpError, match="unsupported|UNSUPPORTED"):         # (the untimed call on a timed plan, as before)
        h.replan_goals(goals, pl, gt.FD)
    nan = goals.copy(); nan[1, 0] = np.inf
    with pytest.raises(wca.WcqpError, match="invalid|INVALID"):
        h.replan_goals(nan, pl, gt.FD, timing=timing)
    # robot 1 turns: its steps are shorter than nominal, and the second stage of its second single support lies in the nominal timeline's
    # first inner double support
    O, fo, ss, ds = gt.timeline(sc["force0"], 1)
    inside = gmt.step_starts(O, fo, ss, ds)[1] + 1
    nss, nds = ut.durations(timing["nominal_step_ticks"], timing["switch_over_swing_ratio"])
    assert gmt.in_single_support(O, fo, ss, ds, inside) and gmt.merge_allowed(O, fo, [nss] * len(ss), [nds] * len(ss), inside, 40, gt.T)
    for M in (-3, 0, 39, gt.T, inside):
        with pytest.raises(wca.WcqpError, match="invalid|INVALID"):
            h.replan_goals(goals, pl, gt.FD, merge_stage=np.array([gt.KEEP, M, gt.AUTO], np.int32), timing=timing)
    assert _timing_rows(wca, h, 3, gt.K_WALK)[0] == WCQP_E_INVALID              # (still no goal call that was taken)
    _same_windows(w0, h.plan_window())
    h.replan_goals(nan, pl, gt.FD, merge_stage=np.array([gt.AUTO, gt.KEEP, gt.AUTO], np.int32), timing=timing)      # (the Inf sits in a KEEP row)
    want = [gmt.merge_auto(*gt.timeline(sc["force0"], i), 40, 20, gt.T) for i in (0, 2)]
    r = h.goal_result()
    assert r["merge_stage"].tolist() == [want[0], 0, want[1]] and (r["n_steps"][[0, 2]] >= 1).all()
    assert _timing_rows(wca, h, 3, gt.K_WALK)[0] == 0
    # an untimed plan: the timed call is UNSUPPORTED and changes nothing, the untimed call works, and the timing getter stays INVALID
    usc = gr.walk_scenario(wca)
    upl = wca.UnicyclePlanner(**gr.WALK)
    u = gr.pipe(wca, 3)
    gr.upload(wca, u, usc, upl)
    u0 = u.plan_window()
    assert call(handle=u, planner=upl._h) == WCQP_E_UNSUPPORTED
    with pytest.raises(wca.WcqpError, match="unsupported|UNSUPPORTED"):
        u.replan_goals(goals, upl, gt.FD, timing=timing)
    _same_windows(u0, u.plan_window())
    assert _timing_rows(wca, u, 3, gr.K_WALK)[0] == WCQP_E_INVALID
    u.replan_goals(goals, upl, gt.FD, merge_stage=np.array([gt.KEEP, gt.KEEP, gt.AUTO], np.int32))
    res = u.goal_result()
    assert set(res) == {k for k, _, _ in wca.capi.GOAL_RESULT} and res["merge_stage"][2] > 0
    assert _timing_rows(wca, u, 3, gr.K_WALK)[0] == WCQP_E_INVALID


def _ik(wca, R):
    return wca.IkSolver(form=wca.IK_FORM_QPOASES, neck_weight=R["neck_weight"] * np.eye(3), joint_reg_weights=np.array(R["reg_w"], float),
                        joint_reg_gains=np.array(R["reg_k"], float), joint_reg_rad=np.deg2rad(wca.synth.WALK_POSTURE_DEG),
                        v_max=wca.synth.WALK_VMAX.copy(), k_pos_com=R["k_pos_com"], k_pos_foot=R["k_pos_foot"], k_att_foot=R["k_att_foot"],
                        k_neck=R["k_neck"])


def _per_step(fs, B, K):
    """the common durations of an untimed footstep batch, changed per robot and per step"""
    i, k = np.arange(B)[:, None], np.arange(K)[None, :]
    return dict(ss_ticks=(int(fs["ss_ticks"]) + (i % 3) - 2 * (k % 2)).astype(np.int32), ds_ticks=(int(fs["ds_ticks"]) + 2 * (i % 2) + (k % 3)).astype(np.int32))


@pytest.mark.gpu
def test_resident_plan(wca):
    """a streamed EXTERNAL handle with resident_plan=True and timed footsteps, 80 ticks in: after set_desired_from_plan stage t = 80 is in
    hand, so an explicit M = t is refused with the handle unchanged, and AUTO with a lead of 5 takes the restated stages of every robot's own
    timeline, all >= t + 1 + 5; the walk goes on, and below each robot's merge stage the plan is bit for bit the old one"""
    import robots
    from helpers import zmp_gains as zg
    fs = rs.scenario(wca)[0]
    B, t, lead, fd = rs.B, 80, 5, 20
    dur = _per_step(fs, B, rs.K)
    timing = dict(min_step_ticks=80, max_step_ticks=120, nominal_step_ticks=100, time_weight=2.5, position_weight=1.0, switch_over_swing_ratio=0.7)
    pl = wca.UnicyclePlanner(**dict(gr.WALK, step_ticks=1, max_steps=rs.K))
    R = robots.ROBOTS[rs.ROBOT]
    pipe = wca.TickPipeline(B, rs.MAXT, wca.MpcSolver(horizon=50), _ik(wca, R), log_ticks=rs.MAXT, k_com=R["k_com"], k_zmp=R["k_zmp"],
                            kin=wca.KinModel(wca.synth.icub_like_model()), external_feedback=True, streamed_trajectories=True,
                            neck_additional_rotation=np.array(R["additional_rotation"]), resident_plan=True, dcm_controller="reactive", k_dcm=rs.K_DCM,
                            zmp_gain_scheduling=True, **zg.ZMP_SCHEDULE[rs.ROBOT])
    pipe.upload_footsteps(fs, dict(fs, **dur))
    assert pipe.info()["plan_timed"] is True
    w0 = pipe.plan_window()

    def tick(k, stage=True):
        if stage:
            pipe.set_desired_from_plan()
        pipe.set_feedback_host(w0["ref_traj"][:, k].copy(), fs["com0"], w0["u_init"], fs["q0"])
        pipe.run(1)
    for k in range(t):
        tick(k)
    goals = np.tile(np.array([0.03, 0.01]), (B, 1))
    pipe.set_desired_from_plan()
    with pytest.raises(wca.WcqpError, match="invalid|INVALID"):
        pipe.replan_goals(goals, pl, fd, merge_stage=np.full(B, t, np.int32), timing=timing)
    _same_windows(w0, pipe.plan_window())
    pipe.replan_goals(goals, pl, fd, min_lead_ticks=lead, timing=timing)
    r = pipe.goal_result()
    want = gmt.merge_auto_batch(np.zeros(B, int), np.full(B, rs.FIRST_DS), fs["n_steps"], dur["ss_ticks"], dur["ds_ticks"], t + 1, lead, rs.T)
    print("merge stages", r["merge_stage"].tolist())
    assert np.array_equal(r["merge_stage"], want) and (r["merge_stage"] >= t + 1 + lead).all() and (r["status"] >= 0).all() and len(set(want.tolist())) >= 3
    assert np.array_equal(r["first_side"], np.where(w0["contact"][np.arange(B), want - 1] & 4, 0, 1))
    taken = np.arange(rs.K)[None, :] < r["n_steps"][:, None]
    m = (r["ss_ticks"] + r["ds_ticks"])
    assert taken.any() and (m[taken] >= 80).all() and (m[taken] <= 120).all() and not m[~taken].any()
    tick(t, stage=False)
    for k in range(t + 1, t + 4):
        tick(k)
    w2 = pipe.plan_window()
    for i in range(B):
        for k in ("left_traj", "right_traj", "contact", "ref_traj"):
            assert np.array_equal(w0[k][i, :want[i]], w2[k][i, :want[i]]), (k, i)
    moved = [i for i in range(B) if not np.array_equal(w0["ref_traj"][i], w2["ref_traj"][i])]
    assert len(moved) >= B - 2 and pipe.download()["tick"] == t + 4


@pytest.mark.gpu
def test_position_handle(wca):
    """three robots of the POSITION tick's scenario (helpers/position_tick.py: three steps behind 10 stages, 70 ticks) with timed footsteps
    uploaded: run(30), replan_goals(timing=) with AUTO and a lead of 5 - the restated merge stages of the robots' own timelines -, run(40).
    Knows no restatement of the run: at q_log[t], with the left sole anchored on stage t's pose of the replanned plan, the stand-alone
    kinematics put the right sole on stage t's pose and the CoM at its height to 1e-9 - every robot, every tick."""
    import robots
    sc = pk.scenario()
    B, T = 3, pk.T
    fs = gr.rows_of(sc["fs"], np.arange(B), pk.B13)
    dur = _per_step(fs, B, fs["side"].shape[1])
    R = robots.ROBOTS[pk.ROBOT]
    pipe = wca.TickPipeline(B, T, wca.MpcSolver(horizon=pk.N, com_height=pk.H), _ik(wca, R), log_ticks=T, k_com=R["k_com"], k_zmp=R["k_zmp"],
                            kin=wca.KinModel(sc["model"]), planned_trajectories=True, neck_additional_rotation=pk.ADD_ROT,
                            **pk.controller_kwargs("reactive_gs"), ik_mode="position", position_ik=dict(q_reg=sc["q_reg"], max_iter=30))
    per = int(fs["ss_ticks"]) + int(fs["ds_ticks"])
    timing = dict(min_step_ticks=per - 5, max_step_ticks=per + 5, nominal_step_ticks=per, time_weight=2.5, position_weight=1.0, switch_over_swing_ratio=0.7)
    pl = wca.UnicyclePlanner(**dict(gr.WALK, step_ticks=1, max_steps=3, max_linear_velocity=0.06, max_angular_velocity=0.3))
    pipe.upload_footsteps(fs, dict(fs, **dur))
    assert pipe.info()["plan_timed"] is True and pipe.info()["ik_mode"] == "position"
    pipe.run(30)
    pipe.replan_goals(np.array([[0.02, 0.0], [0.015, 0.01], [0.02, -0.005]]), pl, 8, min_lead_ticks=5, timing=timing)
    pipe.run(T - 30)
    r = pipe.goal_result()
    want = gmt.merge_auto_batch(np.zeros(B, int), np.full(B, int(fs["first_ds_ticks"])), fs["n_steps"], dur["ss_ticks"], dur["ds_ticks"], 30, 5, T + pk.N + 1)
    print("merge", r["merge_stage"].tolist(), "n_steps", r["n_steps"].tolist(), "status", r["status"].tolist(), "durations", (r["ss_ticks"] + r["ds_ticks"]).tolist())
    assert np.array_equal(r["merge_stage"], want) and (want >= 35).all() and (want < T).all() and (r["n_steps"] >= 1).all()
    o, w = pipe.download(), pipe.plan_window(stage0=0, m=T)
    assert o["tick"] == T and not o["ik_fail"].any()
    kin = wca.KinModel(sc["model"])
    qf = np.ascontiguousarray(o["q_log"].reshape(T * B, 23))
    ident = np.tile(np.concatenate([np.zeros(3), np.eye(3).reshape(9)]), (T * B, 1))
    k0 = kin.jacobians_host(ident, qf, state=np.zeros((T * B, 87)))["state"]
    left = np.swapaxes(w["left_traj"], 0, 1).reshape(T * B, 12)
    pL, RL = k0[:, 0:3], k0[:, 3:12].reshape(-1, 3, 3)
    Rb = left[:, 3:12].reshape(-1, 3, 3) @ np.swapaxes(RL, 1, 2)
    base = np.concatenate([left[:, :3] - np.einsum("bij,bj->bi", Rb, pL), Rb.reshape(-1, 9)], axis=1)
    k = kin.jacobians_host(np.ascontiguousarray(base), qf, state=np.zeros((T * B, 87)))["state"]
    right = np.swapaxes(w["right_traj"], 0, 1).reshape(T * B, 12)
    height = np.swapaxes(w["com_height"], 0, 1).reshape(T * B)
    e_left, e_right, e_h = np.abs(k[:, 0:12] - left).max(), np.abs(k[:, 12:24] - right).max(), np.abs(k[:, 68] - height).max()
    print("left sole", e_left, "right sole", e_right, "CoM height", e_h)
    assert e_left <= 1e-9 and e_right <= 1e-9 and e_h <= 1e-9
