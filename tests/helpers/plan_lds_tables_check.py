"""Run by tests/test_plan_lds_tables.py, one case per process (torch first, then libwcqp): the plan kernels read their launch-invariant
tables - the MPC's gain blocks Gr, the IK's per-variable tables kq, qreg, vlo, vhi, sd, isd - from a block of LDS that every wave fills
once (csrc/ik4_device.h: PlanTables; csrc/mpc.hip: mpc_plan_kernel).  Every case compares a plan with the single wcqp_mpc_solve_device /
wcqp_ik_solve_device calls of the same records, bit for bit, on every output array of every record.

    plan_lds_tables_check.py tables <qpoases|osqp> <ways>      per-joint solver tables (a lane that reads a neighbour's entry changes the result)
    plan_lds_tables_check.py horizon <N>                       combined, MPC-only and IK-only plans at horizon N
    plan_lds_tables_check.py pairs                             two plans of two solver pairs back to back on one stream
    plan_lds_tables_check.py driver                            4096 robots, 16 ways, 20 records, also against the goldens"""
import os, sys
import numpy as np
import torch
torch.cuda.init()
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import walking_controllers_amd as wca

DEV = torch.device("cuda", 0)
MKEYS = ("x0", "ref", "u_prev", "hull_A", "hull_b", "hull_nc")
IKEYS = ("J_left", "J_right", "J_neck", "J_com", "q", "state")
MOUT, IOUT = ("u0", "ms", "ma", "mm"), ("dq", "st", "lo", "up", "fe", "it")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def outs(B):
    z = lambda *s, dt=torch.float64: torch.zeros(*s, dtype=dt, device=DEV)
    return dict(u0=z(B, 2), ms=torch.full((B,), -1, dtype=torch.int32, device=DEV), ma=z(B, dt=torch.int32), mm=z(B),
                dq=z(B, 23), st=torch.full((B,), -1, dtype=torch.int32, device=DEV), lo=z(B, dt=torch.int32), up=z(B, dt=torch.int32),
                fe=z(B, 12), it=z(B, dt=torch.int32))


def input_sets(B, R, horizon, seed=0):
    sets = []
    for n in range(R):
        mb = wca.synth.synth_mpc_batch(B, seed=50 + seed + n, uprev_sigma=0.03, horizon=horizon)
        ib = wca.synth.synth_ik_batch(B, seed=150 + seed + n)
        sets.append(({k: dev(mb[k]) for k in MKEYS}, {k: dev(ib[k]) for k in IKEYS}))
    return sets


def single_calls(mpc, ik, B, sets):
    """the reference of every case: one wcqp_mpc_solve_device and one wcqp_ik_solve_device call per record"""
    ref = [outs(B) for _ in sets]
    torch.cuda.synchronize()
    for (m, i), o in zip(sets, ref):
        if mpc is not None:
            mpc.solve_device(B, m["x0"].data_ptr(), m["ref"].data_ptr(), m["ref"].shape[1], m["u_prev"].data_ptr(), m["hull_A"].data_ptr(),
                             m["hull_b"].data_ptr(), m["hull_nc"].data_ptr(), o["u0"].data_ptr(), o["ms"].data_ptr(), o["ma"].data_ptr(), o["mm"].data_ptr(), 0)
        if ik is not None:
            ik.solve_device(B, i["J_left"].data_ptr(), i["J_right"].data_ptr(), i["J_neck"].data_ptr(), i["J_com"].data_ptr(), i["q"].data_ptr(),
                            i["state"].data_ptr(), o["dq"].data_ptr(), o["st"].data_ptr(), o["lo"].data_ptr(), o["up"].data_ptr(), o["fe"].data_ptr(), o["it"].data_ptr(), 0)
    torch.cuda.synchronize()
    return ref


def records(sets, got, with_mpc=True, with_ik=True):
    recs = (wca.capi.QpStep * len(sets))()
    for r, (m, i), o in zip(recs, sets, got):      # every record its own outputs: whatever the way, nothing is shared
        if with_mpc:
            r.x0, r.ref, r.ref_len, r.u_prev = m["x0"].data_ptr(), m["ref"].data_ptr(), m["ref"].shape[1], m["u_prev"].data_ptr()
            r.hull_A, r.hull_b, r.hull_nc = m["hull_A"].data_ptr(), m["hull_b"].data_ptr(), m["hull_nc"].data_ptr()
            r.u0, r.mpc_status, r.mpc_active, r.mpc_margin = o["u0"].data_ptr(), o["ms"].data_ptr(), o["ma"].data_ptr(), o["mm"].data_ptr()
        if with_ik:
            r.J_left, r.J_right, r.J_neck, r.J_com = (i[k].data_ptr() for k in ("J_left", "J_right", "J_neck", "J_com"))
            r.q, r.state = i["q"].data_ptr(), i["state"].data_ptr()
            r.dq, r.ik_status, r.active_lower, r.active_upper = o["dq"].data_ptr(), o["st"].data_ptr(), o["lo"].data_ptr(), o["up"].data_ptr()
            r.foot_err, r.iters = o["fe"].data_ptr(), o["it"].data_ptr()
    return recs


def same(ref, got, keys, what):
    for n, (a, b) in enumerate(zip(ref, got)):
        for k in keys:
            assert torch.equal(a[k], b[k]), (what, "record", n, k)


def clear(got):
    for o in got:
        for k, v in o.items():
            v.fill_(-1) if k in ("ms", "st") else v.zero_()


def run_plan(mpc, ik, B, sets, ways, ref, what):
    """a plan over `sets` (mpc / ik None: an IK-only / MPC-only plan), launched and replayed: both launches against the single calls"""
    got = [outs(B) for _ in sets]
    recs = records(sets, got, mpc is not None, ik is not None)
    plan = wca.capi.QpPlan(mpc, ik, B, recs, ways=ways)
    st = torch.cuda.Stream(DEV)
    keys = (MOUT if mpc is not None else ()) + (IOUT if ik is not None else ())
    for launch in range(2):
        clear(got)
        torch.cuda.synchronize()
        plan.enqueue(st.cuda_stream)
        torch.cuda.synchronize()
        same(ref, got, keys, (what, "launch", launch))
    plan.close()
    return got


def per_joint_ik(form):
    """an IK solver whose tables differ in every entry: bounds, weights (sd / isd per column), gains and posture per joint, and a
    neck weight with a full Cholesky factor (tests/ik_parameter_cases.py: W), so that the plan kernels see L01, L02, L12 != 0"""
    k = np.arange(23.0)
    W = np.array([[3.6, 1.1, 1.0], [1.1, 8.2, 3.5], [1.0, 3.5, 3.2]])
    return wca.IkSolver(form=form, v_max=0.04 + 0.013 * k, v_min=-(0.05 + 0.011 * k[::-1]), joint_reg_weights=1.0 + 0.37 * k, neck_weight=W,
                        joint_reg_gains=3.0 + 0.21 * k, joint_reg_rad=np.deg2rad(wca.synth.ICUB_JOINT_REG_DEG) + 0.02 * (k - 11.0),
                        jacobian_structure=wca.IK_JAC_MIXED)


def case_tables(form, ways):
    B, R = 5, 3                  # two workgroups, one ragged
    mpc, ik = wca.MpcSolver(horizon=50), per_joint_ik(wca.IK_FORM_QPOASES if form == "qpoases" else wca.IK_FORM_OSQP)
    sets = input_sets(B, R, 50)
    ref = single_calls(mpc, ik, B, sets)
    got = run_plan(mpc, ik, B, sets, ways, ref, ("tables", form, ways))
    run_plan(None, ik, B, sets, ways, ref, ("tables ik-only", form, ways))
    n_active = sum(int(((o["lo"] | o["up"]) != 0).sum()) for o in got)
    print("robots with active bounds:", n_active, "of", B * R, "status:", [o["st"].tolist() for o in got])
    if form == "qpoases":
        assert n_active > 0, "the tight bounds must be active somewhere"


def case_horizon(N):
    B, R = 5, 3
    mpc, ik = wca.MpcSolver(horizon=N), per_joint_ik(wca.IK_FORM_QPOASES)
    sets = input_sets(B, R, N, seed=N)
    ref = single_calls(mpc, ik, B, sets)
    for ways in (2, 0):
        run_plan(mpc, ik, B, sets, ways, ref, ("combined", N, ways))
        run_plan(None, ik, B, sets, ways, ref, ("ik-only", N, ways))
    run_plan(mpc, None, B, sets, 2, ref, ("mpc-only", N))
    assert all((o["ms"] >= 0).all() for o in ref)


def case_pairs():
    B, R = 5, 3
    pa = (wca.MpcSolver(horizon=50), per_joint_ik(wca.IK_FORM_QPOASES))
    pb = (wca.MpcSolver(horizon=21, Q=[[5000.0, 100.0], [100.0, 9000.0]], R=[[4.0e6, 0.0], [0.0, 7.0e6]]),
          wca.IkSolver(form=wca.IK_FORM_QPOASES, v_max=0.3, joint_reg_weights=np.linspace(3.0, 0.5, 23), jacobian_structure=wca.IK_JAC_MIXED))
    sa, sb = input_sets(B, R, 50, seed=7), input_sets(B, R, 21, seed=9)
    ra, rb = single_calls(pa[0], pa[1], B, sa), single_calls(pb[0], pb[1], B, sb)
    assert not torch.equal(ra[0]["dq"], single_calls(None, pb[1], B, sa)[0]["dq"]), "the two IK solvers must differ on the same inputs"
    for kinds in ((True, True), (True, False), (False, True)):        # combined, MPC-only, IK-only
        ga, gb = [outs(B) for _ in sa], [outs(B) for _ in sb]
        plans = [wca.capi.QpPlan(p[0] if kinds[0] else None, p[1] if kinds[1] else None, B, records(s, g, *kinds), ways=2)
                 for p, s, g in ((pa, sa, ga), (pb, sb, gb))]
        keys = (MOUT if kinds[0] else ()) + (IOUT if kinds[1] else ())
        st = torch.cuda.Stream(DEV)
        for launch in range(2):            # A B, then A B again: a launch must see its own handle's tables
            clear(ga); clear(gb)
            torch.cuda.synchronize()
            for p in plans:
                p.enqueue(st.cuda_stream)
            torch.cuda.synchronize()
            same(ra, ga, keys, ("pair A", kinds, launch))
            same(rb, gb, keys, ("pair B", kinds, launch))
        for p in plans:
            p.close()


def case_driver():
    """the geometry bench.py times in the driver's form: 4096 robots, 16 ways, 20 records, every record an input set of its own (the
    golden batch rolled by k B / K rows), every record against the goldens as bench.py checks them - and against the single calls"""
    B, R, ways, MARGIN = 4096, 20, 16, 1e-7
    mb, ib = wca.synth.synth_mpc_batch(B, seed=1234), wca.synth.synth_ik_batch(B, seed=4321)
    base = ({k: dev(mb[k]) for k in MKEYS}, {k: dev(ib[k]) for k in IKEYS})
    roll = lambda d, n: {k: torch.roll(v, shifts=n * (B // R), dims=0).contiguous() for k, v in d.items()}
    sets = [base] + [(roll(base[0], n), roll(base[1], n)) for n in range(1, R)]
    mpc, ik = wca.MpcSolver(), wca.IkSolver(form=wca.IK_FORM_QPOASES, v_max=0.5, jacobian_structure=wca.IK_JAC_MIXED)
    ref = single_calls(mpc, ik, B, sets)
    got = run_plan(mpc, ik, B, sets, ways, ref, "driver")
    gm = np.load(os.path.join(ROOT, "tests", "golden", "mpc_cfg2_b4096.npz"), allow_pickle=False)
    gi = np.load(os.path.join(ROOT, "tests", "golden", "ik_qpoases_v050_b4096.npz"), allow_pickle=False)
    sure_m = (gm["mu_min_active"] > MARGIN) & (gm["slack_min_inactive"] > MARGIN)
    sure_i = (gi["mu_min_active"] > MARGIN) & (gi["slack_min_inactive"] > MARGIN) & (gi["status"] == 0)
    for n in range(R):
        inst = (np.arange(B) - n * (B // R)) % B          # output row -> instance of the unrotated batch
        o = {k: v.cpu().numpy() for k, v in got[n].items()}
        m = inst < int(gm["count"])
        assert (o["ms"][m] == 0).all() and np.abs(o["u0"][m] - gm["u0"][inst[m]]).max() <= 1e-9, n
        s_ = sure_m[inst[m]]
        assert np.array_equal(o["ma"][m].astype(np.uint32)[s_], gm["active"][inst[m]][s_]), n
        m = inst < int(gi["count"])
        gidx = inst[m]
        assert np.array_equal(o["st"][m], gi["status"][gidx]), n
        assert np.abs(o["dq"][m] - gi["dq"][gidx]).max() <= 1e-9, n
        s_ = sure_i[gidx]
        assert np.array_equal(o["lo"][m].astype(np.uint32)[s_], gi["active_lower"][gidx][s_]), n
        assert np.array_equal(o["up"][m].astype(np.uint32)[s_], gi["active_upper"][gidx][s_]), n


if __name__ == "__main__":
    case = sys.argv[1]
    if case == "tables":
        case_tables(sys.argv[2], int(sys.argv[3]))
    elif case == "horizon":
        case_horizon(int(sys.argv[2]))
    elif case == "pairs":
        case_pairs()
    elif case == "driver":
        case_driver()
    else:
        raise SystemExit("unknown case " + case)
    print("plan lds tables ok")
