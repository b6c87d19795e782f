"""
Child process of tests/test_size_limits.py: calls every entry point whose kernels use 32-bit addressing at the sizes named on the
command line (a JSON list of cases) with DUMMY non-NULL pointers, and prints the return codes as one JSON line.

The parent starts it with no HIP device visible, so that a size the guard admits ends in WCQP_E_HIP ("no device") instead of a launch
over the dummy pointers; the probe REFUSES to make any call when it can see a device after all.
"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

DUMMY = 0x10000           # non-NULL, 16-byte aligned, never dereferenced by a guard


def main():
    import walking_controllers_amd as wca
    capi = wca.capi
    if wca.device_count() != 0:
        print("size_limit_probe: a HIP device is visible - refusing to call solve entry points with dummy pointers", file=sys.stderr)
        return 3
    lib = capi.lib()
    cases = json.loads(sys.argv[1])
    out = []
    for c in cases:
        kind, batch = c["entry"], int(c["batch"])
        ref_len = int(c.get("ref_len", 1))
        horizon = int(c.get("horizon", 50))
        mpc = wca.MpcSolver(horizon=horizon)
        ik = wca.IkSolver(form=wca.IK_FORM_QPOASES, v_max=0.4, jacobian_structure=wca.IK_JAC_MIXED)
        d = DUMMY
        if kind == "mpc_solve_device":
            rc = lib.wcqp_mpc_solve_device(mpc._h, batch, d, d, ref_len, d, d, d, d, d, d, None, None, None)
        elif kind == "ik_solve_device":
            rc = lib.wcqp_ik_solve_device(ik._h, batch, d, d, d, d, d, d, d, d, None, None, None, None, None)
        elif kind in ("qp_enqueue_steps", "qp_plan_create", "qp_plan_create_mpc_only", "qp_plan_create_ik_only"):
            rec = (capi.QpStep * 1)()
            r = rec[0]
            if kind != "qp_plan_create_ik_only":
                r.x0 = r.ref = r.u_prev = r.hull_A = r.hull_b = r.hull_nc = r.u0 = r.mpc_status = d
                r.ref_len = ref_len
            if kind != "qp_plan_create_mpc_only":
                r.J_left = r.J_right = r.J_neck = r.J_com = r.q = r.state = r.dq = r.ik_status = d
            if kind == "qp_enqueue_steps":
                rc = lib.wcqp_qp_enqueue_steps(mpc._h, ik._h, batch, 1, rec, None)
            else:
                h = C.c_void_p()
                rc = lib.wcqp_qp_plan_create(mpc._h, ik._h, batch, 1, rec, 1, C.byref(h))
                if rc == 0:
                    lib.wcqp_qp_plan_destroy(h)
        elif kind == "qp_step_from_slabs":
            L = capi.SlabLayout()
            rc = lib.wcqp_slab_layout_for(batch, ref_len, C.byref(L))
            assert rc == 0, rc
            step = capi.QpStep()
            rc = lib.wcqp_qp_step_from_slabs(C.byref(L), d, d, C.byref(step))
        elif kind == "tick_create":
            try:
                wca.TickPipeline(batch, int(c["max_ticks"]), mpc, ik, external_feedback=bool(c.get("external", False)))
                rc = 0
            except wca.WcqpError as e:
                rc = int(str(e).rsplit("(", 1)[1].rstrip(")"))
        else:
            raise SystemExit("unknown entry " + kind)
        out.append(dict(c, rc=int(rc)))
        mpc.close(); ik.close()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
