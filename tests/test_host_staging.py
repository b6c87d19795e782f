"""The *_host entry points stage the caller's arrays through one helper (csrc/host_stage.h, wcqp::HostStage).  These tests call the nine of
them through wca.capi.lib() with numpy buffers of their own, so that they own the memory around every array:

  guard rows       every output array is a view into a larger buffer with 64 sentinel bytes on both sides, intact after the call; every
                   input array equals a copy taken before the call.  Batches 1, 3 and 67: one lane group, an odd count (arrays that are
                   only 8-byte aligned in the block), one robot past a 64-robot workgroup.
  optional arrays  each entry point once with every optional output absent and once with all present: the common arrays are bit-identical.
  shrink and grow  on ONE handle 67 robots, the first 3 of them, 67 again (robots are independent in every one of these kernels): the first
                   and third results bit-identical, the second their first three rows - the five forms that own a growable block.
  the tick forms   a streamed, external, fused-kinematics handle, B = 5, two ticks: set_desired_host, set_sensor_feedback_host and
                   set_feedback_host give bit for bit the download() of the *_device forms, whose code and kernels the helper does not touch
                   (what tests/helpers/*_device_check.py compare against).  That needs device memory of the test's own: torch, which has to
                   initialise before libwcqp does - so this file run as a script is that check, in a process of its own.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, SENTINEL = 64, 0xA5
BATCHES = (1, 3, 67)
BMAX = 67


class Out:
    """an output array: a view into a buffer of its own with GUARD sentinel bytes on both sides"""

    def __init__(self, shape, dtype, fill=None):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self.buf = np.full(n + 2 * GUARD, SENTINEL, np.uint8)
        self.a = self.buf[GUARD:GUARD + n].view(dtype).reshape(shape)
        if fill is not None:
            self.a[...] = fill

    def intact(self):
        return (self.buf[:GUARD] == SENTINEL).all() and (self.buf[-GUARD:] == SENTINEL).all()


def _ptr(x):
    if x is None:
        return None
    return (x.a if isinstance(x, Out) else x).ctypes.data


# ---- the six entry points outside the tick: handle, inputs of BMAX robots, outputs (name -> row shape, dtype, optional), the call ---------

def _forms(wca):
    S = wca.synth
    L = wca.capi.lib()
    mb, ib, kb, pb, gb = S.synth_mpc_batch(BMAX, seed=41), S.synth_ik_batch(BMAX, seed=42), S.synth_walk_kin_batch(BMAX), \
        S.synth_prepare_batch(BMAX), S.synth_goal_batch(BMAX)
    rng = np.random.default_rng(43)
    yaw = rng.uniform(-0.4, 0.4, (2, BMAX))
    feet = []
    for f, y0 in enumerate((0.08, -0.08)):
        T = np.zeros((BMAX, 12))
        T[:, 0:2] = rng.normal(0, 0.02, (BMAX, 2)) + [0.0, y0]
        T[:, 3], T[:, 4], T[:, 6], T[:, 7], T[:, 11] = np.cos(yaw[f]), -np.sin(yaw[f]), np.sin(yaw[f]), np.cos(yaw[f]), 1.0
        feet.append(T)
    q_reg = np.deg2rad(S.WALK_POSTURE_DEG)
    K = 8
    forms = {}
    forms["mpc"] = dict(
        make=lambda: wca.MpcSolver(),
        ins={k: mb[k] for k in ("x0", "ref", "u_prev", "hull_A", "hull_b", "hull_nc")},
        outs=dict(u0=((2,), np.float64, False), status=((), np.int32, False), active=((), np.uint32, True), margin=((), np.float64, True)),
        call=lambda h, B, i, o: L.wcqp_mpc_solve_host(h._h, B, _ptr(i["x0"]), _ptr(i["ref"]), mb["ref"].shape[1], _ptr(i["u_prev"]), _ptr(i["hull_A"]),
                                                      _ptr(i["hull_b"]), _ptr(i["hull_nc"]), _ptr(o["u0"]), _ptr(o["status"]), _ptr(o["active"]),
                                                      _ptr(o["margin"])))
    forms["ik"] = dict(
        make=lambda: wca.IkSolver(form=wca.IK_FORM_QPOASES, v_max=0.4),
        ins={k: ib[k] for k in ("J_left", "J_right", "J_neck", "J_com", "q", "state")},
        outs=dict(dq=((23,), np.float64, False), status=((), np.int32, False), active_lower=((), np.uint32, True), active_upper=((), np.uint32, True),
                  foot_err=((12,), np.float64, True), iters=((), np.int32, True)),
        call=lambda h, B, i, o: L.wcqp_ik_solve_host(h._h, B, *(_ptr(i[k]) for k in ("J_left", "J_right", "J_neck", "J_com", "q", "state")),
                                                     *(_ptr(o[k]) for k in ("dq", "status", "active_lower", "active_upper", "foot_err", "iters"))))
    forms["kin"] = dict(
        make=lambda: wca.KinModel(S.icub_like_model()),
        ins=dict(base=kb["base"], q=kb["q"]),
        # (state goes in AND out: the block the kernel is handed starts as zeros)
        outs=dict(J_left=((6, 29), np.float64, False), J_right=((6, 29), np.float64, False), J_neck=((3, 29), np.float64, False),
                  J_com=((3, 29), np.float64, False), state=((87,), np.float64, True)),
        fill=dict(state=0.0),
        call=lambda h, B, i, o: L.wcqp_kin_jacobians_host(h._h, B, _ptr(i["base"]), _ptr(i["q"]),
                                                          *(_ptr(o[k]) for k in ("J_left", "J_right", "J_neck", "J_com", "state"))))
    forms["prepare"] = dict(
        make=lambda: wca.PrepareSolver(wca.KinModel(S.icub_like_model()), q_reg),
        ins={k: pb[k] for k in ("left_d", "right_d", "com_d", "Rd_neck", "q_guess")},
        outs=dict(q=((23,), np.float64, False), base=((12,), np.float64, True), state=((87,), np.float64, True), status=((), np.int32, False),
                  iters=((), np.int32, True), residual=((2,), np.float64, True)),
        call=lambda h, B, i, o: L.wcqp_prepare_solve_host(h._h, B, *(_ptr(i[k]) for k in ("left_d", "right_d", "com_d", "Rd_neck", "q_guess")),
                                                          *(_ptr(o[k]) for k in ("q", "base", "state", "status", "iters", "residual"))))

    def unicycle_call(h, B, i, o):
        ins = wca.capi.UnicycleInputs(*(_ptr(i[k]) for k in ("left0", "right0", "goals", "first_side")))
        outs = wca.capi.UnicycleOutputs(*(_ptr(o[k]) for k in ("n_steps", "side", "target", "status", "desired_point", "unicycle_end")))
        return L.wcqp_unicycle_plan_host(h._h, B, C.byref(ins), C.byref(outs))
    forms["unicycle"] = dict(
        make=lambda: wca.UnicyclePlanner(max_steps=K),
        ins={k: gb[k] for k in ("left0", "right0", "goals", "first_side")},
        outs=dict(n_steps=((), np.int32, False), side=((K,), np.uint8, False), target=((K, 3), np.float64, False), status=((), np.int32, False),
                  desired_point=((2,), np.float64, True), unicycle_end=((3,), np.float64, True)),
        call=unicycle_call)
    forms["hull"] = dict(
        make=lambda: None,
        ins=dict(left_T=feet[0], right_T=feet[1], contact=rng.integers(0, 4, BMAX).astype(np.uint8)),
        whole=dict(foot_rect=np.array(S.FOOT_RECT, float).reshape(8).copy()),
        outs=dict(hull_A=((8, 2), np.float64, False), hull_b=((8,), np.float64, False), hull_nc=((), np.int32, False)),
        call=lambda h, B, i, o: L.wcqp_hull_from_feet_host(B, _ptr(i["foot_rect"]), _ptr(i["left_T"]), _ptr(i["right_T"]), _ptr(i["contact"]),
                                                           _ptr(o["hull_A"]), _ptr(o["hull_b"]), _ptr(o["hull_nc"])))
    return forms


SCRATCH_FORMS = ("mpc", "ik", "kin", "prepare", "unicycle")
ALL_FORMS = SCRATCH_FORMS + ("hull",)


@pytest.fixture(scope="module")
def forms(wca):
    return _forms(wca)


def _call(form, handle, B, optional=True):
    """one call on the first B robots: rc == 0, the guards intact, the inputs as they were -> {name: array} of the outputs asked for"""
    ins = {k: np.ascontiguousarray(v[:B]) for k, v in form["ins"].items()}
    ins.update({k: v.copy() for k, v in form.get("whole", {}).items()})
    before = {k: v.copy() for k, v in ins.items()}
    outs = {k: (Out((B,) + row, dt, form.get("fill", {}).get(k)) if (optional or not opt) else None) for k, (row, dt, opt) in form["outs"].items()}
    rc = form["call"](handle, B, ins, outs)
    assert rc == 0, rc
    for k, o in outs.items():
        assert o is None or o.intact(), ("guard", k)
    for k in ins:
        assert np.array_equal(ins[k], before[k]), ("input", k)
    return {k: o.a.copy() for k, o in outs.items() if o is not None}


@pytest.fixture(scope="module")
def full(forms):
    """every form on BMAX robots with every output present, on a handle of its own: computed once, shared"""
    return {name: _call(f, f["make"](), BMAX) for name, f in forms.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("name", ALL_FORMS)
def test_guard_rows_and_inputs(forms, full, name, B):
    """guards and inputs (asserted in _call), and - robots are independent - the first B rows of the 67-robot call"""
    f = forms[name]
    out = _call(f, f["make"](), B)
    assert set(out) == set(f["outs"])
    for k, v in out.items():
        assert v.shape[0] == B and np.array_equal(v, full[name][k][:B]), k
        assert not (np.ascontiguousarray(v).view(np.uint8) == SENTINEL).all(), k      # written: no longer the sentinel pattern


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCRATCH_FORMS)
def test_optional_outputs_absent_and_present(forms, full, name):
    """(hull has no optional array: its one run is `full`)"""
    f = forms[name]
    few = _call(f, f["make"](), BMAX, optional=False)
    assert set(few) == {k for k, (_, _, opt) in f["outs"].items() if not opt} and len(few) < len(f["outs"])
    for k, v in few.items():
        assert np.array_equal(v, full[name][k]), k


@pytest.mark.gpu
def test_unicycle_without_step_rows(wca, forms):
    """max_steps = 0: the planner keeps no step rows, side and target are NULL on the host and on the device"""
    f = dict(forms["unicycle"])
    f["outs"] = {k: v for k, v in f["outs"].items() if k not in ("side", "target")}
    call = f["call"]
    f["call"] = lambda h, B, i, o: call(h, B, i, dict(o, side=None, target=None))
    out = _call(f, wca.UnicyclePlanner(max_steps=0), 3)
    assert (out["n_steps"] == 0).all() and np.isfinite(out["desired_point"]).all() and np.isfinite(out["unicycle_end"]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCRATCH_FORMS)
def test_block_shrinks_and_grows(forms, name):
    f = forms[name]
    h = f["make"]()
    a, b, c = _call(f, h, BMAX), _call(f, h, 3), _call(f, h, BMAX)
    for k in a:
        assert np.array_equal(a[k], c[k]), k
        assert np.array_equal(b[k], a[k][:3]), k


@pytest.mark.gpu
def test_tick_host_forms_equal_the_device_forms():
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "tick host staging ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ---- the tick forms, as a script (torch first, then libwcqp) --------------------------------------------------------------------------------

def _tick_main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import walking_controllers_amd as wca
    from helpers import sensor_feedback as sf
    from helpers import streamed_tick as stt

    B, T = 5, 2
    dev = torch.device("cuda", 0)
    S = wca.synth
    L = wca.capi.lib()
    kin = wca.KinModel(S.icub_like_model())
    kb = S.synth_walk_kin_batch(B)
    poses = kin.jacobians_host(kb["base"], kb["q"], state=np.zeros((B, 87)))["state"]
    d = S.synth_planned_walk_batch(B, T, poses, kb, yaw_step=(0.03, 0.08))
    stages = stt.stages_of(d, T)
    rng = np.random.default_rng(31)
    stages["right_twist"] = stages["right_twist"] + 1e-3 * rng.normal(size=stages["right_twist"].shape)
    stages["com_height"] = np.ascontiguousarray(d["state0"][None, :, 68] + 1e-3 * rng.normal(size=(T, B)))
    stages["com_height_vel"] = 1e-3 * rng.normal(size=(T, B))
    fb = [(d["dcm0"] + 1e-3 * rng.normal(size=(B, 2)), d["com0"] + 1e-4 * rng.normal(size=(B, 2)), d["u_init"] + 1e-3 * rng.normal(size=(B, 2)),
           d["q0"] + 1e-3 * rng.normal(size=(B, 23))) for _ in range(T)]
    sens = [(d["q0"] + 1e-3 * rng.normal(size=(B, 23)), 2e-3 * rng.normal(size=(B, 23))) + tuple(sf.wrenches(rng, B)) for _ in range(T)]
    up = {key: d[key] for key in ("ref_traj", "state0", "q0", "dcm0", "com0", "u_init")}
    DES = ("left_pose", "right_pose", "left_twist", "right_twist", "contact", "com_height", "com_height_vel")
    stream = torch.cuda.Stream()

    def loop(form, heights, feedback):
        """feedback: "plain" (with q_meas), "plain_no_q", "sensor" """
        pipe = wca.TickPipeline(B, T, wca.MpcSolver(), wca.IkSolver(form=wca.IK_FORM_QPOASES, v_max=S.WALK_VMAX.copy(),
                                joint_reg_rad=np.deg2rad(S.WALK_POSTURE_DEG)), log_ticks=T, kin=kin, external_feedback=True,
                                streamed_trajectories=True, neck_additional_rotation=np.eye(3))
        info = pipe.info()
        assert info["streamed_trajectories"] and info["kin_handoff"] == "fused"
        pipe.upload(up)
        for t in range(T):
            des = [np.array(stages[k][t], copy=True) if (heights or not k.startswith("com_height")) else None for k in DES]
            f = list(sens[t]) if feedback == "sensor" else list(fb[t][:3]) + [fb[t][3] if feedback == "plain" else None]
            f = [None if x is None else np.array(x, copy=True) for x in f]
            if form == "device":
                with torch.cuda.stream(stream):
                    x = [None if a is None else torch.from_numpy(a).to(dev) for a in des]
                    y = [None if a is None else torch.from_numpy(a).to(dev) for a in f]
                    stream.synchronize()
                    pipe.set_desired_device(*x, stream=stream.cuda_stream)
                    if feedback == "sensor":
                        pipe.set_sensor_feedback_device(*y, stream=stream.cuda_stream)
                    else:
                        pipe.set_feedback_device(*(0 if v is None else v.data_ptr() for v in y), stream=stream.cuda_stream)
                    pipe.run(1, stream=stream.cuda_stream)
                    stream.synchronize()
            else:
                before = [None if a is None else a.copy() for a in des + f]
                rec = wca.capi.TickDesired(*[None if a is None else a.ctypes.data for a in des])
                assert L.wcqp_tick_set_desired_host(pipe._h, C.byref(rec)) == 0
                ptrs = [None if a is None else a.ctypes.data for a in f]
                if feedback == "sensor":
                    assert L.wcqp_tick_set_sensor_feedback_host(pipe._h, *ptrs) == 0
                else:
                    assert L.wcqp_tick_set_feedback_host(pipe._h, *ptrs) == 0
                for a, b in zip(des + f, before):
                    assert a is None or np.array_equal(a, b)
                pipe.run(1)
        return pipe.download()

    runs = {}
    for heights, feedback in ((True, "plain"), (False, "plain_no_q"), (True, "sensor")):
        host, device = loop("host", heights, feedback), loop("device", heights, feedback)
        for key in ("u0_log", "dq_log", "q_des", "ik_fail", "mpc_fail", "measured", "feedback_fail"):
            assert np.array_equal(device[key], host[key]), (heights, feedback, key)
        assert np.abs(host["dq_log"]).max() > 1e-4 and host["feedback_fail"].sum() == 0, (heights, feedback)
        runs[(heights, feedback)] = host
    # the optional arrays are read: with and without them the runs differ
    assert not np.array_equal(runs[(True, "plain")]["dq_log"], runs[(False, "plain_no_q")]["dq_log"])
    print("tick host staging ok")


if __name__ == "__main__":
    _tick_main()
