"""The DEVICE form of the streamed stage (wcqp_tick_set_desired_device) against the host form, in a process of its own: torch brings its own
HIP runtime and has to initialise before libwcqp's does (tests/test_tick_streamed.py runs this).

B = 9 robots on the start of the planned walk.  A handle whose stages and plain feedback come from torch tensors on a non-blocking torch
stream, with its runs on that stream, gives bit for bit what the host forms on the NULL stream give.  One robot's stage made invalid at tick
k (a NaN twist; at another tick of a second run: no foot in contact): that robot keeps its previous stage, is stopped (dq = 0 from tick k
on) and counted in feedback_fail, every other robot is bitwise the clean run.  The binding refuses a tensor of the wrong dtype or shape.
Prints "streamed device ok"."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402  (the GPU runtime first, then libwcqp)
import walking_controllers_amd as wca  # noqa: E402
from helpers import streamed_tick as stt  # noqa: E402

KEYS5 = ("left_pose", "right_pose", "left_twist", "right_twist", "contact")


def main():
    B, T, k, r = 9, 16, 6, 4
    dev = torch.device("cuda", 0)
    S = wca.synth
    kin = wca.KinModel(S.icub_like_model())
    kb = S.synth_walk_kin_batch(B)
    poses = kin.jacobians_host(kb["base"], kb["q"], state=np.zeros((B, 87)))["state"]
    d = S.synth_planned_walk_batch(B, T, poses, kb, yaw_step=(0.03, 0.08))
    stages = stt.stages_of(d, T)
    # the first double support never moves a foot: give the stages a twist and a height of their own, so that every entry is exercised
    rng = np.random.default_rng(31)
    stages["right_twist"] = stages["right_twist"] + 1e-3 * rng.normal(size=stages["right_twist"].shape)
    stages["com_height"] = np.ascontiguousarray(d["state0"][None, :, 68] + 1e-3 * rng.normal(size=(T, B)))
    stages["com_height_vel"] = 1e-3 * rng.normal(size=(T, B))
    fb = [(d["dcm0"] + 1e-3 * rng.normal(size=(B, 2)), d["com0"] + 1e-4 * rng.normal(size=(B, 2)), d["u_init"] + 1e-3 * rng.normal(size=(B, 2)))
          for _ in range(T)]
    mk = lambda: wca.TickPipeline(B, T, wca.MpcSolver(), wca.IkSolver(form=wca.IK_FORM_QPOASES, v_max=S.WALK_VMAX.copy(),
                                  joint_reg_rad=np.deg2rad(S.WALK_POSTURE_DEG)), log_ticks=T, kin=kin, external_feedback=True,
                                  streamed_trajectories=True, neck_additional_rotation=np.eye(3))
    up = {key: d[key] for key in ("ref_traj", "state0", "q0", "dcm0", "com0", "u_init")}
    stream = torch.cuda.Stream()          # non-blocking

    def loop(form, spoil=None):
        pipe = mk()
        pipe.upload(up)
        for t in range(T):
            st = {key: np.array(stages[key][t], copy=True) for key in KEYS5 + ("com_height", "com_height_vel")}
            if spoil is not None:
                spoil(t, st)
            args = [st[key] for key in KEYS5 + ("com_height", "com_height_vel")]
            if form == "device":
                with torch.cuda.stream(stream):
                    x = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in args]
                    f = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in fb[t]]
                    stream.synchronize()
                    pipe.set_desired_device(*x, stream=stream.cuda_stream)
                    pipe.set_feedback_device(*(y.data_ptr() for y in f), stream=stream.cuda_stream)
                    pipe.run(1, stream=stream.cuda_stream)
                    stream.synchronize()
            else:
                pipe.set_desired_host(*args)
                pipe.set_feedback_host(*fb[t])
                pipe.run(1)
        return pipe.download()
    host = loop("host")
    device = loop("device")
    for key in ("u0_log", "dq_log", "q_des", "ik_fail", "mpc_fail", "measured", "feedback_fail"):
        assert np.array_equal(device[key], host[key]), key
    assert np.abs(host["dq_log"]).max() > 1e-4 and host["feedback_fail"].sum() == 0 and host["ik_fail"].sum() == 0

    others = np.arange(B) != r
    for case in ("nan_twist", "no_contact", "fixed_in_air"):
        def spoil(t, st):
            if t != k:
                return
            if case == "nan_twist":
                st["left_twist"][r, 2] = np.nan
            elif case == "no_contact":
                st["contact"][r] = 4
            else:
                st["contact"][r] = 1          # the right foot is the fixed frame and is not in contact
        bad = loop("device", spoil)
        assert list(bad["feedback_fail"]) == [int(i == r) for i in range(B)], (case, bad["feedback_fail"])
        assert bad["ik_fail"][r] == T - k + 1 and (bad["ik_fail"][others] == 0).all(), (case, bad["ik_fail"])
        assert (bad["dq_log"][k:, r] == 0).all() and np.abs(bad["dq_log"][k - 1, r]).max() > 0
        for key in ("u0_log", "dq_log"):
            assert np.array_equal(bad[key][:, others], host[key][:, others]), (case, key)
            assert np.array_equal(bad[key][:k], host[key][:k]), (case, key)
        assert np.array_equal(bad["q_des"][others], host["q_des"][others]), case

    # the binding checks the tensors
    pipe = mk()
    pipe.upload(up)
    good = [torch.zeros(B, 12, dtype=torch.float64, device=dev), torch.zeros(B, 12, dtype=torch.float64, device=dev),
            torch.zeros(B, 6, dtype=torch.float64, device=dev), torch.zeros(B, 6, dtype=torch.float64, device=dev),
            torch.full((B,), 7, dtype=torch.uint8, device=dev)]
    for i, wrong in ((0, torch.zeros(B, 12, dtype=torch.float32, device=dev)), (2, torch.zeros(B, 5, dtype=torch.float64, device=dev)),
                     (4, torch.full((B,), 7, dtype=torch.int32, device=dev)), (3, torch.zeros(B, 6, dtype=torch.float64))):
        x = list(good)
        x[i] = wrong
        try:
            pipe.set_desired_device(*x)
        except ValueError:
            continue
        raise AssertionError(f"tensor {i} was not refused")
    print("streamed device ok")


if __name__ == "__main__":
    main()
