"""The DEVICE form of sensor feedback with the low-pass filters on (wcqp_tick_params.*_cut_frequency) against the host form, in a process of
its own: torch brings its own HIP runtime and has to initialise before libwcqp's does (tests/test_tick_sensor_filters.py runs this).

Six ticks, B = 6, all three filters at 10 Hz: a handle fed from torch tensors on a non-blocking torch stream, with its runs on that stream,
gives bit for bit what a handle fed the same readings through the host form on the NULL stream gives; so does a handle that switches
between the two forms from tick to tick - both forms advance the same filter state.  Prints "sensor filters device ok"."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402  (the GPU runtime first, then libwcqp)
import walking_controllers_amd as wca  # noqa: E402
from helpers import sensor_feedback as sf  # noqa: E402


def main():
    B, T = 6, 6
    dev = torch.device("cuda", 0)
    S = wca.synth
    kin = wca.KinModel(S.icub_like_model())
    kb = S.synth_walk_kin_batch(B)
    poses = kin.jacobians_host(kb["base"], kb["q"], state=np.zeros((B, 87)))["state"]
    d = S.synth_walk_batch(B, T, poses, kb)
    mk = lambda: wca.TickPipeline(B, T, wca.MpcSolver(), wca.IkSolver(form=wca.IK_FORM_QPOASES, v_max=S.WALK_VMAX.copy(),
                                  joint_reg_rad=np.deg2rad(S.WALK_POSTURE_DEG)), log_ticks=T, kin=kin, external_feedback=True,
                                  sensor_filters=dict(joint_velocity=10.0, wrench=10.0, com=10.0))
    rng = np.random.default_rng(31)
    noise = [(0.01 * rng.normal(size=(B, 23)), 0.3 * rng.normal(size=(B, 23))) + tuple(sf.wrenches(rng, B)) for _ in range(T)]
    stream = torch.cuda.Stream()          # non-blocking

    def loop(form):
        pipe = mk()
        assert pipe.info()["sensor_filters"] == 7
        pipe.upload(d)
        q_des, dq_prev = d["q0"].copy(), np.zeros((B, 23))
        meas = []
        for t in range(T):
            r = (q_des + noise[t][0], dq_prev + noise[t][1], noise[t][2], noise[t][3])
            if form(t) == "device":
                with torch.cuda.stream(stream):
                    x = [torch.from_numpy(np.ascontiguousarray(a)).to(dev, non_blocking=False) for a in r]
                    stream.synchronize()
                    pipe.set_sensor_feedback_device(*x, stream=stream.cuda_stream)
                    pipe.run(1, stream=stream.cuda_stream)
                    stream.synchronize()
            else:
                pipe.set_sensor_feedback_host(*r)
                pipe.run(1)
            o = pipe.download()
            meas.append(o["measured"])
            q_des, dq_prev = o["q_des"], o["dq_log"][t]
        o["measured_log"] = np.stack(meas)
        return o
    host = loop(lambda t: "host")
    device = loop(lambda t: "device")
    mixed = loop(lambda t: ("device", "host")[t % 2])
    for o in (device, mixed):
        for k in ("u0_log", "dq_log", "q_des", "ik_fail", "mpc_fail", "measured_log", "feedback_fail"):
            assert np.array_equal(o[k], host[k]), k
    assert np.abs(host["dq_log"]).max() > 1e-3 and host["feedback_fail"].sum() == 0
    print("sensor filters device ok")


if __name__ == "__main__":
    main()
