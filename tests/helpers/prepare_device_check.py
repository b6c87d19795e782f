"""The DEVICE form of the non-linear IK (wcqp_prepare_solve_device) against the host form, in a process of its own: torch brings its own
HIP runtime and has to initialise before libwcqp's does (tests/test_prepare.py runs this).

13 robots with joint limits: the device entry point fed torch tensors on the default stream and on a non-blocking one, and batches of 13, 4
and 1, give bit for bit what the host entry point gives; so does a call that leaves the optional outputs out.  Prints "prepare device ok"."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (the GPU runtime first, then libwcqp)
import walking_controllers_amd as wca  # noqa: E402


def main():
    B = 13
    S = wca.synth
    dev = torch.device("cuda", 0)
    d = S.synth_prepare_batch(B)
    q_reg = np.deg2rad(S.WALK_POSTURE_DEG)
    lo, hi = np.full(23, -3.0), np.full(23, 3.0)
    lo[15] = q_reg[15] - 0.1; lo[21] = q_reg[21] - 0.1          # the ankle pitches: a bound or two active per robot
    sol = wca.PrepareSolver(wca.KinModel(S.icub_like_model()), q_reg, q_min=lo, q_max=hi)
    ref = sol.solve_host(d["left_d"], d["right_d"], d["com_d"], d["q_guess"], d["Rd_neck"])
    assert (ref["status"] == 0).all() and ((ref["q"] == lo) | (ref["q"] == hi)).any()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ins = {k: t(d[k]) for k in ("left_d", "right_d", "com_d", "Rd_neck", "q_guess")}
    ptr = lambda k: ins[k].data_ptr()
    side = torch.cuda.Stream(device=dev)
    for n, stream in ((B, 0), (B, side.cuda_stream), (4, 0), (1, side.cuda_stream)):
        q = torch.zeros(n, 23, dtype=torch.float64, device=dev); base = torch.zeros(n, 12, dtype=torch.float64, device=dev)
        state = torch.zeros(n, 87, dtype=torch.float64, device=dev); res = torch.zeros(n, 2, dtype=torch.float64, device=dev)
        status = torch.full((n,), -1, dtype=torch.int32, device=dev); iters = torch.zeros(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        sol.solve_device(n, ptr("left_d"), ptr("right_d"), ptr("com_d"), ptr("q_guess"), q.data_ptr(), status.data_ptr(), Rd_neck=ptr("Rd_neck"),
                         base=base.data_ptr(), state=state.data_ptr(), iters=iters.data_ptr(), residual=res.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        for k, v in (("q", q), ("base", base), ("state", state), ("residual", res), ("status", status), ("iters", iters)):
            assert np.array_equal(v.cpu().numpy(), ref[k][:n]), (n, stream, k)
    host4 = sol.solve_host(d["left_d"][:4], d["right_d"][:4], d["com_d"][:4], d["q_guess"][:4], d["Rd_neck"][:4])
    for k in ref:
        assert np.array_equal(host4[k], ref[k][:4]), k
    q = torch.zeros(B, 23, dtype=torch.float64, device=dev); status = torch.full((B,), -1, dtype=torch.int32, device=dev)
    sol.solve_device(B, ptr("left_d"), ptr("right_d"), ptr("com_d"), ptr("q_guess"), q.data_ptr(), status.data_ptr(), Rd_neck=ptr("Rd_neck"))
    torch.cuda.synchronize()
    assert np.array_equal(q.cpu().numpy(), ref["q"]) and (status == 0).all()
    print("prepare device ok")


if __name__ == "__main__":
    main()
