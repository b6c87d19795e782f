"""Run by tests/test_size_limits.py in a process of its own per case (torch first, then libwcqp): the largest batch the size guard admits,
built ON THE DEVICE from a small synthetic batch plus a perturbation that depends on the robot's index (no two robots share rows), solved;
then the rows of the LAST 4096 robots - the ones whose byte offsets are closest to 2^32 - copied into a batch of their own and solved again:
the two results must agree bit for bit, and 16 of those robots must match the exact oracle to the figure printed.  Prints one JSON line."""
import json, os, sys
import numpy as np
import torch
torch.cuda.init()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import walking_controllers_amd as wca
from oracle import qp_spec as qs

TAIL, S = 4096, 4096


def mpc_case():
    N = 200
    B = (1 << 32) // ((N + 1) * 16)
    dev = torch.device("cuda", 0)
    small = wca.synth.synth_mpc_batch(S, seed=71, uprev_sigma=0.03, horizon=N)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    idx = torch.arange(B, device=dev) % S
    frac = torch.arange(B, device=dev, dtype=torch.float64) / B
    big = {k: t(small[k])[idx].contiguous() for k in ("x0", "ref", "u_prev", "hull_A", "hull_b", "hull_nc")}
    big["ref"] += (1e-4 * frac)[:, None, None]
    big["x0"] += (1e-4 * frac)[:, None]
    assert big["ref"].shape == (B, N + 1, 2) and big["ref"].numel() * 8 <= 1 << 32
    mpc = wca.MpcSolver(horizon=N)

    def solve(b, n):
        o = dict(u0=torch.zeros(n, 2, dtype=torch.float64, device=dev), st=torch.full((n,), -1, dtype=torch.int32, device=dev),
                 ac=torch.zeros(n, dtype=torch.int32, device=dev), mg=torch.zeros(n, dtype=torch.float64, device=dev))
        torch.cuda.synchronize()
        mpc.solve_device(n, b["x0"].data_ptr(), b["ref"].data_ptr(), N + 1, b["u_prev"].data_ptr(), b["hull_A"].data_ptr(), b["hull_b"].data_ptr(),
                         b["hull_nc"].data_ptr(), o["u0"].data_ptr(), o["st"].data_ptr(), o["ac"].data_ptr(), o["mg"].data_ptr(), 0)
        torch.cuda.synchronize()
        return o
    full = solve(big, B)
    tail_in = {k: v[B - TAIL:].clone() for k, v in big.items()}
    tail = solve(tail_in, TAIL)
    same = all(torch.equal(full[k][B - TAIL:], tail[k]) for k in full)
    st = full["st"].cpu().numpy()
    c = qs.mpc_constants(qs.MPCParams(horizon=N))
    h = {k: v.cpu().numpy() for k, v in tail_in.items()}
    u0 = tail["u0"].cpu().numpy()
    err, checked = 0.0, 0
    for i in list(range(TAIL - 8, TAIL)) + list(range(0, TAIL - 8, (TAIL - 8) // 8))[:8]:
        r = qs.mpc_exact(c, h["x0"][i], h["ref"][i], h["u_prev"][i], h["hull_A"][i], h["hull_b"][i], int(h["hull_nc"][i]))
        err = max(err, float(np.abs(u0[i] - r["u0"]).max())); checked += 1
    print(json.dumps(dict(case="mpc", batch=B, tail=TAIL, tail_bit_identical=bool(same), all_status_solved_or_hull=bool(np.isin(st, (0, 3)).all()),
                          checked=checked, max_err=err)))


def ik_case():
    B = (1 << 32) // (6 * 29 * 8)
    dev = torch.device("cuda", 0)
    small = wca.synth.synth_ik_batch(S, seed=72)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    idx = torch.arange(B, device=dev) % S
    frac = torch.arange(B, device=dev, dtype=torch.float64) / B
    big = {}
    for k in ("J_left", "J_right", "J_neck", "J_com", "q", "state"):
        big[k] = t(small[k])[idx].contiguous()
    for k in ("J_left", "J_right", "J_neck", "J_com"):
        big[k][:, :, 6:] *= (1.0 + 1e-4 * frac)[:, None, None]          # joint columns only: the base blocks keep the MIXED pattern
    big["q"] += (1e-3 * frac)[:, None]
    assert big["J_left"].numel() * 8 <= 1 << 32 < (B + 1) * 1392
    ik = wca.IkSolver(form=wca.IK_FORM_QPOASES, v_max=0.4)

    def solve(b, n):
        o = dict(dq=torch.zeros(n, 23, dtype=torch.float64, device=dev), st=torch.full((n,), -1, dtype=torch.int32, device=dev),
                 lo=torch.zeros(n, dtype=torch.int32, device=dev), up=torch.zeros(n, dtype=torch.int32, device=dev), it=torch.zeros(n, dtype=torch.int32, device=dev))
        torch.cuda.synchronize()
        ik.solve_device(n, b["J_left"].data_ptr(), b["J_right"].data_ptr(), b["J_neck"].data_ptr(), b["J_com"].data_ptr(), b["q"].data_ptr(),
                        b["state"].data_ptr(), o["dq"].data_ptr(), o["st"].data_ptr(), o["lo"].data_ptr(), o["up"].data_ptr(), 0, o["it"].data_ptr(), 0)
        torch.cuda.synchronize()
        return o
    full = solve(big, B)
    tail_in = {k: v[B - TAIL:].clone() for k, v in big.items()}
    tail = solve(tail_in, TAIL)
    same = all(torch.equal(full[k][B - TAIL:], tail[k]) for k in full)
    h = {k: v.cpu().numpy() for k, v in tail_in.items()}
    dq, st = tail["dq"].cpu().numpy(), tail["st"].cpu().numpy()
    p = qs.IKParams(v_max=0.4 * np.ones(23))
    err, checked = 0.0, 0
    for i in [i for i in range(TAIL - 1, -1, -1) if st[i] == 0][:16]:
        r = qs.ik_exact(p, qs.ik_inputs_from_batch(h, i), "qpoases")
        err = max(err, float(np.abs(dq[i] - r["dq"]).max())); checked += 1
    print(json.dumps(dict(case="ik", batch=B, tail=TAIL, tail_bit_identical=bool(same), tail_solved=int((st == 0).sum()), checked=checked, max_err=err)))


def tick_case():
    """a constant-Jacobian tick (internal plant, MPC controller) whose trajectories fill the 32-bit range: batch x traj_len = 2^28 stages of
    16 bytes, run for 3 ticks; host arrays, tiled from a small synthetic batch with a shift of the DCM reference that depends on the robot"""
    from oracle import tick_spec as ts
    N, T_MAX, TICKS, SMALL = 50, 973, 3, 512
    traj_len = T_MAX + N + 1
    B = (1 << 28) // traj_len
    assert traj_len == 1024 and B * traj_len * 16 == 1 << 32 and B <= (1 << 32) // 1392
    small = wca.synth.synth_tick_batch(SMALL, T_MAX)
    idx = np.arange(B) % SMALL
    frac = np.arange(B, dtype=np.float64) / B
    keys = ("ref_traj", "hull_tab_A", "hull_tab_b", "hull_tab_nc", "phase0", "J_left", "J_right", "J_neck", "J_com", "state0", "swing_twist", "q0", "dcm0", "com0", "u_init")
    big = {k: np.ascontiguousarray(small[k][idx]) for k in keys}
    big["ref_traj"] += (1e-5 * frac)[:, None, None]
    big["dcm0"] += (1e-5 * frac)[:, None]
    mk_ik = lambda: wca.IkSolver(form=wca.IK_FORM_QPOASES, v_max=0.45)

    def run(data, n, first):
        pipe = wca.TickPipeline(n, T_MAX, wca.MpcSolver(), mk_ik(), first=first, log_ticks=TICKS)
        pipe.upload(data); pipe.run(TICKS)
        out = pipe.download()
        pipe.close()
        return out
    full = run(big, B, 0)
    tail_in = {k: np.ascontiguousarray(v[B - TAIL:]) for k, v in big.items()}
    del big
    tail = run(tail_in, TAIL, B - TAIL)
    same = all(np.array_equal(full[k][:, B - TAIL:], tail[k]) for k in ("u0_log", "dq_log")) and \
        all(np.array_equal(full[k][B - TAIL:], tail[k]) for k in ("q_des", "dcm", "com", "ik_fail", "mpc_fail"))
    d16 = {k: v[TAIL - 16:] for k, v in tail_in.items()}
    d16["first"] = B - 16
    ref = ts.run_ticks(ts.TickParams(), d16, TICKS, qs.IKParams(v_max=0.45 * np.ones(23)))
    err = max(float(np.abs(tail["u0_log"][:, TAIL - 16:] - ref["u0_log"]).max()), float(np.abs(tail["dq_log"][:, TAIL - 16:] - ref["dq_log"]).max()),
              float(np.abs(tail["q_des"][TAIL - 16:] - ref["q_des"]).max()))
    print(json.dumps(dict(case="tick", batch=B, traj_len=traj_len, ticks=int(full["tick"]), tail=TAIL, tail_bit_identical=bool(same),
                          fails=int(full["ik_fail"].sum() + full["mpc_fail"].sum()), checked=16, max_err=err)))


if __name__ == "__main__":
    {"mpc": mpc_case, "ik": ik_case, "tick": tick_case}[sys.argv[1]]()
