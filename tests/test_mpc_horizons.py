"""
The MPC kernel against the exact oracle at the horizons where its stage loop changes shape.  A lane of a robot's 16-lane row takes
stages t, t+16, t+32, t+48 in one pass (N <= 63) and loops further 64-stage passes for stages 64..N (csrc/mpc_device.h:
mpc_row_solve, mpc_row_extra_passes); test_gpu_parity.py meets the oracle at N = 50 and N = 200 only.  Here: N on both sides of
every lane-group and pass boundary, references shorter than the window whose clamped tail falls in the extra passes, and coupled
weights across the pass boundary.  Same bars as test_gpu_parity.py: 1e-9 on u0, active sets bit for bit on clear-cut instances.

The last three stages of every reference carry seeded noise (sigma 0.02, some 1e2 times the synthetic reference's own): on the
oracle, moving the last stage by 0.05 moves u0 by 1.8e-6 to 4e-5, so a dropped or duplicated tail stage is 1e3 tolerances away.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SOL_TOL = 1e-9
MARGIN = 1e-7
HORIZONS = (1, 2, 15, 16, 17, 63, 64, 65, 80, 127, 128, 129)

_consts = {}


def _constants(qs, N, **kw):
    key = (N, tuple(sorted((k, np.asarray(v).tobytes()) for k, v in kw.items())))
    if key not in _consts:
        _consts[key] = qs.mpc_constants(qs.MPCParams(horizon=N, **kw))
    return _consts[key]


def _batch(wca, B, N):
    b = wca.synth.synth_mpc_batch(B, seed=700 + N, horizon=N, uprev_sigma=0.06, x0_sigma=0.03)
    ref = b["ref"].copy()
    tail = ref[:, -3:, :]                                                 # (N = 1 has two stages in all)
    tail += np.random.default_rng(9000 + N).normal(0.0, 0.02, tail.shape)
    b["ref"] = np.ascontiguousarray(ref)
    return b


def _against_oracle(wca, qs, c, solver, b, ref, what):
    """u0 and the active sets of `solver` on batch b with reference array `ref` against qs.mpc_exact given the same array; returns
    (active hull rows in the oracle's optima, clear-cut instances)."""
    B = b["x0"].shape[0]
    out = solver.solve_host(b["x0"], ref, b["u_prev"], b["hull_A"], b["hull_b"], b["hull_nc"])
    nact = ncc = 0
    worst = 0.0
    for i in range(B):
        r = qs.mpc_exact(c, b["x0"][i], ref[i], b["u_prev"][i], b["hull_A"][i], b["hull_b"][i], int(b["hull_nc"][i]))
        err = np.abs(out["u0"][i] - r["u0"]).max()
        worst = max(worst, err)
        assert out["status"][i] == wca.STATUS_SOLVED, (what, i, out["status"][i])
        assert err <= SOL_TOL, (what, i, err)
        if r["mu_min_active"] > MARGIN and r["slack_min_inactive"] > MARGIN:
            assert int(out["active"][i]) == sum(1 << e for e in r["active"]), (what, i)
            ncc += 1
        nact += len(r["active"])
    print("%-28s B=%-2d active rows %2d clear-cut %2d  worst |u0 - u0_exact| %.2e" % (what, B, nact, ncc, worst))
    return nact, ncc


@pytest.mark.parametrize("N", HORIZONS)
def test_mpc_horizon_against_oracle(wca, qs, N):
    B = 13                                    # three full waves of four robots plus one
    b = _batch(wca, B, N)
    assert b["ref"].shape == (B, N + 1, 2)
    nact, ncc = _against_oracle(wca, qs, _constants(qs, N), wca.MpcSolver(horizon=N), b, b["ref"], "N=%d" % N)
    assert nact >= 4 and ncc >= B - 3          # the hull binds, and the active sets were compared (oracle, B = 12: >= 11 clear-cut)


@pytest.mark.parametrize("N,ref_len", [(200, 1), (200, 7), (200, 64), (200, 65), (200, 130), (64, 64), (63, 63)])
def test_mpc_short_reference_in_the_extra_passes(wca, qs, N, ref_len):
    """ref_len < N + 1: stages past the array repeat its last sample (MPCSolver.cpp:200-214), also where the clamp falls in a
    later 64-stage pass, on a pass boundary, or leaves one stage (the last of the window) to repeat."""
    B = 5
    b = _batch(wca, B, N)
    short = np.ascontiguousarray(b["ref"][:, :ref_len, :])
    if ref_len > 3:
        short[:, -3:, :] += np.random.default_rng(9500 + ref_len).normal(0.0, 0.02, (B, 3, 2))      # the sample that repeats, and its neighbours
    full = np.concatenate([short, np.repeat(short[:, -1:, :], N + 1 - ref_len, axis=1)], axis=1)
    c = _constants(qs, N)
    s = wca.MpcSolver(horizon=N)
    _against_oracle(wca, qs, c, s, b, short, "N=%d ref_len=%d" % (N, ref_len))
    # the padded array written out gives the kernel the same sums in the same order
    a = s.solve_host(b["x0"], short, b["u_prev"], b["hull_A"], b["hull_b"], b["hull_nc"])
    e = s.solve_host(b["x0"], full, b["u_prev"], b["hull_A"], b["hull_b"], b["hull_nc"])
    assert np.array_equal(a["u0"], e["u0"]) and np.array_equal(a["active"], e["active"])


def test_mpc_coupled_weights_across_the_pass_boundary(wca, qs):
    """The coupled Q, R of test_gpu_parity.py::test_mpc_coupled_weights (full 2 x 2 gain blocks) at N = 64: stage 64 is the one
    stage of the first extra pass."""
    N, B = 64, 13
    Q = np.array([[7000.0, 1500.0], [1500.0, 5000.0]]); R = np.array([[9e6, -2e6], [-2e6, 6e6]])
    b = _batch(wca, B, N)
    nact, ncc = _against_oracle(wca, qs, _constants(qs, N, Q=Q, R=R), wca.MpcSolver(horizon=N, Q=Q, R=R), b, b["ref"], "N=64 coupled")
    assert nact >= 4 and ncc >= B - 3
