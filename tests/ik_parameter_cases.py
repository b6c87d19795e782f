"""
The IK parameter cases shared by tests/test_cpu_oracle.py (are the inputs solvable, does the reference agree with itself, do the
inputs tell a right kernel from a wrong one) and tests/test_ik_parameters.py (the kernels against the oracle): neck / CoM weights
with a full Cholesky factor, lower bounds that are not the negated upper ones, intervals that exclude zero, pinned joints,
one-sided bounds, and the weights that keep the base-elimination kernel from running.

Everything here is input data: no case is shaped by what a kernel returns.
"""
import numpy as np

SEED, BATCH = 99, 96
K = np.arange(23.0)
# symmetric positive definite, smallest eigenvalue ~1.3; its Cholesky factor has L10, L20, L21 all far from 0
W = np.array([[3.6, 1.1, 1.0], [1.1, 8.2, 3.5], [1.0, 3.5, 3.2]])
BIG = 1e30                                                 # the ABI's "no bound" (OsqpEigen::INFTY)


def _com_weight():
    M = np.random.default_rng(2718).normal(size=(3, 3))
    return 30.0 * M @ M.T + 20.0 * np.eye(3)


def _sel(idx, val, other):
    a = np.full(23, float(other))
    a[list(idx)] = val
    return a


def _one_sided():
    lo = np.full(23, -0.3); lo[0::2] = -BIG
    hi = np.full(23, 0.25); hi[1::2] = BIG
    return lo, hi


def _zero_weight():
    from oracle.qp_spec import ICUB_JOINT_REG_WEIGHTS
    w = ICUB_JOINT_REG_WEIGHTS.copy()
    w[7] = 0.0
    return w


U = np.array([1.0, 2.0, -1.0])
SYM = (-0.4 * np.ones(23), 0.4 * np.ones(23))
ASYM = (-(0.15 + 0.02 * K[::-1]), 0.10 + 0.025 * K)

# name -> (v_min, v_max, further parameters under the names IKParams and IkSolver share)
CASES = {
    "full_W": (*SYM, dict(neck_weight=W)),
    "asym": (*ASYM, {}),
    "asym_full_W": (*ASYM, dict(neck_weight=W)),
    "excl_zero": (_sel((2, 9, 17), 0.05, -0.4), _sel((5, 20), -0.03, 0.4), {}),
    "pinned": (_sel((4, 15), 0.1, -0.4), _sel((4, 15), 0.1, 0.4), dict(neck_weight=W)),
    "one_sided": (*_one_sided(), {}),
    "tight_tables": (-(0.05 + 0.011 * K[::-1]), 0.04 + 0.013 * K, {}),
    "neck_off": (*SYM, dict(neck_weight=np.zeros((3, 3)))),
    "neck_rank1": (*SYM, dict(neck_weight=np.outer(U, U))),
    "zero_joint_weight": (*SYM, dict(joint_reg_weights=_zero_weight())),
    "com_cost_full": (*SYM, dict(neck_weight=W, use_com_as_constraint=False, com_weight=_com_weight())),
}
NAMES = list(CASES)
WITH_W = [n for n in NAMES if CASES[n][2].get("neck_weight") is W]
ASYMMETRIC = [n for n in NAMES if not np.array_equal(CASES[n][0], -CASES[n][1])]
NO_FAST_KERNEL = ["neck_off", "neck_rank1", "zero_joint_weight"]          # fast_ok = 0 in wcqp_ik_create
OSQP_FORM_TOO = ["full_W", "asym_full_W", "neck_rank1"]


def oracle_params(qs, name, **override):
    lo, hi, kw = CASES[name]
    kw = dict(kw, **override)
    return qs.IKParams(v_min=lo.copy(), v_max=hi.copy(), **kw)


def solver(wca, name, form="qpoases", **more):
    lo, hi, kw = CASES[name]
    f = wca.IK_FORM_QPOASES if form == "qpoases" else wca.IK_FORM_OSQP
    return wca.IkSolver(form=f, v_min=lo, v_max=hi, **kw, **more)


def batch(wca, n=BATCH):
    return wca.synth.synth_ik_batch(n, seed=SEED)


def mask(idx):
    return sum(1 << int(j) for j in idx)


_exact = {}


def exact(qs, wca, name, form="qpoases"):
    """The numpy oracle on the case's BATCH instances, computed once per (case, form): a list of result dicts, None where the
    oracle's phase-1 LP says infeasible.  Shared and never modified."""
    key = (name, form)
    if key not in _exact:
        b = batch(wca)
        p = oracle_params(qs, name)
        rows = []
        for i in range(BATCH):
            try:
                rows.append(qs.ik_exact(p, qs.ik_inputs_from_batch(b, i), form))
            except qs.QPInfeasible:
                rows.append(None)
        _exact[key] = rows
    return _exact[key]


def clear_cut(r, margin=1e-7):
    return r["mu_min_active"] > margin and r["slack_min_inactive"] > margin
