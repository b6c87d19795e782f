"""
The IK kernels against the exact oracle on the parameter axes that tests/test_gpu_parity.py holds fixed (tests/ik_parameter_cases.py):
  * neck / CoM weights whose Cholesky factor is full (L10, L20, L21 != 0): a transposed factor or a wrong stride moves dq by 3e-4
    or more on these inputs (tests/test_cpu_oracle.py::test_ik_cases_tell_a_transposed_weight_factor);
  * lower bounds that are not the negated upper ones, intervals that exclude zero, pinned joints, one-sided bounds: reading -v_max
    for v_min moves dq on at least 79 of 96 instances (test_ik_cases_tell_a_mirrored_lower_bound);
  * weights that keep the base-elimination kernel from running (fast_ok = 0), which must route, not refuse.
Same bars as test_gpu_parity.py::test_ik_against_oracle_live: 1e-9 on dq, active sets bit for bit on clear-cut instances.
"""
import numpy as np
import pytest

import ik_parameter_cases as ic

pytestmark = pytest.mark.gpu

SOL_TOL = 1e-9
MARGIN = 1e-7
ALGS = {0: "default", 5: "base_elim", 4: "nullspace_16l", 3: "nullspace_mfma"}

CASE_FORMS = [(n, "qpoases") for n in ic.NAMES] + [(n, "osqp") for n in ic.OSQP_FORM_TOO]
CASE_ALGS = [(n, f, a) for n, f in CASE_FORMS for a in ((0, 4, 3) if n == "com_cost_full" else (0, 5, 4, 3))]


def _args(b, n=None):
    return tuple(b[k][:n] for k in ("J_left", "J_right", "J_neck", "J_com", "q", "state"))


def _against_oracle(wca, name, form, out, ex, what):
    """The bars of the module docstring on `out` (a solve_host result) against `ex` (ic.exact rows); returns the number checked."""
    lo, hi, _ = ic.CASES[name]
    B = len(out["status"])
    checked, worst = 0, 0.0
    for i in range(B):
        r = ex[i]
        if r is None:
            assert out["status"][i] == wca.STATUS_INFEASIBLE, (what, i, out["status"][i])
            continue
        assert out["status"][i] == wca.STATUS_SOLVED, (what, i, out["status"][i])
        dq = out["dq"][i]
        err = np.abs(dq - r["dq"]).max()
        worst = max(worst, err)
        assert err <= SOL_TOL, (what, i, err)
        al, au = int(out["active_lower"][i]), int(out["active_upper"][i])
        if name != "pinned" and ic.clear_cut(r, MARGIN):
            assert al == ic.mask(r["lower"]) and au == ic.mask(r["upper"]), (what, i)
        assert np.abs(out["foot_err"][i] - np.concatenate([r["foot_err_left"], r["foot_err_right"]])).max() <= 1e-8, (what, i)
        if form == "qpoases":
            assert (dq >= lo - 1e-12).all() and (dq <= hi + 1e-12).all(), (what, i)
            for j in range(23):
                if (al >> j) & 1:
                    assert abs(dq[j] - lo[j]) <= 1e-12, (what, i, j, "lower")
                if (au >> j) & 1:
                    assert abs(dq[j] - hi[j]) <= 1e-12, (what, i, j, "upper")
        else:
            assert al == 0 and au == 0, (what, i)          # the osqp back-end's limit rows are zero rows: nothing binds
        checked += 1
    print("%-18s %-8s %-15s B=%-3d checked %3d  worst |dq - dq_exact| %.2e" % (name, form, what, B, checked, worst))
    return checked


@pytest.mark.parametrize("name,form,algorithm", CASE_ALGS, ids=["%s-%s-%s" % (n, f, ALGS[a]) for n, f, a in CASE_ALGS])
def test_ik_parameter_case_against_oracle(wca, qs, name, form, algorithm):
    b, ex = ic.batch(wca), ic.exact(qs, wca, name, form)
    if form == "qpoases":                    # the case is not vacuous: bounds of both sides hold in the oracle's optimum
        assert sum(len(r["lower"]) for r in ex if r is not None) >= 1 and sum(len(r["upper"]) for r in ex if r is not None) >= 1
    out = ic.solver(wca, name, form, algorithm=algorithm).solve_host(*_args(b))
    checked = _against_oracle(wca, name, form, out, ex, ALGS[algorithm])
    assert checked >= (0.7 if name == "tight_tables" else 0.8) * ic.BATCH
    if name == "pinned":
        # a pinned joint sits on its bound exactly (the snap to the bound), and is reported on one side or the other
        assert (out["dq"][:, [4, 15]] == 0.1).all()
        both = out["active_lower"] | out["active_upper"]
        assert ((both >> 4) & 1 == 1).all() and ((both >> 15) & 1 == 1).all()


@pytest.mark.parametrize("name", ic.NO_FAST_KERNEL)
def test_ik_parameters_without_the_fast_kernel_route_to_the_general_one(wca, qs, name):
    """A neck weight that is not positive definite, or a joint weight of zero, rules out the base-elimination kernel (fast_ok = 0 in
    wcqp_ik_create).  The default algorithm then runs the general kernel: the oracle's optimum, never WCQP_STATUS_STRUCTURE - also
    when the caller declares its Jacobians MIXED, which only the base-elimination kernel would check."""
    b, ex = ic.batch(wca), ic.exact(qs, wca, name)
    args = _args(b)
    general = ic.solver(wca, name, algorithm=4).solve_host(*args)
    for js, what in ((wca.IK_JAC_AUTO, "auto"), (wca.IK_JAC_MIXED, "mixed")):
        out = ic.solver(wca, name, algorithm=0, jacobian_structure=js).solve_host(*args)
        assert (out["status"] != wca.STATUS_STRUCTURE).all()
        assert _against_oracle(wca, name, "qpoases", out, ex, "default/" + what) == ic.BATCH
        for k in ("dq", "status", "active_lower", "active_upper"):
            assert np.array_equal(out[k], general[k]), (what, k)          # the same kernel solved them


@pytest.mark.parametrize("algorithm", list(ALGS), ids=list(ALGS.values()))
@pytest.mark.parametrize("batch", [1, 3, 5])
def test_ik_parameters_on_ragged_batches(wca, qs, batch, algorithm):
    """asym_full_W with 1 to 3 rows of a four-robot wave empty: the first `batch` robots of the case, against the same oracle rows."""
    b, ex = ic.batch(wca), ic.exact(qs, wca, "asym_full_W")
    out = ic.solver(wca, "asym_full_W", algorithm=algorithm).solve_host(*(np.ascontiguousarray(a) for a in _args(b, batch)))
    assert _against_oracle(wca, "asym_full_W", "qpoases", out, ex[:batch], ALGS[algorithm]) == batch
