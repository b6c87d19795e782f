"""Numpy restatement of the batched non-linear IK (include/wcqp.h: wcqp_prepare_*) on oracle.kin_spec.forward / jacobians,
one robot at a time, and - independent of any iteration - the certificate of an optimum.

The problem: minimise w_q/2 |q - q_reg|^2 + w_n/2 |log(R_neck Rd_neck')|^2 subject to p_right = pd_right, log(R_right Rd_right') = 0,
com = com_d, q_min <= q <= q_max, with the left sole anchored at its desired pose.  The iteration: a QP per step on the Jacobians reduced
to the joints by the anchored sole, the step capped outside the QP.  The QP here is solved through its dense KKT system with numpy's LU -
not the kernel's Woodbury / Schur-complement / Cholesky path: the QP is strictly convex, so both arrive at the one optimum."""
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from oracle import kin_spec

SOLVED, MAX_ITER, INFEASIBLE, NUMERIC = 0, 1, 2, 4
BOUND_TOL = 1e-13


@dataclass
class Params:
    q_reg: np.ndarray
    w_q: float = 0.5
    w_n: float = 1.0
    step_cap: float = 0.3
    tol_step: float = 1e-12
    tol_constraint: float = 1e-10
    max_iter: int = 100
    q_min: Optional[np.ndarray] = None
    q_max: Optional[np.ndarray] = None


def log_rot(R):
    """rotation vector of R: the axial vector of its antisymmetric part is sin(theta) axis, theta = atan2(|v|, (trace - 1) / 2)"""
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s2 = float(v @ v)
    cth = 0.5 * (np.trace(R) - 1.0)
    if s2 < 1e-8 and cth > 0.0:
        f = 1.0 + s2 * (1.0 / 6.0 + s2 * (3.0 / 40.0))
    else:
        s = np.sqrt(s2)
        f = np.arctan2(s, cth) / s
    return f * v


def anchored_base(model, left_d, q):
    """[p 3 | R 9] of the root link with the left sole on its desired pose: world_T_base = T_L (base_T_sole(q))^-1"""
    k = kin_spec.forward(model, np.concatenate([np.zeros(3), np.eye(3).reshape(9)]), q)
    ps, Rs = k["frames"][0]
    Rb = left_d[3:12].reshape(3, 3) @ Rs.T
    return np.concatenate([left_d[:3] - Rb @ ps, Rb.reshape(9)])


def linearise(model, tg, q, par):
    """c (9), A = [JR~; Jc~] (9 x n), phi_n (3), N = Jn~ (3 x n), base - everything one iteration reads - at q"""
    base = anchored_base(model, tg["left_d"], q)
    J = kin_spec.jacobians(model, base, q)
    X = np.linalg.solve(J["J_left"][:, :6], J["J_left"][:, 6:])
    red = lambda M: M[:, 6:] - M[:, :6] @ X
    A = np.vstack([red(J["J_right"]), red(J["J_com"])])
    c = np.concatenate([J["p_right"] - tg["right_d"][:3], log_rot(J["R_right"] @ tg["right_d"][3:12].reshape(3, 3).T), J["com"] - tg["com_d"]])
    neck = par.w_n > 0.0 and tg.get("Rd_neck") is not None
    N = red(J["J_neck"]) if neck else np.zeros((3, model["dof"]))
    phi = log_rot(J["R_neck"] @ tg["Rd_neck"].reshape(3, 3).T) if neck else np.zeros(3)
    return dict(c=c, A=A, N=N, phi=phi, base=base, J=J, w_n=par.w_n if neck else 0.0)


def _limits(par, n):
    lo = np.full(n, -np.inf) if par.q_min is None else np.asarray(par.q_min, float)
    hi = np.full(n, np.inf) if par.q_max is None else np.asarray(par.q_max, float)
    return lo, hi


def solve_qp(H, g, A, c, lo, hi, max_changes=96):
    """min 1/2 x'Hx + g'x, A x = -c, lo <= x <= hi: active-set walk over dense KKT solves.  -> (x, lambda, active {joint: side}) or None"""
    n, m = H.shape[0], A.shape[0]
    W = {}
    for _ in range(max_changes):
        idx = list(W)
        E = np.vstack([A] + [np.eye(n)[[i]] for i in idx])
        d = np.concatenate([-c, [hi[i] if W[i] > 0 else lo[i] for i in idx]])
        KKT = np.block([[H, E.T], [E, np.zeros((len(d), len(d)))]])
        if np.linalg.cond(KKT) > 1e13:
            return None
        sol = np.linalg.solve(KKT, np.concatenate([-g, d]))
        x, lam = sol[:n], sol[n:]
        for i in idx:
            x[i] = hi[i] if W[i] > 0 else lo[i]
        free = [i for i in range(n) if i not in W]
        viol = [(max(lo[i] - x[i], x[i] - hi[i]), i) for i in free]
        worst = max(viol) if viol else (0.0, -1)
        if worst[0] > BOUND_TOL:
            i = worst[1]
            if len(W) >= n - m:
                return None
            W[i] = 1.0 if x[i] - hi[i] > lo[i] - x[i] else -1.0
            continue
        mult = [(lam[m + k] * W[i], i) for k, i in enumerate(idx)]
        if mult and min(mult)[0] < -BOUND_TOL:
            del W[min(mult)[1]]
            continue
        return x, lam[:m], dict(W)
    return None


def solve(model, tg, q_guess, par):
    """The iteration of include/wcqp.h for one robot.  tg: left_d [12], right_d [12], com_d [3], Rd_neck [9] or None."""
    n = model["dof"]
    lo, hi = _limits(par, n)
    qg = np.clip(np.asarray(q_guess, float), lo, hi)
    q = qg.copy()
    fail = lambda st, it: dict(q=qg, status=st, iters=it)
    for it in range(1, par.max_iter + 1):
        L = linearise(model, tg, q, par)
        H = par.w_q * np.eye(n) + L["w_n"] * L["N"].T @ L["N"]
        g = par.w_q * (q - par.q_reg) + L["w_n"] * L["N"].T @ L["phi"]
        res = solve_qp(H, g, L["A"], L["c"], lo - q, hi - q)
        if res is None:
            return fail(INFEASIBLE, it)
        dq, lam, W = res
        mx = np.abs(dq).max()
        if not np.isfinite(mx):
            return fail(NUMERIC, it)
        q = np.clip(q + min(1.0, par.step_cap / mx if mx > 0 else 1.0) * dq, lo, hi)
        if mx < par.tol_step and np.abs(L["c"]).max() < par.tol_constraint:
            return dict(q=q, status=SOLVED, iters=it, lam=lam, active=W, base=anchored_base(model, tg["left_d"], q))
    return fail(MAX_ITER, par.max_iter)


def certificate(model, q, tg, par):
    """Independent of any iteration: at q, the constraint residual max |c|; the joints on a limit (exactly) and the signs of their
    multipliers; the stationarity residual max |g + A' lambda + mu| with (lambda, mu) the LEAST-SQUARES fit over the equality rows and
    the joints on a limit.  -> dict(constraint, stationarity, mult_ok, active, inside)"""
    n = model["dof"]
    lo, hi = _limits(par, n)
    L = linearise(model, tg, q, par)
    g = par.w_q * (q - par.q_reg) + L["w_n"] * L["N"].T @ L["phi"]
    on_hi = [i for i in range(n) if q[i] == hi[i]]
    on_lo = [i for i in range(n) if q[i] == lo[i]]
    act = on_hi + on_lo
    Bm = np.hstack([L["A"].T] + [np.eye(n)[:, [i]] for i in act])
    z = np.linalg.lstsq(Bm, -g, rcond=None)[0]
    r = g + Bm @ z
    mu = z[9:]
    ok = all(mu[k] >= -1e-9 for k in range(len(on_hi))) and all(mu[len(on_hi) + k] <= 1e-9 for k in range(len(on_lo)))
    return dict(constraint=float(np.abs(L["c"]).max()), stationarity=float(np.abs(r).max()), mult_ok=bool(ok), active=sorted(act),
                inside=bool(np.all(q >= lo) and np.all(q <= hi)))
