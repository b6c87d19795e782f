"""The merge rule of wcqp_tick_replan_goals_timed over a robot's own timeline (include/wcqp.h states it, csrc/goal_merge.h is it), restated
by enumeration next to helpers/goal_merge.py: the plan's stages are labelled one by one - single support or not -, its merge points are
listed, and the first one at or above the floor is taken.  A plan in force is (O, fo, ss, ds): generated from stage O, fo stages of double
support, then step k with ss[k] stages of single and ds[k] of double support (len(ss) = len(ds) = n steps)."""
import numpy as np

TOO_LATE = -2


def step_starts(O, fo, ss, ds):
    """s_k: the first stage of step k's single support - s_0 = O + fo, s_{k+1} = s_k + ss_k + ds_k"""
    s, at = [], O + fo
    for a, b in zip(ss, ds):
        s.append(at)
        at += int(a) + int(b)
    return s


def single_support_stages(O, fo, ss, ds):
    """the set of stages inside one of the plan's single supports"""
    out = set()
    for s_k, a in zip(step_starts(O, fo, ss, ds), ss):
        out.update(range(s_k, s_k + int(a)))
    return out


def in_single_support(O, fo, ss, ds, M):
    return M in single_support_stages(O, fo, ss, ds)


def merge_allowed(O, fo, ss, ds, M, t0, T):
    """an explicit merge stage, as wcqp_tick_replan_footsteps_timed checks it"""
    return M >= 1 and M >= t0 and M < T and M >= O and not in_single_support(O, fo, ss, ds, M)


def merge_points(O, fo, ss, ds):
    """(the inner merge points s_k + ss_k for k = 0 .. n - 2, and L = s_{n-1} + ss_{n-1}, or O for a plan of no step)"""
    s = step_starts(O, fo, ss, ds)
    inner = [s_k + int(a) for s_k, a in zip(s[:-1], ss[:-1])]
    return inner, (s[-1] + int(ss[-1]) if len(s) else O)


def merge_auto(O, fo, ss, ds, t0, lead, T):
    """M_i, or TOO_LATE: the smallest merge point >= max(t0 + lead, 1, O) if it is a stage below T"""
    lo = max(t0 + lead, 1, O)
    inner, L = merge_points(O, fo, ss, ds)
    for M in inner:
        if M >= lo:
            return M if M < T else TOO_LATE
    M = max(lo, L)
    return M if M < T else TOO_LATE


def merge_auto_batch(origin, first_ds, n_steps, ss_ticks, ds_ticks, t0, lead, T):
    """over a batch: ss_ticks / ds_ticks [B][K] rows, of which robot i's first n_steps[i] entries are its plan's"""
    return np.array([merge_auto(int(o), int(f), list(a[:int(n)]), list(b[:int(n)]), t0, lead, T)
                     for o, f, n, a, b in zip(origin, first_ds, n_steps, ss_ticks, ds_ticks)], np.int32)


def table(O, fo, ss, ds, t0s, leads, n_stage):
    """What tests/cpp/goal_merge_timed_check.cpp prints for one plan, as arrays: single [n_stage] (M), allowed [t0][T][M], auto [t0][lead][T],
    M and T over 0 .. n_stage - 1.  Built from the enumerated stage labels and merge points, vectorised over the arguments."""
    M = np.arange(n_stage)
    single = np.isin(M, sorted(single_support_stages(O, fo, ss, ds)))
    t0 = np.asarray(t0s)[:, None, None]
    T = M[None, :, None]
    allowed = (M >= 1) & (M >= t0) & (M < T) & (M >= O) & ~single
    inner, L = merge_points(O, fo, ss, ds)
    lo = np.maximum(np.maximum(np.asarray(t0s)[:, None] + np.asarray(leads)[None, :], 1), O)          # [t0][lead]
    cand = np.maximum(lo, L)                       # at or above L every stage is a merge point
    for m in reversed(inner):                      # ... and below it the first inner one at or above the floor
        cand = np.where(m >= lo, m, cand)
    auto = np.where(cand[:, :, None] < M[None, None, :], cand[:, :, None], TOO_LATE)
    return single, allowed, auto
