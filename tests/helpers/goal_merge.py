"""The merge stage wcqp_tick_replan_goals chooses for WCQP_TICK_MERGE_AUTO (include/wcqp.h states the rule, csrc/goal_merge.h is it),
restated by enumeration: the plan's merge points are listed, and the first one at or above the floor is taken."""
import numpy as np

TOO_LATE = -2


def step_starts(O, fo, n, ss, ds):
    """s_k: the first stage of step k's single support"""
    return [O + fo + k * (ss + ds) for k in range(n)]


def in_single_support(O, fo, n, ss, ds, M):
    """the closed form wcqp_tick_replan_footsteps refuses a merge stage by"""
    r = M - O
    if r < fo:
        return False
    k, u = divmod(r - fo, ss + ds)
    return k < n and u < ss


def merge_allowed(O, fo, n, ss, ds, M, t0, T):
    return M >= 1 and M >= t0 and M < T and M >= O and not in_single_support(O, fo, n, ss, ds, M)


def merge_auto(O, fo, n, ss, ds, t0, lead, T):
    """M_i, or TOO_LATE: the smallest merge point >= max(t0 + lead, 1, O) if it is a stage below T.  Merge points: s_k + ss for k = 0 .. n - 2,
    and every stage >= L = s_{n-1} + ss (n = 0: O)."""
    lo = max(t0 + lead, 1, O)
    s = step_starts(O, fo, n, ss, ds)
    inner = [s_k + ss for s_k in s[:-1]]
    L = s[-1] + ss if n else O
    for M in inner:
        if M >= lo:
            return M if M < T else TOO_LATE
    M = max(lo, L)
    return M if M < T else TOO_LATE


def merge_auto_batch(origin, first_ds, n_steps, ss, ds, t0, lead, T):
    return np.array([merge_auto(int(o), int(f), int(n), ss, ds, t0, lead, T) for o, f, n in zip(origin, first_ds, n_steps)], np.int32)


def reference_rule(merge_points_from_now, lead=20):
    """setPlannerInput's three cases on merge points counted from the current tick (WalkingModule.cpp:1263-1308)"""
    m = list(merge_points_from_now)
    if m and m[0] > lead:
        return m[0]
    if len(m) > 1:
        return m[1]
    return lead
