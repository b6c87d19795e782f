// Where a running generated walk may be cut for a new goal (wcqp_tick_replan_goals, include/wcqp.h, which states the rule; tests/helpers/
// goal_merge.py restates it): pure host arithmetic on the plan in force.  No HIP header: tests/cpp/goal_merge_check.cpp builds it alone.
#pragma once

namespace wcqp_goal {

// Robot i's plan in force: generated from stage `origin`, `first_ds` stages of double support, then `n_steps` steps of ss + ds stages.
// Step k's single support starts at s_k = origin + first_ds + k (ss + ds).
struct PlanInForce { int origin, first_ds, n_steps, ss, ds; };

constexpr int kTooLate = -2;      // WCQP_GOAL_TOO_LATE

// M lies inside one of the plan's single supports: [s_k, s_k + ss) of a step k < n_steps
inline bool in_single_support(const PlanInForce& p, int M) {
    const long long r = (long long)M - p.origin - p.first_ds, per = (long long)p.ss + p.ds;
    if (r < 0) return false;
    const long long k = r / per, u = r - k * per;
    return k < p.n_steps && u < p.ss;
}

// An explicit merge stage, as wcqp_tick_replan_footsteps takes it: not stage 0, not a stage the enqueued ticks have consumed (t0: the ticks
// enqueued so far, plus 1 when a resident plan's stage has been staged), within the T stages, behind the plan's own origin, both feet down
inline bool merge_allowed(const PlanInForce& p, int M, int t0, int T) {
    return M >= 1 && M >= t0 && M < T && M >= p.origin && !in_single_support(p, M);
}

// AUTO: the plan's merge points are the first stage of each inner double support, s_k + ss for k = 0 .. n - 2, and every stage >= L, where
// L = s_{n-1} + ss (n = 0: L = origin) - the last double support and standing.  The smallest one that is >= max(t0 + min_lead, 1, origin),
// or kTooLate when that is no stage below T.
inline int merge_auto(const PlanInForce& p, int t0, int min_lead, int T) {
    long long lo = (long long)t0 + min_lead;
    if (lo < 1) lo = 1;
    if (lo < p.origin) lo = p.origin;
    const long long per = (long long)p.ss + p.ds;
    const long long first = (long long)p.origin + p.first_ds + p.ss;                       // s_0 + ss
    const long long L = p.n_steps > 0 ? first + (long long)(p.n_steps - 1) * per : (long long)p.origin;
    long long M = lo;
    if (lo < L) {
        // the first s_k + ss at or above lo; k <= n - 1 because lo < L, and k = n - 1 gives L itself
        const long long k = lo > first ? (lo - first + per - 1) / per : 0;
        M = first + k * per;
    }
    return M < T ? (int)M : kTooLate;
}

// Robot i's TIMED plan in force (wcqp_tick_upload_footsteps_timed): every step has its own durations, dur = ss_0, ds_0, ss_1, ds_1, ...
// (2 n_steps entries; unread for n_steps = 0).  s_0 = origin + first_ds, s_{k+1} = s_k + ss_k + ds_k.  With all ss_k = ss and ds_k = ds the
// three functions below are the three above (tests/helpers/goal_merge_timed.py restates them).
struct TimedPlanInForce { int origin, first_ds, n_steps; const int* dur; };

// M lies inside one of the plan's single supports: [s_k, s_k + ss_k) of a step k < n_steps
inline bool in_single_support(const TimedPlanInForce& p, int M) {
    long long s_k = (long long)p.origin + p.first_ds;
    for (int k = 0; k < p.n_steps && s_k <= M; ++k) {
        if (M < s_k + p.dur[2 * k]) return true;
        s_k += (long long)p.dur[2 * k] + p.dur[2 * k + 1];
    }
    return false;
}

// An explicit merge stage, as wcqp_tick_replan_footsteps_timed takes it: the rule above on the per-step timeline
inline bool merge_allowed(const TimedPlanInForce& p, int M, int t0, int T) {
    return M >= 1 && M >= t0 && M < T && M >= p.origin && !in_single_support(p, M);
}

// AUTO: the merge points are s_k + ss_k for k = 0 .. n - 2 and every stage >= L = s_{n-1} + ss_{n-1} (n = 0: L = origin).  The smallest one
// that is >= max(t0 + min_lead, 1, origin), or kTooLate when that is no stage below T.
inline int merge_auto(const TimedPlanInForce& p, int t0, int min_lead, int T) {
    long long lo = (long long)t0 + min_lead;
    if (lo < 1) lo = 1;
    if (lo < p.origin) lo = p.origin;
    long long M = lo;
    long long s_k = (long long)p.origin + p.first_ds;
    for (int k = 0; k < p.n_steps; ++k) {
        // the first s_k + ss_k at or above lo; the last one is L itself, and at or above L every stage is a merge point
        const long long m_k = s_k + p.dur[2 * k];
        if (m_k >= lo) { M = m_k; break; }
        s_k = m_k + p.dur[2 * k + 1];
    }
    return M < T ? (int)M : kTooLate;
}

}  // namespace wcqp_goal
