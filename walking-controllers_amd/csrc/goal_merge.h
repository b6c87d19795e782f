// The timeline of a generated plan, stated once for timed and untimed plans alike, and what the host decides on it: where a running walk
// may be cut for a new goal (wcqp_tick_replan_goals, include/wcqp.h, which states the rule; tests/helpers/goal_merge.py and
// goal_merge_timed.py restate it), how many support-polygon sets a plan reaches, how many stages it spans, and whether its stage indices
// fit - and whether a running plan may be rebased (wcqp_tick_rebase_plan).  Pure host arithmetic in long long.  No HIP header:
// tests/cpp/goal_merge_check.cpp, goal_merge_timed_check.cpp, timeline_count_check.cpp and rebase_check.cpp build it alone.
#pragma once

namespace wcqp_goal {

// One robot's plan: generated from stage `origin`, `first_ds` stages of double support, then `n_steps` steps, step k of ss(k) stages of
// single and ds(k) of double support.  Step k's single support starts at s_k: s_0 = origin + first_ds, s_{k+1} = s_k + ss(k) + ds(k).
// The durations are one common (ss, ds) - an untimed plan - or per-step rows, step k's at [k * stride] of two arrays that stay the
// caller's: rows i of a wcqp_tick_step_timing (stride 1) or a handle's interleaved ss_0, ds_0, ss_1, ... (stride 2).  Rows of a plan
// without steps are not read.
struct Timeline {
    int origin, first_ds, n_steps;
    int common_ss, common_ds;
    const int *ss_k, *ds_k;
    int stride;                   // 0: the common durations

    static Timeline uniform(int origin, int first_ds, int n_steps, int ss, int ds) { return {origin, first_ds, n_steps, ss, ds, nullptr, nullptr, 0}; }
    static Timeline per_step(int origin, int first_ds, int n_steps, const int* ss_k, const int* ds_k, int stride) {
        return {origin, first_ds, n_steps, 0, 0, ss_k, ds_k, stride};
    }
    long long ss(int k) const { return stride ? ss_k[(long long)k * stride] : common_ss; }
    long long ds(int k) const { return stride ? ds_k[(long long)k * stride] : common_ds; }
    long long first_step() const { return (long long)origin + first_ds; }      // s_0

    // every step it takes has a stage of single and a stage of double support at least
    bool durations_valid() const {
        for (int k = 0; k < n_steps; ++k)
            if (ss(k) < 1 || ds(k) < 1) return false;
        return true;
    }
    // the stages its steps occupy behind the first double support, the last step's double support as the plan resolves it: final_ds
    // stages, or - 0 - its own
    long long span(int final_ds) const {
        long long sum = 0;
        for (int k = 0; k < n_steps; ++k) sum += ss(k) + (k == n_steps - 1 && final_ds > 0 ? final_ds : ds(k));
        return sum;
    }
    // the changes of contact pair at stages <= reach - per step the stance foot alone at s_k, both again at s_k + ss(k) -: the
    // support-polygon sets the plan builds behind its origin's where a tick reaches `reach`
    int sets_up_to(long long reach) const {
        int sets = 0;
        long long s_k = first_step();
        for (int k = 0; k < n_steps && s_k <= reach; ++k) {
            sets += 1 + (s_k + ss(k) <= reach ? 1 : 0);
            s_k += ss(k) + ds(k);
        }
        return sets;
    }
};

// Stage indices are 32-bit: a plan that starts at stage `start` and spans `span` more stays below 2^30.  Where the steps are not at hand
// the callers bound the span by span_bound: K steps of at most `longest` stages, and a last double support on top.
inline bool stages_fit(long long start, long long span) { return start + span <= (1ll << 30); }
inline long long span_bound(int K, long long longest, int final_ds) { return (long long)K * longest + final_ds; }

constexpr int kTooLate = -2;      // WCQP_GOAL_TOO_LATE

// M lies inside one of the plan's single supports: [s_k, s_k + ss(k)) of a step k < n_steps
inline bool in_single_support(const Timeline& p, int M) {
    long long s_k = p.first_step();
    for (int k = 0; k < p.n_steps && s_k <= M; ++k) {
        if (M < s_k + p.ss(k)) return true;
        s_k += p.ss(k) + p.ds(k);
    }
    return false;
}

// An explicit merge stage, as wcqp_tick_replan_footsteps takes it: not stage 0, not a stage the enqueued ticks have consumed (t0: the ticks
// enqueued so far, plus 1 when a resident plan's stage has been staged), within the T stages, behind the plan's own origin, both feet down
inline bool merge_allowed(const Timeline& p, int M, int t0, int T) {
    return M >= 1 && M >= t0 && M < T && M >= p.origin && !in_single_support(p, M);
}

// AUTO: the plan's merge points are the first stage of each inner double support, s_k + ss(k) for k = 0 .. n - 2, and every stage >= L, where
// L = s_{n-1} + ss(n-1) (n = 0: L = origin) - the last double support and standing.  The smallest one that is >= max(t0 + min_lead, 1, origin),
// or kTooLate when that is no stage below T.
inline int merge_auto(const Timeline& p, int t0, int min_lead, int T) {
    long long lo = (long long)t0 + min_lead;
    if (lo < 1) lo = 1;
    if (lo < p.origin) lo = p.origin;
    long long M = lo;
    long long s_k = p.first_step();
    for (int k = 0; k < p.n_steps; ++k) {
        // the first s_k + ss(k) at or above lo; the last one is L itself, and at or above L every stage is a merge point
        const long long m_k = s_k + p.ss(k);
        if (m_k >= lo) { M = m_k; break; }
        s_k = m_k + p.ds(k);
    }
    return M < T ? (int)M : kTooLate;
}

// The plan stands - its steps are over, the last double support included - from a stage <= max_ticks on: every change of contact pair
// it holds lies at a stage a tick can reach (so each has its support-polygon set), and stage T - 1 is a standing stage
inline bool stands_within(const Timeline& p, int max_ticks, int final_ds) { return p.first_step() + p.span(final_ds) <= max_ticks; }

// A rebase by `shift` stages (wcqp_tick_rebase_plan, include/wcqp.h, which states the rule; tests/helpers/plan_rebase.py restates it):
// even - the MPC -> IK hand-off record is addressed by the tick's parity -, 2 at least, no more than the ticks enqueued, and on a plan
// that stands within max_ticks.  The origin of `p` may be negative: a plan rebased before.
inline bool rebase_allowed(const Timeline& p, int shift, int ticks_enqueued, int max_ticks, int final_ds) {
    return shift >= 2 && (shift & 1) == 0 && shift <= ticks_enqueued && stands_within(p, max_ticks, final_ds);
}
// WCQP_TICK_REBASE_AUTO: the largest even shift <= the ticks enqueued (below 2: no rebase is allowed)
inline int rebase_auto(int ticks_enqueued) { return ticks_enqueued > 0 ? ticks_enqueued & ~1 : 0; }

}  // namespace wcqp_goal
