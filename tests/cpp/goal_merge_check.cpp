// csrc/goal_merge.h on its own (it includes no HIP header): the merge stage of WCQP_TICK_MERGE_AUTO for a table of plans, one line per
// case - "n O fo ss ds t0 lead T M allowed" - which tests/test_goal_replan_host.py compares with tests/helpers/goal_merge.py.  `allowed`
// is merge_allowed(M), the check an explicit merge stage gets (1 for every M the rule returns; -1 where it returns TOO_LATE).
// The table: n in {0, 1, 2, 6} steps of ss + ds = 30 + 20 behind fo = 20, origins 0 and 105, t0 over every stage of the plan, leads 0, 20 and
// 60 (>= per), with T = 460 (some t0 + lead run past it: TOO_LATE) and a short T = 130.
#include <cstdio>
#include "goal_merge.h"

int main() {
    const int ss = 30, ds = 20, fo = 20;
    const int ns[] = {0, 1, 2, 6}, origins[] = {0, 105}, leads[] = {0, 20, 60}, Ts[] = {460, 130};
    long rows = 0;
    for (int n : ns)
        for (int O : origins)
            for (int lead : leads)
                for (int T : Ts) {
                    const wcqp_goal::Timeline p = wcqp_goal::Timeline::uniform(O, fo, n, ss, ds);
                    const int end = O + fo + n * (ss + ds) + ds;      // one stage past the plan's last double support
                    for (int t0 = 0; t0 <= end && t0 < T; ++t0) {
                        const int M = wcqp_goal::merge_auto(p, t0, lead, T);
                        const int ok = M == wcqp_goal::kTooLate ? -1 : (wcqp_goal::merge_allowed(p, M, t0, T) ? 1 : 0);
                        std::printf("%d %d %d %d %d %d %d %d %d %d\n", n, O, fo, ss, ds, t0, lead, T, M, ok);
                        ++rows;
                    }
                }
    // the far corners: nothing overflows
    const wcqp_goal::Timeline big = wcqp_goal::Timeline::uniform(1 << 29, 1 << 29, 1 << 20, 1 << 9, 1 << 9);
    const int M = wcqp_goal::merge_auto(big, 2147483647, 2147483647, 2147483647);
    std::printf("corner %d\n", M);
    std::printf("goal_merge ok %ld\n", rows);
    return 0;
}
