// csrc/goal_merge.h on its own (it includes no HIP header): the set count and the span of a timeline - the arithmetic a replan admits a
// robot by - over the enumeration of goal_merge_timed_check.cpp, which tests/test_goal_replan_timed_host.py recounts.
// The plans: n in 0..3 steps, every ss_k and ds_k in 1..3, origins 0 and 2, first double supports of 1 and 2 stages.  Per plan, with
// S = end + 3 stages (end = O + fo + the steps' stages):
//   P n O fo ss_0 ds_0 ...            the plan
//   C <S numbers>                     sets_up_to(reach), reach = 0 .. S - 1
//   N <3 numbers>                     span(final_ds), final_ds = 0 (the last step's own ds), 1 and 4
// A plan of equal durations is also built from its common (ss, ds); the last lines count those comparisons and their mismatches.
#include <cstdio>
#include <string>
#include "goal_merge.h"

int main() {
    long plans = 0, uniform = 0, mismatches = 0;
    const int finals[3] = {0, 1, 4};
    for (int n = 0; n <= 3; ++n) {
        int combos = 1;
        for (int k = 0; k < 2 * n; ++k) combos *= 3;
        for (int code = 0; code < combos; ++code) {
            int dur[6] = {0, 0, 0, 0, 0, 0};
            int steps = 0;
            bool same = true;
            for (int k = 0, c = code; k < 2 * n; ++k, c /= 3) {
                dur[k] = 1 + c % 3;
                steps += dur[k];
                if (k >= 2 && dur[k] != dur[k - 2]) same = false;
            }
            for (int O = 0; O <= 2; O += 2)
                for (int fo = 1; fo <= 2; ++fo) {
                    const wcqp_goal::Timeline p = wcqp_goal::Timeline::per_step(O, fo, n, dur, dur + 1, 2);
                    const wcqp_goal::Timeline u = wcqp_goal::Timeline::uniform(O, fo, n, n ? dur[0] : 1, n ? dur[1] : 1);
                    const int S = O + fo + steps + 3;
                    std::string line = "P " + std::to_string(n) + " " + std::to_string(O) + " " + std::to_string(fo);
                    for (int k = 0; k < 2 * n; ++k) line += " " + std::to_string(dur[k]);
                    line += "\nC";
                    for (int reach = 0; reach < S; ++reach) {
                        line += " " + std::to_string(p.sets_up_to(reach));
                        if (same) { ++uniform; mismatches += p.sets_up_to(reach) != u.sets_up_to(reach); }
                    }
                    line += "\nN";
                    for (int f : finals) {
                        line += " " + std::to_string(p.span(f));
                        if (same) { ++uniform; mismatches += p.span(f) != u.span(f); }
                    }
                    if (!p.durations_valid() || !wcqp_goal::stages_fit(p.first_step(), p.span(0))) ++mismatches;
                    std::puts(line.c_str());
                    ++plans;
                }
        }
    }
    // the far corners: nothing overflows, a zero duration is found, and the stage-index bound lies where it is stated
    const int far[4] = {1 << 29, 1 << 29, 1 << 29, 0};
    const wcqp_goal::Timeline big = wcqp_goal::Timeline::per_step(1 << 29, 1 << 29, 2, far, far + 1, 2);
    std::printf("corner %d %d %lld %lld %d %d %d %d\n", big.sets_up_to(2147483647), big.sets_up_to((5ll << 29) - 1), big.span(0), big.span(1 << 29),
                (int)big.durations_valid(), (int)wcqp_goal::stages_fit(1 << 29, 1 << 29), (int)wcqp_goal::stages_fit(1 << 29, (1 << 29) + 1),
                (int)(wcqp_goal::span_bound(1 << 20, 1 << 20, 7) == (1ll << 40) + 7));
    std::printf("uniform %ld mismatches %ld\n", uniform, mismatches);
    std::printf("timeline_count ok %ld\n", plans);
    return mismatches == 0 ? 0 : 1;
}
