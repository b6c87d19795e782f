// csrc/goal_merge.h on its own (it includes no HIP header): the three functions of a plan in force on per-step rows over an exhaustive small
// enumeration, which tests/test_goal_replan_timed_host.py compares with tests/helpers/goal_merge_timed.py.
// The plans: n in 0..3 steps, every ss_k and ds_k in 1..3, origins 0 and 2, first double supports of 1 and 2 stages.  Per plan, with
// S = end + 3 stages (end = O + fo + the steps' stages: M and T run over 0 .. end + 2):
//   P n O fo ss_0 ds_0 ...            the plan
//   S <S bits>                        in_single_support(M), M = 0 .. S - 1
//   A t0 <S words of S bits>          merge_allowed(M, t0, T): word T, bit M; t0 = 0..4
//   U t0 lead <S numbers>             merge_auto(t0, lead, T), T = 0 .. S - 1; t0, lead = 0..4
// Where every step has the same ss and the same ds, the three functions are also compared here on a timeline built from that common
// (ss, ds) against the one built from the equal per-step rows: the last lines count the comparisons and the mismatches.  Both run the one
// per-step walk of the header, so this comparison checks the two ways to build a timeline; that the walk gives the untimed rule's closed
// form rests on the two independent Python restatements, helpers/goal_merge.py (closed form) and helpers/goal_merge_timed.py (enumeration).
#include <cstdio>
#include <string>
#include "goal_merge.h"

int main() {
    long plans = 0, uniform = 0, mismatches = 0;
    std::string line;
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
                    std::printf("P %d %d %d", n, O, fo);
                    for (int k = 0; k < 2 * n; ++k) std::printf(" %d", dur[k]);
                    line = "\nS ";
                    for (int M = 0; M < S; ++M) {
                        const bool in = wcqp_goal::in_single_support(p, M);
                        line += in ? '1' : '0';
                        if (same) { ++uniform; mismatches += in != wcqp_goal::in_single_support(u, M); }
                    }
                    for (int t0 = 0; t0 <= 4; ++t0) {
                        line += "\nA " + std::to_string(t0);
                        for (int T = 0; T < S; ++T) {
                            line += ' ';
                            for (int M = 0; M < S; ++M) {
                                const bool ok = wcqp_goal::merge_allowed(p, M, t0, T);
                                line += ok ? '1' : '0';
                                if (same) { ++uniform; mismatches += ok != wcqp_goal::merge_allowed(u, M, t0, T); }
                            }
                        }
                    }
                    for (int t0 = 0; t0 <= 4; ++t0)
                        for (int lead = 0; lead <= 4; ++lead) {
                            line += "\nU " + std::to_string(t0) + " " + std::to_string(lead);
                            for (int T = 0; T < S; ++T) {
                                const int M = wcqp_goal::merge_auto(p, t0, lead, T);
                                line += " " + std::to_string(M);
                                if (same) { ++uniform; mismatches += M != wcqp_goal::merge_auto(u, t0, lead, T); }
                            }
                        }
                    std::puts(line.c_str());
                    ++plans;
                }
        }
    }
    // the far corners: nothing overflows
    const int far[4] = {1 << 29, 1 << 29, 1 << 29, 1 << 29};
    const wcqp_goal::Timeline big = wcqp_goal::Timeline::per_step(1 << 29, 1 << 29, 2, far, far + 1, 2);
    std::printf("corner %d %d %d\n", wcqp_goal::merge_auto(big, 2147483647, 2147483647, 2147483647), wcqp_goal::merge_auto(big, 0, 0, 2147483647),
                (int)wcqp_goal::in_single_support(big, 2147483647));
    std::printf("uniform %ld mismatches %ld\n", uniform, mismatches);
    std::printf("goal_merge_timed ok %ld\n", plans);
    return mismatches == 0 ? 0 : 1;
}
