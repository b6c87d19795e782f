// csrc/goal_merge.h on its own (it includes no HIP header): the admission rule of wcqp_tick_rebase_plan, rebase_allowed, and AUTO's shift,
// which tests/test_plan_rebase_host.py compares with the restatement of tests/helpers/plan_rebase.py.
// The plans: n in 0..2 steps, every ss_k and ds_k in 1..3, origins -6, -1, 0 and 2 (a plan rebased before has a negative one), first double
// supports of 1 and 2 stages, a final_ds of 0 (the last step's own ds), 1 and 4.  With `stand` the first standing stage of the plan, per plan:
//   P n O fo final_ds stand ss_0 ds_0 ...    the plan
//   R max_ticks <words>                      max_ticks = stand - 1, stand (standing exactly at max_ticks), stand + 1: one word per ticks_enqueued
//                                            in 0..6, one digit per shift in -1..8 (odd and even, equal to ticks_enqueued and one above it)
// A plan of equal durations is also built from its common (ss, ds); the last lines count those comparisons and their mismatches.
#include <cstdio>
#include <string>
#include "goal_merge.h"

int main() {
    long plans = 0, uniform = 0, mismatches = 0;
    const int finals[3] = {0, 1, 4}, origins[4] = {-6, -1, 0, 2};
    for (int n = 0; n <= 2; ++n) {
        int combos = 1;
        for (int k = 0; k < 2 * n; ++k) combos *= 3;
        for (int code = 0; code < combos; ++code) {
            int dur[4] = {0, 0, 0, 0};
            bool same = true;
            for (int k = 0, c = code; k < 2 * n; ++k, c /= 3) {
                dur[k] = 1 + c % 3;
                if (k >= 2 && dur[k] != dur[k - 2]) same = false;
            }
            for (int O : origins)
                for (int fo = 1; fo <= 2; ++fo)
                    for (int fin : finals) {
                        const wcqp_goal::Timeline p = wcqp_goal::Timeline::per_step(O, fo, n, dur, dur + 1, 2);
                        const wcqp_goal::Timeline u = wcqp_goal::Timeline::uniform(O, fo, n, n ? dur[0] : 1, n ? dur[1] : 1);
                        const long long stand = p.first_step() + p.span(fin);
                        std::string line = "P " + std::to_string(n) + " " + std::to_string(O) + " " + std::to_string(fo) + " " + std::to_string(fin) +
                                           " " + std::to_string(stand);
                        for (int k = 0; k < 2 * n; ++k) line += " " + std::to_string(dur[k]);
                        for (int mt = (int)stand - 1; mt <= (int)stand + 1; ++mt) {
                            line += "\nR " + std::to_string(mt);
                            if (wcqp_goal::stands_within(p, mt, fin) != (stand <= mt)) ++mismatches;
                            for (int te = 0; te <= 6; ++te) {
                                line += " ";
                                for (int shift = -1; shift <= 8; ++shift) {
                                    const bool ok = wcqp_goal::rebase_allowed(p, shift, te, mt, fin);
                                    line += ok ? "1" : "0";
                                    if (same) { ++uniform; mismatches += ok != wcqp_goal::rebase_allowed(u, shift, te, mt, fin); }
                                }
                            }
                        }
                        std::puts(line.c_str());
                        ++plans;
                    }
        }
    }
    // AUTO: the largest even shift <= the ticks enqueued, and allowed exactly from two ticks on (on a plan that stands)
    std::string au = "auto";
    const wcqp_goal::Timeline still = wcqp_goal::Timeline::uniform(-40, 3, 0, 1, 1);
    for (int te = 0; te <= 9; ++te) {
        const int r = wcqp_goal::rebase_auto(te);
        au += " " + std::to_string(r);
        if (wcqp_goal::rebase_allowed(still, r, te, 5, 0) != (te >= 2)) ++mismatches;
    }
    std::puts(au.c_str());
    // the far corner: a plan at the stage-index bound overflows nothing
    const int far[2] = {1 << 29, 1 << 29};
    const wcqp_goal::Timeline big = wcqp_goal::Timeline::per_step(-(1 << 30), 1 << 29, 1, far, far + 1, 2);
    std::printf("corner %d %d\n", (int)wcqp_goal::rebase_allowed(big, 1 << 30, 1 << 30, 1 << 29, 0), (int)wcqp_goal::rebase_allowed(big, 1 << 30, 1 << 30, (1 << 29) - 1, 0));
    std::printf("uniform %ld mismatches %ld\n", uniform, mismatches);
    std::printf("rebase_check ok %ld\n", plans);
    return mismatches == 0 ? 0 : 1;
}
