/* Offsets and sizes of wcqp_unicycle_params, wcqp_unicycle_inputs and wcqp_unicycle_outputs (include/wcqp.h), for
 * tests/test_unicycle_planner.py to compare with capi's ctypes mirrors: one line per struct, every field in declaration order, then the size. */
#include <stddef.h>
#include <stdio.h>
#include "wcqp.h"

#define P(f) printf("%zu ", offsetof(wcqp_unicycle_params, f))
#define I(f) printf("%zu ", offsetof(wcqp_unicycle_inputs, f))
#define O(f) printf("%zu ", offsetof(wcqp_unicycle_outputs, f))
int main(void) {
    P(dT); P(reference_position); P(unicycle_gain); P(slow_when_turning_gain); P(max_linear_velocity); P(max_angular_velocity);
    P(max_step_length); P(min_step_length); P(min_width); P(nominal_width); P(max_angle_variation); P(min_angle_variation);
    P(step_ticks); P(max_steps);
    printf("%zu\n", sizeof(wcqp_unicycle_params));
    I(left0); I(right0); I(goal); I(first_side);
    printf("%zu\n", sizeof(wcqp_unicycle_inputs));
    O(n_steps); O(side); O(target); O(status); O(desired_point); O(unicycle_end);
    printf("%zu\n", sizeof(wcqp_unicycle_outputs));
    return 0;
}
