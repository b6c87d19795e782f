/* Offsets and sizes of wcqp_tick_footsteps and wcqp_tick_plan_window (include/wcqp.h), for tests/test_tick_footsteps.py to compare with
 * capi's ctypes mirrors: every field in declaration order, then the size. */
#include <stddef.h>
#include <stdio.h>
#include "wcqp.h"

#define F(f) printf("%zu ", offsetof(wcqp_tick_footsteps, f))
#define W(f) printf("%zu ", offsetof(wcqp_tick_plan_window, f))
int main(void) {
    F(max_steps); F(n_steps); F(side); F(target); F(first_ds_ticks); F(ss_ticks); F(ds_ticks); F(final_ds_ticks); F(lift); F(zmp_delta_left);
    F(zmp_delta_right);
    printf("%zu\n", sizeof(wcqp_tick_footsteps));
    W(left_traj); W(right_traj); W(left_twist); W(right_twist); W(contact); W(com_height); W(com_height_vel); W(ref_traj); W(dcm_vel_traj);
    W(hull_A); W(hull_b); W(hull_nc); W(u_init);
    printf("%zu\n", sizeof(wcqp_tick_plan_window));
    return 0;
}
