/* Offsets and size of wcqp_tick_replan (include/wcqp.h), for tests/test_tick_replan.py to compare with capi's ctypes mirror: every field in
 * declaration order, then the size. */
#include <stddef.h>
#include <stdio.h>
#include "wcqp.h"

#define F(f) printf("%zu ", offsetof(wcqp_tick_replan, f))
int main(void) {
    F(merge_stage); F(max_steps); F(n_steps); F(side); F(target); F(first_ds_ticks);
    printf("%zu\n", sizeof(wcqp_tick_replan));
    return 0;
}
