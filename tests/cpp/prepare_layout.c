/* Offsets and size of wcqp_prepare_params (include/wcqp.h), for tests/test_prepare.py to compare with capi's ctypes mirror: every field
 * in declaration order, then the size. */
#include <stddef.h>
#include <stdio.h>
#include "wcqp.h"

#define F(f) printf("%zu ", offsetof(wcqp_prepare_params, f))
int main(void) {
    F(w_q); F(w_n); F(step_cap); F(tol_step); F(tol_constraint); F(max_iter); F(q_reg); F(q_min); F(q_max);
    printf("%zu\n", sizeof(wcqp_prepare_params));
    return 0;
}
