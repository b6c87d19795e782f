/* Offsets of the ZMP gain-scheduling fields of include/wcqp.h, for tests/test_tick_zmp_gains.py to compare with capi's ctypes mirrors. */
#include <stddef.h>
#include <stdio.h>
#include "wcqp.h"

int main(void) {
    printf("%zu %zu %zu %zu %zu %zu\n", sizeof(wcqp_tick_params), offsetof(wcqp_tick_params, k_dcm), offsetof(wcqp_tick_params, zmp_gain_scheduling),
           offsetof(wcqp_tick_params, k_com_stance), offsetof(wcqp_tick_params, k_zmp_stance), offsetof(wcqp_tick_params, zmp_smoothing_time));
    printf("%zu %zu %zu\n", sizeof(wcqp_tick_outputs), offsetof(wcqp_tick_outputs, active_upper), offsetof(wcqp_tick_outputs, zmp_gains));
    printf("%zu %zu %zu\n", sizeof(wcqp_tick_info), offsetof(wcqp_tick_info, launches_per_tick), offsetof(wcqp_tick_info, zmp_gain_scheduling));
    return 0;
}
