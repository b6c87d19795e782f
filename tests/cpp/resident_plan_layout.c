/* Offsets and sizes of wcqp_tick_params_ext and wcqp_tick_info_ext (include/wcqp.h), for tests/test_tick_resident_plan.py to compare with
 * capi's ctypes mirrors - per struct the field's offset, its size, the struct's size - and, last, the sizes of wcqp_tick_params and
 * wcqp_tick_info, which the feature leaves as they were. */
#include <stddef.h>
#include <stdio.h>
#include "wcqp.h"

int main(void) {
    printf("%zu %zu %zu\n", offsetof(wcqp_tick_params_ext, resident_plan), sizeof(((wcqp_tick_params_ext*)0)->resident_plan),
           sizeof(wcqp_tick_params_ext));
    printf("%zu %zu %zu\n", offsetof(wcqp_tick_info_ext, resident_plan), sizeof(((wcqp_tick_info_ext*)0)->resident_plan),
           sizeof(wcqp_tick_info_ext));
    printf("%zu %zu\n", sizeof(wcqp_tick_params), sizeof(wcqp_tick_info));
    return 0;
}
