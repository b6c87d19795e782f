// The tick kernels with the REACTIVE DCM controller (wcqp_tick_params.dcm_controller; ik4_tick_reactive_kernel and
// tick_reactive_prime_kernel of ik4.hip) as a translation unit - and so a code object - of their own: ik4.hip's kernels keep the
// places they have in theirs.
#define WCQP_IK4_REACTIVE_TU
#include "ik4.hip"
