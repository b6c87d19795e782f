// The tick kernels with ZMP-CoM gain scheduling (wcqp_tick_params.zmp_gain_scheduling; ik4_tick_gs_kernel and tick_gs_prime_kernel of
// ik4.hip, either DCM controller) as a translation unit - and so a code object - of their own: the kernels of ik4.hip and of
// ik4_reactive.hip keep the places they have in theirs.
#define WCQP_IK4_GS_TU
#include "ik4.hip"
