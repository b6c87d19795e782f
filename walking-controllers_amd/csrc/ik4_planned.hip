// The tick kernels with planned trajectories (wcqp_tick_params.planned_trajectories; ik4_tick_plan_kernel and tick_plan_prime_kernel of
// ik4.hip, either DCM controller, with or without gain scheduling) as a translation unit - and so a code object - of their own: the
// kernels of ik4.hip, ik4_reactive.hip and ik4_zmp_gs.hip keep the places they have in theirs.
#define WCQP_IK4_PLAN_TU
#include "ik4.hip"
