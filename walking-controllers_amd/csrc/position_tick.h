// The POSITION mode of the closed-loop tick (wcqp_tick_params.ik_mode = WCQP_TICK_IK_POSITION, include/wcqp.h): what the tick handle
// (tick_handle.h, tick.hip) and the kernel (position_tick.hip) share, and the host code the two users of the non-linear IK - wcqp_prepare_create and
// wcqp_tick_create - build its tables with (prepare.hip).  Internal, not ABI.
#pragma once
#include <vector>
#include "wcqp_internal.h"
#include "tick_device.h"

namespace wcqp {

// a wcqp_prepare_params as the kernels take it: the model table of the 16-lane walk, the parameter rows q_reg | q_min | q_max, the scalars
struct PrepareHost {
    std::vector<double> tab, par;
    int kin_rounds = 0; unsigned pm[3] = {0u, 0u, 0u};
    double w_q = 0.0, w_n = 0.0, step_cap = 0.0, tol_step = 0.0, tol_c = 0.0;
    int max_iter = 0, use_limits = 0;
};
// what wcqp_prepare_create refuses from the scalars alone: WCQP_OK or WCQP_E_INVALID (dof: the length of q_reg / q_min / q_max)
int prepare_check_scalars(const wcqp_prepare_params* p);
// ... and from the arrays: a NULL or non-finite q_reg, only one of q_min / q_max, crossed or NaN limits
int prepare_check_arrays(const wcqp_prepare_params* p);
// the tables (after the two checks): WCQP_E_UNSUPPORTED for a tree the 16-lane walk cannot run
int prepare_host_tables(wcqp_kin_t kin, const wcqp_prepare_params* p, PrepareHost* out);

// the record position_tick_kernel takes beside the handle's TickDevPL (whose layout stays what it was)
struct PosTickDev {
    const double* kin_tab; int kin_rounds; unsigned pm[3];
    const double* par;                         // q_reg [23] | q_min [23] | q_max [23]
    double w_q, w_n, step_cap, tol_step, tol_c;
    int max_iter, use_limits;
    double* q_log;                             // [log_ticks][B][dof]
    long long* ik_iters;                       // [B]
    unsigned *alo, *aup;                       // [B] the limits active in the last QP of the last tick (a tick that ends SOLVED; else 0)
};
// n_inner ticks from the tick index tick2[phase], one launch (td_dev: the handle's TickDevPL in device memory).  external: a streamed
// handle of the EXTERNAL plant - the chain on the measured state and the robot's live record, n_inner = 1 (WCQP_E_INVALID otherwise)
int position_tick_enqueue(const wcqp_tick::TickDevPL* td_dev, const PosTickDev& a, int batch, bool external, bool reactive, bool gain_sched, int phase,
                          int n_inner, hipStream_t stream);

}  // namespace wcqp
