// The non-linear IK of wcqp_prepare_solve_* (prepare.hip) on rows another kernel left in device memory, their number known to the device
// alone (wcqp_tick_recover_robots, tick_plan.hip).  Internal, not ABI.
#pragma once
#include <vector>
#include "wcqp_internal.h"

namespace wcqp {

// DEVICE pointers, rows as wcqp_prepare_solve_device takes and returns them.  *n_rows <= max_rows rows are solved: the launch covers
// max_rows, and a wave whose first row lies at or past *n_rows leaves before it reads one.  A row's result is bit for bit what the public
// entry points give for its inputs: prepare_kernel, the same code, on a batch of *n_rows
struct PrepareRows {
    int max_rows;
    const int* n_rows;
    const double *left_d, *right_d, *com_d, *Rd_neck /* or NULL */, *q_guess;
    double *q, *state, *residual;
    int *status, *iters;
};
// enqueue-only once the handle's tables are on the device (the first solve of a handle, this one or a public one, puts them there)
int prepare_enqueue_rows(wcqp_prepare_t h, const PrepareRows& r, hipStream_t stream);
// the model table the handle's kernel walks (kin_fused_tables of its wcqp_kin_t at wcqp_prepare_create)
const std::vector<double>& prepare_model_table(wcqp_prepare_t h);

}  // namespace wcqp
