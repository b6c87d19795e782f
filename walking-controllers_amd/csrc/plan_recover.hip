// Stopped robots stood up on the device (wcqp_tick_recover_robots; include/wcqp.h states THE RECOVERED ROBOT,
// tests/helpers/plan_recover.py restates its targets and the host composition it equals).  Between the ticks already enqueued and the
// restart of plan_restart.hip, in stream order:
//   plan_recover_gather_kernel  16 lanes per slot, four slots per wave - the rows prepare_kernel reads: decides whether the slot goes on
//                               (IF_STOPPED: ik_fail > 0; soles from the plan: record S is a double support), and writes the rows of the
//                               slots that go on - the caller's, or the soles and height of record S, the standing ZMP of the soles, the
//                               robot's q_des - PACKED to the front of the call's block: a wave ballot of its four decisions and ONE atomic
//                               add of the wave's count on a device counter give each slot its row.  The order of the packed rows is
//                               whatever the waves' atomics make it - a row's IK does not depend on where it lies (prepare.hip)
//   prepare_kernel              (prepare.hip, prepare_rows.h) over the packed rows alone: it reads the counter
//   plan_recover_gate_kernel    16 lanes per slot: a slot restarts iff it went on and its IK ended SOLVED; the packed q / pose block go
//                               to the slot's rows of PlanRestartDev (q0, state0, com0 = the block's CoM), status / iters / residual to
//                               the slot's result row (a slot that did not go on: its decision, 0, 0)
// Plain vector loads and stores, 64-bit row offsets into the records.
#include "plan_gen.h"

namespace {

using namespace wcqp_tick;

__global__ __launch_bounds__(64) void plan_recover_gather_kernel(PlanRecoverDev g) {
    const int lane = threadIdx.x, grp = lane >> 4, j = lane & 15;
    const long r_raw = (long)blockIdx.x * 4 + grp;
    const bool live = r_raw < g.n_robots;
    const size_t r = (size_t)(live ? r_raw : (long)g.n_robots - 1);
    const size_t i = (size_t)g.robots[r];
    const double* recS = g.rec + (i * (size_t)g.traj_len + (size_t)g.stage) * kPlanRec;
    int code = 0;
    if (g.mode[r] == WCQP_TICK_RESTART_IF_STOPPED && !(g.ik_fail[i] > 0)) code = WCQP_RECOVER_NOT_STOPPED;
    else if (!g.left_in && ((int)recS[kPlanFlags] & 3) != 3) code = WCQP_RECOVER_NOT_STANDING;
    const bool go = live && code == 0;
    // the wave's slots that go on take consecutive rows from the counter
    const unsigned long long votes = __ballot(go && j == 0);
    int base = 0;
    if (lane == 0 && votes != 0ull) base = atomicAdd(g.count, __popcll(votes));
    base = __shfl(base, 0);
    const int p = base + __popcll(votes & ((1ull << (grp * 16)) - 1ull));
    if (live && j == 0) g.pos[r] = go ? p : code;
    if (!go) return;
    const double* left = g.left_in ? g.left_in + r * 12 : recS + kPlanLeft;
    const double* right = g.right_in ? g.right_in + r * 12 : recS + kPlanRight;
    if (j < 12) { g.p_left[(size_t)p * 12 + j] = left[j]; g.p_right[(size_t)p * 12 + j] = right[j]; }
    if (j < 3) {
        double c;
        if (g.com_in) c = g.com_in[r * 3 + j];
        else if (j == 2) c = recS[kPlanHeight];
        else {
#pragma clang fp contract(off)
            const double zl = zmp_point_ax(left, g.delta[0], j), zr = zmp_point_ax(right, g.delta[1], j);
            c = 0.5 * (zl + zr);
        }
        g.p_com[(size_t)p * 3 + j] = c;
    }
    if (g.neck_in && j < 9) g.p_neck[(size_t)p * 9 + j] = g.neck_in[r * 9 + j];
    for (int e = j; e < kDof; e += 16) g.p_q[(size_t)p * kDof + e] = g.q_in ? g.q_in[r * kDof + e] : g.q_des[i * kDof + e];
}

__global__ __launch_bounds__(64) void plan_recover_gate_kernel(PlanRecoverDev g) {
    const int lane = threadIdx.x, j = lane & 15;
    const long r_raw = (long)blockIdx.x * 4 + (lane >> 4);
    if (r_raw >= g.n_robots) return;
    const size_t r = (size_t)r_raw;
    const int p = g.pos[r];
    if (p < 0) {       // the slot did not go on: nothing of the robot changes
        if (j == 0) { g.decided[r] = 0; g.status[r] = p; g.iters[r] = 0; }
        if (j < 2) g.residual[r * 2 + j] = 0.0;
        return;
    }
    const double* st = g.o_state + (size_t)p * kStateLen;
    for (int e = j; e < kStateLen; e += 16) g.state0[r * kStateLen + e] = st[e];
    for (int e = j; e < kDof; e += 16) g.q0[r * kDof + e] = g.o_q[(size_t)p * kDof + e];
    if (j < 2) { g.com0[r * 2 + j] = st[66 + j]; g.residual[r * 2 + j] = g.o_res[(size_t)p * 2 + j]; }
    if (j == 0) {
        const int status = g.o_status[p];
        g.decided[r] = status == WCQP_STATUS_SOLVED ? 1 : 0;
        g.status[r] = status; g.iters[r] = g.o_iters[p];
    }
}

bool complete(const PlanRecoverDev& g) {
    if (!g.robots || !g.mode || !g.ik_fail || !g.q_des || !g.rec || !g.pos || !g.count || !g.p_left || !g.p_right || !g.p_com || !g.p_q) return false;
    if ((g.left_in == nullptr) != (g.right_in == nullptr) || (g.neck_in && !g.p_neck)) return false;
    if (!g.o_q || !g.o_state || !g.o_res || !g.o_status || !g.o_iters || !g.state0 || !g.q0 || !g.com0 || !g.decided || !g.status || !g.iters || !g.residual) return false;
    // (stage S has a record)
    return g.n_robots >= 1 && g.traj_len >= 1 && g.stage >= 0 && g.stage < g.traj_len;
}

}  // namespace

namespace wcqp {

int plan_recover_gather_enqueue(const PlanRecoverDev& g, hipStream_t stream) {
    if (!complete(g)) return WCQP_E_INVALID;
    hipLaunchKernelGGL(plan_recover_gather_kernel, dim3((unsigned)((g.n_robots + 3) / 4)), dim3(64), 0, stream, g);
    WCQP_HIP_TRY(hipGetLastError());
    return WCQP_OK;
}

int plan_recover_gate_enqueue(const PlanRecoverDev& g, hipStream_t stream) {
    if (!complete(g)) return WCQP_E_INVALID;
    hipLaunchKernelGGL(plan_recover_gate_kernel, dim3((unsigned)((g.n_robots + 3) / 4)), dim3(64), 0, stream, g);
    WCQP_HIP_TRY(hipGetLastError());
    return WCQP_OK;
}

}  // namespace wcqp
