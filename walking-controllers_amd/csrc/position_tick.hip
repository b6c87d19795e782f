// The POSITION mode of the closed-loop tick (wcqp_tick_params.ik_mode = WCQP_TICK_IK_POSITION; include/wcqp.h states the semantics): the
// reference's `use_QP-IK 0` path, in which WalkingIK::computeIK gives the joint POSITIONS of every tick directly instead of velocities
// that are integrated (citations relative to the reference's modules/Walking_module):
//   src/WalkingModule.cpp:745-769                the non-linear IK of the tick: computeIK(left.front(), right.front(), desiredCoMPosition, qDesired)
//   src/WalkingInverseKinematics.cpp:346-424     computeIK
// One launch walks the ticks of a wcqp_tick_run call (ticks_per_launch caps them), in the layout of prepare_kernel: 16 lanes per robot,
// four robots per wave, one wave per workgroup.  Per tick a wave runs
//   the chain      the stage's record, the LIPM reference, the MPC or the reactive law, the gain schedule where set, the ZMP-CoM law with
//                  its integrator, the internal plant - the device functions of tick_device.h the planned velocity tick's prime kernel
//                  calls (ik4_tick.hip: tick_variant_prime_kernel).  It reads nothing the IK writes and runs for a stopped robot too.
//   the iteration  the targets of the tick (the record's soles, p_star with the record's CoM height, the neck rule) into LDS, then the
//                  blocks of prepare_device.h from the previous tick's joints - which stay in this lane's registers from tick to tick -
//                  until the wave's four robots have stopped or spent the tick's budget
//   the post step  q_des, q_log, ik_fail, ik_iters, the active limits; lane 0 of workgroup 0 advances the tick index at the end.
// The handle is not skewed: nothing of tick t + 1 runs before tick t is done, there is no prime launch.  Plain vector loads and stores only.
// On a streamed handle of the EXTERNAL plant (WCQP_TICK_OPT_POSITION_STREAMED) a launch carries ONE tick, whose chain runs on the measured
// state and the live record the feedback and desired-stage kernels left: position_tick_external_kernel, the same body.
#include "position_tick.h"
#include "prepare_device.h"

namespace {

using namespace wcqp_prep;
using wcqp::PosTickDev;

// The body of both kernels below.  EXT: the handle is a streamed one on the EXTERNAL plant (WCQP_TICK_OPT_POSITION_STREAMED, include/wcqp.h) -
// the chain is the streamed velocity tick's (tick_variant_prime_kernel<true, REACT, GS, true>): the measured DCM, CoM and ZMP are what the
// feedback or sensor kernel left in the per-axis records, the stage is the robot's ONE live record (plan_rec<true>), which also names the
// robot's own hull set.  Everything behind the hand-off fence is the same text for both.
template <bool EXT, bool REACT, bool GS>
__device__ __forceinline__ void position_tick_body(const wcqp_tick::TickDevPL* tdp, const PosTickDev& a, int phase, int n_inner, double* kmodel,
                                                   double (*smem)[P_PER], double (*s_hull)[WCQP_HULL_ROWS][4]) {
    // the handle's record stays in device memory (as in the skewed kernels, ik4_device.h: kernel-argument loads would be hoisted out of
    // the loop over ticks and held in registers across the whole body)
    const wcqp_tick::TickDevPL& td = *tdp;
    const int lane = threadIdx.x, grp = lane >> 4, j = lane & 15;
    for (int k = lane; k < kKinTabSize; k += 64) kmodel[k] = a.kin_tab[k];
    const int batch = td.batch;
    const long inst_raw = (long)blockIdx.x * 4 + grp;
    const bool live = inst_raw < batch;
    const long i = live ? inst_raw : (long)batch - 1;       // (a dead slot repeats the last robot and stores nothing)
    double* S = smem[grp];
    const bool var1 = j < kDof - 16;                 // slot 1 is joint 16 + j
    const int cs[2] = {j, var1 ? 16 + j : 0};
    const bool use_neck = a.w_n > 0.0;
    const double wq = a.w_q, wn = use_neck ? a.w_n : 0.0, iwq = 1.0 / wq;
    double qreg[2], qlo[2], qhi[2], qc[2];
#pragma unroll
    for (int s_ = 0; s_ < 2; ++s_) {
        qreg[s_] = a.par[cs[s_]];
        qlo[s_] = a.use_limits ? a.par[kDof + cs[s_]] : -HUGE_VAL;
        qhi[s_] = a.use_limits ? a.par[2 * kDof + cs[s_]] : HUGE_VAL;
        // the joints the previous tick commanded (tick 0: q0, which the upload checked to be finite), clipped into the limits
        qc[s_] = fmin(fmax(td.q_des[i * kDof + cs[s_]], qlo[s_]), qhi[s_]);
    }
    int kup[2][3], ksub[2];
    __syncthreads();                                 // the model table is in LDS
    const int kfj = walk_links<3>(kmodel, j, cs, kup, ksub);
    unsigned onL[2], onR[2], onN[2];
#pragma unroll
    for (int s_ = 0; s_ < 2; ++s_) {
        onL[s_] = (a.pm[0] >> cs[s_]) & 1u; onR[s_] = (a.pm[1] >> cs[s_]) & 1u; onN[s_] = use_neck ? (a.pm[2] >> cs[s_]) & 1u : 0u;
    }
    const int t0 = td.tick2[phase];
    // (EXT: the feedback, sensor and desired-stage kernels stop a robot they reject by raising ik_fail; read here, at the start of the
    // launch - which then carries that one tick - it is how the rejection reaches the IK)
    long long fails = td.ik_fail[i], spent = a.ik_iters[i];
#pragma unroll 1
    for (int k = 0; k < n_inner; ++k) {
        __asm__ volatile("" ::: "memory");           // nothing of the body is hoisted out of the loop over ticks
        const int t = t0 + k;
        // ================= the chain of tick t (tick_variant_prime_kernel<EXT, REACT, GS, true>)
        {
            wcqp_tick::TickMpcRegs mreg;
            wcqp_tick::ZmpRegs zreg;
            double2 r0, rd = make_double2(0.0, 0.0);
            if constexpr (REACT) wcqp_tick::tick_react_issue(td, j, i, t, mreg, r0, rd);
            else {
                wcqp_tick::tick_mpc_issue(td, j, i, t, mreg);
                if constexpr (GS) rd = wcqp_tick::zmp_vel_issue(td, i, t);
            }
            const int code = wcqp_tick::plan_code((int)wcqp_tick::plan_rec<EXT>(td, i, t)[wcqp_tick::kPlanFlags]);
            double2 kg = make_double2(0.0, 0.0);
            if constexpr (GS) {
                wcqp_tick::zmp_state_issue(td, i, zreg);
                kg = wcqp_tick::zmp_gains_at(td, td.zg, wcqp_tick::zmp_smoother_advance(td, i, j == 0 && live, rd, zreg));
            }
            if constexpr (REACT) wcqp_tick::tick_react_finish<EXT, GS>(td, j, i, live, t, mreg, r0, wcqp_tick::tick_react_law(td, j, mreg, r0, rd), nullptr, kg);
            else wcqp_tick::tick_mpc_finish<false, EXT, GS, true, EXT>(td, j, i, live, t, mreg, s_hull[grp], nullptr, code, nullptr, kg);
        }
        // p_star of tick t is in the hand-off row of parity t & 1, written by lanes 0 / 1 of this robot: visible to its other lanes
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        // ================= the targets: the record's soles, (p_star x, p_star y, the record's CoM height), RotZ(meanYaw) neck_add
        {
            const double* rec = wcqp_tick::plan_rec<EXT>(td, i, t);
            const double* hd = td.hand + ((size_t)(t & 1) * batch + i) * wcqp_tick::kHandLen;
            if (j < 12) { S[P_TG + j] = rec[wcqp_tick::kPlanLeft + j]; S[P_TG + TG_RIGHT + j] = rec[wcqp_tick::kPlanRight + j]; }
            if (j < 2) S[P_TG + TG_COM + j] = hd[j];
            if (j == 2) S[P_TG + TG_COM + 2] = rec[wcqp_tick::kPlanHeight];
            if (j < 9)
                S[P_TG + TG_NECK + j] = wcqp_tick::plan_neck(td.pl.neck_add, j, rec[wcqp_tick::kPlanLeft + 3], rec[wcqp_tick::kPlanLeft + 6],
                                                             rec[wcqp_tick::kPlanRight + 3], rec[wcqp_tick::kPlanRight + 6]);
        }
        wcqp::wave_lds_fence();
        // ================= the iteration, from the joints in hand.  A robot stopped on an earlier tick runs none: the tick counts at once
        const double qg[2] = {qc[0], qc[1]};
        int status = fails > 0 ? WCQP_STATUS_MAX_ITER : -1;      // -1: iterating
        int iters = 0, nw = 0;
        unsigned wmask = 0u;
        while (__ballot(status < 0) != 0ull) {
            double pb[3], Rb[9], e4[2][4], cmax;
            prep_linearise(kmodel, S, j, cs, var1, kup, ksub, kfj, a.kin_rounds, onL, onR, onN, use_neck, wq, wn, qc, qreg, qlo, qhi, pb, Rb, e4, cmax);
            if (status < 0) {
                const int fail = prep_qp(S, j, cs, var1, wq, wn, iwq, nw, wmask);
                prep_step(S, cs, fail, cmax, a.step_cap, a.tol_step, a.tol_c, a.max_iter, qg, qlo, qhi, qc, iters, status);
                wcqp::wave_lds_fence();
            }
        }
        // ================= the post step
        const bool ok = status == WCQP_STATUS_SOLVED;
        if (!ok) fails += 1;
        spent += iters;
        if (live) {
            td.q_des[i * kDof + cs[0]] = qc[0];
            if (var1) td.q_des[i * kDof + cs[1]] = qc[1];
            if (t < td.log_ticks) {
                double* ql = a.q_log + ((size_t)t * batch + i) * kDof;
                ql[cs[0]] = qc[0];
                if (var1) ql[cs[1]] = qc[1];
            }
            if (j == 0) {
                unsigned lo = 0u, up = 0u;
                if (ok) {
                    const int* WI = reinterpret_cast<const int*>(S + P_WI);
                    for (int b = 0; b < nw; ++b) { if (S[P_WS + b] > 0.0) up |= 1u << WI[b]; else lo |= 1u << WI[b]; }
                }
                a.alo[i] = lo; a.aup[i] = up;
                td.ik_fail[i] = fails;
                a.ik_iters[i] = spent;
            }
        }
        wcqp::wave_lds_fence();                      // (lane 0 has read the active-set lists: the next tick's QP may overwrite them)
    }
    // advanceReferenceSignals (WalkingModule.cpp:816): the next launch reads the other copy of the tick index
    if (blockIdx.x == 0 && threadIdx.x == 0) td.tick2[1 - phase] = t0 + n_inner;
}

// a planned handle with the internal plant: the ticks of a run call
template <bool REACT, bool GS>
__global__ __launch_bounds__(64) void position_tick_kernel(const wcqp_tick::TickDevPL* tdp, PosTickDev a, int phase, int n_inner) {
    __shared__ __attribute__((aligned(16))) double kmodel[kKinTabSize];
    __shared__ __attribute__((aligned(16))) double smem[4][P_PER];
    __shared__ __attribute__((aligned(16))) double s_hull[4][WCQP_HULL_ROWS][4];      // the MPC's hull rows (1 KB)
    position_tick_body<false, REACT, GS>(tdp, a, phase, n_inner, kmodel, smem, s_hull);
}
// a streamed handle on the EXTERNAL plant: ONE tick, behind its desired stage and its feedback
template <bool REACT, bool GS>
__global__ __launch_bounds__(64) void position_tick_external_kernel(const wcqp_tick::TickDevPL* tdp, PosTickDev a, int phase) {
    __shared__ __attribute__((aligned(16))) double kmodel[kKinTabSize];
    __shared__ __attribute__((aligned(16))) double smem[4][P_PER];
    __shared__ __attribute__((aligned(16))) double s_hull[4][WCQP_HULL_ROWS][4];
    position_tick_body<true, REACT, GS>(tdp, a, phase, 1, kmodel, smem, s_hull);
}

}  // namespace

namespace wcqp {

int position_tick_enqueue(const wcqp_tick::TickDevPL* td_dev, const PosTickDev& a, int batch, bool external, bool reactive, bool gain_sched, int phase,
                          int n_inner, hipStream_t stream) {
    const dim3 grid((unsigned)((batch + 3) / 4)), block(64);
    if (external) {
        if (n_inner != 1) return WCQP_E_INVALID;
        if (reactive) {
            if (gain_sched) hipLaunchKernelGGL((position_tick_external_kernel<true, true>), grid, block, 0, stream, td_dev, a, phase);
            else hipLaunchKernelGGL((position_tick_external_kernel<true, false>), grid, block, 0, stream, td_dev, a, phase);
        } else {
            if (gain_sched) hipLaunchKernelGGL((position_tick_external_kernel<false, true>), grid, block, 0, stream, td_dev, a, phase);
            else hipLaunchKernelGGL((position_tick_external_kernel<false, false>), grid, block, 0, stream, td_dev, a, phase);
        }
    } else if (reactive) {
        if (gain_sched) hipLaunchKernelGGL((position_tick_kernel<true, true>), grid, block, 0, stream, td_dev, a, phase, n_inner);
        else hipLaunchKernelGGL((position_tick_kernel<true, false>), grid, block, 0, stream, td_dev, a, phase, n_inner);
    } else {
        if (gain_sched) hipLaunchKernelGGL((position_tick_kernel<false, true>), grid, block, 0, stream, td_dev, a, phase, n_inner);
        else hipLaunchKernelGGL((position_tick_kernel<false, false>), grid, block, 0, stream, td_dev, a, phase, n_inner);
    }
    WCQP_HIP_TRY(hipGetLastError());
    return WCQP_OK;
}

}  // namespace wcqp
