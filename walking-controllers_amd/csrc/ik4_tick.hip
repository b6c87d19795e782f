// The skewed tick with any of the chain's features - the reactive DCM controller (wcqp_tick_params.dcm_controller), ZMP-CoM gain
// scheduling (zmp_gain_scheduling), planned trajectories (planned_trajectories) - as ONE family of kernels in a code object of its own:
// ik4.hip's code object carries the headline's kernels and stays as it is.  A new feature of the tick is one more flag of
// these kernels and of TickVariant (ik_common.h).  The device code is ik4_device.h's (ik4_body, ik4_tick_walk, tick_variant_visit), its
// sizes, LDS map, build knobs and stamps ik4_layout.h's.
#include "ik4_device.h"

namespace {

// the walk of ik4_kernel<true, JSRC, LOG, EXT> with the features' chain.  kgains: the MPC's gain blocks with fused kinematics (the reactive
// controller reads none)
template <int JSRC, bool LOG, bool EXT, bool REACT, bool GS, bool PL>
__global__ __launch_bounds__(64, WCQP_IK4_WAVES)
void ik4_tick_variant_kernel(const IkDeviceParams* __restrict__ prm, int batch,
                             const double* __restrict__ JL, const double* __restrict__ JR,
                             const double* __restrict__ JN, const double* __restrict__ JC,
                             const double* qpos, const double* __restrict__ state,
                             double* __restrict__ dq_out, int* __restrict__ status_out,
                             unsigned* __restrict__ alo_out, unsigned* __restrict__ aup_out,
                             double* __restrict__ ferr_out, int* __restrict__ iters_out, const wcqp_tick::TickDev* __restrict__ tdp, int phase, int n_inner, int skip_last_mpc)
{
    __shared__ __attribute__((aligned(16))) double smem[4][PER_INST];
    __shared__ __attribute__((aligned(16))) double kmodel[JSRC == 2 ? wcqp_tick::kKinTabSize : 2];
    __shared__ __attribute__((aligned(16))) double kgains[JSRC == 2 && !REACT ? 4 * wcqp_tick::kGainsLdsStages : 2];
    ik4_tick_walk<JSRC, LOG, EXT, REACT, GS, PL>(prm, batch, JL, JR, JN, JC, qpos, state, dq_out, status_out, alo_out, aup_out, ferr_out, iters_out,
                                                 tdp, phase, n_inner, skip_last_mpc, smem, kmodel, REACT ? nullptr : kgains);
}

// The chain of ONE tick of such a handle for every robot, on its own: primes its skewed tick after an upload (tick_mpc_prime_kernel of
// ik4.hip with the features).  The MPC, or (REACT) the reactive controller; GS: the smoother state and the velocity stage loaded with the
// chain's other loads, setPhase, then the controller's finish with the tick's gains; PL: the contact pair from the planner's flags of
// tick t (a change rebuilds the hull rows from its desired feet).  td: the slice of the handle's record the flags read
template <bool GS, bool PL>
using TickPrimeRecord = std::conditional_t<PL, wcqp_tick::TickDevPL, std::conditional_t<GS, wcqp_tick::TickDevGS, wcqp_tick::TickDev>>;
template <bool EXT, bool REACT, bool GS, bool PL>
__global__ __launch_bounds__(64)
void tick_variant_prime_kernel(TickPrimeRecord<GS, PL> td, int t)
{
    __shared__ __attribute__((aligned(16))) double s_hull[4][WCQP_HULL_ROWS][4];
    const int lane = threadIdx.x, grp = lane >> 4, j = lane & 15;
    // (the reactive controller alone reads no hull rows and forms the robot index from the lane: the instructions it had in a kernel of its own)
    const long inst_raw = (long)blockIdx.x * 4 + (REACT && !GS && !PL ? lane >> 4 : grp);
    const bool live = inst_raw < td.batch;
    const long inst = live ? inst_raw : (long)td.batch - 1;
    wcqp_tick::TickMpcRegs mreg;
    wcqp_tick::ZmpRegs zreg;
    double2 r0, rd = make_double2(0.0, 0.0);
    if constexpr (REACT) wcqp_tick::tick_react_issue(td, j, inst, t, mreg, r0, rd);
    else {
        wcqp_tick::tick_mpc_issue(td, j, inst, t, mreg);
        if constexpr (GS) rd = wcqp_tick::zmp_vel_issue(td, inst, t);
    }
    int code = -1;
    if constexpr (PL) code = wcqp_tick::plan_code((int)wcqp_tick::plan_rec<PL && EXT>(td, inst, t)[wcqp_tick::kPlanFlags]);
    double2 kg = make_double2(0.0, 0.0);
    if constexpr (GS) {
        wcqp_tick::zmp_state_issue(td, inst, zreg);
        kg = wcqp_tick::zmp_gains_at(td, td.zg, wcqp_tick::zmp_smoother_advance(td, inst, j == 0 && live, rd, zreg));
    }
    if constexpr (REACT) wcqp_tick::tick_react_finish<EXT, GS>(td, j, inst, live, t, mreg, r0, wcqp_tick::tick_react_law(td, j, mreg, r0, rd), nullptr, kg);
    else wcqp_tick::tick_mpc_finish<false, EXT, GS, PL, PL && EXT>(td, j, inst, live, t, mreg, s_hull[grp], nullptr, code, nullptr, kg);
}

}  // namespace

namespace wcqp_ik {

void ik4_launch_tick_variant(const IkDeviceParams* prm, const wcqp_tick::TickDev& td, const wcqp_tick::TickDev* td_dev, const TickVariant& v,
                             const IkIo& io, int n_inner, int skip_last_mpc, hipStream_t stream) {
    tick_variant_visit(v, [&](auto j, auto l, auto e, auto r, auto g, auto p) {
        if constexpr (r || g || p)
            hipLaunchKernelGGL((ik4_tick_variant_kernel<j, l, e, r, g, p>), dim3((unsigned)((td.batch + 3) / 4)), dim3(64), 0, stream, prm, td.batch,
                               io.JL, io.JR, io.JN, io.JC, io.q, io.state, io.dq, io.status, io.alo, io.aup, io.ferr, io.iters,
                               td_dev, td.phase, n_inner, skip_last_mpc);
    });
}

void ik4_launch_tick_prime_variant(const wcqp_tick::TickDevPL& td, const TickVariant& v, int t, hipStream_t stream) {
    tick_variant_visit(v, [&](auto, auto, auto e, auto r, auto g, auto p) {
        if constexpr (r || g || p)
            hipLaunchKernelGGL((tick_variant_prime_kernel<e, r, g, p>), dim3((unsigned)((td.batch + 3) / 4)), dim3(64), 0, stream,
                               static_cast<const TickPrimeRecord<g, p>&>(td), t);
    });
}

}  // namespace wcqp_ik
