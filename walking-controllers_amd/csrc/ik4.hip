// Jacobian QP-IK, fourth kernel (ik4_device.h: the algorithm and the device code; ik4_layout.h: sizes, LDS map, knobs, stamps): the
// base-eliminated kernel's code object - the stand-alone solve, the plans of steps, the plain skewed tick and its MPC prime.  It holds the
// headline's kernel, qp_plan_kernel, and what is put beside it moves it: no new kernel goes in here - the skewed tick with any
// of the chain's features runs the variant kernels of ik4_tick.hip, a code object of their own - and a change of the plan kernels themselves (the
// last: their launch-invariant tables in LDS) is measured against the parent commit in the bench's forms; the other kernels keep their instructions.
#include "ik4_device.h"

namespace {

template <bool TICK, int JSRC, bool LOG = false, bool EXT = false>
__global__ __launch_bounds__(64, WCQP_IK4_WAVES)
void ik4_kernel(const IkDeviceParams* __restrict__ prm, int batch,
                const double* __restrict__ JL, const double* __restrict__ JR,
                const double* __restrict__ JN, const double* __restrict__ JC,
                const double* qpos, const double* __restrict__ state,
                double* __restrict__ dq_out, int* __restrict__ status_out,
                unsigned* __restrict__ alo_out, unsigned* __restrict__ aup_out,
                double* __restrict__ ferr_out, int* __restrict__ iters_out, const wcqp_tick::TickDev* __restrict__ tdp, int phase, int n_inner, int skip_last_mpc)
{
    __shared__ __attribute__((aligned(16))) double smem[4][PER_INST];
    if constexpr (TICK) {
        __shared__ __attribute__((aligned(16))) double kmodel[JSRC == 2 ? wcqp_tick::kKinTabSize : 2];
        __shared__ __attribute__((aligned(16))) double kgains[JSRC == 2 ? 4 * wcqp_tick::kGainsLdsStages : 2];
        ik4_tick_walk<JSRC, LOG, EXT, false>(prm, batch, JL, JR, JN, JC, qpos, state, dq_out, status_out, alo_out, aup_out, ferr_out, iters_out,
                                             tdp, phase, n_inner, skip_last_mpc, smem, kmodel, kgains);
    } else {
        ik4_body<TICK, JSRC>(prm, batch, JL, JR, JN, JC, qpos, state, dq_out, status_out, alo_out, aup_out, ferr_out, iters_out, wcqp_tick::TickDev{}, smem, xcd_group((int)blockIdx.x, (int)gridDim.x));
    }
}

// The MPC chain of ONE tick for every robot, on its own: primes the skewed tick after an upload (MPC(0) has to have run
// before the first fused launch, which carries IK(0) and MPC(1)).  (tick_variant_prime_kernel of ik4_tick.hip is this kernel with the
// chain's features; the body is not shared through a device function: that moves the code of this one.)
template <bool EXT>
__global__ __launch_bounds__(64)
void tick_mpc_prime_kernel(wcqp_tick::TickDev td, int t)
{
    __shared__ __attribute__((aligned(16))) double s_hull[4][WCQP_HULL_ROWS][4];
    const int lane = threadIdx.x, grp = lane >> 4, j = lane & 15;
    const long inst_raw = (long)blockIdx.x * 4 + grp;
    const bool live = inst_raw < td.batch;
    const long inst = live ? inst_raw : (long)td.batch - 1;
    wcqp_tick::TickMpcRegs mreg;
    wcqp_tick::tick_mpc_issue(td, j, inst, t, mreg);
    wcqp_tick::tick_mpc_finish<false, EXT>(td, j, inst, live, t, mreg, s_hull[grp]);
}


// Both QPs of a batch of robot-ticks in ONE launch (wcqp_qp_enqueue_steps, a record whose two calls go to the same
// stream): workgroups 0 .. ik_blocks-1 are the IK kernel above, the rest the DCM-MPC kernel of mpc.hip (same device
// functions, same results).  At the BASELINE batch each is one wave per SIMD, so the MPC waves run in the slots the IK
// waves leave idle while their inputs are on the way, and the host pays one launch per step instead of two.
__global__ __launch_bounds__(64, WCQP_IK4_WAVES)
void qp_pair_kernel(const IkDeviceParams* __restrict__ prm, int batch,
                    const double* __restrict__ JL, const double* __restrict__ JR,
                    const double* __restrict__ JN, const double* __restrict__ JC,
                    const double* qpos, const double* __restrict__ state,
                    double* __restrict__ dq_out, int* __restrict__ status_out,
                    unsigned* __restrict__ alo_out, unsigned* __restrict__ aup_out,
                    double* __restrict__ ferr_out, int* __restrict__ iters_out, int ik_blocks, MpcPairArgs m)
{
    __shared__ __attribute__((aligned(16))) double smem[4][PER_INST];
    // IK workgroups first: they are the long ones.  (Alternating the two kinds in dispatch order was measured: the MPC waves
    // then take slots from IK waves that have not started yet - 17.7 vs 14.5 us at 4096 robots, 158 vs 116 us at 65536.)
    const bool is_mpc = (int)blockIdx.x >= ik_blocks;
    const int blk = is_mpc ? (int)blockIdx.x - ik_blocks : xcd_group((int)blockIdx.x, ik_blocks);
    if (is_mpc) {
        static_assert(wcqp_mpc::kInstPerWave * WCQP_HULL_ROWS * 4 <= 4 * PER_INST, "the hull rows fit the IK's LDS");
        double (*s_hull)[WCQP_HULL_ROWS][4] = reinterpret_cast<double (*)[WCQP_HULL_ROWS][4]>(&smem[0][0]);
        const int lane = threadIdx.x;
        const int sub = lane / wcqp_mpc::kLanesPerInstance, t = lane % wcqp_mpc::kLanesPerInstance;
        const long inst_raw = (long)blk * wcqp_mpc::kInstPerWave + sub;
        const bool live = inst_raw < batch;
        const long inst = live ? inst_raw : (long)batch - 1;
        const double2* rp = reinterpret_cast<const double2*>(m.ref) + inst * m.ref_len;
        double ux, uy, margin;
        int st;
        unsigned mask;
        wcqp_mpc::mpc_row_solve(m.c, t, inst, m.x0, rp, m.ref_len, m.u_prev, m.hull_A, m.hull_b, m.hull_nc, inst, s_hull[sub], ux, uy, st, mask, margin);
        if (t == 0 && live) {
            reinterpret_cast<double2*>(m.u0)[inst] = make_double2(ux, uy);
            m.status[inst] = st;
            if (m.active) m.active[inst] = mask;
            if (m.margin) m.margin[inst] = margin;
        }
        return;
    }
    ik4_body<false>(prm, batch, JL, JR, JN, JC, qpos, state, dq_out, status_out, alo_out, aup_out, ferr_out, iters_out, wcqp_tick::TickDev{}, smem, blk);
}

// A PLAN of steps (wcqp_qp_plan_*): every record is one batch of robot-ticks - one DCM-MPC QP and one QP-IK per robot, as
// wcqp_qp_enqueue_steps would launch it - and ONE launch walks through all of them.  Consecutive records are independent
// batches, so nothing orders them: workgroup (way w, robot group g) solves robots 4g .. 4g+3 of records w, w + ways, ... on
// its own - no launch, ramp-up or tail per step, the MPC of a record in the shadow of its IK's Jacobian loads, and with
// `ways` workgroups per robot group the BASELINE batch (1024 robot groups) fills both wave slots of every SIMD.
template <bool WITH_MPC>
__device__ __forceinline__
void plan_walk(const IkDeviceParams* __restrict__ prm, int batch, const wcqp_qp_step* __restrict__ recs, int n_steps, int ways, int groups,
               const wcqp_mpc::MpcDeviceConsts& c, unsigned* queue, double (*smem)[PER_INST], double* ptab)
{
    constexpr int TAB = WITH_MPC ? WCQP_PLAN_LDS : (WCQP_PLAN_LDS & 2);
    // ways > 0: workgroup (way, robot group) walks through records way, way + ways, ... of its group.
    // ways = 0, work queues: unit u = (robot group u / n_steps, record u % n_steps), GROUP-major: the resident waves then work inside a
    // window of a few dozen robot groups (record-major at 65536 robots every unit of a wave lies 11 MB further on in each of the
    // twelve input arrays - a new page per array per record: 15 % slower than the fixed ways; group-major it is on a par).  kPlanQueues ticket counters,
    // kPlanQueueStride bytes apart (one counter serves ~8e7 tickets/s - measured: every wave behind ONE counter ran at half the
    // rate of the fixed ways, at every batch size - and the launch needs 1.5e8); ticket k of queue q is unit k kPlanQueues + q.
    // A wave draws from its home queue, asking for the next ticket behind the record's loads (ik4_body; the answer is needed at the
    // bottom: the atomic's round trip rides under the record's arithmetic), and goes round the other queues once its own has run out; it leaves
    // when all of them have.  queue[kPlanQueues * stride] counts the waves that are done: the last one zeroes everything.
    const bool dynamic = ways == 0;
    unsigned z = threadIdx.x;
    __asm__ volatile("" : "+v"(z));
    z >>= 6;          // an opaque per-lane zero in the ticket address: with a wave-uniform address hipcc's atomic optimizer rewrites the add into
                      // "count the lanes, one atomic, s_waitcnt vmcnt(0), redistribute" - a synchronous round trip at the top of every record
    constexpr unsigned QS = wcqp_ik::kPlanQueueStride / 4u;
    const unsigned total = (unsigned)n_steps * (unsigned)groups;
    unsigned home = blockIdx.x % wcqp_ik::kPlanQueues;
    // the next unit of any queue, starting at `home` (synchronous): total when every queue has run out
    auto draw = [&]() -> unsigned {
#ifndef WCQP_PLAN_STEAL
#define WCQP_PLAN_STEAL (wcqp_ik::kPlanQueues - 1u)
#endif
        // (every queue is the HOME of gridDim.x / kPlanQueues waves, which draw from it until it is empty: a queue is drained whether or
        // not anybody else visits it, so how many OTHER queues a wave tries before it leaves is a matter of balance, not of correctness)
        for (unsigned tried = 0; tried <= WCQP_PLAN_STEAL; ++tried) {
            unsigned k = 0;
            if (threadIdx.x == 0) k = __hip_atomic_fetch_add(queue + home * QS + z, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned u = (unsigned)__builtin_amdgcn_readfirstlane((int)k) * wcqp_ik::kPlanQueues + home;
            if (u < total) return u;
            home = (home + 1u) % wcqp_ik::kPlanQueues;
        }
        return total;
    };
    int r = (int)blockIdx.x / groups, blk = (int)blockIdx.x % groups;
#ifndef WCQP_PLAN_NO_XCD_MAP
    // XCD-aware (xcd_group above): XCD x walks the contiguous eighth x of the robot groups - its k-th workgroup is way k / n, group x n + k mod n.
    // PMC: the launch fetches 3 % fewer bytes (the 4 % by which its traffic exceeded its algorithmic bytes), +0.5 to +1.5 % QP/s
    // (profiles/r04_xcd_map_ab.txt).
    if ((groups & 7) == 0) {
        const int n = groups >> 3, x = (int)blockIdx.x & 7, k = (int)blockIdx.x >> 3;
        r = k / n; blk = x * n + k % n;
    }
#endif
    // the launch-invariant tables on their way to LDS (ik4_device.h: PlanTables): the loads here, in front of the first record's (and of the first ticket's round trip); that
    // record's body stores them behind its own loads.  (A wave without a record issues them for nothing: the registers are dead at once.)
    PlanTables pt;
    plan_tables_issue<TAB>(prm, c, WITH_MPC, ptab, pt);
    if (dynamic) {
        const unsigned u = draw();
        r = u < total ? (int)(u % (unsigned)n_steps) : n_steps; blk = u < total ? (int)(u / (unsigned)n_steps) : 0;
    }
#pragma unroll 1
    while (r < n_steps) {
        __asm__ volatile("" ::: "memory");        // nothing of the body is hoisted out of the loop
        // (the record's pointers come out of memory: as_global says what a kernel argument would have said - gptr.h)
        using wcqp::as_global;
        const wcqp_qp_step& s = recs[r];
        MpcPairArgs m{c, WITH_MPC ? as_global(s.x0) : nullptr, WITH_MPC ? as_global(s.ref) : nullptr, s.ref_len, WITH_MPC ? as_global(s.u_prev) : nullptr,
                      WITH_MPC ? as_global(s.hull_A) : nullptr, WITH_MPC ? as_global(s.hull_b) : nullptr, WITH_MPC ? as_global(s.hull_nc) : nullptr,
                      WITH_MPC ? as_global(s.u0) : nullptr, WITH_MPC ? as_global(s.mpc_status) : nullptr, WITH_MPC ? as_global(s.mpc_active) : nullptr,
                      WITH_MPC ? as_global(s.mpc_margin) : nullptr,
                      dynamic ? queue + home * QS + z : nullptr, 0u, WITH_MPC};
        ik4_body<false, 0, true, false, false, false, false, false, TAB>(prm, batch, as_global(s.J_left), as_global(s.J_right), as_global(s.J_neck), as_global(s.J_com), as_global(s.q), as_global(s.state),
                                 as_global(s.dq), as_global(s.ik_status), as_global(s.active_lower), as_global(s.active_upper),
                                 as_global(s.foot_err), as_global(s.iters), wcqp_tick::TickDev{}, smem, blk, 0, true, nullptr, nullptr, &m, nullptr, nullptr, nullptr, &pt);
        wcqp::wave_lds_fence();
        // (the fill's registers are the first record's only: carried round the loop as zeros they are dead from here on)
        pt.fill = false; pt.f_ik[0] = pt.f_ik[1] = pt.f_ik[2] = 0.0; pt.f_gr[0] = pt.f_gr[1] = make_double2(0.0, 0.0);
        if (dynamic) {
            unsigned u = (unsigned)__builtin_amdgcn_readfirstlane((int)m.ticket) * wcqp_ik::kPlanQueues + home;
            if (u >= total) { home = (home + 1u) % wcqp_ik::kPlanQueues; u = draw(); }
            r = u < total ? (int)(u % (unsigned)n_steps) : n_steps; blk = u < total ? (int)(u / (unsigned)n_steps) : 0;
        } else {
            r += ways;
        }
    }
    if (dynamic && threadIdx.x == 0) {
        __threadfence();
        if (atomicAdd(queue + wcqp_ik::kPlanQueues * QS, 1u) == gridDim.x - 1) {
            for (unsigned q = 0; q <= wcqp_ik::kPlanQueues; ++q) queue[q * QS] = 0u;
        }
    }
}

__global__ __launch_bounds__(64, WCQP_IK4_WAVES)
void qp_plan_kernel(const IkDeviceParams* __restrict__ prm, int batch, const wcqp_qp_step* __restrict__ recs, int n_steps, int ways, int groups,
                    wcqp_mpc::MpcDeviceConsts c, unsigned* queue)
{
    __shared__ __attribute__((aligned(16))) double smem[4][PER_INST];
    __shared__ __attribute__((aligned(16))) double ptab[PT_SIZE];
    plan_walk<true>(prm, batch, recs, n_steps, ways, groups, c, queue, smem, ptab);
}
// an IK-only plan (no record has an MPC part: BASELINE config 3 on its own): the same walk without the MPC share, under a name of its
// own so that profiles of the two do not mix
__global__ __launch_bounds__(64, WCQP_IK4_WAVES) WCQP_IK_PLAN_REGS
void ik_plan_kernel(const IkDeviceParams* __restrict__ prm, int batch, const wcqp_qp_step* __restrict__ recs, int n_steps, int ways, int groups,
                    wcqp_mpc::MpcDeviceConsts c, unsigned* queue)
{
    __shared__ __attribute__((aligned(16))) double smem[4][PER_INST];
    __shared__ __attribute__((aligned(16))) double ptab[PT_GR];          // (no MPC part: the IK's tables alone)
    plan_walk<false>(prm, batch, recs, n_steps, ways, groups, c, queue, smem, ptab);
}

}  // namespace

namespace wcqp_ik {

int ik4_plan_queue_grid(int batch, int n_steps) {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) return -1;
    const long long total = (long long)((batch + 3) / 4) * n_steps, slots = (long long)cus * 4 * WCQP_IK4_WAVES;   // waves that are resident at once
    return (int)(total < slots ? total : slots);
}

int ik4_launch_plan(const IkDeviceParams* d_prm, int batch, const wcqp_qp_step* d_recs, int n_steps, int ways,
                    const wcqp_mpc::MpcDeviceConsts& c, hipStream_t stream, unsigned* d_queue, int queue_grid, bool ik_only) {
    if (!d_prm || !d_recs || batch < 1 || n_steps < 1 || ways < 0 || (ways == 0 && (!d_queue || queue_grid < 1))) return WCQP_E_INVALID;
    const int groups = (batch + 3) / 4;
    if ((long long)groups * n_steps >= (1ll << 31)) return WCQP_E_INVALID;
    const unsigned grid = ways == 0 ? (unsigned)queue_grid : (unsigned)(groups * ways);
    if (ik_only) hipLaunchKernelGGL(ik_plan_kernel, dim3(grid), dim3(64), 0, stream, d_prm, batch, d_recs, n_steps, ways, groups, c, d_queue);
    else hipLaunchKernelGGL(qp_plan_kernel, dim3(grid), dim3(64), 0, stream, d_prm, batch, d_recs, n_steps, ways, groups, c, d_queue);
    WCQP_HIP_TRY(hipGetLastError());
    return WCQP_OK;
}

int ik4_launch_pair(const IkDeviceParams* d_prm, int batch, const IkIo& io,
                    const wcqp_mpc::MpcDeviceConsts& c, const double* x0, const double* ref, int ref_len, const double* u_prev,
                    const double* hull_A, const double* hull_b, const int* hull_nc,
                    double* u0, int* mstatus, unsigned* mactive, double* mmargin, hipStream_t stream) {
    const int ik_blocks = (batch + 3) / 4;
    const int mpc_blocks = (batch + wcqp_mpc::kInstPerWave - 1) / wcqp_mpc::kInstPerWave;
    MpcPairArgs m{c, x0, ref, ref_len, u_prev, hull_A, hull_b, hull_nc, u0, mstatus, mactive, mmargin};
    hipLaunchKernelGGL(qp_pair_kernel, dim3((unsigned)(ik_blocks + mpc_blocks)), dim3(64), 0, stream, d_prm, batch,
                       io.JL, io.JR, io.JN, io.JC, io.q, io.state, io.dq, io.status, io.alo, io.aup, io.ferr, io.iters, ik_blocks, m);
    WCQP_HIP_TRY(hipGetLastError());
    return WCQP_OK;
}

// one launch of ik4_kernel: the stand-alone solve (td_dev = NULL) or a tick form
template <bool TICK, int JSRC, bool LOG = false, bool EXT = false>
static void ik4_launch_as(const IkDeviceParams* prm, int batch, const IkIo& io, const wcqp_tick::TickDev* td_dev, int phase,
                          int n_inner, int skip_last_mpc, hipStream_t stream) {
    hipLaunchKernelGGL((ik4_kernel<TICK, JSRC, LOG, EXT>), dim3((unsigned)((batch + 3) / 4)), dim3(64), 0, stream, prm, batch,
                       io.JL, io.JR, io.JN, io.JC, io.q, io.state, io.dq, io.status, io.alo, io.aup, io.ferr, io.iters,
                       td_dev, phase, n_inner, skip_last_mpc);
}

int ik4_launch(const IkDeviceParams* d_prm, int batch, const IkIo& io, hipStream_t stream) {
    ik4_launch_as<false, 0>(d_prm, batch, io, nullptr, 0, 1, 0, stream);
    WCQP_HIP_TRY(hipGetLastError());
    return WCQP_OK;
}

// The one check of a skewed handle's record against its variant: both launchers below run it, and the variant kernels of ik4_tick.hip are
// launched only through them
static int tick_check(const wcqp_tick::TickDevPL& td, const TickVariant& v) {
    if (!td.skew || !td.mst || !td.hand || !td.live_A || !td.live_b || !td.live_nc || !td.sel_built) return WCQP_E_INVALID;
    if (v.jsrc == 1 && (!td.jcomp || td.cstride < 1)) return WCQP_E_INVALID;
    // (the MPC's gain blocks sit in LDS beside the model: a horizon limit the reactive controller, which reads no gains, does not have)
    if (v.jsrc == 2 && (!td.kin_tab || !td.kin_mode || td.kin_rounds < 0 || td.kin_rounds > 3 || (!v.react && td.horizon >= wcqp_tick::kGainsLdsStages)))
        return WCQP_E_INVALID;
    if (v.log && !td.log_rows) return WCQP_E_INVALID;
    if (v.ext && v.jsrc == 1) return WCQP_E_INVALID;          // external feedback: dense Jacobians or fused kinematics
    if ((v.react || v.gs) && !td.dcm_vel) return WCQP_E_INVALID;
    if (v.gs && !td.zg.zs) return WCQP_E_INVALID;
    // planned trajectories (the internal plant) and streamed ones (EXTERNAL): fused kinematics, no logger rows
    if (v.pl && (!td.pl.rec || v.jsrc != 2 || v.log)) return WCQP_E_INVALID;
    return WCQP_OK;
}

int ik4_launch_tick(const void* d_prm, const wcqp_tick::TickDevPL& td, const wcqp_tick::TickDev* td_dev, const TickVariant& v, const IkIo& io,
                    int n_inner, int skip_last_mpc, hipStream_t stream) {
    // (whether a handle may run several ticks per launch is decided at wcqp_tick_create; external feedback: one tick per launch)
    if (!d_prm || !td_dev || n_inner < 1 || (v.ext && n_inner != 1)) return WCQP_E_INVALID;
    if (const int rc = tick_check(td, v)) return rc;
    const IkDeviceParams* prm = static_cast<const IkDeviceParams*>(d_prm);
    if (!v.plain()) ik4_launch_tick_variant(prm, td, td_dev, v, io, n_inner, skip_last_mpc, stream);
    else tick_variant_visit(v, [&](auto j, auto l, auto e, auto r, auto g, auto p) {
        if constexpr (!(r || g || p)) ik4_launch_as<true, j, l, e>(prm, td.batch, io, td_dev, td.phase, n_inner, skip_last_mpc, stream);
    });
    WCQP_HIP_TRY(hipGetLastError());
    return WCQP_OK;
}

int ik4_launch_tick_prime(const wcqp_tick::TickDevPL& td, const TickVariant& v, int t, hipStream_t stream) {
    if (const int rc = tick_check(td, v)) return rc;
    const dim3 grid((unsigned)((td.batch + 3) / 4));
    const wcqp_tick::TickDev& base = td;
    // (the plain form's one flag, EXT - the caller's measured ZMP - is mapped here and not through tick_variant_visit: that would name the
    // two MPC prime kernels in the other order, and so move them in this code object)
    if (!v.plain()) ik4_launch_tick_prime_variant(td, v, t, stream);
    else if (v.ext) hipLaunchKernelGGL(tick_mpc_prime_kernel<true>, grid, dim3(64), 0, stream, base, t);
    else hipLaunchKernelGGL(tick_mpc_prime_kernel<false>, grid, dim3(64), 0, stream, base, t);
    WCQP_HIP_TRY(hipGetLastError());
    return WCQP_OK;
}

}  // namespace wcqp_ik
