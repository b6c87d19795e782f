// Jacobian QP-IK, third kernel: the null-space formulation of ik2.hip on 16 lanes per instance
// (four instances per wave64, one DPP row each).
//
// Same QP, inputs, outputs and reference citations as ik.hip / ik2.hip.  Why another layout:
// s_memtime stamps and latency micro-benchmarks (tools/ubench/lat.hip) showed that the kernel is
// a chain of ~45 serial cross-lane steps (arg-max ~110 cycles, crossbar / LDS round trip ~75,
// v_readlane -> use ~40) in which a dependent fp64 FMA costs 4 cycles: the steps cost the same
// whether they serve 2 instances per wave or 4, and the FMAs between them are almost free.  So
//   * lane j of an instance's 16 owns TWO columns of [A | b]: j and j + 16 (column 29 = b);
//   * an instance is one DPP row: every reduction is 4 DPP steps, no row exchange;
//   * the reduced Hessian row k lives on lane k (k = compact index), not on the variable's lane;
//   * the Gram product is one fp64 MFMA tile per instance, X' = D_B F formed on the fly.
//   * bounds: Goldfarb-Idnani dual active set; first bound straight-line, working sets of up to 4 bounds
//     replicated in registers, larger ones slot-per-lane (see phase 5).
// LDS is 632 doubles per instance (20.2 KB per block: 8 blocks per CU); the default IK kernel of the library.
// Template parameter TICK: the tick pipeline's glue / post steps fused in (tick_device.h).
#include <cmath>
#include <limits>
#include "ik_common.h"
#include "tick_device.h"

namespace {

using namespace wcqp_ik;

typedef double v4d __attribute__((ext_vector_type(4)));

constexpr int MEQ = 15;               // equality rows (CoM as constraint)
constexpr int NCOST = 3;              // cost rows: J_neck
constexpr int NN = kNV - MEQ;         // 14 free variables
constexpr int KMAX = NN;
constexpr int LDR = KMAX | 1;         // 15: odd, row-per-lane b64 accesses spread over the banks
constexpr int LDH = 18;

// ---- LDS layout per instance (doubles) ---------------------------------------------------------
// Leading dimensions of 18 doubles make the row-per-lane b128 reads (lane j reads row j) conflict
// free: 36 j mod 64 are 16 distinct multiples of 4 banks.  PER_INST = 24 mod 32 doubles puts the
// four instances of a wave 16 banks apart, so a broadcast read that serves two instances in one
// lane group does not collide either (at a multiple of 32 doubles every such read was 2-way).
constexpr int LDF = 18;
constexpr int OFF_F = 0;              // [15][LDF]  F[r][k] = (A_B^-1 A_N)[r][k], column NN = b'
constexpr int OFF_P = 15 * LDF;       // 270
//   set-up
constexpr int OFF_ST = OFF_P;         // [112] state + q (dead after the gradient)
constexpr int OFF_CB = OFF_P + 112;   // [4][16] entries of a panel's 4 pivot columns; before that the task rhs b
constexpr int OFF_RD = OFF_P + 176;   // [16][8] per row r: {g, 3 neck-row entries, D} of its basic variable
constexpr int OFF_GRV = OFF_P + 304;  // [16] reduced gradient by compact index
constexpr int OFF_DN = OFF_P + 320;   // [16] Lambda entry of the free variable with compact index k
constexpr int OFF_YTT = OFF_P;        // [5][16] rows 15..19 of Y^T: (W N Z)' and zero padding  (over ST)
constexpr int OFF_XTT = OFF_P + 80;   // [5][16] rows 15..19 of X^T: (N Z)' and zero padding    (over ST/CB)
constexpr int OFF_HM = OFF_P;         // [16][LDH] Gram tile (over everything up to RD, all dead by then)
constexpr int OFF_COL = OFF_P;        // [2][16] sweep columns (over the tile once its rows are in registers)
constexpr int OFF_XNV = OFF_P + 32;   // [16] x_N by compact index
constexpr int OFF_XBV = OFF_P + 48;   // [16] x_B by row
//   active set (over the set-up area)
constexpr int OFF_RINV = OFF_P;       // [KMAX][LDR]
constexpr int OFF_TPB = OFF_P + 212;  // [32] column tau_p by variable
constexpr int OFF_ZB = OFF_P + 244;   // [32] primal step by variable
constexpr int OFF_RV = OFF_P + 276;   // [16] dual step per slot
constexpr int OFF_CV = OFF_P + 292;   // [16]
constexpr int OFF_TKB = OFF_P + 308;  // [16] t by compact index
constexpr int OFF_TBV = OFF_P + 324;  // [16] -F t by row
constexpr int OFF_WI = OFF_P + 340;   // [16] ints: variable of slot a
constexpr int P_SIZE = 352;
constexpr int PER_INST = 632;         // >= OFF_P + P_SIZE = 622, = 24 mod 32
static_assert(OFF_WI + 8 <= OFF_P + P_SIZE && OFF_DN + 16 <= OFF_P + P_SIZE && OFF_HM + 16 * LDH <= OFF_GRV && OFF_P + P_SIZE <= PER_INST, "LDS overlays");
static_assert(PER_INST % 32 == 24 || PER_INST % 32 == 8, "instances 16 banks apart");
static_assert(PER_INST * 8 * 4 * 8 <= 160 * 1024, "8 blocks per CU");

#ifdef WCQP_IK_STAMPS
#define WCQP_STAMP(k) do { unsigned long long t__; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t__) :: "memory"); \
                           if (lane == __ffsll((long long)__ballot(true)) - 1) reinterpret_cast<unsigned long long*>(ferr_out)[(size_t)blockIdx.x * 16 + (k)] = t__; } while (0)
#else
#define WCQP_STAMP(k) do { } while (0)
#endif

// TICK: the receding-horizon pipeline's glue (ZMP-CoM law, plant; tick_device.h) runs in the prologue
// and its post step (joint integration, next contact pair, tick counter) in the epilogue, so that a
// tick is two launches (MPC, this) instead of four.  The body is ik3_kernel_body.inc (shared with ik3_tick_gs_kernel).
#ifndef WCQP_IK3_WAVES
#define WCQP_IK3_WAVES 2
#endif
// LIST: solves only the instances whose status reads WCQP_STATUS_STRUCTURE (what ik4.hip leaves behind for Jacobians
// whose base blocks are not in MIXED form): a workgroup scans 64 status words, compacts the flagged ones into LDS and
// loops over them four at a time; without any, the launch is batch / 64 workgroups that load one word and exit.
template <bool TICK, bool LIST>
__global__ __launch_bounds__(64, WCQP_IK3_WAVES)
void ik3_kernel(const IkDeviceParams* __restrict__ prm, int batch,
                const double* __restrict__ JL, const double* __restrict__ JR,
                const double* __restrict__ JN, const double* __restrict__ JC,
                const double* qpos, const double* __restrict__ state,
                double* __restrict__ dq_out, int* __restrict__ status_out,
                unsigned* __restrict__ alo_out, unsigned* __restrict__ aup_out,
                double* __restrict__ ferr_out, int* __restrict__ iters_out,
                wcqp_tick::TickDev td)
{
    __shared__ __attribute__((aligned(16))) double smem[4][PER_INST];
    __shared__ int s_list[64];
    constexpr bool GS = false;
#include "ik3_kernel_body.inc"
}

// the tick kernel (ik3_kernel<true, false>) with ZMP-CoM gain scheduling (wcqp_tick_params.zmp_gain_scheduling)
template <bool TICK, bool LIST, bool GS>
__global__ __launch_bounds__(64, WCQP_IK3_WAVES)
void ik3_tick_gs_kernel(const IkDeviceParams* __restrict__ prm, int batch,
                        const double* __restrict__ JL, const double* __restrict__ JR,
                        const double* __restrict__ JN, const double* __restrict__ JC,
                        const double* qpos, const double* __restrict__ state,
                        double* __restrict__ dq_out, int* __restrict__ status_out,
                        unsigned* __restrict__ alo_out, unsigned* __restrict__ aup_out,
                        double* __restrict__ ferr_out, int* __restrict__ iters_out,
                        wcqp_tick::TickDevGS td)
{
    static_assert(TICK && !LIST && GS, "the scheduled form of the tick kernel");
    __shared__ __attribute__((aligned(16))) double smem[4][PER_INST];
    __shared__ int s_list[64];
#include "ik3_kernel_body.inc"
}

}  // namespace

namespace wcqp_ik {

template <bool TICK, bool LIST>
static int ik3_launch_as(unsigned grid, const IkDeviceParams* d_prm, int batch, const IkIo& io, const wcqp_tick::TickDev& td, hipStream_t stream) {
    hipLaunchKernelGGL((ik3_kernel<TICK, LIST>), dim3(grid), dim3(64), 0, stream, d_prm, batch,
                       io.JL, io.JR, io.JN, io.JC, io.q, io.state, io.dq, io.status, io.alo, io.aup, io.ferr, io.iters, td);
    WCQP_HIP_TRY(hipGetLastError());
    return WCQP_OK;
}

int ik3_launch(const IkDeviceParams* d_prm, int batch, const IkIo& io, hipStream_t stream) {
    return ik3_launch_as<false, false>((unsigned)((batch + 3) / 4), d_prm, batch, io, wcqp_tick::TickDev{}, stream);
}

int ik3_launch_list(const IkDeviceParams* d_prm, int batch, const IkIo& io, hipStream_t stream) {
    return ik3_launch_as<false, true>((unsigned)((batch + 63) / 64), d_prm, batch, io, wcqp_tick::TickDev{}, stream);
}

// the tick form: ik3_kernel<true, false>, or with gain scheduling ik3_tick_gs_kernel
int ik3_launch_tick(const void* d_prm, const wcqp_tick::TickDevGS& td, const IkIo& io, hipStream_t stream) {
    if (!d_prm) return WCQP_E_INVALID;
    const IkDeviceParams* prm = static_cast<const IkDeviceParams*>(d_prm);
    if (!td.gain_sched) return ik3_launch_as<true, false>((unsigned)((td.batch + 3) / 4), prm, td.batch, io, td, stream);
    if (!td.dcm_vel || !td.zg.zs) return WCQP_E_INVALID;
    hipLaunchKernelGGL((ik3_tick_gs_kernel<true, false, true>), dim3((unsigned)((td.batch + 3) / 4)), dim3(64), 0, stream,
                       prm, td.batch, io.JL, io.JR, io.JN, io.JC, io.q, io.state, io.dq, io.status, io.alo, io.aup, io.ferr, io.iters, td);
    WCQP_HIP_TRY(hipGetLastError());
    return WCQP_OK;
}

}  // namespace wcqp_ik
