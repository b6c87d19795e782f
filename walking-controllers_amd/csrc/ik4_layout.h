// The base-eliminated QP-IK kernel (ik4_device.h: the algorithm): its sizes, the map of an instance's LDS block, the build knobs, the
// diagnostic stamps and the two cross-row swaps of the Gram tile - what the device code (ik4_device.h) and the kernels (ik4.hip,
// ik4_tick.hip) read, and what a kernel that reuses parts of this one will.
#pragma once
#include "ik_common.h"

namespace {

using namespace wcqp_ik;

typedef double v4d __attribute__((ext_vector_type(4)));

constexpr int NR = 12;                // rows of C = [Nt (3); A_right (6); A_com (3)]
constexpr int NROWS_IN = 18;          // J_left 6, J_right 6, J_com 3, J_neck 3
constexpr int KMAX = kDof - 9;        // 14: largest working set (n - m_eq)
constexpr int LDC = 14;               // leading dimension of C^T (k-major) and of the Gram tile: b128 row accesses of 16
                                      // lanes land on 16 distinct groups of 4 banks (28 j mod 64)

// ---- LDS layout per instance (doubles) ---------------------------------------------------------
// region A, three lives:
//   set-up
constexpr int OFF_ST = 0;             // [112] state + q
constexpr int OFF_BV = 112;           // [18]  task rhs b (15) and neck target e (3)
constexpr int OFF_DB = 130;           // [18]  B_R - B_L, B_C - B_L (row-major 3x3 each)
//   Gram .. end
constexpr int OFF_CT = 0;             // [24][LDC] (+2): C^T k-major, row 12 = g~, row 13 = 0; k = 23: zero column
constexpr int OFF_PB = 0;             // [12][18] foot-error partial products (epilogue)
constexpr int A_SIZE = 340;
// region B
constexpr int OFF_COL = A_SIZE;       // [2][16] sweep columns
constexpr int OFF_YV = A_SIZE + 32;   // [16] y
constexpr int OFF_DV = A_SIZE + 48;   // [16] d = [t; b'] by row
//   active set (region B is dead after x~)
constexpr int OFF_YPV = A_SIZE;       // [16] M^-1 C v
constexpr int OFF_RV = A_SIZE + 16;   // [16] dual step per slot      (working sets of more than KS bounds)
constexpr int OFF_CV = A_SIZE + 32;   // [16]
constexpr int OFF_ROWB = A_SIZE + 48; // [16] row of the leaving slot
//   variable of slot a (working sets of more than KS bounds): an int in entry 13 of row a of C^T (the zero row of the Gram
//   tile, dead once the MFMAs have read it)
constexpr int PER_INST = 440;         // = 24 mod 32: the four instances of a wave sit 16 banks apart; 14080 B per workgroup (408 would do for the
                                      // solve; the fused kinematics' joint frames want the rest: K_* below)
// ---- fused kinematics (JSRC = 2): scratch of the kinematics phase, over the same region (everything of it is dead before the pose block
// and C^T are written).  Joint frames [23][K_FS]: 12 doubles at a stride of 14 - the b128 accesses of 16 lanes then land on 8 distinct
// groups of 4 banks (2 passes, the minimum for a b128) instead of 4 groups (4 passes) at a stride of 12: PMC showed 24 % of the tick
// kernel's LDS-active cycles as bank conflicts.  The two spare doubles behind frames 16..21 hold the anchor pose (k_sd).
constexpr int K_FS = 14, K_TW = 0, K_FRB = 322, K_FR = 358;          // joint frames, attached frames in base / world coordinates [3][12] each
constexpr int K_MS = 394, K_MH = 410;                               // stashes: the MPC chain's per-axis records [2][8], its hull rows [8][3]
constexpr int K_PF = 434;                                           // stash: the planner's contact flags of tick t + 1 (planned trajectories)
__host__ __device__ constexpr int k_sd(int m) { return K_TW + (16 + (m >> 1)) * K_FS + 12 + (m & 1); }      // anchor pose [12] / CoM [3]
static_assert(K_MH + 24 <= K_PF && K_PF < PER_INST, "the flags stash is clear of the others");
static_assert(kDof * K_FS <= K_FRB && K_FR + 36 <= K_MS && K_MH + 24 <= PER_INST && k_sd(11) < kDof * K_FS && k_sd(0) >= 32 * 4, "kinematics scratch fits; the prefix sums [32][4] stay clear of the anchor pose");
static_assert(OFF_CT + 24 * LDC + 2 <= A_SIZE && OFF_DB + 18 <= A_SIZE && OFF_PB + 12 * 18 <= A_SIZE, "LDS overlays");
static_assert(OFF_ROWB + 16 <= PER_INST && OFF_DV + 16 <= PER_INST && (PER_INST % 32 == 24 || PER_INST % 32 == 8), "instances 16 banks apart");
static_assert(KMAX <= 24, "one slot index per C^T row");
static_assert(PER_INST * 8 * 4 * 11 <= 160 * 1024, "11 blocks per CU");

#ifndef WCQP_IK4_WAVES
#define WCQP_IK4_WAVES 2
#endif
// Register cap of ik_plan_kernel (the IK-only plan).  gfx90a and later have ONE register file of 512 entries per SIMD lane for VGPRs and
// AGPRs together, allocated in blocks of 8, and hipcc's amdgpu_num_vgpr counts HALF of it: amdgpu_num_vgpr(108) caps the kernel at 216
// VGPRs.  Two waves of 216 leave 80 registers of a SIMD free - room for ONE wave of mpc_plan_kernel (72) beside them.
#ifdef WCQP_IK_PLAN_VGPR_HALF
#define WCQP_IK_PLAN_REGS __attribute__((amdgpu_num_vgpr(WCQP_IK_PLAN_VGPR_HALF)))
#else
#define WCQP_IK_PLAN_REGS
#endif
#ifndef WCQP_IK4_KS
#define WCQP_IK4_KS 4                 // bounds kept replicated in registers (more: the slot-per-lane loop)
#endif

// Diagnostic stamps: s_memtime at the phase boundaries of ik4_body.  A stamp reads lane, td, blk, ferr_out and TICK of the scope it stands in.
#define WCQP_STAMP_CLOCK(t__) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t__) :: "memory")
// the TICK kernels' stamps: per workgroup, the last tick of a launch wins (TickDev::stamps; tools/stamps_tick.py)
#define WCQP_STAMP_AT(k) do { if constexpr (TICK) { unsigned long long t__; WCQP_STAMP_CLOCK(t__); \
                                   if (lane == 0 && td.stamps) td.stamps[(size_t)blk * 16 + (k)] = t__; } } while (0)
#if defined(WCQP_TICK_KSTAMPS)
// diagnostic build (tools/build_variant.sh kstamps -DWCQP_TICK_KSTAMPS -DWCQP_TICK_STAMPS): the KINEMATICS phase of the fused tick in detail - stamps 0, 12 and 14 as
// below, slots 1..9 are its sub-phases (WCQP_KSTAMP); WCQP_KSTAMPS=1 tools/stamps_tick.py
#define WCQP_STAMP(k) do { if constexpr ((k) == 0 || (k) == 12 || (k) == 14) WCQP_STAMP_AT(k); } while (0)
#define WCQP_KSTAMP(k) WCQP_STAMP_AT(k)
#elif defined(WCQP_TICK_STAMPS)
// diagnostic build (tools/build_variant.sh tstamps -DWCQP_TICK_STAMPS): the phase boundaries of the TICK kernel's body
#define WCQP_STAMP(k) WCQP_STAMP_AT(k)
#elif defined(WCQP_IK_STAMPS)
#define WCQP_STAMP(k) do { unsigned long long t__; WCQP_STAMP_CLOCK(t__); \
                           if (lane == __ffsll((long long)__ballot(true)) - 1) reinterpret_cast<unsigned long long*>(ferr_out)[(size_t)blockIdx.x * 16 + (k)] = t__; } while (0)
#else
#define WCQP_STAMP(k) do { } while (0)
#endif
#ifndef WCQP_KSTAMP
#define WCQP_KSTAMP(k) do { } while (0)
#endif

// (a, b) -> (rows {a0, a1, b0, b1}, rows {a2, a3, b2, b3}) of the four 16-lane rows (checked on the GPU:
// tools/ubench/permlane_test.hip)
__device__ __forceinline__ void swap32(double& a, double& b) {
    const auto l = __builtin_amdgcn_permlane32_swap((unsigned)__double2loint(a), (unsigned)__double2loint(b), false, false);
    const auto h = __builtin_amdgcn_permlane32_swap((unsigned)__double2hiint(a), (unsigned)__double2hiint(b), false, false);
    a = __hiloint2double((int)h[0], (int)l[0]); b = __hiloint2double((int)h[1], (int)l[1]);
}
// (a, b) -> (rows {a0, b0, a2, b2}, rows {a1, b1, a3, b3})
__device__ __forceinline__ void swap16(double& a, double& b) {
    const auto l = __builtin_amdgcn_permlane16_swap((unsigned)__double2loint(a), (unsigned)__double2loint(b), false, false);
    const auto h = __builtin_amdgcn_permlane16_swap((unsigned)__double2hiint(a), (unsigned)__double2hiint(b), false, false);
    a = __hiloint2double((int)h[0], (int)l[0]); b = __hiloint2double((int)h[1], (int)l[1]);
}

}  // namespace
