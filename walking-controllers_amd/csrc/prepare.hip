// Batched non-linear inverse kinematics (include/wcqp.h: wcqp_prepare_*, which states the problem and the iteration): the posture a walk
// starts from - the reference's WalkingModule::prepareRobot through WalkingIK::computeIK (citations relative to
// /root/reference/modules/Walking_module):
//   src/WalkingModule.cpp:880-1005               prepareRobot: the targets (left sole = the fixed base, right sole, CoM), the neck rule :944-984
//   src/WalkingInverseKinematics.cpp:239-305     setFullModelFeetConstraint / prepareIK: constraints, costs, limits
//   src/WalkingInverseKinematics.cpp:346-424     computeIK
// One launch runs ALL Gauss-Newton iterations: 16 lanes per robot, four robots per wave, one wave per workgroup, as sensors.hip - the
// kinematics are the walk of kin_device.h (walk_*) on this kernel's LDS map with three attached frames.  New here: the Jacobian columns
// of the right sole, the neck and the CoM reduced to the joints by the anchored left sole (its base block [I -S; 0 I] is inverted in
// closed form, as ik4 eliminates the base: the column of a left-leg joint c becomes -[a_c x (p_f - p_c); a_c] in every other frame and
// -a_c x (com - p_c) joins its CoM column), the log map, and the 23-variable QP with nine equality rows and a box, solved in range
// space: H = w_q I + w_n N'N is inverted by the 3 x 3 Woodbury identity, the rows of the equalities and of the active bounds meet in a
// Schur complement of at most 23 rows that is Cholesky-factored in LDS, and an active-set walk adds the most violated bound or drops the
// bound whose multiplier has the wrong sign until neither exists (the QP is strictly convex: the optimum does not depend on the walk).
// A wave loops until its four robots have stopped; a stopped robot takes one more pass of the kinematics - at its final joints, or at
// the clipped guess - to write its outputs, and stores nothing afterwards.  Plain vector loads and stores only.
#include <cmath>
#include <cstring>
#include <new>
#include <vector>
#include "wcqp_internal.h"
#include "kin_device.h"

namespace {

using namespace wcqp_kin;
constexpr int kDof = kWalkDof;
constexpr int kStateLen = WCQP_IK_STATE_LEN;
constexpr int kMaxActive = kDof - 9;          // bounds that can be active next to nine independent equality rows
constexpr int kMaxChanges = 96;               // active-set changes per QP
constexpr double kBoundTol = 1e-13;           // a bound is violated / a multiplier has the wrong sign beyond this

// LDS per robot (doubles).  X: the joint frames [23][P_FS] while the tree is walked, then the prefix sums [32][4] (and, for the output
// pass, the link moments [23][4] behind them), then - the kinematics done - the Schur complement [24][24] of the QP.
constexpr int P_FS = 14, P_SS = 24;
constexpr int P_X = 0, P_E4 = 128, P_FRB = 576, P_FR = 612, P_TG = 648, P_N = 688, P_A = 760, P_G = 976, P_M = 1216, P_KT = 1306, P_T1 = 1336,
              P_K = 1366, P_GR = 1376, P_LO = 1400, P_HI = 1424, P_DQ = 1448, P_LAM = 1472, P_C = 1496, P_WI = 1508, P_WB = 1516, P_WS = 1532,
              P_BASE = 1548, P_PER = 1560;
constexpr int TG_RIGHT = 12, TG_COM = 24, TG_NECK = 28;
static_assert(kDof * P_FS <= P_FRB && P_E4 + kDof * 4 <= P_FRB && P_SS * P_SS <= P_FRB && P_BASE + 12 <= P_PER, "prepare kernel LDS layout");

struct PrepDev {
    const double* kin_tab; int kin_rounds; unsigned pm[3];
    int batch;
    const double *left_d, *right_d, *com_d, *Rd_neck, *q_guess;
    double *q, *base, *state, *residual;
    int *status, *iters;
    const double* par;                         // q_reg [23] | q_min [23] | q_max [23]
    double w_q, w_n, step_cap, tol_step, tol_c;
    int max_iter, use_limits;
};

// rotation vector of Ra Rd': v = (the antisymmetric part's axial vector) = sin(theta) axis, theta = atan2(|v|, (trace - 1) / 2);
// theta / sin(theta) by its series in s = |v| near zero (rotations by nearly pi are outside what a posture target asks for)
__device__ __forceinline__ void log_rot(const double* Ra, const double* Rd, double* phi) {
    double R[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) R[3 * r + c] = Ra[3 * r] * Rd[3 * c] + Ra[3 * r + 1] * Rd[3 * c + 1] + Ra[3 * r + 2] * Rd[3 * c + 2];
    const double v[3] = {0.5 * (R[7] - R[5]), 0.5 * (R[2] - R[6]), 0.5 * (R[3] - R[1])};
    const double s2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
    const double cth = 0.5 * (R[0] + R[4] + R[8] - 1.0);
    double f;
    if (s2 < 1e-8 && cth > 0.0) {
        f = 1.0 + s2 * (1.0 / 6.0 + s2 * (3.0 / 40.0));
    } else {
        const double s = sqrt(s2);
        f = atan2(s, cth) / s;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) phi[k] = f * v[k];
}

// walk_local_frames of kin_device.h with every fused multiply-add of R0 Rot(axis, q) spelled out.  Left to the compiler (contraction is
// on), the second slot's product came out with the two first terms of its middle column fused the other way round than in the first
// slot and in the stand-alone kinematics kernel - a last-place difference in four entries of the right sole's rotation.  The order
// here is the one that kernel's code has, element (r, c) = fma(A[r][2], B[2][c], fma(A[r][0], B[0][c], A[r][1] B[1][c])), so that the pose
// block this kernel writes is wcqp_kin_jacobians_* at (base, q) bit for bit.
__device__ __forceinline__ void local_frames_pinned(const double* kmodel, const int (&cs)[2], double q0, double q1, double (&Ra)[2][9], double (&pa)[2][3]) {
#pragma unroll
    for (int s_ = 0; s_ < 2; ++s_) {
        const double* mt = kmodel + cs[s_] * kKinTabJoint;
        double R0[9], ax[3];
#pragma unroll
        for (int k = 0; k < 9; ++k) R0[k] = mt[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) { pa[s_][k] = mt[9 + k]; ax[k] = mt[12 + k]; }
        double sn, cs_;
        joint_sincos(s_ == 0 ? q0 : q1, sn, cs_);
        const double v = 1.0 - cs_;
        const double s0 = sn * ax[0], s1 = sn * ax[1], s2 = sn * ax[2], m0 = v * ax[0], m1 = v * ax[1], m2 = v * ax[2];
        const double Rq[9] = {__builtin_fma(ax[0], m0, cs_), __builtin_fma(m0, ax[1], -s2), __builtin_fma(m0, ax[2], s1),
                              __builtin_fma(ax[0], m1, s2),  __builtin_fma(ax[1], m1, cs_), __builtin_fma(m1, ax[2], -s0),
                              __builtin_fma(ax[0], m2, -s1), __builtin_fma(ax[1], m2, s0),  __builtin_fma(ax[2], m2, cs_)};
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c)
                Ra[s_][3 * r + c] = __builtin_fma(R0[3 * r + 2], Rq[6 + c], __builtin_fma(R0[3 * r], Rq[c], R0[3 * r + 1] * Rq[3 + c]));
    }
}

__global__ __launch_bounds__(64) void prepare_kernel(PrepDev a) {
    __shared__ __attribute__((aligned(16))) double kmodel[kKinTabSize];
    __shared__ __attribute__((aligned(16))) double smem[4][P_PER];
    const int lane = threadIdx.x, grp = lane >> 4, j = lane & 15;
    for (int k = lane; k < kKinTabSize; k += 64) kmodel[k] = a.kin_tab[k];
    const long inst_raw = (long)blockIdx.x * 4 + grp;
    const bool live = inst_raw < a.batch;
    const size_t i = (size_t)(live ? inst_raw : (long)a.batch - 1);
    double* S = smem[grp];
    const bool var1 = j < kDof - 16;                 // slot 1 is joint 16 + j
    const int cs[2] = {j, var1 ? 16 + j : 0};
    const bool use_neck = a.Rd_neck != nullptr && a.w_n > 0.0;
    const double wq = a.w_q, wn = use_neck ? a.w_n : 0.0, iwq = 1.0 / wq;
    // ---- inputs, and whether all of this robot's are finite
    double tl = 0.0, tr = 0.0, tc = 0.0, tn = 0.0;
    if (j < 12) { tl = a.left_d[i * 12 + j]; tr = a.right_d[i * 12 + j]; }
    if (j < 3) tc = a.com_d[i * 3 + j];
    if (j < 9 && a.Rd_neck) tn = a.Rd_neck[i * 9 + j];
    double qg[2] = {a.q_guess[i * kDof + cs[0]], var1 ? a.q_guess[i * kDof + cs[1]] : 0.0};
    const bool lane_bad = !(isfinite(tl) && isfinite(tr) && isfinite(tc) && isfinite(tn) && isfinite(qg[0]) && isfinite(qg[1]));
    const bool bad = ((__ballot(lane_bad) >> (grp * 16)) & 0xffffull) != 0ull;
    if (bad) {
        // nothing non-finite reaches an output: the robot is evaluated at the sanitised guess with both soles at the origin
        const double id = (j == 3 || j == 7 || j == 11) ? 1.0 : 0.0;
        tl = id; tr = id; tc = 0.0; tn = (j == 0 || j == 4 || j == 8) ? 1.0 : 0.0;
    }
    if (j < 12) { S[P_TG + j] = tl; S[P_TG + TG_RIGHT + j] = tr; }
    if (j < 3) S[P_TG + TG_COM + j] = tc;
    if (j < 9) S[P_TG + TG_NECK + j] = tn;
    double qreg[2], qlo[2], qhi[2];
#pragma unroll
    for (int s_ = 0; s_ < 2; ++s_) {
        qreg[s_] = a.par[cs[s_]];
        qlo[s_] = a.use_limits ? a.par[kDof + cs[s_]] : -HUGE_VAL;
        qhi[s_] = a.use_limits ? a.par[2 * kDof + cs[s_]] : HUGE_VAL;
        if (!isfinite(qg[s_])) qg[s_] = 0.0;
        qg[s_] = fmin(fmax(qg[s_], qlo[s_]), qhi[s_]);          // the guess, clipped into the limits
    }
    int kup[2][3], ksub[2];
    __syncthreads();                                 // the model table is in LDS
    const int kfj = walk_links<3>(kmodel, j, cs, kup, ksub);
    unsigned onL[2], onR[2], onN[2];
#pragma unroll
    for (int s_ = 0; s_ < 2; ++s_) {
        onL[s_] = (a.pm[0] >> cs[s_]) & 1u; onR[s_] = (a.pm[1] >> cs[s_]) & 1u; onN[s_] = use_neck ? (a.pm[2] >> cs[s_]) & 1u : 0u;
    }
    int status = bad ? WCQP_STATUS_NUMERIC : -1;     // -1: iterating
    bool stored = !live;
    int iters = 0, nw = 0;                           // nw: active bounds of the last QP (their list is in LDS)
    unsigned wmask = 0u;
    double qc[2] = {qg[0], qg[1]};
    double* TW = S + P_X;
    double* PS = S + P_X;
    for (;;) {
        // ================= the kinematics at qc: the walk of kin_device.h with the left sole anchored at its desired pose
        double pb[3], Rb[9], pw[2][3], aw[2][3], e4[2][4];
        {
            double Ra[2][9], pa[2][3];
            local_frames_pinned(kmodel, cs, qc[0], qc[1], Ra, pa);
            walk_tree_to_base<P_FS>(TW, cs, var1, kup, a.kin_rounds, Ra, pa);
        }
        {
            double Rf[9], pf[3];
            walk_attached_frames<P_FS, 3>(kmodel, TW, S + P_FRB, j, kfj, Rf, pf);
            double sdp[3], sdR[9];
#pragma unroll
            for (int k = 0; k < 3; ++k) sdp[k] = S[P_TG + k];
#pragma unroll
            for (int k = 0; k < 9; ++k) sdR[k] = S[P_TG + 3 + k];
            base_from_anchor(sdp, sdR, S + P_FRB, Rb, pb);
            if (j < 3) frame_to_world(Rb, pb, Rf, pf, S + P_FR + j * 12);
        }
        walk_joints_to_world<P_FS>(kmodel, TW, cs, var1, Rb, pb, pw, aw, e4);
        wcqp::wave_lds_fence();          // the joint frames are dead: the prefix sums overlay them; the world frames are complete
        walk_prefix_sums(PS, j, e4);
        double tot[4], ctot[3], iM;
        walk_com_total(kmodel, PS, Rb, pb, tot, ctot, iM);
        // ---- constraint values c = p_right - pd_right | log(R_right Rd_right') | com - com_d, and the neck's rotation vector (every lane)
        double cv[9], phin[3] = {0.0, 0.0, 0.0};
        {
            const double* FRr = S + P_FR + 12;
            double Ract[9], Rdes[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) { Ract[k] = FRr[k]; Rdes[k] = S[P_TG + TG_RIGHT + 3 + k]; }
            log_rot(Ract, Rdes, cv + 3);
#pragma unroll
            for (int k = 0; k < 3; ++k) { cv[k] = FRr[9 + k] - S[P_TG + TG_RIGHT + k]; cv[6 + k] = ctot[k] - S[P_TG + TG_COM + k]; }
            if (use_neck) {
#pragma unroll
                for (int k = 0; k < 9; ++k) { Ract[k] = S[P_FR + 24 + k]; Rdes[k] = S[P_TG + TG_NECK + k]; }
                log_rot(Ract, Rdes, phin);
            }
        }
        double cmax = 0.0;
#pragma unroll
        for (int k = 0; k < 9; ++k) cmax = fmax(cmax, fabs(cv[k]));
        if (!(cmax < HUGE_VAL)) cmax = HUGE_VAL;     // (fmax drops a NaN)
#pragma unroll
        for (int k = 0; k < 9; ++k) if (!isfinite(cv[k])) cmax = HUGE_VAL;
        // ---- this lane's columns of the anchored Jacobians [JR~; Jc~] (A, nine rows) and Jn~ (N), gradient and box of the QP
#pragma unroll
        for (int s_ = 0; s_ < 2; ++s_) {
            if (s_ == 0 || var1) {
                const int c = cs[s_];
                const double* FRr = S + P_FR + 12;
                const double sr = (double)onR[s_] - (double)onL[s_], sn = (double)onN[s_] - (double)(use_neck ? onL[s_] : 0u);
                const double dr[3] = {FRr[9] - pw[s_][0], FRr[10] - pw[s_][1], FRr[11] - pw[s_][2]};
                double lin[3], linc[3], lcl[3];
                cross3(aw[s_], dr, lin);
                walk_com_column(PS, c, ksub[s_], pw[s_], aw[s_], iM, linc);
                const double dc[3] = {ctot[0] - pw[s_][0], ctot[1] - pw[s_][1], ctot[2] - pw[s_][2]};
                cross3(aw[s_], dc, lcl);
                double g = wq * (qc[s_] - qreg[s_]);
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    S[P_A + k * 24 + c] = sr * lin[k];
                    S[P_A + (3 + k) * 24 + c] = sr * aw[s_][k];
                    S[P_A + (6 + k) * 24 + c] = linc[k] - (double)onL[s_] * lcl[k];
                    S[P_N + k * 24 + c] = sn * aw[s_][k];
                    g += wn * (sn * aw[s_][k]) * phin[k];
                }
                S[P_GR + c] = g;
                S[P_LO + c] = qlo[s_] - qc[s_];
                S[P_HI + c] = qhi[s_] - qc[s_];
            }
        }
        if (j == 0) {
#pragma unroll
            for (int k = 0; k < 9; ++k) S[P_C + k] = cv[k];
        }
        wcqp::wave_lds_fence();
        // ================= a stopped robot writes its outputs from this pass, once
        if (status >= 0 && !stored) {
            // the CoM as the stand-alone kinematics kernel sums it (kin.hip: joint j on lane 6 + j of 32, a scan per 16-lane row), so that
            // the pose block equals wcqp_kin_jacobians_* at (base, q) bit for bit
#pragma unroll
            for (int s_ = 0; s_ < 2; ++s_)
                if (s_ == 0 || var1) { st2(S + P_E4 + cs[s_] * 4, e4[s_][0], e4[s_][1]); st2(S + P_E4 + cs[s_] * 4 + 2, e4[s_][2], e4[s_][3]); }
            if (j == 0) {
#pragma unroll
                for (int k = 0; k < 3; ++k) S[P_BASE + k] = pb[k];
#pragma unroll
                for (int k = 0; k < 9; ++k) S[P_BASE + 3 + k] = Rb[k];
            }
            wcqp::wave_lds_fence();
            double t0[4], t1[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                t0[k] = row_scan(j >= 6 ? S[P_E4 + (j - 6) * 4 + k] : 0.0);
                t1[k] = row_scan(j < 13 ? S[P_E4 + (10 + j) * 4 + k] : 0.0);
            }
            wcqp::wave_lds_fence();
            if (j == 15) {
                const double* rt = kmodel + kKinTabRoot;
                const double rootc[3] = {rt[0], rt[1], rt[2]};
                const double root_mass = rt[3];
                double cr[3], tt[4];
                mat3_vec(Rb, rootc, cr);
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    double r4 = root_mass * (pb[k] + cr[k]);
                    __asm__ volatile("" : "+v"(r4));     // a product and a sum there, not one fused operation
                    tt[k] = (t1[k] + t0[k]) + r4;
                }
                tt[3] = (t1[3] + t0[3]) + root_mass;
                const double im = 1.0 / tt[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) S[P_E4 + k] = tt[k] * im;
            }
            // stationarity at the returned joints: g + A' lambda on the joints off their bounds (on a bound the multiplier takes the rest)
            double sres = 0.0;
            if (status == WCQP_STATUS_SOLVED) {
#pragma unroll
                for (int s_ = 0; s_ < 2; ++s_) {
                    if ((s_ == 0 || var1) && !((wmask >> cs[s_]) & 1u)) {
                        double r = S[P_GR + cs[s_]];
                        for (int k = 0; k < 9; ++k) r += S[P_A + k * 24 + cs[s_]] * S[P_LAM + k];
                        sres = fmax(sres, fabs(r));
                        if (!isfinite(r)) sres = HUGE_VAL;
                    }
                }
            }
            S[P_DQ + j] = sres;
            wcqp::wave_lds_fence();
            for (int k = 0; k < 16; ++k) sres = fmax(sres, S[P_DQ + k]);
            a.q[i * kDof + cs[0]] = qc[0];
            if (var1) a.q[i * kDof + cs[1]] = qc[1];
            if (a.base && j < 12) a.base[i * 12 + j] = S[P_BASE + j];
            if (a.state) {
                double* st = a.state + i * kStateLen;
                for (int e = j; e < kStateLen; e += 16) {
                    double v = 0.0;
                    if (e < 24) { const int f = e / 12, r = e % 12; v = r < 3 ? S[P_FR + f * 12 + 9 + r] : S[P_FR + f * 12 + r - 3]; }
                    else if (e < 48) v = S[P_TG + e - 24];
                    else if (e < 57) v = S[P_FR + 24 + e - 48];
                    else if (e < 66) v = a.Rd_neck ? S[P_TG + TG_NECK + e - 57] : S[P_FR + 24 + e - 57];
                    else if (e < 69) v = S[P_E4 + e - 66];
                    else if (e < 72) v = S[P_TG + TG_COM + e - 69];
                    st[e] = v;
                }
            }
            if (j == 0) {
                a.status[i] = status;
                if (a.iters) a.iters[i] = iters;
                if (a.residual) {
                    const bool ok = status == WCQP_STATUS_SOLVED;
                    a.residual[i * 2] = ok ? cmax : HUGE_VAL;
                    a.residual[i * 2 + 1] = ok ? sres : HUGE_VAL;
                }
            }
            stored = true;
        }
        if (__ballot(!stored) == 0ull) break;
        // ================= one Gauss-Newton iteration of a robot that is still iterating: the QP, then the step
        if (status < 0) {
            int fail = -1;
            // K = (w_q / w_n I + N N')^-1 : H^-1 v = (v - N' K N v) / w_q
            if (wn > 0.0) {
                double nn[6] = {wq / wn, 0.0, 0.0, wq / wn, 0.0, wq / wn};      // 00 01 02 11 12 22
                for (int c = 0; c < kDof; ++c) {
                    const double n0 = S[P_N + c], n1 = S[P_N + 24 + c], n2 = S[P_N + 48 + c];
                    nn[0] += n0 * n0; nn[1] += n0 * n1; nn[2] += n0 * n2; nn[3] += n1 * n1; nn[4] += n1 * n2; nn[5] += n2 * n2;
                }
                const double c00 = nn[3] * nn[5] - nn[4] * nn[4], c01 = nn[2] * nn[4] - nn[1] * nn[5], c02 = nn[1] * nn[4] - nn[2] * nn[3];
                const double det = nn[0] * c00 + nn[1] * c01 + nn[2] * c02;
                if (!(det > 0.0) || !isfinite(det)) fail = WCQP_STATUS_NUMERIC;
                const double id = 1.0 / det;
                if (j == 0) {
                    S[P_K + 0] = c00 * id; S[P_K + 1] = c01 * id; S[P_K + 2] = c02 * id;
                    S[P_K + 3] = c01 * id; S[P_K + 4] = (nn[0] * nn[5] - nn[2] * nn[2]) * id; S[P_K + 5] = (nn[1] * nn[2] - nn[0] * nn[4]) * id;
                    S[P_K + 6] = c02 * id; S[P_K + 7] = (nn[1] * nn[2] - nn[0] * nn[4]) * id; S[P_K + 8] = (nn[0] * nn[3] - nn[1] * nn[1]) * id;
                }
            } else if (j < 9) {
                S[P_K + j] = 0.0;
            }
            // T1 = N [A' | g]  (3 x 10)
            for (int e = j; e < 30; e += 16) {
                const int k = e / 10, r = e % 10;
                const double* src = r < 9 ? S + P_A + r * 24 : S + P_GR;
                double acc = 0.0;
                for (int c = 0; c < kDof; ++c) acc += S[P_N + k * 24 + c] * src[c];
                S[P_T1 + e] = acc;
            }
            wcqp::wave_lds_fence();
            for (int e = j; e < 30; e += 16) {
                const int k = e / 10, r = e % 10;
                S[P_KT + e] = S[P_K + 3 * k] * S[P_T1 + r] + S[P_K + 3 * k + 1] * S[P_T1 + 10 + r] + S[P_K + 3 * k + 2] * S[P_T1 + 20 + r];
            }
            wcqp::wave_lds_fence();
            // G = H^-1 A' (23 x 9) and the unconstrained minimiser x0 = -H^-1 g (column 9), this lane's rows
#pragma unroll
            for (int s_ = 0; s_ < 2; ++s_) {
                if (s_ == 0 || var1) {
                    const int c = cs[s_];
                    const double n0 = S[P_N + c], n1 = S[P_N + 24 + c], n2 = S[P_N + 48 + c];
                    for (int r = 0; r < 10; ++r) {
                        const double v = r < 9 ? S[P_A + r * 24 + c] : -S[P_GR + c];
                        const double corr = n0 * S[P_KT + r] + n1 * S[P_KT + 10 + r] + n2 * S[P_KT + 20 + r];
                        S[P_G + c * 10 + r] = (r < 9 ? v - corr : v + corr) * iwq;
                    }
                }
            }
            wcqp::wave_lds_fence();
            // M = A G (9 x 9) and A x0 (column 9)
            for (int e = j; e < 90; e += 16) {
                const int r = e / 10, col = e % 10;
                double acc = 0.0;
                for (int c = 0; c < kDof; ++c) acc += S[P_A + r * 24 + c] * S[P_G + c * 10 + col];
                S[P_M + e] = acc;
            }
            wcqp::wave_lds_fence();
            // ---- the active-set walk.  Rows of the Schur complement: the nine equalities, then the active bounds in list order
            nw = 0; wmask = 0u;
            int* WI = reinterpret_cast<int*>(S + P_WI);
            for (int chg = 0; fail < 0; ++chg) {
                if (chg > kMaxChanges) { fail = WCQP_STATUS_MAX_ITER; break; }
                const int ns = 9 + nw;
                for (int row = j; row < ns; row += 16) {
                    const int wr = row >= 9 ? WI[row - 9] : 0;
                    for (int col = 0; col <= row; ++col) {
                        double v;
                        if (row < 9) v = S[P_M + row * 10 + col];
                        else if (col < 9) v = S[P_G + wr * 10 + col];
                        else {
                            const int wc = WI[col - 9];
                            double acc = wr == wc ? 1.0 : 0.0;
                            for (int k = 0; k < 3; ++k)
                                acc -= S[P_N + k * 24 + wr] * (S[P_K + 3 * k] * S[P_N + wc] + S[P_K + 3 * k + 1] * S[P_N + 24 + wc] + S[P_K + 3 * k + 2] * S[P_N + 48 + wc]);
                            v = acc * iwq;
                        }
                        S[P_X + row * P_SS + col] = v;
                    }
                    S[P_LAM + row] = row < 9 ? S[P_M + row * 10 + 9] + S[P_C + row] : S[P_G + wr * 10 + 9] - S[P_WB + row - 9];
                }
                wcqp::wave_lds_fence();
                // Cholesky in place (lower triangle), lane j owns rows j and 16 + j
                for (int p = 0; p < ns; ++p) {
                    const double d = S[P_X + p * P_SS + p];
                    const double orig = p < 9 ? S[P_M + p * 10 + p] : iwq;
                    if (!(d > 1e-12 * orig)) { fail = isfinite(d) && isfinite(orig) ? WCQP_STATUS_INFEASIBLE : WCQP_STATUS_NUMERIC; break; }
                    const double sd = sqrt(d), isd = 1.0 / sd;
                    wcqp::wave_lds_fence();
                    for (int row = j; row < ns; row += 16) {
                        if (row == p) S[P_X + p * P_SS + p] = sd;
                        else if (row > p) S[P_X + row * P_SS + p] *= isd;
                    }
                    wcqp::wave_lds_fence();
                    for (int row = j; row < ns; row += 16) {
                        if (row > p) {
                            const double l = S[P_X + row * P_SS + p];
                            for (int col = p + 1; col <= row; ++col) S[P_X + row * P_SS + col] -= l * S[P_X + col * P_SS + p];
                        }
                    }
                    wcqp::wave_lds_fence();
                }
                if (fail >= 0) break;
                // L y = rhs, L' lambda = y (column sweeps)
                for (int p = 0; p < ns; ++p) {
                    const double y = S[P_LAM + p] / S[P_X + p * P_SS + p];
                    wcqp::wave_lds_fence();
                    for (int row = j; row < ns; row += 16) {
                        if (row == p) S[P_LAM + p] = y;
                        else if (row > p) S[P_LAM + row] -= S[P_X + row * P_SS + p] * y;
                    }
                    wcqp::wave_lds_fence();
                }
                for (int p = ns - 1; p >= 0; --p) {
                    const double x = S[P_LAM + p] / S[P_X + p * P_SS + p];
                    wcqp::wave_lds_fence();
                    for (int row = j; row < ns; row += 16) {
                        if (row == p) S[P_LAM + p] = x;
                        else if (row < p) S[P_LAM + row] -= S[P_X + p * P_SS + row] * x;
                    }
                    wcqp::wave_lds_fence();
                }
                // dq = x0 - H^-1 E' lambda, this lane's joints; a joint on an active bound sits on it exactly
#pragma unroll
                for (int s_ = 0; s_ < 2; ++s_) {
                    if (s_ == 0 || var1) {
                        const int c = cs[s_];
                        double v = S[P_G + c * 10 + 9];
                        for (int r = 0; r < 9; ++r) v -= S[P_G + c * 10 + r] * S[P_LAM + r];
                        const double n0 = S[P_N + c], n1 = S[P_N + 24 + c], n2 = S[P_N + 48 + c];
                        for (int b = 0; b < nw; ++b) {
                            const int wc = WI[b];
                            double h = c == wc ? 1.0 : 0.0;
                            for (int k = 0; k < 3; ++k)
                                h -= (k == 0 ? n0 : (k == 1 ? n1 : n2)) * (S[P_K + 3 * k] * S[P_N + wc] + S[P_K + 3 * k + 1] * S[P_N + 24 + wc] + S[P_K + 3 * k + 2] * S[P_N + 48 + wc]);
                            v -= h * iwq * S[P_LAM + 9 + b];
                        }
                        if ((wmask >> c) & 1u) {
                            for (int b = 0; b < nw; ++b) if (WI[b] == c) v = S[P_WB + b];
                        }
                        S[P_DQ + c] = v;
                    }
                }
                wcqp::wave_lds_fence();
                // the most violated bound among the free joints (every lane of the robot decides the same)
                double worst = kBoundTol; int wj = -1; double wside = 0.0;
                for (int c = 0; c < kDof; ++c) {
                    if ((wmask >> c) & 1u) continue;
                    const double d = S[P_DQ + c];
                    if (!isfinite(d)) { fail = WCQP_STATUS_NUMERIC; break; }
                    const double vl = S[P_LO + c] - d, vh = d - S[P_HI + c];
                    if (vl > worst) { worst = vl; wj = c; wside = -1.0; }
                    if (vh > worst) { worst = vh; wj = c; wside = 1.0; }
                }
                if (fail >= 0) break;
                if (wj >= 0) {
                    if (nw >= kMaxActive) { fail = WCQP_STATUS_INFEASIBLE; break; }
                    wcqp::wave_lds_fence();
                    if (j == 0) { WI[nw] = wj; S[P_WB + nw] = wside > 0.0 ? S[P_HI + wj] : S[P_LO + wj]; S[P_WS + nw] = wside; }
                    wmask |= 1u << wj; ++nw;
                    wcqp::wave_lds_fence();
                    continue;
                }
                // the active bound whose multiplier has the wrong sign the most (upper: lambda >= 0, lower: lambda <= 0)
                double low = -kBoundTol; int wb = -1;
                for (int b = 0; b < nw; ++b) {
                    const double m = S[P_LAM + 9 + b] * S[P_WS + b];
                    if (m < low) { low = m; wb = b; }
                }
                if (wb < 0) break;                   // the optimum of the QP
                const int gone = WI[wb];
                wcqp::wave_lds_fence();
                if (j == 0) {
                    for (int b = wb; b + 1 < nw; ++b) { WI[b] = WI[b + 1]; S[P_WB + b] = S[P_WB + b + 1]; S[P_WS + b] = S[P_WS + b + 1]; }
                }
                wmask &= ~(1u << gone); --nw;
                wcqp::wave_lds_fence();
            }
            // ---- the step
            double maxdq = 0.0;
            if (fail < 0) {
                for (int c = 0; c < kDof; ++c) maxdq = fmax(maxdq, fabs(S[P_DQ + c]));
                if (!(maxdq < HUGE_VAL)) fail = WCQP_STATUS_NUMERIC;
            }
            ++iters;
            if (fail < 0) {
                const double alpha = maxdq > a.step_cap ? a.step_cap / maxdq : 1.0;
#pragma unroll
                for (int s_ = 0; s_ < 2; ++s_) {
                    const double v = qc[s_] + alpha * S[P_DQ + cs[s_]];
                    qc[s_] = fmin(fmax(v, qlo[s_]), qhi[s_]);
                }
                if (maxdq < a.tol_step && cmax < a.tol_c) status = WCQP_STATUS_SOLVED;
                else if (iters >= a.max_iter) fail = WCQP_STATUS_MAX_ITER;
            }
            if (fail >= 0) { status = fail; qc[0] = qg[0]; qc[1] = qg[1]; }
            wcqp::wave_lds_fence();
        }
    }
}

}  // namespace

struct wcqp_prepare_s {
    PrepDev dev{};
    std::vector<double> tab, par;
    double* d_tab = nullptr;                   // the model table, then the parameter rows
    wcqp::DeviceScratch scratch;
};

namespace {
int ensure_device(wcqp_prepare_s* h) {
    if (h->d_tab) return WCQP_OK;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        std::fprintf(stderr, "[wcqp] no HIP device: the prepare kernel has no CPU fallback\n");
        return WCQP_E_HIP;
    }
    const size_t nt = h->tab.size(), np = h->par.size();
    WCQP_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&h->d_tab), (nt + np) * sizeof(double)));
    WCQP_HIP_TRY(hipMemcpy(h->d_tab, h->tab.data(), nt * sizeof(double), hipMemcpyHostToDevice));
    WCQP_HIP_TRY(hipMemcpy(h->d_tab + nt, h->par.data(), np * sizeof(double), hipMemcpyHostToDevice));
    h->dev.kin_tab = h->d_tab;
    h->dev.par = h->d_tab + nt;
    return WCQP_OK;
}
}  // namespace

extern "C" {

int wcqp_prepare_create(wcqp_kin_t kin, const wcqp_prepare_params* p, wcqp_prepare_t* out) {
    if (!kin || !p || !out || !p->q_reg) return WCQP_E_INVALID;
    if (!std::isfinite(p->w_q) || !(p->w_q > 0.0) || !std::isfinite(p->w_n) || !(p->w_n >= 0.0)) return WCQP_E_INVALID;
    if (!std::isfinite(p->step_cap) || !(p->step_cap > 0.0)) return WCQP_E_INVALID;
    if (!std::isfinite(p->tol_step) || !(p->tol_step >= 0.0) || !std::isfinite(p->tol_constraint) || !(p->tol_constraint >= 0.0)) return WCQP_E_INVALID;
    if (p->max_iter < 1) return WCQP_E_INVALID;
    if ((p->q_min == nullptr) != (p->q_max == nullptr)) return WCQP_E_INVALID;
    wcqp_prepare_s* h = new (std::nothrow) wcqp_prepare_s();
    if (!h) return WCQP_E_NOMEM;
    int n_rounds = 0, stride = 0, off_d = 0;
    // the tree must be one the 16-lane walk runs (the condition of the tick's FUSED hand-off)
    if (!wcqp::kin_fused_tables(kin, h->tab, &n_rounds) || !wcqp::kin_compact_layout(kin, h->dev.pm, &stride, &off_d)) { delete h; return WCQP_E_UNSUPPORTED; }
    h->par.assign(3 * kDof, 0.0);
    for (int k = 0; k < kDof; ++k) {
        if (!std::isfinite(p->q_reg[k])) { delete h; return WCQP_E_INVALID; }
        h->par[k] = p->q_reg[k];
        if (p->q_min) {
            if (!(p->q_min[k] <= p->q_max[k])) { delete h; return WCQP_E_INVALID; }       // (a NaN limit fails too)
            h->par[kDof + k] = p->q_min[k]; h->par[2 * kDof + k] = p->q_max[k];
        }
    }
    PrepDev& d = h->dev;
    d.kin_rounds = n_rounds;
    d.w_q = p->w_q; d.w_n = p->w_n; d.step_cap = p->step_cap; d.tol_step = p->tol_step; d.tol_c = p->tol_constraint;
    d.max_iter = p->max_iter; d.use_limits = p->q_min ? 1 : 0;
    *out = h;
    return WCQP_OK;
}

int wcqp_prepare_destroy(wcqp_prepare_t h) {
    if (!h) return WCQP_E_INVALID;
    if (h->d_tab) (void)hipFree(h->d_tab);
    h->scratch.release();
    delete h;
    return WCQP_OK;
}

int wcqp_prepare_solve_device(wcqp_prepare_t h, int32_t batch, const double* left_d, const double* right_d, const double* com_d,
                              const double* Rd_neck, const double* q_guess,
                              double* q, double* base, double* state, int32_t* status, int32_t* iters, double* residual, void* stream) {
    if (!h || batch < 0) return WCQP_E_INVALID;
    if (!left_d || !right_d || !com_d || !q_guess || !q || !status) return WCQP_E_INVALID;
    if (!wcqp::fits32(batch, kStateLen * 8)) return WCQP_E_UNSUPPORTED;
    if (batch == 0) return WCQP_OK;
    const int rc = ensure_device(h);
    if (rc != WCQP_OK) return rc;
    PrepDev a = h->dev;
    a.batch = batch;
    a.left_d = left_d; a.right_d = right_d; a.com_d = com_d; a.Rd_neck = Rd_neck; a.q_guess = q_guess;
    a.q = q; a.base = base; a.state = state; a.status = status; a.iters = iters; a.residual = residual;
    hipLaunchKernelGGL(prepare_kernel, dim3((unsigned)((batch + 3) / 4)), dim3(64), 0, (hipStream_t)stream, a);
    WCQP_HIP_TRY(hipGetLastError());
    return WCQP_OK;
}

int wcqp_prepare_solve_host(wcqp_prepare_t h, int32_t batch, const double* left_d, const double* right_d, const double* com_d,
                            const double* Rd_neck, const double* q_guess,
                            double* q, double* base, double* state, int32_t* status, int32_t* iters, double* residual) {
    if (!h || batch < 0) return WCQP_E_INVALID;
    if (!left_d || !right_d || !com_d || !q_guess || !q || !status) return WCQP_E_INVALID;
    if (!wcqp::fits32(batch, kStateLen * 8)) return WCQP_E_UNSUPPORTED;
    if (batch == 0) return WCQP_OK;
    int rc = ensure_device(h);
    if (rc != WCQP_OK) return rc;
    const size_t B = (size_t)batch;
    const size_t o_l = 0, o_r = o_l + B * 12, o_c = o_r + B * 12, o_n = o_c + B * 3, o_g = o_n + B * 9, o_q = o_g + B * kDof, o_b = o_q + B * kDof,
                 o_s = o_b + B * 12, o_res = o_s + B * kStateLen, o_st = o_res + B * 2, total = o_st + B;     // status | iters: B ints each
    rc = h->scratch.reserve(total * sizeof(double));
    if (rc != WCQP_OK) return rc;
    double* d = static_cast<double*>(h->scratch.ptr);
    int32_t* di = reinterpret_cast<int32_t*>(d + o_st);
    WCQP_HIP_TRY(hipMemcpy(d + o_l, left_d, B * 12 * 8, hipMemcpyHostToDevice));
    WCQP_HIP_TRY(hipMemcpy(d + o_r, right_d, B * 12 * 8, hipMemcpyHostToDevice));
    WCQP_HIP_TRY(hipMemcpy(d + o_c, com_d, B * 3 * 8, hipMemcpyHostToDevice));
    if (Rd_neck) WCQP_HIP_TRY(hipMemcpy(d + o_n, Rd_neck, B * 9 * 8, hipMemcpyHostToDevice));
    WCQP_HIP_TRY(hipMemcpy(d + o_g, q_guess, B * kDof * 8, hipMemcpyHostToDevice));
    rc = wcqp_prepare_solve_device(h, batch, d + o_l, d + o_r, d + o_c, Rd_neck ? d + o_n : nullptr, d + o_g,
                                   d + o_q, d + o_b, d + o_s, di, di + B, d + o_res, nullptr);
    if (rc != WCQP_OK) return rc;
    WCQP_HIP_TRY(hipDeviceSynchronize());
    WCQP_HIP_TRY(hipMemcpy(q, d + o_q, B * kDof * 8, hipMemcpyDeviceToHost));
    if (base) WCQP_HIP_TRY(hipMemcpy(base, d + o_b, B * 12 * 8, hipMemcpyDeviceToHost));
    if (state) WCQP_HIP_TRY(hipMemcpy(state, d + o_s, B * kStateLen * 8, hipMemcpyDeviceToHost));
    WCQP_HIP_TRY(hipMemcpy(status, di, B * 4, hipMemcpyDeviceToHost));
    if (iters) WCQP_HIP_TRY(hipMemcpy(iters, di + B, B * 4, hipMemcpyDeviceToHost));
    if (residual) WCQP_HIP_TRY(hipMemcpy(residual, d + o_res, B * 2 * 8, hipMemcpyDeviceToHost));
    return WCQP_OK;
}

}  // extern "C"
