// The iteration of the batched non-linear IK (include/wcqp.h: wcqp_prepare_*, which states the problem and the iteration) as device
// functions, shared by the kernel that runs it once per robot (prepare.hip: prepare_kernel) and the one that runs it on every tick of a
// walk (position_tick.hip: position_tick_kernel).  16 lanes per robot, two joints per lane (slot 0: joint j, slot 1: joint 16 + j), one
// LDS block of P_PER doubles per robot; the three blocks of one pass:
//   prep_linearise   the kinematics at qc with the left sole anchored at its desired pose, the constraint values, the anchored Jacobian
//                    columns, gradient and box of the QP - into LDS
//   prep_qp          the QP: H = w_q I + w_n N'N inverted by the 3 x 3 Woodbury identity, the Schur complement of the equality rows and the
//                    active bounds, its Cholesky factor, the active-set walk
//   prep_step        the capped step and the stop rule
// The callers own everything else: the targets in LDS (P_TG), the guess, what a stopped robot stores.  Plain vector loads and stores only.
#pragma once
#include "wcqp_internal.h"
#include "kin_device.h"

namespace wcqp_prep {

using namespace wcqp_kin;
constexpr int kDof = kWalkDof;
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

#if defined(__HIPCC__)
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
// block prepare_kernel writes is wcqp_kin_jacobians_* at (base, q) bit for bit.
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

// ================= the kinematics at qc: the walk of kin_device.h with the left sole anchored at its desired pose (S + P_TG), then the
// constraint values, this lane's columns of the anchored Jacobians, the gradient and the box - everything prep_qp reads, in LDS.
// Leaves the base (pb, Rb) and this lane's link moments e4 (what an output pass needs) and cmax = max |c| (HUGE_VAL when not finite).
// kup / ksub / kfj: walk_links<3>; onL / onR / onN: whether this lane's joints lie on the path of the left sole, the right sole, the neck.
__device__ __forceinline__ void prep_linearise(const double* kmodel, double* S, int j, const int (&cs)[2], bool var1, const int (&kup)[2][3],
                                               const int (&ksub)[2], int kfj, int kin_rounds, const unsigned (&onL)[2], const unsigned (&onR)[2],
                                               const unsigned (&onN)[2], bool use_neck, double wq, double wn, const double (&qc)[2],
                                               const double (&qreg)[2], const double (&qlo)[2], const double (&qhi)[2],
                                               double (&pb)[3], double (&Rb)[9], double (&e4)[2][4], double& cmax) {
    double* TW = S + P_X;
    double* PS = S + P_X;
    double pw[2][3], aw[2][3];
    {
        double Ra[2][9], pa[2][3];
        local_frames_pinned(kmodel, cs, qc[0], qc[1], Ra, pa);
        walk_tree_to_base<P_FS>(TW, cs, var1, kup, kin_rounds, Ra, pa);
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
    cmax = 0.0;
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
}

// ================= the QP of one Gauss-Newton iteration, from what prep_linearise left in LDS: dq into S + P_DQ, the equality rows'
// multipliers into S + P_LAM, the active bounds into the lists at P_WI / P_WB / P_WS (nw of them; wmask: their joints).
// Returns -1, or the WCQP_STATUS_* the robot fails with.
__device__ __forceinline__ int prep_qp(double* S, int j, const int (&cs)[2], bool var1, double wq, double wn, double iwq, int& nw, unsigned& wmask) {
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
    return fail;
}

// ================= the step and the stop rule: q += min(1, step_cap / max |dq|) dq, clipped into the limits; SOLVED when max |dq| < tol_step
// and max |c| < tol_c, MAX_ITER with the budget spent; for every status other than SOLVED qc goes back to the clipped guess qg.
// `fail`: what prep_qp returned.  Counts the iteration.
__device__ __forceinline__ void prep_step(const double* S, const int (&cs)[2], int fail, double cmax, double step_cap, double tol_step, double tol_c,
                                          int max_iter, const double (&qg)[2], const double (&qlo)[2], const double (&qhi)[2], double (&qc)[2],
                                          int& iters, int& status) {
    double maxdq = 0.0;
    if (fail < 0) {
        for (int c = 0; c < kDof; ++c) maxdq = fmax(maxdq, fabs(S[P_DQ + c]));
        if (!(maxdq < HUGE_VAL)) fail = WCQP_STATUS_NUMERIC;
    }
    ++iters;
    if (fail < 0) {
        const double alpha = maxdq > step_cap ? step_cap / maxdq : 1.0;
#pragma unroll
        for (int s_ = 0; s_ < 2; ++s_) {
            const double v = qc[s_] + alpha * S[P_DQ + cs[s_]];
            qc[s_] = fmin(fmax(v, qlo[s_]), qhi[s_]);
        }
        if (maxdq < tol_step && cmax < tol_c) status = WCQP_STATUS_SOLVED;
        else if (iters >= max_iter) fail = WCQP_STATUS_MAX_ITER;
    }
    if (fail >= 0) { status = fail; qc[0] = qg[0]; qc[1] = qg[1]; }
}
#endif

}  // namespace wcqp_prep
