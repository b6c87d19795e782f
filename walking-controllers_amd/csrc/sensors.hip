// Sensor feedback of the tick pipeline (include/wcqp.h: wcqp_tick_set_sensor_feedback_*): what the reference evaluates from the robot's
// joint encoders and foot wrenches every tick before its controllers run (citations relative to /root/reference/modules/Walking_module):
//   src/WalkingModule.cpp:1147-1165           updateFKSolver: base anchored at the desired pose of the fixed-frame foot, measured joints
//   src/WalkingForwardKinematics.cpp:258-337  setInternalRobotState (zero base twist), evaluateCoM, evaluateDCM
//   src/WalkingModule.cpp:826-878             evaluateZMP
// The kinematics are the walk of kin_device.h (walk_*) at the MEASURED joints: the functions the fused tick kernel (ik4_device.h, JSRC = 2)
// runs at the desired ones - the model table in LDS, 16 lanes per robot with lane j owning joints j and 16 + j, pointer jumping for the
// joint frames, a row scan for the subtree first moments - here with this kernel's LDS map and two attached frames (the soles).  With
// q_meas = q_des the sole poses and the CoM therefore agree with the tick's own to rounding: it is one text, not two kept in step.  No Jacobian
// leaves the kernel: the CoM velocity is the joint block of the MIXED CoM Jacobian times dq_meas, reduced across the robot's row.
#include "tick_device.h"
#include "kin_device.h"
#include "sensors.h"

namespace {

using namespace wcqp_tick;

// LDS per robot (doubles): joint frames [23][S_FS] (the subtree prefix sums [32][4] overlay them once the joints are in world
// coordinates), the two soles in base and in world coordinates [2][12] each, the anchor's desired pose [12], the CoM velocity [2]
constexpr int S_FS = 14, S_TW = 0, S_FRB = 322, S_FR = 346, S_SD = 370, S_V = 382;
constexpr int S_PER = 392;          // = 8 mod 32: the four robots of a wave sit apart in the banks
static_assert(kDof * S_FS <= S_FRB && 32 * 4 <= S_FRB && S_V + 2 <= S_PER, "sensor kernel LDS layout");

// One robot per 16 lanes, four per wave, one wave per workgroup.
// PL (streamed trajectories, wcqp_tick_set_desired_*): the stance side is the fixed-frame bit of the stage the caller handed over for tick t
// and the anchor that stage's desired sole pose (the robot's record, tick_device.h: kPlanRec) - what tick t's own kinematics take
// FILT (a cut frequency > 0, wcqp_tick_params): the reference's first-order low-pass filters on the joint velocities, on fz tx ty of both
// wrenches and on the CoM position and velocity (sensors.h: lowpass_coeffs, the record layout).  The state of the last RUN tick is read
// from a.filt_src with the sensor inputs - in flight under the kinematics - and this tick's goes to a.filt_dst, the handle's other slot: a
// second call for the same tick starts from the same state.  Lane j owns the state of its joints j and 16 + j, lanes 0 .. 5 write one
// wrench component each, lanes 0 / 1 their axis of the CoM.  The rejection is known before the kinematics (finiteness of the RAW readings,
// the total of the FILTERED normal forces), so the joint and wrench records are stored there, while their previous values are still in
// registers: a rejected robot's record is carried over unchanged - its filters hold - and nothing non-finite ever enters one.  The
// robot's FRESH mark (sensors.h: kFiltFresh, set by wcqp_tick_reset_robots) is loaded with the record and makes this reading the robot's
// first, as a.filt_first makes it everybody's; lane 6 stores it with the record: carried over when rejected, cleared when accepted.
template <bool PL, bool FILT>
__global__ __launch_bounds__(64) void tick_sensor_kernel(SensorDev a) {
    using namespace wcqp_kin;
    __shared__ __attribute__((aligned(16))) double kmodel[kKinTabSize];
    __shared__ __attribute__((aligned(16))) double smem[4][S_PER];
    const int lane = threadIdx.x, grp = lane >> 4, j = lane & 15;
    for (int k = lane; k < kKinTabSize; k += 64) kmodel[k] = a.kin_tab[k];
    const long inst_raw = (long)blockIdx.x * 4 + grp;
    const bool live = inst_raw < a.batch;
    const size_t i = (size_t)(live ? inst_raw : (long)a.batch - 1);
    double* S = smem[grp];
    const bool var1 = j < kDof - 16;                 // slot 1 is joint 16 + j
    const int cs[2] = {j, var1 ? 16 + j : 0};
    // ---- inputs, and whether all of this robot's are finite
    const double* qi = a.q + i * kDof;
    const double* dqi = a.dq + i * kDof;
    const double q0 = qi[j], q1 = var1 ? qi[16 + j] : 0.0;
    const double dq0 = dqi[j], dq1 = var1 ? dqi[16 + j] : 0.0;
    const double wv = j < 6 ? a.wl[i * 6 + j] : (j < 12 ? a.wr[i * 6 + j - 6] : 0.0);
    const bool lane_bad = !(isfinite(q0) && isfinite(q1) && isfinite(dq0) && isfinite(dq1) && isfinite(wv));
    const bool bad = ((__ballot(lane_bad) >> (grp * 16)) & 0xffffull) != 0ull;
    // what the ZMP reads of the two wrenches - fz, tx, ty - on every lane, in flight with the rest (the same addresses across the row)
    const double* wli = a.wl + i * 6;
    const double* wri = a.wr + i * 6;
    double fzL = wli[2], txL = wli[3], tyL = wli[4], fzR = wri[2], txR = wri[3], tyR = wri[4];
    double dqf0 = dq0, dqf1 = dq1;                   // what v_com is formed with
    double2 sc_p = make_double2(0.0, 0.0), sc_v = sc_p;      // FILT: {u_prev, y_prev} of this lane's axis of the CoM, position and velocity
    bool rejected = bad;
    if constexpr (FILT) {
        const double* fs = a.filt_src + i * kFiltRec;
        const double2 sd0 = ld2(fs + 2 * cs[0]), sd1 = ld2(fs + 2 * cs[1]);
        double2 sw[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) sw[k] = ld2(fs + kFiltWrench + 2 * k);
        sc_p = ld2(fs + kFiltCom + 4 * (j & 1)); sc_v = ld2(fs + kFiltCom + 4 * (j & 1) + 2);
        const double fresh = fs[kFiltFresh];         // (wcqp_tick_reset_robots: this robot's filters start at its next accepted reading)
        const bool first = a.filt_first != 0 || fresh != 0.0;
        if (a.filt_mask & 1) {
            dqf0 = first ? dq0 : a.fb[0] * (dq0 + sd0.x) + a.fa[0] * sd0.y;
            dqf1 = (first || !var1) ? dq1 : a.fb[0] * (dq1 + sd1.x) + a.fa[0] * sd1.y;     // (stays 0 on a lane without a second joint)
        }
        const double wu[6] = {fzL, txL, tyL, fzR, txR, tyR};
        double wf[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) wf[k] = ((a.filt_mask & 2) && !first) ? a.fb[1] * (wu[k] + sw[k].x) + a.fa[1] * sw[k].y : wu[k];
        fzL = wf[0]; txL = wf[1]; tyL = wf[2]; fzR = wf[3]; txR = wf[4]; tyR = wf[5];
        rejected = bad || !(fzR + fzL >= 0.1);       // evaluateZMP sees the filtered forces only
        if (live) {
            double* fd = a.filt_dst + i * kFiltRec;
            if (a.filt_mask & 1) {
                st2(fd + 2 * j, rejected ? sd0.x : dq0, rejected ? sd0.y : dqf0);
                if (var1) st2(fd + 2 * (16 + j), rejected ? sd1.x : dq1, rejected ? sd1.y : dqf1);
            }
            if (a.filt_mask & 2) {
#pragma unroll
                for (int k = 0; k < 6; ++k)
                    if (j == k) st2(fd + kFiltWrench + 2 * k, rejected ? sw[k].x : wu[k], rejected ? sw[k].y : wf[k]);
            }
            if (j == 6) fd[kFiltFresh] = rejected ? fresh : 0.0;
        }
    }
    // the stance side of tick t, as the tick kernel carries it: (t + phase0) % (2 step_ticks) >= step_ticks -> the right sole anchors
    int side;
    if constexpr (PL) {
        const double* rc = a.rec + i * kPlanRec;
        side = plan_side((int)rc[kPlanFlags]);
        if (j < 12) S[S_SD + j] = rc[kPlanLeft + side * 12 + j];
    } else {
        const int cyc = (a.t + a.phase0[i]) % (2 * a.step_ticks);
        side = cyc >= a.step_ticks ? 1 : 0;
        if (j < 12) S[S_SD + j] = a.state[i * kStateLen + 24 + side * 12 + j];     // its desired pose: p (3), R (9)
    }
    int kup[2][3], ksub[2];
    __syncthreads();                                 // the model table is in LDS
    // the walk of kin_device.h - the fused tick kernel's (ik4_device.h, JSRC = 2) - at the measured joints, on this kernel's LDS map
    const int kfj = walk_links<2>(kmodel, j, cs, kup, ksub);
    double* TW = S + S_TW;
    {
        double Ra[2][9], pa[2][3];
        walk_local_frames(kmodel, cs, q0, q1, Ra, pa);
        // walk_tree_to_base and (below) walk_prefix_sums, written out: called as functions they cost the FILT kernels' register figures
        // (DESIGN.md 8.2); the rounds' stores are the shared leaf
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            if (r >= a.kin_rounds) break;
#pragma unroll
            for (int s_ = 0; s_ < 2; ++s_) {
                if (s_ == 0 || var1) {
                    frame_store(TW + cs[s_] * S_FS, Ra[s_], pa[s_]);
                }
            }
            wcqp::wave_lds_fence();
#pragma unroll
            for (int s_ = 0; s_ < 2; ++s_) {
                const int u = kup[s_][r];
                if (u >= 0 && (s_ == 0 || var1)) {
                    const double* T = TW + u * S_FS;
                    double Rp[9], pp[3], Rn[9], pn[3];
#pragma unroll
                    for (int k = 0; k < 9; ++k) Rp[k] = T[k];
#pragma unroll
                    for (int k = 0; k < 3; ++k) pp[k] = T[9 + k];
                    frame_mul(Rp, pp, Ra[s_], pa[s_], Rn, pn);
#pragma unroll
                    for (int k = 0; k < 9; ++k) Ra[s_][k] = Rn[k];
#pragma unroll
                    for (int k = 0; k < 3; ++k) pa[s_][k] = pn[k];
                }
            }
            wcqp::wave_lds_fence();
        }
#pragma unroll
        for (int s_ = 0; s_ < 2; ++s_) {
            if (s_ == 0 || var1) {
                frame_store(TW + cs[s_] * S_FS, Ra[s_], pa[s_]);
            }
        }
    }
    wcqp::wave_lds_fence();
    // the two soles in base coordinates: lanes 0 (left) and 1 (right)
    double Rf[9], pf[3];
    walk_attached_frames<S_FS, 2>(kmodel, TW, S + S_FRB, j, kfj, Rf, pf);
    // base pose from the anchor sole's desired pose and its frame at q_meas
    double pb[3], Rb[9];
    {
        double sdp[3], sdR[9];
#pragma unroll
        for (int k = 0; k < 3; ++k) sdp[k] = S[S_SD + k];
#pragma unroll
        for (int k = 0; k < 9; ++k) sdR[k] = S[S_SD + 3 + k];
        base_from_anchor(sdp, sdR, S + S_FRB + side * 12, Rb, pb);
    }
    // the soles in world coordinates (the MEASURED poses the ZMP is mapped with)
    if (j < 2) frame_to_world(Rb, pb, Rf, pf, S + S_FR + j * 12);
    double pw[2][3], aw[2][3], e4[2][4];
    walk_joints_to_world<S_FS>(kmodel, TW, cs, var1, Rb, pb, pw, aw, e4);
    wcqp::wave_lds_fence();          // the joint frames are dead: the prefix sums overlay them
    double* PS = S + S_TW;           // [32][4]
    {
        double p0s[4], p1s[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { p0s[k] = row_scan(e4[0][k]); p1s[k] = row_scan(e4[1][k]); }
        st2(PS + j * 4, p0s[0], p0s[1]); st2(PS + j * 4 + 2, p0s[2], p0s[3]);
        wcqp::wave_lds_fence();
        const double2 t01 = ld2(PS + 15 * 4), t23 = ld2(PS + 15 * 4 + 2);
        st2(PS + (16 + j) * 4, p1s[0] + t01.x, p1s[1] + t01.y); st2(PS + (16 + j) * 4 + 2, p1s[2] + t23.x, p1s[3] + t23.y);
        wcqp::wave_lds_fence();
    }
    double tot[4], ctot[3], iM;
    walk_com_total(kmodel, PS, Rb, pb, tot, ctot, iM);
    // v_com = J_com[:, joints] dq_meas (the base twist is zero, WalkingFK::setInternalRobotState): this lane's two CoM columns
    // (a_c x (c_sub(c) - p_c) m_sub(c) / M, as the fused tick forms them) times its two joint velocities, summed over the row
    double vx = 0.0, vy = 0.0;
#pragma unroll
    for (int s_ = 0; s_ < 2; ++s_) {
        double lin[3];
        walk_com_column(PS, cs[s_], ksub[s_], pw[s_], aw[s_], iM, lin);
        const double w = s_ == 0 ? dqf0 : dqf1;      // (0 on a lane without a second joint)
        vx += lin[0] * w; vy += lin[1] * w;
    }
    vx = row_scan(vx); vy = row_scan(vy);
    if (j == 15) st2(S + S_V, vx, vy);
    wcqp::wave_lds_fence();
    // ---- the rejection (every lane), lanes 0 / 1: axis j of the DCM and of the ZMP (WalkingModule::evaluateZMP), the write-back
    if (!live) return;
    const double totalZ = fzR + fzL;
    if constexpr (!FILT) rejected = bad || !(totalZ >= 0.1);
    double* qm = a.q_meas + i * kDof;
    if (!rejected) {
        qm[j] = q0;
        if (var1) qm[16 + j] = q1;
    } else if (a.t == 0) {
        // rejected on tick 0: the desired joints, as the plain form without q_meas
        qm[j] = a.q_des[i * kDof + j];
        if (var1) qm[16 + j] = a.q_des[i * kDof + 16 + j];
    }
    if (j >= 2) return;
    double* rec = a.mst + (i * 2 + j) * 8;
    if (rejected) {
        // updateModule returns false: the measured state of the previous tick stays - what its chain read, kept in the hand-off record of
        // parity t - 1 (tick 0: the uploaded state) - and the robot is stopped like one whose IK failed
        if (a.t > 0) {
            const double* hd = a.hand + ((size_t)((a.t - 1) & 1) * a.batch + i) * kHandLen;
            rec[2] = hd[4 + j]; rec[6] = hd[6 + j]; rec[7] = hd[10 + j];
        }
        if constexpr (FILT) {
            if (a.filt_mask & 4) {
                double* fd = a.filt_dst + i * kFiltRec + kFiltCom + 4 * j;
                st2(fd, sc_p.x, sc_p.y); st2(fd + 2, sc_v.x, sc_v.y);
            }
        }
        if (j == 0) {
            a.feedback_fail[i] += 1;
            if (a.ik_fail[i] == 0) a.ik_fail[i] = 1;
        }
        return;
    }
    double v = S[S_V + j], cm = ctot[j];
    if constexpr (FILT) {
        // evaluateCoM / evaluateDCM with use_filters: the filtered position goes to the ZMP-CoM controller too (getCoMPosition)
        if (a.filt_mask & 4) {
            const double cf = a.fb[2] * (cm + sc_p.x) + a.fa[2] * sc_p.y, vf = a.fb[2] * (v + sc_v.x) + a.fa[2] * sc_v.y;
            double* fd = a.filt_dst + i * kFiltRec + kFiltCom + 4 * j;
            st2(fd, cm, cf); st2(fd + 2, v, vf);
            cm = cf; v = vf;
        }
    }
    const double dcm = cm + v / a.omega;
    const double defL = fzL < 0.001 ? 0.0 : 1.0, defR = fzR < 0.001 ? 0.0 : 1.0;
    // the foot's ZMP in its sole frame (-ty / fz, tx / fz, 0), mapped to world by the sole's measured pose (undefined: the sole origin)
    const double zLx = defL != 0.0 ? -tyL / fzL : 0.0, zLy = defL != 0.0 ? txL / fzL : 0.0;
    const double zRx = defR != 0.0 ? -tyR / fzR : 0.0, zRy = defR != 0.0 ? txR / fzR : 0.0;
    const double* FL = S + S_FR;
    const double* FR = S + S_FR + 12;
    const double wL = FL[3 * j] * zLx + FL[3 * j + 1] * zLy + FL[9 + j];
    const double wR = FR[3 * j] * zRx + FR[3 * j + 1] * zRy + FR[9 + j];
    const double zmp = ((fzL * defL) / totalZ) * wL + ((fzR * defR) / totalZ) * wR;
    rec[2] = cm; rec[6] = dcm; rec[7] = zmp;
}

}  // namespace

namespace wcqp {
int sensor_feedback_enqueue(const wcqp_tick::SensorDev& a, hipStream_t stream) {
    const dim3 grid((unsigned)((a.batch + 3) / 4));
    if (a.filt_mask != 0) {
        if (!a.filt_src || !a.filt_dst) return WCQP_E_INVALID;
        if (a.rec) hipLaunchKernelGGL((tick_sensor_kernel<true, true>), grid, dim3(64), 0, stream, a);
        else hipLaunchKernelGGL((tick_sensor_kernel<false, true>), grid, dim3(64), 0, stream, a);
    } else if (a.rec) {
        hipLaunchKernelGGL((tick_sensor_kernel<true, false>), grid, dim3(64), 0, stream, a);
    } else {
        hipLaunchKernelGGL((tick_sensor_kernel<false, false>), grid, dim3(64), 0, stream, a);
    }
    WCQP_HIP_TRY(hipGetLastError());
    return WCQP_OK;
}

void lowpass_coeffs(double cut_hz, double Ts, double* fb, double* fa) {
    const double tau = 1.0 / (2.0 * M_PI * cut_hz);
    *fb = Ts / (2.0 * tau + Ts);
    *fa = (2.0 * tau - Ts) / (2.0 * tau + Ts);
}
}  // namespace wcqp
