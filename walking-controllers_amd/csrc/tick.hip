// Device-resident tick pipeline (BASELINE configs 4/5, SURVEY.md §8f-1 tick harness and
// §8f-2 MPC->IK glue).  See include/wcqp.h for the contract and oracle/tick_spec.py for the
// CPU restatement every number is checked against.  The handle is tick_handle.h's; what puts planned, generated, replanned or streamed
// trajectories into it, or reads them back, is tick_plan.hip.
//
// Reference call order reproduced (citations relative to /root/reference/modules/Walking_module):
//   src/WalkingModule.cpp:578-597   StableDCMModel::integrateModel        -> tick_glue_kernel (consumer)
//   src/WalkingModule.cpp:604-636   MPC bracket                           -> mpc_condensed_kernel
//   src/WalkingModule.cpp:638-656   reactive DCM controller (use_mpc 0)   -> tick_reactive_kernel (in-order forms), tick_react_* (skewed)
//   src/WalkingModule.cpp:657-662   ZMP gain scheduling (setPhase)        -> zmp_* (tick_device.h; zmp_gain_scheduling)
//   src/WalkingModule.cpp:657-695   WalkingZMPController + desired CoM    -> tick_glue_kernel
//   src/WalkingModule.cpp:709-740   IK bracket                            -> ik_kernel
//   src/WalkingModule.cpp:741-744   velocity integration                  -> tick_post_kernel
//   src/WalkingModule.cpp:816       advanceReferenceSignals               -> tick counter in HBM
#include <cmath>
#include <cstring>
#include <new>
#include <vector>
#include "tick_handle.h"
#include "sensors.h"

namespace {

using namespace wcqp_tick;

// GS (zmp_gain_scheduling): setPhase of the tick first - one step of the robot's gain smoother - and the law with its gains; d is a TickDevGS
template <bool GS>
__device__ __forceinline__ void tick_glue_robot(const TickDev& d) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.batch) return;
    const int t = d.tick2[d.phase];
    const int code = d.sel[i];
    const int st = d.mpc_status[i];
    const bool ok = st == WCQP_STATUS_SOLVED || st == WCQP_STATUS_OUTSIDE_HULL;
    if (!ok) d.mpc_fail[i] += 1;
    double2 kg = make_double2(0.0, 0.0);
    if constexpr (GS) kg = zmp_gains_tick(static_cast<const TickDevGS&>(d), i, t, true);
    double* s = d.state + (size_t)i * kStateLen;
    for (int ax = 0; ax < 2; ++ax) {
        double g_com;
        tick_glue_axis<GS>(d, i, t, ax, ok, d.u0[2 * i + ax], g_com, s[69 + ax], s[72 + ax], kg);
        if (!d.kin_mode) s[66 + ax] = g_com;
    }
    tick_glue_height(d, i, s);
    for (int k = 0; k < 6; ++k) tick_glue_twist(d, i, code, k, t, s[75 + k], s[81 + k]);
}
__global__ void tick_glue_kernel(TickDev d) { tick_glue_robot<false>(d); }
__global__ void tick_glue_gs_kernel(TickDevGS d) { tick_glue_robot<true>(d); }

__global__ void tick_post_kernel(TickDev d) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= d.batch * kDof) return;
    const int i = g / kDof;
    const int t = d.tick2[d.phase];
    const bool ok = d.ik_status[i] == WCQP_STATUS_SOLVED;
    tick_post_joint(d, i, t, g % kDof, ok, d.dq[g]);
    if (g % kDof == 0) tick_post_instance(d, i, t, ok);
    if (g == 0) d.tick2[1 - d.phase] = t + 1;      // advanceReferenceSignals (WalkingModule.cpp:816)
}

// the reactive DCM controller in the MPC launch's place (the in-order forms: the glue reads u0 / mpc_status as it does the MPC's):
// WalkingDCMReactiveController::evaluateControl (WM/src/WalkingDCMReactiveController.cpp:63-82) at the plant's DCM
__global__ void tick_reactive_kernel(TickDev d) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= d.batch * 2) return;
    const int i = g >> 1, ax = g & 1;
    const size_t w = ((size_t)i * d.traj_len + d.tick2[d.phase]) * 2 + ax;
    d.u0[g] = reactive_zmp(d, d.ref_traj[w], d.dcm_vel[w], d.dcm[g]);
    if (ax == 0) d.mpc_status[i] = WCQP_STATUS_SOLVED;
}

// the forward difference (ref[s + 1] - ref[s]) / dT of the stages [from, to) of every robot's reference: the DCM velocity of the
// reactive controller and of gain scheduling when none was uploaded, kept in step with wcqp_tick_splice_reference (stream order, behind the strided copy)
__global__ void tick_vel_diff_kernel(TickDev d, int from, int to) {
    const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int n = to - from;
    if (g >= (long)d.batch * n * 2) return;
    const long i = g / (2 * n);
    const int s = from + (int)((g / 2) % n), ax = (int)(g & 1);
    const size_t w = ((size_t)i * d.traj_len + s) * 2 + ax;
    const_cast<double*>(d.dcm_vel.get())[w] = (d.ref_traj[w + 2] - d.ref_traj[w]) / d.dT;
}

// external feedback: the caller's measured state into the places the next tick reads its plant state from - the skewed
// chain's per-axis records (mst: com [2], dcm [6], measured ZMP [7]) - and the measured joints into q_meas (NULL: the desired ones).
// A robot with a NaN or an Inf anywhere in its feedback is REJECTED by the rule of the sensor form (sensors.hip; include/wcqp.h): it keeps
// the measured state tick t - 1 used (the hand-off record of parity t - 1; tick 0: the uploaded state, with the desired joints), is
// counted in feedback_fail and stopped like a robot whose IK failed.  (A second call before the tick runs replaces the first: a robot it
// rejects keeps what the first call gave it, and feedback_fail counts calls.)  One thread per (robot, joint): each looks at the robot's whole
// feedback itself (29 values out of L2) - no exchange between threads that may sit in different workgroups.
__global__ void tick_feedback_kernel(TickDev d, const double* __restrict__ dcm, const double* __restrict__ com, const double* __restrict__ zmp,
                                     const double* __restrict__ q, double* __restrict__ q_meas, long long* __restrict__ feedback_fail, int t) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= d.batch * kDof) return;
    const int i = g / kDof, jj = g % kDof;
    bool ok = true;
    for (int k = 0; k < 2; ++k) ok = ok && isfinite(dcm[2 * i + k]) && isfinite(com[2 * i + k]) && isfinite(zmp[2 * i + k]);
    if (q) for (int k = 0; k < kDof; ++k) ok = ok && isfinite(q[(size_t)i * kDof + k]);
    if (!ok) {
        if (t == 0) q_meas[g] = d.q_des[g];
        if (jj < 2 && t > 0) {
            double* r = d.mst + ((size_t)i * 2 + jj) * 8;
            const double* hd = d.hand + ((size_t)((t - 1) & 1) * d.batch + i) * kHandLen;
            r[2] = hd[4 + jj]; r[6] = hd[6 + jj]; r[7] = hd[10 + jj];
        }
        if (jj == 0) {
            feedback_fail[i] += 1;
            if (d.ik_fail[i] == 0) d.ik_fail[i] = 1;
        }
        return;
    }
    q_meas[g] = q ? q[g] : d.q_des[g];
    if (jj < 2) {
        double* r = d.mst + ((size_t)i * 2 + jj) * 8;
        r[2] = com[2 * i + jj]; r[6] = dcm[2 * i + jj]; r[7] = zmp[2 * i + jj];
    }
}

}  // namespace

namespace wcqp {
// The gain smoother of zmp_gain_scheduling (include/wcqp.h): the third-order minimum-jerk approximation
//     H(s) = w / (s^3 + a2 s^2 + a1 s + w),   w = 150 / T^3, a2 = 9 / T, a1 = 60 / T^2   (unit DC gain),
// discretised with the bilinear (Tustin) transform s = K (1 - z^-1) / (1 + z^-1), K = 2 / dT.  The reference's smoother,
// iCub::ctrl::minJerkTrajGen, is upstream code outside the reference: this is the project's restatement, and the one place that
// defines it.  y[n] = sum_k nb[k] u[n - k] - sum_k na[k] y[n - 1 - k].
void zmp_smoother_coeffs(double T, double dT, double nb[4], double na[3]) {
    const double K = 2.0 / dT, K2 = K * K, K3 = K2 * K;
    const double a2 = 9.0 / T, a1 = 60.0 / (T * T), w = 150.0 / (T * T * T);
    // denominator K^3 (1 - z)^3 + a2 K^2 (1 - z)^2 (1 + z) + a1 K (1 - z)(1 + z)^2 + w (1 + z)^3, numerator w (1 + z)^3 (z = z^-1)
    const double d0 = K3 + a2 * K2 + a1 * K + w;
    const double d1 = -3.0 * K3 - a2 * K2 + a1 * K + 3.0 * w;
    const double d2 = 3.0 * K3 - a2 * K2 - a1 * K + 3.0 * w;
    const double d3 = -K3 + a2 * K2 - a1 * K + w;
    const double g = w / d0;
    nb[0] = g; nb[1] = 3.0 * g; nb[2] = 3.0 * g; nb[3] = g;
    na[0] = d1 / d0; na[1] = d2 / d0; na[2] = d3 / d0;
}
}  // namespace wcqp

namespace {

// zmp_gains_at (tick_device.h) on the host, operation for operation
void zmp_gains_host(const TickDev& d, const ZmpSched& z, double s, double* kg) {
#pragma clang fp contract(off)
    kg[0] = z.k_com_st + (d.k_com - z.k_com_st) * s;
    kg[1] = z.k_zmp_st + (d.k_zmp - z.k_zmp_st) * s;
}

// one launch sequence of n_inner ticks (n_inner <= ticks_per_launch, which is 1 unless the handle may run several) with
// the given phase (which copy of the tick index it reads: see TickDev::tick2)
int enqueue_tick(wcqp_tick_s* h, int phase, hipStream_t s, int n_inner = 1, int skip_last_mpc = 0) {
    TickDev d = h->d;
    d.phase = phase & 1;
    const int B = d.batch;
    const int N = wcqp::mpc_horizon(h->mpc);
    if (n_inner > h->ticks_per_launch) return WCQP_E_INVALID;
    if (h->position)
        return wcqp::position_tick_enqueue(static_cast<const TickDevPL*>(h->d_dev), h->pos, B, h->external, d.reactive != 0, d.gain_sched != 0, d.phase,
                                           n_inner, s);
    if (h->kin && !d.kin_fused) {
        h->kt.phase = d.phase;
        const int rck = wcqp::kin_enqueue_tick(h->kin, B, h->kt, d.q_des, h->J_left, h->J_right, h->J_neck, h->J_com, d.state, s);
        if (rck != WCQP_OK) return rck;
    }
    const wcqp_ik::IkIo io{h->J_left, h->J_right, h->J_neck, h->J_com, d.q_des, d.state, d.dq, d.ik_status, h->ik_lo, h->ik_up,
                           h->log_ferr, nullptr};
    // base-eliminated IK kernel: IK + post step of this tick and MPC + glue + plant of the NEXT one in ONE launch (skewed tick)
    if (h->form == TickForm::SKEWED)
        return wcqp_ik::ik4_launch_tick(wcqp::ik_device_params(h->ik), h->dpl(d), h->d_dev, h->variant, io, n_inner, skip_last_mpc, s);
    const bool gs = d.gain_sched != 0;
    if (d.reactive) {
        hipLaunchKernelGGL(tick_reactive_kernel, dim3((2 * B + 127) / 128), dim3(128), 0, s, d);
    } else {
        const int rc = wcqp::mpc_enqueue(h->mpc, B, d.dcm, d.ref_traj, N + 1, d.traj_len, d.tick2 + d.phase, d.u_prev,
                                         d.hull_tab_A, d.hull_tab_b, d.hull_tab_nc, d.hull_sets, d.hull_sets > 1 ? d.sel : nullptr,
                                         d.u0, d.mpc_status, h->mpc_active, h->mpc_margin, s);
        if (rc != WCQP_OK) return rc;
    }
    if (h->form == TickForm::MPC_IK16)
        return wcqp_ik::ik3_launch_tick(wcqp::ik_device_params(h->ik), h->dgs(d), io, s);
    if (gs) hipLaunchKernelGGL(tick_glue_gs_kernel, dim3((B + 127) / 128), dim3(128), 0, s, h->dgs(d));
    else hipLaunchKernelGGL(tick_glue_kernel, dim3((B + 127) / 128), dim3(128), 0, s, d);
    const int rc = wcqp_ik_solve_device(h->ik, B, io.JL, io.JR, io.JN, io.JC, io.q, io.state, io.dq, io.status, io.alo, io.aup, nullptr, nullptr, s);
    if (rc != WCQP_OK) return rc;
    hipLaunchKernelGGL(tick_post_kernel, dim3((B * kDof + 255) / 256), dim3(256), 0, s, d);
    WCQP_HIP_TRY(hipGetLastError());
    return WCQP_OK;
}

// The staging rows of wcqp_tick_set_feedback_host and of wcqp_tick_set_sensor_feedback_host, each array named once: the call lays out
// the caller's arrays, wcqp_tick_create the same rows with every array present (wcqp::stage_sizing) for the block's capacity
struct FeedbackStage {
    wcqp::HostStage st;
    wcqp::StageSlot<double> dcm, com, zmp, q;
    FeedbackStage(size_t B, const double* dcm_meas, const double* com_meas, const double* zmp_meas, const double* q_meas)
        : dcm(st.in(dcm_meas, B * 2)), com(st.in(com_meas, B * 2)), zmp(st.in(zmp_meas, B * 2)),
          q(st.in(q_meas, B * kDof, /*the joints are not fed back without it*/ true)) {}
};
struct SensorStage {
    wcqp::HostStage st;
    wcqp::StageSlot<double> q, dq, wl, wr;
    SensorStage(size_t B, const double* q_meas, const double* dq_meas, const double* wrench_left, const double* wrench_right)
        : q(st.in(q_meas, B * kDof)), dq(st.in(dq_meas, B * kDof)), wl(st.in(wrench_left, B * 6)), wr(st.in(wrench_right, B * 6)) {}
};

}  // namespace

// An option list as its values by key (0 where a key is absent).  What the list itself can be refused for - a negative count, a NULL list
// with a count, an unknown key, a key given twice - is refused here; what a VALUE can be refused for, by the rule of its key in create_tick
constexpr int kTickOptKeys = WCQP_TICK_OPT_POSITION_STREAMED;       // keys are 1 .. kTickOptKeys
struct TickOptions { int32_t value[kTickOptKeys + 1] = {}; };
static int parse_tick_options(const wcqp_tick_option* opts, int32_t n_opts, TickOptions* o) {
    if (n_opts < 0 || (n_opts > 0 && !opts)) return WCQP_E_INVALID;
    bool seen[kTickOptKeys + 1] = {};
    for (int32_t k = 0; k < n_opts; ++k) {
        const int32_t key = opts[k].key;
        if (key < 1 || key > kTickOptKeys || seen[key]) return WCQP_E_INVALID;
        seen[key] = true;
        o->value[key] = opts[k].value;
    }
    return WCQP_OK;
}

// the one body of wcqp_tick_create, wcqp_tick_create_ext and wcqp_tick_create_opts (which has refused a NULL params or out, and the list):
// every other refusal is stated here, once
static int create_tick(const wcqp_tick_params* params, const TickOptions& opt, wcqp_tick_t* out) {
    if (params->batch < 1 || params->max_ticks < 1) return WCQP_E_INVALID;
    if (params->step_ticks < 2 || params->ds_ticks < 0 || params->ds_ticks > params->step_ticks) return WCQP_E_INVALID;
    if (params->ik.dof != kDof) return WCQP_E_UNSUPPORTED;
    // ZMP gain scheduling: finite stance gains, a finite smoothing time > 0 (refused before anything touches the device)
    const bool gs = params->zmp_gain_scheduling != 0;
    if (params->zmp_gain_scheduling != 0 && params->zmp_gain_scheduling != 1) return WCQP_E_INVALID;
    if (gs && (!std::isfinite(params->k_com_stance) || !std::isfinite(params->k_zmp_stance) || !std::isfinite(params->zmp_smoothing_time) ||
               !(params->zmp_smoothing_time > 0.0)))
        return WCQP_E_INVALID;
    // planned trajectories: the fused-kinematics skewed tick of the default IK kernel and the internal plant, without logger rows (what can
    // be told from the parameters alone is refused here, before anything touches the device; the tree and the route below, before the
    // tick's allocations)
    const bool planned = params->planned_trajectories != 0;
    if (params->planned_trajectories != 0 && params->planned_trajectories != 1) return WCQP_E_INVALID;
    if (planned) {
        for (int k = 0; k < 9; ++k) if (!std::isfinite(params->neck_additional_rotation[k])) return WCQP_E_INVALID;
        const int alg = params->ik.algorithm;
        if (!params->use_kinematics || params->kin_handoff != WCQP_KIN_HANDOFF_FUSED || params->logger_ticks > 0 ||
            params->plant != WCQP_TICK_PLANT_INTERNAL || (alg != WCQP_IK_ALG_DEFAULT && alg != WCQP_IK_ALG_BASE_ELIM) ||
            (params->dcm_controller == WCQP_TICK_DCM_MPC && params->mpc.horizon >= kGainsLdsStages))
            return WCQP_E_UNSUPPORTED;
    }
    // streamed trajectories: the EXTERNAL plant's per-tick hand-over of the desired stage - the fused-kinematics skewed tick of the default
    // IK kernel without logger rows, and not a planned handle (refused here from the parameters, the tree and the route below)
    const bool streamed = params->streamed_trajectories != 0;
    if (params->streamed_trajectories != 0 && params->streamed_trajectories != 1) return WCQP_E_INVALID;
    if (streamed) {
        for (int k = 0; k < 9; ++k) if (!std::isfinite(params->neck_additional_rotation[k])) return WCQP_E_INVALID;
        const int alg = params->ik.algorithm;
        if (!params->use_kinematics || params->kin_handoff != WCQP_KIN_HANDOFF_FUSED || params->logger_ticks > 0 || planned ||
            params->plant != WCQP_TICK_PLANT_EXTERNAL || (alg != WCQP_IK_ALG_DEFAULT && alg != WCQP_IK_ALG_BASE_ELIM) ||
            (params->dcm_controller == WCQP_TICK_DCM_MPC && params->mpc.horizon >= kGainsLdsStages))
            return WCQP_E_UNSUPPORTED;
    }
    // the options: every key so far is a switch
    for (int key = 1; key <= kTickOptKeys; ++key) if (opt.value[key] != 0 && opt.value[key] != 1) return WCQP_E_INVALID;
    // a resident plan: a capability of a streamed handle
    const bool resident = opt.value[WCQP_TICK_OPT_RESIDENT_PLAN] != 0;
    if (resident && !streamed) return WCQP_E_UNSUPPORTED;
    // the POSITION mode: the problem's parameters by the rules of wcqp_prepare_create, then what the mode does not run with - a mode of a
    // planned handle with the internal plant or, with WCQP_TICK_OPT_POSITION_STREAMED, of a streamed handle (which the block above has
    // held to the EXTERNAL plant, the FUSED hand-off, no logger rows, the default IK algorithm and an MPC horizon below kGainsLdsStages)
    if (params->ik_mode != WCQP_TICK_IK_VELOCITY && params->ik_mode != WCQP_TICK_IK_POSITION) return WCQP_E_INVALID;
    const bool position = params->ik_mode == WCQP_TICK_IK_POSITION;
    const bool position_streamed = opt.value[WCQP_TICK_OPT_POSITION_STREAMED] != 0;
    if (position) {
        if (wcqp::prepare_check_scalars(&params->position_ik) != WCQP_OK || wcqp::prepare_check_arrays(&params->position_ik) != WCQP_OK) return WCQP_E_INVALID;
        const int alg = params->ik.algorithm;
        if (position_streamed ? !streamed : (!planned || streamed || params->plant != WCQP_TICK_PLANT_INTERNAL)) return WCQP_E_UNSUPPORTED;
        if (params->logger_ticks > 0 || (alg != WCQP_IK_ALG_DEFAULT && alg != WCQP_IK_ALG_BASE_ELIM)) return WCQP_E_UNSUPPORTED;
    }
    if (position_streamed && !position) return WCQP_E_UNSUPPORTED;
    // the sensor form's low-pass filters: a cut frequency > 0 switches one on - where there is a sensor form at all
    const double cuts[3] = {params->joint_velocity_cut_frequency, params->wrench_cut_frequency, params->com_cut_frequency};
    int filt_mask = 0;
    for (int k = 0; k < 3; ++k) {
        if (!std::isfinite(cuts[k]) || cuts[k] < 0.0) return WCQP_E_INVALID;
        if (cuts[k] > 0.0) filt_mask |= 1 << k;
    }
    if (filt_mask && (params->plant != WCQP_TICK_PLANT_EXTERNAL || !params->use_kinematics)) return WCQP_E_UNSUPPORTED;
    // the tick kernels address the handle's per-robot arrays with 32-bit offsets (wcqp::fits32; from the parameters alone, before anything
    // touches the device): the trajectories ref_traj / dcm_vel [B][max_ticks + N + 1][2], the two MPC -> IK hand-off records [2][B][kHandLen]
    // and the IK's arrays, J_left / J_right [B][6][29] the widest.  (The planned-trajectory records use 64-bit offsets.)
    if (!wcqp::fits32(params->batch, ((long long)params->max_ticks + (params->mpc.horizon > 0 ? params->mpc.horizon : 0) + 1) * 16) ||
        !wcqp::fits32(2ll * params->batch, kHandLen * 8) || !wcqp::ik_batch_fits32(params->batch))
        return WCQP_E_UNSUPPORTED;
    if (const int rcd = wcqp::require_device("tick pipeline"); rcd != WCQP_OK) return rcd;
    wcqp_tick_s* h = new (std::nothrow) wcqp_tick_s();
    if (!h) return WCQP_E_NOMEM;
    h->p = *params;
    const bool reactive = params->dcm_controller == WCQP_TICK_DCM_REACTIVE;
    if ((params->dcm_controller != WCQP_TICK_DCM_MPC && !reactive) || (reactive && !std::isfinite(params->k_dcm))) { delete h; return WCQP_E_INVALID; }
    // (a reactive handle keeps the MPC handle for the horizon and the LIPM's discretisation, without its condensed gains)
    int rc = wcqp_mpc_create(&params->mpc, &h->mpc);
    if (rc == WCQP_OK && position) {
        // `ik` is not read: the handle's velocity IK is a neutral one of the default kernel (nothing launches it; it carries the route)
        wcqp_ik_params neutral{};
        neutral.dof = params->ik.dof; neutral.use_com_as_constraint = 1; neutral.form = WCQP_IK_FORM_QPOASES;
        for (int k = 0; k < kDof; ++k) neutral.joint_reg_weights[k] = 1.0;      // (what the default route asks for: positive weights, W_neck > 0)
        for (int k = 0; k < 3; ++k) neutral.neck_weight[4 * k] = 1.0;
        rc = wcqp_ik_create(&neutral, &h->ik);
    } else if (rc == WCQP_OK) {
        rc = wcqp_ik_create(&params->ik, &h->ik);
    }
    if (rc == WCQP_OK && params->use_kinematics) {
        if (params->kin.dof != kDof) rc = WCQP_E_UNSUPPORTED;
        if (rc == WCQP_OK) rc = wcqp_kin_create(&params->kin, &h->kin);
    }
    if (rc == WCQP_OK && (planned || streamed)) {
        // planned / streamed trajectories where FUSED would not be taken - another IK route (CoM as a cost, say) or a tree the fused kernel cannot
        // walk: refused from the handles' host state, before any device allocation (the prepare calls below are the first)
        unsigned m3[3];
        int cs_ = 0, cd_ = 0, rounds = 0;
        std::vector<double> tab;
        if (wcqp::ik_route(h->ik) != wcqp::IkRoute::BASE_ELIM || !h->kin || !wcqp::kin_compact_layout(h->kin, m3, &cs_, &cd_) ||
            !wcqp::kin_fused_tables(h->kin, tab, &rounds))
            rc = WCQP_E_UNSUPPORTED;
    }
    wcqp::PrepareHost ptab;
    if (rc == WCQP_OK && position) rc = wcqp::prepare_host_tables(h->kin, &params->position_ik, &ptab);      // (the tree: refused above already)
    if (rc == WCQP_OK && h->kin) rc = wcqp::kin_prepare(h->kin);
    if (rc == WCQP_OK && !reactive) rc = wcqp::mpc_prepare(h->mpc);
    if (rc == WCQP_OK) rc = wcqp::ik_prepare(h->ik);
    if (rc != WCQP_OK) { wcqp_tick_destroy(h); return rc; }
    // the tick's Jacobians are MIXED free-floating ones (uploaded or from wcqp_kin_*): an instance that is not comes
    // back WCQP_STATUS_STRUCTURE and counts as an IK failure
    h->d.hot_start = params->ik_cold_start_only ? 0 : 1;
    if (params->ticks_per_launch < 0 || params->logger_ticks < 0) { wcqp_tick_destroy(h); return WCQP_E_INVALID; }
    if (params->plant != WCQP_TICK_PLANT_INTERNAL && params->plant != WCQP_TICK_PLANT_EXTERNAL) { wcqp_tick_destroy(h); return WCQP_E_INVALID; }
    h->external = params->plant == WCQP_TICK_PLANT_EXTERNAL;
    const wcqp::IkRoute route = wcqp::ik_route(h->ik);
    h->form = route == wcqp::IkRoute::BASE_ELIM ? TickForm::SKEWED : route == wcqp::IkRoute::NULLSPACE_16L ? TickForm::MPC_IK16 : TickForm::FOUR_LAUNCH;
    const size_t B = (size_t)params->batch;
    const int N = params->mpc.horizon;
    TickDev& d = h->d;
    d.batch = params->batch; d.first = params->first; d.traj_len = params->max_ticks + N + 1;
    d.log_ticks = params->log_ticks > 0 ? params->log_ticks : 0;
    d.step_ticks = params->step_ticks; d.ds_ticks = params->ds_ticks;
    d.inv_ss = d.step_ticks - d.ds_ticks > 0 ? 1.0 / (double)(d.step_ticks - d.ds_ticks) : 0.0;
    d.dT = params->mpc.sampling_time; d.k_com = params->k_com; d.k_zmp = params->k_zmp;
    d.noise = params->noise; d.seed = params->seed; d.com_height = params->mpc.com_height;
    d.omega = std::sqrt(params->mpc.gravity / params->mpc.com_height);
    wcqp::mpc_dynamics(h->mpc, &d.a, &d.b);
    double *ref = nullptr, *hA = nullptr, *hb = nullptr, *sw = nullptr;
    int *hn = nullptr, *ph = nullptr;
    rc = WCQP_OK;
#define A_(ptr, n) if (rc == WCQP_OK) rc = dev_alloc(h, &(ptr), (n))
#define STAGE_(blk, bytes) do { (blk).cap = (bytes); A_((blk).ptr, (blk).cap); } while (0)      // a host form's staging rows, sized by its layout
    const double* const any = wcqp::stage_sizing<double>();
    const size_t hsets = 3;       // rows for {left, right, both} in contact: uploaded, or (kinematics mode) built at upload from the desired foot poses
    A_(ref, B * d.traj_len * 2); A_(hA, B * hsets * 16); A_(hb, B * hsets * 8); A_(hn, B * hsets); A_(ph, B); A_(sw, B * 6);
    A_(d.dcm, B * 2); A_(d.com, B * 2); A_(d.zmp_meas, B * 2); A_(d.u_prev, B * 2); A_(d.u0, B * 2);
    A_(d.c_ref, B * 2); A_(d.v_ref, B * 2); A_(d.v_ref_prev, B * 2); A_(d.p_star, B * 2); A_(d.v_star_prev, B * 2);
    A_(d.q_des, B * kDof); A_(d.dq_prev, B * kDof); A_(d.dq, B * kDof);
    A_(d.sel, B);
    A_(d.state, B * kStateLen); A_(d.mpc_status, B); A_(d.ik_status, B); A_(d.mpc_fail, B); A_(d.ik_fail, B);
    A_(d.hot_try, B); A_(d.hot_hit, B);
    A_(d.tick2, 2); A_(d.u0_log, (size_t)d.log_ticks * B * 2); A_(d.dq_log, (size_t)d.log_ticks * B * kDof);
    A_(h->J_left, B * 6 * 29); A_(h->J_right, B * 6 * 29); A_(h->J_neck, B * 3 * 29); A_(h->J_com, B * 3 * 29);
    A_(h->mpc_active, B); A_(h->mpc_margin, B); A_(h->ik_lo, B); A_(h->ik_up, B);
    // skewed tick (base-eliminated fused kernel): state of the MPC chain, MPC -> IK hand-off, one live hull row set per robot
    d.skew = h->form == TickForm::SKEWED ? 1 : 0;

    double* jcomp = nullptr;
    unsigned cm[3] = {0u, 0u, 0u};
    int cstride = 0, coff_d = 0;
    if (params->kin_handoff < 0 || params->kin_handoff > 2) { wcqp_tick_destroy(h); return WCQP_E_INVALID; }
    const bool masks_ok = d.skew && h->kin && wcqp::kin_compact_layout(h->kin, cm, &cstride, &coff_d);
    // kinematics fused into the solve kernel (default), or a kinematics launch per tick handing over compact records / dense Jacobians
    std::vector<double> ktab;
    const bool fusedk = masks_ok && params->kin_handoff == WCQP_KIN_HANDOFF_FUSED && (reactive || N < kGainsLdsStages) &&
                        wcqp::kin_fused_tables(h->kin, ktab, &d.kin_rounds);
    const bool compact = masks_ok && !fusedk && params->kin_handoff != WCQP_KIN_HANDOFF_DENSE;
    // external feedback: the default (base-eliminated) kernel with constant Jacobians or fused kinematics, without logger rows
    if (h->external && (!d.skew || params->logger_ticks > 0 || (h->kin && !fusedk))) { wcqp_tick_destroy(h); return WCQP_E_UNSUPPORTED; }
    if ((planned || streamed) && (!d.skew || !fusedk)) { wcqp_tick_destroy(h); return WCQP_E_UNSUPPORTED; }      // (checked above, before any allocation)
    if (h->external) { A_(h->q_meas, B * kDof); d.q_meas = h->q_meas; STAGE_(h->fb_stage, FeedbackStage(B, any, any, any, any).st.total); A_(h->feedback_fail, B); }
    if (h->external && h->kin) {
        STAGE_(h->sens_stage, SensorStage(B, any, any, any, any).st.total);
        if (rc == WCQP_OK && hipEventCreateWithFlags(&h->run.done, hipEventDisableTiming) != hipSuccess) rc = WCQP_E_HIP;
        if (filt_mask) {
            A_(h->filt_state, 2 * B * kFiltRec);
            h->filt_mask = filt_mask;
            for (int k = 0; k < 3; ++k)
                if (filt_mask & (1 << k)) wcqp::lowpass_coeffs(cuts[k], params->mpc.sampling_time, &h->filt_fb[k], &h->filt_fa[k]);
        }
    }
    if (reactive) { d.reactive = 1; d.k_dcm = params->k_dcm; }
    // the DCM velocity: the reactive controller's input, and with gain scheduling the stance flag's (MPC handles then read it too)
    if (reactive || gs) { double* vel = nullptr; A_(vel, B * d.traj_len * 2); d.dcm_vel = vel; }
    if (gs) {
        d.gain_sched = 1;
        h->zg.k_com_st = params->k_com_stance; h->zg.k_zmp_st = params->k_zmp_stance;
        wcqp::zmp_smoother_coeffs(params->zmp_smoothing_time, params->mpc.sampling_time, h->zg.nb, h->zg.na);
        A_(h->zg.zs, B * 4);
    }
    if (planned) {
        // the records, [B][traj_len][kPlanRec] (64-bit sizes: 8192 robots x 1251 stages is 3.3 GB)
        double* rec = nullptr;
        A_(rec, B * (size_t)d.traj_len * kPlanRec);
        h->planned = true; h->pl.rec = rec; h->plan_rec = rec;
        for (int k = 0; k < 9; ++k) h->pl.neck_add[k] = params->neck_additional_rotation[k];
    }
    if (streamed) {
        // one record and one row set per robot, the pairs, the host form's staging rows
        A_(h->st_rec, B * kPlanRec); A_(h->st_set_A, B * 16); A_(h->st_set_b, B * 8); A_(h->st_set_nc, B); A_(h->st_pair, B * 2);
        STAGE_(h->des_stage, wcqp::desired_stage_bytes(B));
        h->streamed = true;
        h->pl.rec = h->st_rec; h->pl.set_A = h->st_set_A; h->pl.set_b = h->st_set_b; h->pl.set_nc = h->st_set_nc;
        for (int k = 0; k < 9; ++k) h->pl.neck_add[k] = params->neck_additional_rotation[k];
        // a resident plan beside them: the records of a planned handle, which only the plan's own kernels and the staging kernel address
        if (resident) { A_(h->plan_rec, B * (size_t)d.traj_len * kPlanRec); h->resident = true; }
    }
    if (d.skew) {
        A_(d.mst, B * 16); A_(d.hand, 2 * B * kHandLen); A_(d.live_A, B * 16); A_(d.live_b, B * 8); A_(d.live_nc, B); A_(d.sel_built, B);
        if (compact) A_(jcomp, B * (size_t)cstride);
        if (params->logger_ticks > 0) { A_(d.log_rows, (size_t)params->logger_ticks * B * kLoggerCols); d.logger_ticks = params->logger_ticks; }
        if (params->logger_ticks > 0 && !compact && !fusedk) A_(h->log_ferr, B * 12);      // (records: the kernel forms no foot errors)
        if (fusedk) {
            double* kt = nullptr;
            A_(kt, ktab.size());
            if (rc == WCQP_OK && hipMemcpy(kt, ktab.data(), ktab.size() * 8, hipMemcpyHostToDevice) != hipSuccess) rc = WCQP_E_HIP;
            d.kin_tab = kt;
        }
    }
    if (position) {
        // the model table and the parameter rows of the non-linear IK, the joint log and the iteration counters
        double* ptd = nullptr;
        const size_t nt = ptab.tab.size(), np = ptab.par.size();
        A_(ptd, nt + np); A_(h->pos.q_log, (size_t)d.log_ticks * B * kDof); A_(h->pos.ik_iters, B);
        if (rc == WCQP_OK && (hipMemcpy(ptd, ptab.tab.data(), nt * 8, hipMemcpyHostToDevice) != hipSuccess ||
                              hipMemcpy(ptd + nt, ptab.par.data(), np * 8, hipMemcpyHostToDevice) != hipSuccess))
            rc = WCQP_E_HIP;
        wcqp::PosTickDev& a = h->pos;
        a.kin_tab = ptd; a.par = ptd + nt; a.kin_rounds = ptab.kin_rounds;
        for (int k = 0; k < 3; ++k) a.pm[k] = ptab.pm[k];
        a.w_q = ptab.w_q; a.w_n = ptab.w_n; a.step_cap = ptab.step_cap; a.tol_step = ptab.tol_step; a.tol_c = ptab.tol_c;
        a.max_iter = ptab.max_iter; a.use_limits = ptab.use_limits;
        a.alo = h->ik_lo; a.aup = h->ik_up;
        h->position = true;
    }
#undef STAGE_
#undef A_
    if (rc != WCQP_OK) { wcqp_tick_destroy(h); return rc; }
    wcqp::mpc_device_consts(h->mpc, &d.mpc);
    d.horizon = N; d.hull_sets = (int)hsets;
    if (compact) { d.compact = 1; d.jcomp = jcomp; d.cmaskL = cm[0]; d.cmaskR = cm[1]; d.cmaskN = cm[2]; d.cstride = cstride; d.coff_d = coff_d; }
    if (fusedk) { d.kin_fused = 1; d.cmaskL = cm[0]; d.cmaskR = cm[1]; d.cmaskN = cm[2]; }
    // several ticks per launch: whenever a tick is ONE launch of the fused kernel (no kinematics launch in between), and not
    // with external feedback (a tick cannot run ahead of its feedback)
    const bool multi_tick = d.skew && (!h->kin || fusedk) && !h->external;
    h->ticks_per_launch = multi_tick ? (params->ticks_per_launch > 0 ? params->ticks_per_launch : (1 << 20)) : 1;
    if (h->kin) {
        double* h0 = nullptr;
        if (dev_alloc(h, &h0, B) != WCQP_OK) { wcqp_tick_destroy(h); return WCQP_E_NOMEM; }
        d.kin_mode = 1; d.com_h0 = h0;
        h->kt.tick2 = d.tick2; h->kt.phase0 = ph; h->kt.step_ticks = d.step_ticks;
        if (compact) { h->kt.jcomp = jcomp; h->kt.cstride = cstride; h->kt.coff_d = coff_d; }
    }
    d.ref_traj = ref; d.hull_tab_A = hA; d.hull_tab_b = hb; d.hull_tab_nc = hn; d.phase0 = ph; d.swing_twist = sw;
#ifdef WCQP_TICK_STAMPS
    if (d.skew && dev_alloc(h, &d.stamps, ((B + 3) / 4) * 16) != WCQP_OK) { wcqp_tick_destroy(h); return WCQP_E_NOMEM; }
#endif
    if (d.skew) {
        // the skewed kernels read the handle's TickDevPL behind the pointer, whatever the variant: the plain and reactive ones its TickDev,
        // the scheduled ones its TickDevGS
        TickDevPL* dp = nullptr;
        if (dev_alloc(h, &dp, 1) != WCQP_OK) { wcqp_tick_destroy(h); return WCQP_E_NOMEM; }
        const TickDevPL g = h->dpl(d);
        if (hipMemcpy(dp, &g, sizeof(TickDevPL), hipMemcpyHostToDevice) != hipSuccess) { wcqp_tick_destroy(h); return WCQP_E_HIP; }
        h->d_dev = dp;
        h->variant.jsrc = d.kin_fused ? 2 : d.compact ? 1 : 0;
        h->variant.log = d.logger_ticks > 0;
        h->variant.ext = d.q_meas && !h->variant.log;
        h->variant.react = d.reactive != 0; h->variant.gs = d.gain_sched != 0; h->variant.pl = h->planned || h->streamed;
    }
    *out = h;
    return WCQP_OK;
}

extern "C" {

int wcqp_tick_create(const wcqp_tick_params* params, wcqp_tick_t* out) { return wcqp_tick_create_ext(params, nullptr, out); }

int wcqp_tick_create_ext(const wcqp_tick_params* params, const wcqp_tick_params_ext* ext, wcqp_tick_t* out) {
    const wcqp_tick_option one{WCQP_TICK_OPT_RESIDENT_PLAN, ext ? ext->resident_plan : 0};
    return wcqp_tick_create_opts(params, &one, 1, out);
}

int wcqp_tick_create_opts(const wcqp_tick_params* params, const wcqp_tick_option* opts, int32_t n_opts, wcqp_tick_t* out) {
    if (!params || !out) return WCQP_E_INVALID;
    TickOptions opt;
    if (const int rc = parse_tick_options(opts, n_opts, &opt); rc != WCQP_OK) return rc;
    return create_tick(params, opt, out);
}

int wcqp_tick_get_option(wcqp_tick_t h, int32_t key, int32_t* value) {
    if (!h || !value) return WCQP_E_INVALID;
    if (key == WCQP_TICK_OPT_RESIDENT_PLAN) *value = h->resident ? 1 : 0;
    else if (key == WCQP_TICK_OPT_POSITION_STREAMED) *value = h->position && h->streamed ? 1 : 0;
    else if (key == WCQP_TICK_OPT_PLAN_SHIFT) *value = (int32_t)(h->plan_shift < INT32_MAX ? h->plan_shift : INT32_MAX);      // (reported only)
    else if (key == WCQP_TICK_OPT_PLAN_TIMED) *value = h->holds_plan() && h->uploaded && h->generated && h->gp.timed ? 1 : 0;      // (reported only)
    else if (key == WCQP_TICK_OPT_SWING_PROFILE) *value = h->holds_plan() && h->uploaded && h->generated && h->gp.shaped() ? 1 : 0;      // (reported only)
    else return WCQP_E_INVALID;
    return WCQP_OK;
}

int wcqp_tick_destroy(wcqp_tick_t h) {
    if (!h) return WCQP_E_INVALID;
    if (h->graph_exec) (void)hipGraphExecDestroy(h->graph_exec);
    if (h->graph) (void)hipGraphDestroy(h->graph);
    for (void* p : h->allocs) (void)hipFree(p);
    for (void* p : {(void*)h->set_A, (void*)h->set_b, (void*)h->set_nc}) if (p) (void)hipFree(p);
    for (StagedBlock* b : {&h->splice, &h->rp, &h->run}) b->release();
    h->goal.release();
    h->rebase.release();
    h->restart.release();
    for (hipEvent_t e : h->gen_ev) if (e) (void)hipEventDestroy(e);
    if (h->copy_stream) (void)hipStreamDestroy(h->copy_stream);
    if (h->kin) wcqp_kin_destroy(h->kin);
    if (h->mpc) wcqp_mpc_destroy(h->mpc);
    if (h->ik) wcqp_ik_destroy(h->ik);
    delete h;
    return WCQP_OK;
}

}  // extern "C"

// The tail both uploads share (wcqp_tick_upload, wcqp_tick_upload_footsteps), once the trajectories are in place: the state records of the
// chain, the pose block and joints, the initial DCM / CoM / command, the smoothers, filters and counters at rest, tick 0.  pair0 >= 0: the
// contact pair of stage 0 where `in` holds no contact array.
#define UP_(dst, src, n) WCQP_HIP_TRY(hipMemcpy(const_cast<void*>(static_cast<const void*>(dst)), (src), (n), hipMemcpyHostToDevice))
int wcqp::upload_state(wcqp_tick_s* h, const wcqp_tick_inputs* in, int pair0) {
    TickDev& d = h->d;
    const size_t B = (size_t)d.batch;
    if (d.skew) {
        // state of the MPC chain per axis: c_ref, v_ref_prev, com, u_prev (= measured ZMP), p_star, v_star_prev, dcm, spare
        std::vector<double> mst(B * 16, 0.0);
        for (size_t i = 0; i < B; ++i)
            for (int ax = 0; ax < 2; ++ax) {
                double* r = &mst[(i * 2 + ax) * 8];
                r[0] = in->com0[2 * i + ax]; r[2] = in->com0[2 * i + ax]; r[3] = in->u_init[2 * i + ax];
                r[4] = in->com0[2 * i + ax]; r[6] = in->dcm0[2 * i + ax]; r[7] = in->u_init[2 * i + ax];
            }
        WCQP_HIP_TRY(hipMemcpy(d.mst, mst.data(), B * 16 * 8, hipMemcpyHostToDevice));
        WCQP_HIP_TRY(hipMemset(d.sel_built, 0xff, B * 4));           // -1: every robot builds / copies its live rows at tick 0
        WCQP_HIP_TRY(hipMemset(d.live_nc, 0, B * 4));
    }
    if (h->kin) {
        std::vector<double> h0(B);
        for (size_t i = 0; i < B; ++i) h0[i] = in->state0[i * kStateLen + 68];       // desired CoM height = the initial one
        WCQP_HIP_TRY(hipMemcpy(const_cast<double*>(d.com_h0.get()), h0.data(), B * 8, hipMemcpyHostToDevice));
    } else {
        if (in->hull_tab_A && in->hull_tab_b && in->hull_tab_nc) {
            UP_(d.hull_tab_A, in->hull_tab_A, B * 3 * 128); UP_(d.hull_tab_b, in->hull_tab_b, B * 3 * 64); UP_(d.hull_tab_nc, in->hull_tab_nc, B * 3 * 4);
        }
        UP_(h->J_left, in->J_left, B * 6 * 29 * 8); UP_(h->J_right, in->J_right, B * 6 * 29 * 8);
        UP_(h->J_neck, in->J_neck, B * 3 * 29 * 8); UP_(h->J_com, in->J_com, B * 3 * 29 * 8);
    }
    UP_(d.state, in->state0, B * kStateLen * 8); UP_(d.q_des, in->q0, B * kDof * 8);
    if (h->kin && !h->planned && !h->streamed) {     // (planned / streamed: the live rows are built from the records at the first tick - sel_built = -1)
        // setConvexHullConstraint (...PredictiveController.cpp:364-435) for the three contact pairs, from the DESIRED foot
        // poses just uploaded (the planned footsteps, WalkingModule.cpp:609-613): the MPC of a tick selects its rows by the pair
        const int rch = wcqp::hull_tables_from_state((int)B, h->p.foot_rect, d.state, kStateLen, const_cast<double*>(d.hull_tab_A.get()),
                                                     const_cast<double*>(d.hull_tab_b.get()), const_cast<int*>(d.hull_tab_nc.get()), nullptr);
        if (rch != WCQP_OK) return rch;
        WCQP_HIP_TRY(hipDeviceSynchronize());
    }
    UP_(d.dcm, in->dcm0, B * 16); UP_(d.com, in->com0, B * 16); UP_(d.c_ref, in->com0, B * 16); UP_(d.p_star, in->com0, B * 16);
    UP_(d.zmp_meas, in->u_init, B * 16); UP_(d.u_prev, in->u_init, B * 16);
    WCQP_HIP_TRY(hipMemset(d.v_ref_prev, 0, B * 16)); WCQP_HIP_TRY(hipMemset(d.v_star_prev, 0, B * 16));
    // the gain smoothers at rest at the stance gains (WalkingZMPController::initialize): s = 0, state 0
    if (d.gain_sched) WCQP_HIP_TRY(hipMemset(h->zg.zs, 0, B * 32));
    WCQP_HIP_TRY(hipMemset(d.dq_prev, 0, B * kDof * 8)); WCQP_HIP_TRY(hipMemset(d.tick2, 0, 8));
    {   // contact pair of tick 0 (later ticks: tick_post_kernel)
        std::vector<int> sel(B);
        for (size_t i = 0; i < B; ++i) {
            if (pair0 >= 0) { sel[i] = pair0; continue; }                 // (a generated plan: stage 0 is a double support)
            if (h->planned) { sel[i] = (int)(in->contact[i * d.traj_len] & 3u) - 1; continue; }
            if (h->streamed) { sel[i] = 2; continue; }      // (the skewed kernels take the pair from the stage's record)
            const int cyc = in->phase0[i] % (2 * d.step_ticks), sidx = cyc % d.step_ticks;
            sel[i] = sidx < d.ds_ticks ? 2 : cyc / d.step_ticks;
        }
        WCQP_HIP_TRY(hipMemcpy(d.sel, sel.data(), B * 4, hipMemcpyHostToDevice));
    }
    WCQP_HIP_TRY(hipMemset(d.mpc_fail, 0, B * 8)); WCQP_HIP_TRY(hipMemset(d.ik_fail, 0, B * 8));
    WCQP_HIP_TRY(hipMemset(d.hot_try, 0, B * 8)); WCQP_HIP_TRY(hipMemset(d.hot_hit, 0, B * 8));
    WCQP_HIP_TRY(hipMemset(h->ik_lo, 0, B * 4)); WCQP_HIP_TRY(hipMemset(h->ik_up, 0, B * 4));      // no previous active set at tick 0
    if (h->feedback_fail) WCQP_HIP_TRY(hipMemset(h->feedback_fail, 0, B * 8));
    if (h->position) WCQP_HIP_TRY(hipMemset(h->pos.ik_iters, 0, B * 8));
    if (h->filt_state) {
        // the filters at rest: the CoM position filter AT com0 and its velocity filter at 0 (the reference starts them at (0, 0, com_height)
        // and 0 once, WM/src/WalkingForwardKinematics.cpp:153-160: its robot stands at the origin); the joint-velocity and wrench filters
        // start at the first reading (RobotHelper::resetFilters), which the first sensor call is told
        std::vector<double> fs(B * kFiltRec, 0.0);
        for (size_t i = 0; i < B; ++i)
            for (int ax = 0; ax < 2; ++ax) fs[i * kFiltRec + kFiltCom + 4 * ax] = fs[i * kFiltRec + kFiltCom + 4 * ax + 1] = in->com0[2 * i + ax];
        WCQP_HIP_TRY(hipMemcpy(h->filt_state, fs.data(), B * kFiltRec * 8, hipMemcpyHostToDevice));
        WCQP_HIP_TRY(hipMemset(h->filt_state + B * kFiltRec, 0, B * kFiltRec * 8));
        h->filt_cur = 0; h->filt_started = false; h->filt_pending = false;
    }
    if (h->external) {
        h->meas0.resize(B * 6);
        for (size_t i = 0; i < B; ++i)
            for (int ax = 0; ax < 2; ++ax) {
                h->meas0[i * 6 + ax] = in->dcm0[2 * i + ax]; h->meas0[i * 6 + 2 + ax] = in->com0[2 * i + ax]; h->meas0[i * 6 + 4 + ax] = in->u_init[2 * i + ax];
            }
    }
    // (hipMemset does not wait, and the copies / kernels above ran on the NULL stream: the run call that follows may name a non-blocking
    // stream - wcqp_stream_create makes such - which would not wait for them either)
    WCQP_HIP_TRY(hipDeviceSynchronize());
    h->uploaded = true;
    h->ticks_enqueued = 0;
    h->plan_shift = 0;
    h->phase = 0;
    h->feedback_set = false;
    h->desired_set = false; h->plan_staged = false;
    h->run.pending = false;
    // (the device was synchronised above: nothing of a goal, rebase or restart call before this upload is owed or on its way any more,
    // and wcqp_tick_get_restart_result has no call of this upload to report)
    h->goal.pending = false; h->goal.owed.clear(); h->rebase.pending = false;
    h->restart.pending = false; h->restart.owed.clear(); h->restart.called = false;
    return WCQP_OK;
}

extern "C" {


int wcqp_tick_upload(wcqp_tick_t h, const wcqp_tick_inputs* in) {
    if (!h || !in) return WCQP_E_INVALID;
    // (planned trajectories: no synthetic gait - phase0 and swing_twist may be NULL)
    if (!in->ref_traj || !in->state0 || !in->q0 || !in->dcm0 || !in->com0 || !in->u_init) return WCQP_E_INVALID;
    if (!h->planned && !h->streamed && (!in->phase0 || !in->swing_twist)) return WCQP_E_INVALID;
    if (h->holds_plan()) { const int rcv = wcqp::validate_plan(h, in); if (rcv != WCQP_OK) return rcv; }
    if (!h->kin && (!in->J_left || !in->J_right || !in->J_neck || !in->J_com)) return WCQP_E_INVALID;
    // (the reactive controller reads no hull rows)
    if (!h->kin && !h->d.reactive && (!in->hull_tab_A || !in->hull_tab_b || !in->hull_tab_nc)) return WCQP_E_INVALID;
    TickDev& d = h->d;
    const size_t B = (size_t)d.batch;
    // Non-finite inputs (include/wcqp.h): a NaN or an Inf in the reference trajectory (and its velocity), the initial DCM / CoM / command or
    // the initial joints would enter a robot's state on the first tick that reads it and never leave: refused here, before anything of
    // the handle changes (a handle uploaded before keeps that upload)
    {
        auto finite = [](const double* a, size_t n) { bool ok = true; for (size_t k = 0; k < n; ++k) ok = ok && std::isfinite(a[k]); return ok; };
        if (!finite(in->ref_traj, B * d.traj_len * 2) || !finite(in->dcm0, B * 2) || !finite(in->com0, B * 2) || !finite(in->u_init, B * 2) ||
            !finite(in->q0, B * kDof) || ((d.reactive || d.gain_sched) && in->dcm_vel_traj && !finite(in->dcm_vel_traj, B * d.traj_len * 2)))
            return WCQP_E_INVALID;
    }
    // from here on the device state changes: a call that fails on the way leaves the handle unrunnable until the next good upload
    h->uploaded = false;
    WCQP_HIP_TRY(hipDeviceSynchronize());
    UP_(d.ref_traj, in->ref_traj, B * d.traj_len * 16);
    if (d.reactive || d.gain_sched) {
        // the planner's DCM velocity, or the forward difference (ref[t + 1] - ref[t]) / dT (the last stage, which no tick reads: 0)
        h->vel_explicit = in->dcm_vel_traj != nullptr;
        if (h->vel_explicit) {
            UP_(d.dcm_vel, in->dcm_vel_traj, B * d.traj_len * 16);
        } else {
            std::vector<double> vel(B * d.traj_len * 2, 0.0);
            for (size_t i = 0; i < B; ++i)
                for (size_t k = 0; k + 1 < (size_t)d.traj_len; ++k)
                    for (int ax = 0; ax < 2; ++ax) {
                        const size_t w = (i * d.traj_len + k) * 2 + ax;
                        vel[w] = (in->ref_traj[w + 2] - in->ref_traj[w]) / d.dT;
                    }
            UP_(d.dcm_vel, vel.data(), B * d.traj_len * 16);
        }
    }
    if (h->holds_plan()) {
        const int rcp = wcqp::upload_plan(h, in);
        if (rcp != WCQP_OK) return rcp;
        h->generated = false;
    }
    if (h->streamed) { const int rcs = wcqp::reset_streamed_stage(h); if (rcs != WCQP_OK) return rcs; }
    if (h->holds_plan() || h->streamed) {
        WCQP_HIP_TRY(hipMemset(const_cast<int*>(d.phase0.get()), 0, B * 4));
        WCQP_HIP_TRY(hipMemset(const_cast<double*>(d.swing_twist.get()), 0, B * 48));
    } else {
        UP_(d.phase0, in->phase0, B * 4); UP_(d.swing_twist, in->swing_twist, B * 48);
    }
    return wcqp::upload_state(h, in, -1);
}
#undef UP_

// what both forms of wcqp_tick_set_feedback_* ask before they touch anything
static int feedback_ready(const wcqp_tick_s* h, const double* dcm_meas, const double* com_meas, const double* zmp_meas) {
    if (!h || !dcm_meas || !com_meas || !zmp_meas) return WCQP_E_INVALID;
    if (!h->external) return WCQP_E_UNSUPPORTED;
    if (!h->uploaded) return WCQP_E_INVALID;
    return WCQP_OK;
}

int wcqp_tick_set_feedback_device(wcqp_tick_t h, const double* dcm_meas, const double* com_meas, const double* zmp_meas, const double* q_meas, void* stream) {
    if (const int rc = feedback_ready(h, dcm_meas, com_meas, zmp_meas); rc != WCQP_OK) return rc;
    const int n = h->d.batch * kDof;
    hipLaunchKernelGGL(tick_feedback_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, h->d, dcm_meas, com_meas, zmp_meas, q_meas, h->q_meas,
                       h->feedback_fail, h->ticks_for_handoff());
    WCQP_HIP_TRY(hipGetLastError());
    h->feedback_set = true;
    h->filt_pending = false;      // (this tick supplies the filters no sample: they hold, whatever a replaced sensor call computed)
    return WCQP_OK;
}

int wcqp_tick_set_feedback_host(wcqp_tick_t h, const double* dcm_meas, const double* com_meas, const double* zmp_meas, const double* q_meas) {
    if (const int rc = feedback_ready(h, dcm_meas, com_meas, zmp_meas); rc != WCQP_OK) return rc;
    // (a wcqp_tick_reset_robots call on a non-blocking stream re-records the run's event behind its kernels: wait for them, as the sensor form does)
    if (const int rc = h->run.wait(); rc != WCQP_OK) return rc;
    FeedbackStage s((size_t)h->d.batch, dcm_meas, com_meas, zmp_meas, q_meas);
    // (synchronous copies on the NULL stream: they wait for what the handle's last tick left running on a blocking stream, and the
    // host arrays are consumed when they return)
    int rc = s.st.upload(h->fb_stage.ptr, h->fb_stage.cap);
    if (rc == WCQP_OK) rc = wcqp_tick_set_feedback_device(h, s.st[s.dcm], s.st[s.com], s.st[s.zmp], s.st[s.q], nullptr);
    if (rc != WCQP_OK) return rc;
    // the copy kernel ran on the NULL stream; the tick that consumes the feedback may be enqueued on ANY stream - a non-blocking one
    // (wcqp_stream_create) would not wait for it - so the feedback is in place when this call returns, and the staging rows are free
    WCQP_HIP_TRY(hipStreamSynchronize(nullptr));
    return WCQP_OK;
}

// ... and both forms of wcqp_tick_set_sensor_feedback_*
static int sensor_feedback_ready(const wcqp_tick_s* h, const double* q_meas, const double* dq_meas, const double* wrench_left, const double* wrench_right) {
    if (!h || !q_meas || !dq_meas || !wrench_left || !wrench_right) return WCQP_E_INVALID;
    if (!h->external || !h->kin || !h->feedback_fail) return WCQP_E_UNSUPPORTED;
    if (!h->uploaded) return WCQP_E_INVALID;
    if (h->streamed && !h->desired_set) return WCQP_E_INVALID;       // (the anchor is tick t's stage: wcqp_tick_set_desired_* goes first)
    return WCQP_OK;
}

int wcqp_tick_set_sensor_feedback_device(wcqp_tick_t h, const double* q_meas, const double* dq_meas, const double* wrench_left,
                                         const double* wrench_right, void* stream) {
    if (const int rc = sensor_feedback_ready(h, q_meas, dq_meas, wrench_left, wrench_right); rc != WCQP_OK) return rc;
    const TickDev& d = h->d;
    SensorDev a{};
    a.q = q_meas; a.dq = dq_meas; a.wl = wrench_left; a.wr = wrench_right;
    a.q_des = d.q_des; a.state = d.state; a.phase0 = d.phase0; a.kin_tab = d.kin_tab;
    a.mst = d.mst; a.hand = d.hand; a.q_meas = h->q_meas; a.ik_fail = d.ik_fail; a.feedback_fail = h->feedback_fail;
    a.batch = d.batch; a.t = h->ticks_for_handoff(); a.step_ticks = d.step_ticks; a.kin_rounds = d.kin_rounds; a.omega = d.omega;
    a.rec = h->streamed ? h->st_rec : nullptr;
    if (h->filt_mask) {
        const size_t slot = (size_t)d.batch * kFiltRec;
        a.filt_src = h->filt_state + (size_t)h->filt_cur * slot; a.filt_dst = h->filt_state + (size_t)(h->filt_cur ^ 1) * slot;
        a.filt_mask = h->filt_mask; a.filt_first = h->filt_started ? 0 : 1;
        for (int k = 0; k < 3; ++k) { a.fb[k] = h->filt_fb[k]; a.fa[k] = h->filt_fa[k]; }
    }
    const int rc = wcqp::sensor_feedback_enqueue(a, (hipStream_t)stream);
    if (rc != WCQP_OK) return rc;
    h->feedback_set = true;
    h->filt_pending = h->filt_mask != 0;
    return WCQP_OK;
}

int wcqp_tick_set_sensor_feedback_host(wcqp_tick_t h, const double* q_meas, const double* dq_meas, const double* wrench_left,
                                       const double* wrench_right) {
    if (const int rc = sensor_feedback_ready(h, q_meas, dq_meas, wrench_left, wrench_right); rc != WCQP_OK) return rc;
    // the last run may have been enqueued on a non-blocking stream, which the NULL stream below does not wait for: wait for its end
    if (const int rc = h->run.wait(); rc != WCQP_OK) return rc;
    SensorStage s((size_t)h->d.batch, q_meas, dq_meas, wrench_left, wrench_right);
    int rc = s.st.upload(h->sens_stage.ptr, h->sens_stage.cap);
    if (rc == WCQP_OK) rc = wcqp_tick_set_sensor_feedback_device(h, s.st[s.q], s.st[s.dq], s.st[s.wl], s.st[s.wr], nullptr);
    if (rc != WCQP_OK) return rc;
    // in place when this call returns: the tick may be enqueued on any stream, and the staging rows are free for the next call
    WCQP_HIP_TRY(hipStreamSynchronize(nullptr));
    return WCQP_OK;
}

int wcqp_tick_run(wcqp_tick_t h, int32_t n_ticks, int32_t use_graph, void* stream) {
    if (!h || n_ticks < 0 || !h->uploaded) return WCQP_E_INVALID;
    // the trajectories hold max_ticks + N + 1 stages per instance: a tick beyond that would read its neighbour's
    if ((long)h->ticks_enqueued + n_ticks > (long)h->p.max_ticks) return WCQP_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    if (n_ticks == 0) return WCQP_OK;
    if (h->external && (n_ticks != 1 || !h->feedback_set)) return WCQP_E_INVALID;      // one tick per call, each behind its own feedback
    if (h->streamed && !h->desired_set) return WCQP_E_INVALID;                          // ... and, streamed, behind its own desired stage
    int left = n_ticks;
    // Everything that can be refused on the host is refused BEFORE anything is enqueued (the prime launch below already advances
    // the MPC chain); an enqueue that fails after that leaves device state nobody can name - the handle then wants a new upload.
    struct NeedsUpload { wcqp_tick_s* h; bool armed = true; ~NeedsUpload() { if (armed) h->uploaded = false; } } guard{h};
    if (h->d.skew && (!h->d_dev || !h->d.mst || !h->d.hand)) { guard.armed = false; return WCQP_E_INVALID; }
    const bool skewed = h->d.skew && !h->position;     // (a POSITION handle keeps the skewed handle's records, but runs every tick in order)
    if (skewed) {
        // the fused launch of tick t carries IK(t) and MPC(t+1): the MPC of the call's first tick goes first, on its own, and
        // the call's LAST tick does not run the MPC of the tick after it - between calls nothing is ahead of anything
        const int rc = wcqp_ik::ik4_launch_tick_prime(h->dpl(h->d), h->variant, h->ticks_enqueued, s);
        if (rc != WCQP_OK) return rc;
    }
    // the fused kernel walks through several ticks per launch (the waves need no per-tick synchronisation): no graph needed
    if (h->ticks_per_launch > 1) {
        while (left > 0) {
            const int k = left < h->ticks_per_launch ? left : h->ticks_per_launch;
            const int rc = enqueue_tick(h, h->phase, s, k, k == left ? 1 : 0);
            if (rc != WCQP_OK) return rc;
            h->phase ^= 1; h->ticks_enqueued += k; left -= k;
        }
        guard.armed = false;
        return WCQP_OK;
    }
    if (skewed) left -= 1;      // the last tick of the call is a plain launch of its own (below)
    // kGraphTicks ticks per graph (the tick index lives in HBM, so the graph is tick-invariant): one
    // hipGraphLaunch costs about as much as four plain launches.  The graph is captured with phases 0, 1, 0, ...
    // and therefore replayed only from phase 0; from phase 1 a plain tick goes first.
    constexpr int kGraphTicks = 8;
    auto plain = [&]() -> int {
        const int rc = enqueue_tick(h, h->phase, s);
        if (rc == WCQP_OK) { h->phase ^= 1; ++h->ticks_enqueued; --left; }
        return rc;
    };
    if (use_graph && left >= kGraphTicks + 1 && h->phase) { const int rc = plain(); if (rc != WCQP_OK) return rc; }
    if (use_graph && !h->graph_exec && left >= kGraphTicks) {
        hipStream_t cs = nullptr;
        WCQP_HIP_TRY(hipStreamCreate(&cs));
        // (lazy device state of the solver handles exists since create: capture forbids allocations)
        WCQP_HIP_TRY(hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal));
        int rc = WCQP_OK;
        for (int k = 0; k < kGraphTicks && rc == WCQP_OK; ++k) rc = enqueue_tick(h, k & 1, cs);
        hipGraph_t g = nullptr;
        const hipError_t e = hipStreamEndCapture(cs, &g);
        (void)hipStreamDestroy(cs);
        if (rc != WCQP_OK) { if (g) (void)hipGraphDestroy(g); return rc; }
        if (e != hipSuccess || !g) return WCQP_E_HIP;
        h->graph = g;
        WCQP_HIP_TRY(hipGraphInstantiate(&h->graph_exec, h->graph, nullptr, nullptr, 0));
    }
    if (use_graph && h->graph_exec && !h->phase) {
        for (; left >= kGraphTicks; left -= kGraphTicks, h->ticks_enqueued += kGraphTicks) WCQP_HIP_TRY(hipGraphLaunch(h->graph_exec, s));
    }
    while (left > 0) { const int rc = plain(); if (rc != WCQP_OK) return rc; }
    if (skewed) {
        const int rc = enqueue_tick(h, h->phase, s, 1, 1);
        if (rc != WCQP_OK) return rc;
        h->phase ^= 1; ++h->ticks_enqueued;
    }
    if (h->run.done) { if (const int rc = h->run.guard(s); rc != WCQP_OK) return rc; }    // (sensor feedback: the host form waits for it)
    guard.armed = false;
    h->feedback_set = false;
    h->desired_set = false; h->plan_staged = false;
    // the tick consumed a sensor reading: what that call wrote is the filters' state from here on
    if (h->filt_pending) { h->filt_cur ^= 1; h->filt_started = true; h->filt_pending = false; }
    return WCQP_OK;
}

int wcqp_tick_splice_reference(wcqp_tick_t h, int32_t from_tick, int32_t n_stages, const double* ref_tail, void* stream) {
    if (!h || !h->uploaded || !ref_tail || n_stages < 1) return WCQP_E_INVALID;
    if (h->planned) return WCQP_E_UNSUPPORTED;           // (planned trajectories: the splice has no tail for the feet)
    const TickDev& d = h->d;
    // stages the ticks already enqueued have consumed as their own reference DCM stay as they are; everything a later
    // tick's window can see may change
    if (from_tick < h->ticks_enqueued || (long)from_tick + n_stages > (long)d.traj_len) return WCQP_E_INVALID;
    if (h->vel_explicit) return WCQP_E_UNSUPPORTED;      // (uploaded velocities - reactive controller, gain scheduling: the splice has no tail for them)
    for (size_t k = 0; k < (size_t)d.batch * (size_t)n_stages * 2; ++k) if (!std::isfinite(ref_tail[k])) return WCQP_E_INVALID;      // (as the upload: no NaN / Inf into the reference)
    // `ref_tail` is the caller's HOST memory and the copy below is ordered behind ticks that may still run for a long time: the
    // rows are therefore taken NOW - staged into device memory of the handle on a copy stream of its own, waited for before
    // this call returns - and the caller may release `ref_tail` as soon as it has.
    const size_t bytes = (size_t)d.batch * (size_t)n_stages * 16;
    if (const int rc = h->splice.take(h->copy_stream, ref_tail, bytes, bytes); rc != WCQP_OK) return rc;      // (waits until the previous merge has left the staging rows)
    // strided copy: row i of the tail goes to stages [from_tick, from_tick + n_stages) of instance i, in stream order
    // behind the ticks already enqueued (the trajectory pointer the kernels - and any captured graph - hold does not change)
    WCQP_HIP_TRY(hipMemcpy2DAsync(const_cast<double*>(d.ref_traj.get()) + (size_t)from_tick * 2, (size_t)d.traj_len * 16, h->splice.mem.ptr, (size_t)n_stages * 16,
                                  (size_t)n_stages * 16, (size_t)d.batch, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    if (d.reactive || d.gain_sched) {
        // the forward difference of the stages the new ones touch: [from_tick - 1, from_tick + n_stages), the last stage excepted
        const int lo = from_tick > 0 ? from_tick - 1 : 0, hi = from_tick + n_stages < d.traj_len ? from_tick + n_stages : d.traj_len - 1;
        if (hi > lo) {
            const long n = (long)d.batch * (hi - lo) * 2;
            hipLaunchKernelGGL(tick_vel_diff_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d, lo, hi);
            WCQP_HIP_TRY(hipGetLastError());
        }
    }
    return h->splice.guard((hipStream_t)stream);
}

#ifdef WCQP_TICK_STAMPS
// diagnostic builds only: the phase stamps of every workgroup's last tick ([workgroups][16])
int wcqp_tick_debug_stamps(wcqp_tick_t h, unsigned long long* out, int32_t n) {
    if (!h || !out || !h->d.stamps || n > ((h->d.batch + 3) / 4) * 16) return WCQP_E_INVALID;
    WCQP_HIP_TRY(hipDeviceSynchronize());
    WCQP_HIP_TRY(hipMemcpy(out, h->d.stamps, (size_t)n * 8, hipMemcpyDeviceToHost));
    return WCQP_OK;
}
#endif

int wcqp_tick_get_info(wcqp_tick_t h, wcqp_tick_info* out) {
    if (!h || !out) return WCQP_E_INVALID;
    const TickDev& d = h->d;
    out->kin_handoff = !h->kin ? -1 : d.kin_fused ? WCQP_KIN_HANDOFF_FUSED : d.compact ? WCQP_KIN_HANDOFF_COMPACT : WCQP_KIN_HANDOFF_DENSE;
    out->ticks_per_launch = h->ticks_per_launch;
    out->dcm_controller = d.reactive ? WCQP_TICK_DCM_REACTIVE : WCQP_TICK_DCM_MPC;
    out->zmp_gain_scheduling = d.gain_sched ? 1 : 0;
    out->planned_trajectories = h->planned ? 1 : 0;
    out->streamed_trajectories = h->streamed ? 1 : 0;
    out->sensor_filters = h->filt_mask;
    out->plan_generated = h->holds_plan() && h->uploaded && h->generated ? 1 : 0;
    out->plan_record_ms = out->plan_generated ? (double)h->gen_record_ms : 0.0;
    out->ik_mode = h->position ? WCQP_TICK_IK_POSITION : WCQP_TICK_IK_VELOCITY;
    // a kinematics launch unless fused; then the skewed kernel (1), MPC / reactive + the 16-lane kernel (2) or controller, glue, IK, post (4)
    out->launches_per_tick = (h->kin && !d.kin_fused ? 1 : 0) + (h->form == TickForm::SKEWED ? 1 : h->form == TickForm::MPC_IK16 ? 2 : 4);
    return WCQP_OK;
}

int wcqp_tick_get_info_ext(wcqp_tick_t h, wcqp_tick_info_ext* out) {
    if (!h || !out) return WCQP_E_INVALID;
    out->resident_plan = h->resident ? 1 : 0;
    return WCQP_OK;
}

int wcqp_tick_download(wcqp_tick_t h, const wcqp_tick_outputs* out) {
    if (!h || !out) return WCQP_E_INVALID;
    if ((out->measured || out->feedback_fail) && !h->external) return WCQP_E_UNSUPPORTED;
    if ((out->q_log || out->ik_iters) && !h->position) return WCQP_E_UNSUPPORTED;
    if (out->dq_log && h->position) return WCQP_E_UNSUPPORTED;          // (a POSITION handle forms no velocity)
    const TickDev& d = h->d;
    const size_t B = (size_t)d.batch;
    WCQP_HIP_TRY(hipDeviceSynchronize());
#define DN_(dst, src, n) if (dst) WCQP_HIP_TRY(hipMemcpy((dst), (src), (n), hipMemcpyDeviceToHost))
    DN_(out->u0_log, d.u0_log, (size_t)d.log_ticks * B * 16); DN_(out->dq_log, d.dq_log, (size_t)d.log_ticks * B * kDof * 8);
    DN_(out->q_des, d.q_des, B * kDof * 8);
    if (h->position) { DN_(out->q_log, h->pos.q_log, (size_t)d.log_ticks * B * kDof * 8); DN_(out->ik_iters, h->pos.ik_iters, B * 8); }
    DN_(out->active_lower, h->ik_lo, B * 4); DN_(out->active_upper, h->ik_up, B * 4);
    if (out->logger) {
        if (!d.log_rows) return WCQP_E_UNSUPPORTED;          // logger_ticks = 0, or an IK algorithm without the fused tick kernel
        WCQP_HIP_TRY(hipMemcpy(out->logger, d.log_rows, (size_t)d.logger_ticks * B * kLoggerCols * 8, hipMemcpyDeviceToHost));
    }
    if (d.skew) {
        // the state of the MPC chain lives in per-axis records (TickDev::mst): com at [2], dcm at [6]
        if (out->dcm || out->com) {
            std::vector<double> mst(B * 16);
            WCQP_HIP_TRY(hipMemcpy(mst.data(), d.mst, B * 16 * 8, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < B; ++i)
                for (int ax = 0; ax < 2; ++ax) {
                    if (out->com) out->com[2 * i + ax] = mst[(i * 2 + ax) * 8 + 2];
                    if (out->dcm) out->dcm[2 * i + ax] = mst[(i * 2 + ax) * 8 + 6];
                }
        }
    } else {
        DN_(out->dcm, d.dcm, B * 16); DN_(out->com, d.com, B * 16);
    }
    DN_(out->mpc_fail, d.mpc_fail, B * 8); DN_(out->ik_fail, d.ik_fail, B * 8);
    DN_(out->hot_try, d.hot_try, B * 8); DN_(out->hot_hit, d.hot_hit, B * 8); DN_(out->tick, d.tick2 + h->phase, 4);
    if (out->feedback_fail) {
        if (h->feedback_fail) WCQP_HIP_TRY(hipMemcpy(out->feedback_fail, h->feedback_fail, B * 8, hipMemcpyDeviceToHost));
        else std::memset(out->feedback_fail, 0, B * 8);          // (no sensor form without kinematics: nothing was rejected)
    }
#undef DN_
    if (out->measured) {
        // what the chain of the last executed tick read as measured com / dcm / ZMP: the plant state at the start of tick t in its
        // hand-off record (parity t & 1; no later tick has run, so no later chain step has overwritten it)
        if (h->ticks_for_handoff() == 0) {
            if (h->meas0.size() != B * 6) return WCQP_E_INVALID;
            std::memcpy(out->measured, h->meas0.data(), B * 48);
        } else {
            std::vector<double> hd(B * kHandLen);
            WCQP_HIP_TRY(hipMemcpy(hd.data(), d.hand + (size_t)((h->ticks_for_handoff() - 1) & 1) * B * kHandLen, B * kHandLen * 8, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < B; ++i)
                for (int ax = 0; ax < 2; ++ax) {
                    out->measured[i * 6 + ax] = hd[i * kHandLen + 6 + ax];
                    out->measured[i * 6 + 2 + ax] = hd[i * kHandLen + 4 + ax];
                    out->measured[i * 6 + 4 + ax] = hd[i * kHandLen + 10 + ax];
                }
        }
    }
    if (out->zmp_gains) {
        if (d.gain_sched) {
            // the smoother output s of the last executed tick -> its gains (the two operations of zmp_gains_at, tick_device.h)
            std::vector<double> zs(B * 4);
            WCQP_HIP_TRY(hipMemcpy(zs.data(), h->zg.zs, B * 32, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < B; ++i) zmp_gains_host(d, h->zg, zs[i * 4 + 3], out->zmp_gains + 2 * i);
        } else {
            for (size_t i = 0; i < B; ++i) { out->zmp_gains[2 * i] = d.k_com; out->zmp_gains[2 * i + 1] = d.k_zmp; }
        }
    }
    return WCQP_OK;
}

}  // extern "C"
