// Footsteps from per-robot goals (include/wcqp.h: wcqp_unicycle_*, which states the planner): the reference's setGoal path (citations
// relative to the reference's modules/Walking_module):
//   src/WalkingModule.cpp:1263-1308          setPlannerInput: the goal
//   src/TrajectoryGenerator.cpp:442-484      updateTrajectories: the unicycle's start and its desired point
//   src/TrajectoryGenerator.cpp:114-132      the planner's parameters (plannerParams.ini)
// One lane per robot, 64 robots per wave, one wave per workgroup; the per-robot body is unicycle_device.h's, which goal_plan_kernel
// (tick_plan.hip) runs too.  Dead lanes of the last wave repeat the last robot and store nothing.
// Plain vector loads and stores only; the parameters travel as the kernel argument.
// The untimed and the timed host form share one body (plan_host): the duration rows are optional staged outputs.
#include <cmath>
#include <new>
#include <vector>
#include "wcqp_internal.h"
#include "unicycle_device.h"

namespace {

using namespace wcqp_unicycle;

struct UniDev {
    UniPar p;
    int batch;
    const double *left0, *right0, *goal;
    const uint8_t* first_side;
    int32_t *n_steps, *status;
    uint8_t* side;
    double *target, *desired_point, *unicycle_end;
};

// the timed form's argument: the same, the candidates' range and score, and the two duration rows
struct UniTimedDev {
    UniDev d;
    UniTiming tm;
};

// (the two front ends load their robot's UniStart in the same written-out lines: as one device function the kernels' instruction streams
// move - DESIGN §8.23)
__global__ __launch_bounds__(64) void unicycle_kernel(UniDev a) {
    const long raw = (long)blockIdx.x * 64 + threadIdx.x;
    const bool live = raw < a.batch;
    const size_t i = (size_t)(live ? raw : (long)a.batch - 1);
    const UniStart in{a.left0[i * 12], a.left0[i * 12 + 1], a.left0[i * 12 + 3], a.left0[i * 12 + 6],
                      a.right0[i * 12], a.right0[i * 12 + 1], a.right0[i * 12 + 3], a.right0[i * 12 + 6],
                      a.goal[i * 2], a.goal[i * 2 + 1], (int)a.first_side[i]};
    plan_robot(a.p, in, UniRows{a.n_steps, a.status, a.side, a.target, a.desired_point, a.unicycle_end}, i, live);
}

__global__ __launch_bounds__(64) void unicycle_timed_kernel(UniTimedDev t) {
    const UniDev& a = t.d;
    const long raw = (long)blockIdx.x * 64 + threadIdx.x;
    const bool live = raw < a.batch;
    const size_t i = (size_t)(live ? raw : (long)a.batch - 1);
    const UniStart in{a.left0[i * 12], a.left0[i * 12 + 1], a.left0[i * 12 + 3], a.left0[i * 12 + 6],
                      a.right0[i * 12], a.right0[i * 12 + 1], a.right0[i * 12 + 3], a.right0[i * 12 + 6],
                      a.goal[i * 2], a.goal[i * 2 + 1], (int)a.first_side[i]};
    plan_robot_timed(a.p, t.tm, in, UniRows{a.n_steps, a.status, a.side, a.target, a.desired_point, a.unicycle_end}, i, live);
}

bool pos(double v) { return std::isfinite(v) && v > 0.0; }

}  // namespace

struct wcqp_unicycle_s {
    UniPar par{};
    bool device_seen = false;
    wcqp::DeviceScratch scratch;
};

namespace {

int ensure_device(wcqp_unicycle_s* h) {
    if (h->device_seen) return WCQP_OK;
    if (const int rc = wcqp::require_device("unicycle planner"); rc != WCQP_OK) return rc;
    h->device_seen = true;
    return WCQP_OK;
}

// what both forms refuse before they look for a device
int check_call(wcqp_unicycle_t h, int32_t batch, const wcqp_unicycle_inputs* in, const wcqp_unicycle_outputs* out) {
    if (!h || !in || !out || batch < 0) return WCQP_E_INVALID;
    if (!in->left0 || !in->right0 || !in->goal || !in->first_side || !out->n_steps || !out->status) return WCQP_E_INVALID;
    if (h->par.K > 0 && (!out->side || !out->target)) return WCQP_E_INVALID;
    if (!wcqp::fits32(batch, 96) || !wcqp::fits32(batch, 24ll * h->par.K)) return WCQP_E_UNSUPPORTED;
    return WCQP_OK;
}

// the timed forms' own refusals, and the timing as the kernel takes it
int check_timing(wcqp_unicycle_t h, const wcqp_unicycle_timing* tm, int32_t* ss_ticks, int32_t* ds_ticks, UniTiming* out) {
    if (!h || !tm) return WCQP_E_INVALID;
    if (tm->min_step_ticks < 2 || tm->min_step_ticks > tm->nominal_step_ticks || tm->nominal_step_ticks > tm->max_step_ticks) return WCQP_E_INVALID;
    if (!std::isfinite(tm->time_weight) || !(tm->time_weight >= 0.0) || !std::isfinite(tm->position_weight) || !(tm->position_weight >= 0.0))
        return WCQP_E_INVALID;
    if (!pos(tm->switch_over_swing_ratio)) return WCQP_E_INVALID;
    if (h->par.K > 0 && (!ss_ticks || !ds_ticks)) return WCQP_E_INVALID;
    out->m_min = tm->min_step_ticks; out->m_max = tm->max_step_ticks;
    out->inv_nom = 1.0 / ((double)tm->nominal_step_ticks * h->par.dT);
    out->time_w = tm->time_weight; out->pos_w = tm->position_weight;
    out->rho = tm->switch_over_swing_ratio / (1.0 + tm->switch_over_swing_ratio);
    out->ss_ticks = ss_ticks; out->ds_ticks = ds_ticks;
    return WCQP_OK;
}

// what the host forms find in their arrays: a non-finite entry that is read, a first_side above 1, a desired point that overflows
int check_host_arrays(const UniPar& p, size_t B, const wcqp_unicycle_inputs* in) {
    for (size_t i = 0; i < B; ++i) {
        const double* l = in->left0 + i * 12; const double* r = in->right0 + i * 12; const double* g = in->goal + i * 2;
        if (!(std::isfinite(l[0]) && std::isfinite(l[1]) && std::isfinite(l[3]) && std::isfinite(l[6]) && std::isfinite(r[0]) && std::isfinite(r[1]) &&
              std::isfinite(r[3]) && std::isfinite(r[6]) && std::isfinite(g[0]) && std::isfinite(g[1])) || in->first_side[i] > 1)
            return WCQP_E_INVALID;
        // the desired point, as the kernel forms it: finite inputs overflow it only near 1e308
        const double* s = in->first_side[i] ? l : r;
        const double th = std::atan2(s[6], s[3]), c = std::cos(th), sn = std::sin(th), off = in->first_side[i] ? -p.half_w : p.half_w;
        const double ax = p.dx + g[0], ay = p.dy + g[1];
        if (!std::isfinite((s[0] - sn * off) + (c * ax - sn * ay)) || !std::isfinite((s[1] + c * off) + (sn * ax + c * ay))) return WCQP_E_INVALID;
    }
    return WCQP_OK;
}

UniDev device_args(wcqp_unicycle_t h, int32_t batch, const wcqp_unicycle_inputs* in, const wcqp_unicycle_outputs* out) {
    UniDev a{};
    a.p = h->par; a.batch = batch;
    a.left0 = in->left0; a.right0 = in->right0; a.goal = in->goal; a.first_side = in->first_side;
    a.n_steps = out->n_steps; a.status = out->status; a.side = out->side; a.target = out->target;
    a.desired_point = out->desired_point; a.unicycle_end = out->unicycle_end;
    return a;
}

}  // namespace

extern "C" {

int wcqp_unicycle_create(const wcqp_unicycle_params* q, wcqp_unicycle_t* out) {
    if (!q || !out) return WCQP_E_INVALID;
    if (!pos(q->dT) || !std::isfinite(q->reference_position[0]) || q->reference_position[0] == 0.0 || !std::isfinite(q->reference_position[1]))
        return WCQP_E_INVALID;
    if (!pos(q->unicycle_gain) || !std::isfinite(q->slow_when_turning_gain) || !(q->slow_when_turning_gain >= 0.0)) return WCQP_E_INVALID;
    if (!pos(q->max_linear_velocity) || !pos(q->max_angular_velocity)) return WCQP_E_INVALID;
    if (!pos(q->max_step_length) || !pos(q->min_step_length) || q->min_step_length >= q->max_step_length) return WCQP_E_INVALID;
    if (!pos(q->min_width) || !pos(q->nominal_width) || q->min_width > q->nominal_width) return WCQP_E_INVALID;
    if (!pos(q->max_angle_variation) || !pos(q->min_angle_variation)) return WCQP_E_INVALID;
    if (q->step_ticks < 1 || q->max_steps < 0) return WCQP_E_INVALID;
    wcqp_unicycle_s* h = new (std::nothrow) wcqp_unicycle_s();
    if (!h) return WCQP_E_NOMEM;
    UniPar& p = h->par;
    p.dT = q->dT; p.dx = q->reference_position[0]; p.dy = q->reference_position[1]; p.kd = q->unicycle_gain / q->reference_position[0];
    p.g = q->slow_when_turning_gain; p.vmax = q->max_linear_velocity; p.wmax = q->max_angular_velocity;
    p.len_max = q->max_step_length; p.len_min = q->min_step_length; p.width_min = q->min_width; p.half_w = 0.5 * q->nominal_width;
    p.ang_max = q->max_angle_variation; p.ang_min = q->min_angle_variation;
    p.D = q->step_ticks; p.K = q->max_steps;
    *out = h;
    return WCQP_OK;
}

int wcqp_unicycle_destroy(wcqp_unicycle_t h) {
    if (!h) return WCQP_E_INVALID;
    h->scratch.release();
    delete h;
    return WCQP_OK;
}

int wcqp_unicycle_plan_device(wcqp_unicycle_t h, int32_t batch, const wcqp_unicycle_inputs* in, const wcqp_unicycle_outputs* out, void* stream) {
    int rc = check_call(h, batch, in, out);
    if (rc != WCQP_OK) return rc;
    if (batch == 0) return WCQP_OK;
    rc = ensure_device(h);
    if (rc != WCQP_OK) return rc;
    const UniDev a = device_args(h, batch, in, out);
    hipLaunchKernelGGL(unicycle_kernel, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, (hipStream_t)stream, a);
    WCQP_HIP_TRY(hipGetLastError());
    return WCQP_OK;
}

int wcqp_unicycle_plan_timed_device(wcqp_unicycle_t h, const wcqp_unicycle_timing* tm, int32_t batch, const wcqp_unicycle_inputs* in,
                                    const wcqp_unicycle_outputs* out, int32_t* ss_ticks, int32_t* ds_ticks, void* stream) {
    int rc = check_call(h, batch, in, out);
    if (rc != WCQP_OK) return rc;
    UniTimedDev t{};
    rc = check_timing(h, tm, ss_ticks, ds_ticks, &t.tm);
    if (rc != WCQP_OK) return rc;
    if (batch == 0) return WCQP_OK;
    rc = ensure_device(h);
    if (rc != WCQP_OK) return rc;
    t.d = device_args(h, batch, in, out);
    hipLaunchKernelGGL(unicycle_timed_kernel, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, (hipStream_t)stream, t);
    WCQP_HIP_TRY(hipGetLastError());
    return WCQP_OK;
}

// Both host forms (timed or not: wcqp_unicycle_plan_host has no timing and no duration rows): the checks, the arrays staged in one block, the
// device form
static int plan_host(wcqp_unicycle_t h, bool timed, const wcqp_unicycle_timing* tm, int32_t batch, const wcqp_unicycle_inputs* in,
                     const wcqp_unicycle_outputs* out, int32_t* ss_ticks, int32_t* ds_ticks) {
    int rc = check_call(h, batch, in, out);
    if (rc != WCQP_OK) return rc;
    UniTiming unused{};
    if (timed) rc = check_timing(h, tm, ss_ticks, ds_ticks, &unused);
    if (rc != WCQP_OK) return rc;
    const size_t B = (size_t)batch, K = (size_t)h->par.K;
    rc = check_host_arrays(h->par, B, in);
    if (rc != WCQP_OK) return rc;
    if (batch == 0) return WCQP_OK;
    rc = ensure_device(h);
    if (rc != WCQP_OK) return rc;
    // doubles first, then the 32-bit rows (the timed form's duration rows last of them), then the bytes; no step rows at all when the
    // planner keeps none (K = 0)
    wcqp::HostStage st;
    const auto d_l = st.in(in->left0, B * 12), d_r = st.in(in->right0, B * 12), d_g = st.in(in->goal, B * 2);
    const auto d_t = st.out(out->target, B * K * 3, true), d_dp = st.out(out->desired_point, B * 2), d_ue = st.out(out->unicycle_end, B * 3);
    const auto d_n = st.out(out->n_steps, B), d_st = st.out(out->status, B);
    const auto d_ss = st.out(timed ? ss_ticks : nullptr, B * K, true), d_ds = st.out(timed ? ds_ticks : nullptr, B * K, true);
    const auto d_fs = st.in(in->first_side, B);
    const auto d_sd = st.out(out->side, B * K, true);
    rc = st.upload(h->scratch);
    if (rc != WCQP_OK) return rc;
    const wcqp_unicycle_inputs din{st[d_l], st[d_r], st[d_g], st[d_fs]};
    const wcqp_unicycle_outputs dout{st[d_n], st[d_sd], st[d_t], st[d_st], st[d_dp], st[d_ue]};
    rc = timed ? wcqp_unicycle_plan_timed_device(h, tm, batch, &din, &dout, st[d_ss], st[d_ds], nullptr) : wcqp_unicycle_plan_device(h, batch, &din, &dout, nullptr);
    return rc != WCQP_OK ? rc : st.download();
}

int wcqp_unicycle_plan_host(wcqp_unicycle_t h, int32_t batch, const wcqp_unicycle_inputs* in, const wcqp_unicycle_outputs* out) {
    return plan_host(h, false, nullptr, batch, in, out, nullptr, nullptr);
}

int wcqp_unicycle_plan_timed_host(wcqp_unicycle_t h, const wcqp_unicycle_timing* tm, int32_t batch, const wcqp_unicycle_inputs* in,
                                  const wcqp_unicycle_outputs* out, int32_t* ss_ticks, int32_t* ds_ticks) {
    return plan_host(h, true, tm, batch, in, out, ss_ticks, ds_ticks);
}

}  // extern "C"

const wcqp_unicycle::UniPar* wcqp::unicycle_par(wcqp_unicycle_t h) { return h ? &h->par : nullptr; }
int wcqp::unicycle_timing(wcqp_unicycle_t h, const wcqp_unicycle_timing* tm, int32_t* ss_ticks, int32_t* ds_ticks, wcqp_unicycle::UniTiming* out) {
    return check_timing(h, tm, ss_ticks, ds_ticks, out);
}
