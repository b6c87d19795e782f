// Footsteps from per-robot goals (include/wcqp.h: wcqp_unicycle_*, which states the planner): the reference's setGoal path (citations
// relative to /root/reference/modules/Walking_module):
//   src/WalkingModule.cpp:1263-1308          setPlannerInput: the goal
//   src/TrajectoryGenerator.cpp:442-484      updateTrajectories: the unicycle's start and its desired point
//   src/TrajectoryGenerator.cpp:114-132      the planner's parameters (plannerParams.ini)
// One lane per robot, 64 robots per wave, one wave per workgroup.  A robot's plan is one serial chain of at most K x D RK4 steps, and the
// feasibility test rides on it: every sample is tested as it is reached, the state of the last feasible one stays in registers, and the
// unicycle rewinds to it when the D samples of a step are through - nothing is integrated twice and no path array exists.  The cosine
// and sine of a sample's heading serve its candidate, the first RK4 stage of the next sample and - when the candidate becomes a footprint
// - the stance frame of the next step.  Every lane walks the same K x D trip counts (a robot that has ended idles behind a predicate); a
// wave leaves the step loop when all of its robots have ended.  Dead lanes of the last wave repeat the last robot and store nothing.
// Plain vector loads and stores only; the parameters travel as the kernel argument.
#include <cmath>
#include <new>
#include <vector>
#include "wcqp_internal.h"

namespace {

struct UniPar {
    double dT, dx, dy, kd;                     // kd = unicycle_gain / d_x
    double g, vmax, wmax;
    double len_max, len_min, width_min, half_w, ang_max, ang_min;
    int D, K;
};

struct UniDev {
    UniPar p;
    int batch;
    const double *left0, *right0, *goal;
    const uint8_t* first_side;
    int32_t *n_steps, *status;
    uint8_t* side;
    double *target, *desired_point, *unicycle_end;
};

constexpr double kTwoPi = 6.283185307179586476925286766559;

__device__ __forceinline__ double wrap_angle(double a) { return a - kTwoPi * rint(a / kTwoPi); }

// the unicycle's velocity at (x, y) with heading cosine / sine (c, s), towards the desired point (px, py)
__device__ __forceinline__ void uni_rate(const UniPar& p, double x, double y, double c, double s, double px, double py,
                                         double& fx, double& fy, double& fw) {
    const double ex = (x + (c * p.dx - s * p.dy)) - px;
    const double ey = (y + (s * p.dx + c * p.dy)) - py;
    double v = -p.kd * ((p.dx * c - p.dy * s) * ex + (p.dx * s + p.dy * c) * ey);
    double w = -p.kd * (c * ey - s * ex);
    v = fmin(fmax(v, -p.vmax), p.vmax);
    w = fmin(fmax(w, -p.wmax), p.wmax);
    v = v / (1.0 + p.g * fabs(w));
    fx = v * c; fy = v * s; fw = w;
}

__global__ __launch_bounds__(64) void unicycle_kernel(UniDev a) {
    const UniPar& p = a.p;
    const long raw = (long)blockIdx.x * 64 + threadIdx.x;
    const bool live = raw < a.batch;
    const size_t i = (size_t)(live ? raw : (long)a.batch - 1);
    // ---- inputs, and whether all of this robot's are finite
    double lx = a.left0[i * 12], ly = a.left0[i * 12 + 1], lc = a.left0[i * 12 + 3], ls = a.left0[i * 12 + 6];
    double rx = a.right0[i * 12], ry = a.right0[i * 12 + 1], rc = a.right0[i * 12 + 3], rs = a.right0[i * 12 + 6];
    double gx = a.goal[i * 2], gy = a.goal[i * 2 + 1];
    int sw = a.first_side[i];                          // the swing foot: 0 left, 1 right
    bool bad = !(isfinite(lx) && isfinite(ly) && isfinite(lc) && isfinite(ls) && isfinite(rx) && isfinite(ry) && isfinite(rc) && isfinite(rs) &&
                 isfinite(gx) && isfinite(gy)) || sw > 1;
    if (bad) { lx = ly = ls = rx = ry = rs = gx = gy = 0.0; lc = rc = 1.0; sw = 0; }     // (nothing non-finite enters the chain)
    const double lth = atan2(ls, lc), rth = atan2(rs, rc);
    // swing foot (sx, sy, sth), stance foot (tx, ty, tth) with its heading cosine / sine (tc, ts)
    double sx = sw ? rx : lx, sy = sw ? ry : ly, sth = sw ? rth : lth;
    double tx = sw ? lx : rx, ty = sw ? ly : ry, tth = sw ? lth : rth;
    double tc, ts;
    sincos(tth, &ts, &tc);
    // the unicycle: (0, -w/2) from a left stance foot, (0, +w/2) from a right one
    const double off = sw ? -p.half_w : p.half_w;
    double ux = tx - ts * off, uy = ty + tc * off, uth = tth, uc = tc, us = ts;
    const double ax = p.dx + gx, ay = p.dy + gy;
    double px = ux + (tc * ax - ts * ay), py = uy + (ts * ax + tc * ay);
    if (!(isfinite(px) && isfinite(py))) { bad = true; px = py = 0.0; }
    int status = bad ? WCQP_UNICYCLE_INVALID_INPUT : -1;          // -1: planning
    int n_steps = 0;
    const double h2 = 0.5 * p.dT, h6 = p.dT / 6.0;
    const unsigned K = (unsigned)p.K;
#pragma unroll 1
    for (unsigned k = 0; k < K; ++k) {
        if (__ballot(status < 0) == 0ull) break;
        const double sgn = sw ? -1.0 : 1.0, lat = sgn * p.half_w;
        double x = ux, y = uy, th = uth, c = uc, s = us;
        int best = 0;
        double bx = 0.0, by = 0.0, bth = 0.0, bc = 1.0, bs = 0.0, bcx = 0.0, bcy = 0.0;
#pragma unroll 1
        for (int m = 1; m <= p.D; ++m) {
            double f1x, f1y, f1w, f2x, f2y, f2w, f3x, f3y, f3w, f4x, f4y, f4w, cq, sq;
            uni_rate(p, x, y, c, s, px, py, f1x, f1y, f1w);
            sincos(th + h2 * f1w, &sq, &cq);
            uni_rate(p, x + h2 * f1x, y + h2 * f1y, cq, sq, px, py, f2x, f2y, f2w);
            sincos(th + h2 * f2w, &sq, &cq);
            uni_rate(p, x + h2 * f2x, y + h2 * f2y, cq, sq, px, py, f3x, f3y, f3w);
            sincos(th + p.dT * f3w, &sq, &cq);
            uni_rate(p, x + p.dT * f3x, y + p.dT * f3y, cq, sq, px, py, f4x, f4y, f4w);
            x = x + h6 * (f1x + 2.0 * f2x + 2.0 * f3x + f4x);
            y = y + h6 * (f1y + 2.0 * f2y + 2.0 * f3y + f4y);
            th = th + h6 * (f1w + 2.0 * f2w + 2.0 * f3w + f4w);
            sincos(th, &s, &c);
            // candidate m: the swing foot beside the unicycle, seen from the stance foot
            const double cx = x - s * lat, cy = y + c * lat;
            const double ex = cx - tx, ey = cy - ty;
            const double rlon = tc * ex + ts * ey, rlat = tc * ey - ts * ex;
            const bool feasible = sqrt(rlon * rlon + rlat * rlat) <= p.len_max && sgn * rlat >= p.width_min &&
                                  fabs(wrap_angle(th - tth)) <= p.ang_max;
            if (feasible) { best = m; bx = x; by = y; bth = th; bc = c; bs = s; bcx = cx; bcy = cy; }
        }
        if (status < 0) {
            if (best == 0) {
                status = WCQP_UNICYCLE_STUCK;
            } else {
                const double ex = bcx - sx, ey = bcy - sy, dyaw = wrap_angle(bth - sth);
                if (sqrt(ex * ex + ey * ey) < p.len_min && fabs(dyaw) < p.ang_min) {
                    status = WCQP_UNICYCLE_DONE;
                } else {
                    if (live) {
                        a.side[i * K + k] = (uint8_t)sw;
                        double* t = a.target + (i * K + k) * 3;
                        t[0] = bcx; t[1] = bcy; t[2] = dyaw;
                    }
                    ++n_steps;
                    // the foot that landed is the next stance foot; the unicycle rewinds to the sample it landed at
                    sx = tx; sy = ty; sth = tth;
                    tx = bcx; ty = bcy; tth = bth; tc = bc; ts = bs;
                    ux = bx; uy = by; uth = bth; uc = bc; us = bs;
                    sw = 1 - sw;
                }
            }
        }
    }
    if (status < 0) status = WCQP_UNICYCLE_TRUNCATED;
    if (!live) return;
    for (unsigned k = (unsigned)n_steps; k < K; ++k) {
        a.side[i * K + k] = 0;
        double* t = a.target + (i * K + k) * 3;
        t[0] = 0.0; t[1] = 0.0; t[2] = 0.0;
    }
    a.n_steps[i] = n_steps;
    a.status[i] = status;
    if (a.desired_point) { a.desired_point[i * 2] = bad ? 0.0 : px; a.desired_point[i * 2 + 1] = bad ? 0.0 : py; }
    if (a.unicycle_end) {
        a.unicycle_end[i * 3] = bad ? 0.0 : ux; a.unicycle_end[i * 3 + 1] = bad ? 0.0 : uy; a.unicycle_end[i * 3 + 2] = bad ? 0.0 : uth;
    }
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
    UniDev a{};
    a.p = h->par; a.batch = batch;
    a.left0 = in->left0; a.right0 = in->right0; a.goal = in->goal; a.first_side = in->first_side;
    a.n_steps = out->n_steps; a.status = out->status; a.side = out->side; a.target = out->target;
    a.desired_point = out->desired_point; a.unicycle_end = out->unicycle_end;
    hipLaunchKernelGGL(unicycle_kernel, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, (hipStream_t)stream, a);
    WCQP_HIP_TRY(hipGetLastError());
    return WCQP_OK;
}

int wcqp_unicycle_plan_host(wcqp_unicycle_t h, int32_t batch, const wcqp_unicycle_inputs* in, const wcqp_unicycle_outputs* out) {
    int rc = check_call(h, batch, in, out);
    if (rc != WCQP_OK) return rc;
    const size_t B = (size_t)batch, K = (size_t)h->par.K;
    const UniPar& p = h->par;
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
    if (batch == 0) return WCQP_OK;
    rc = ensure_device(h);
    if (rc != WCQP_OK) return rc;
    // doubles first, then the 32-bit rows, then the bytes; no step rows at all when the planner keeps none (K = 0)
    wcqp::HostStage st;
    const auto d_l = st.in(in->left0, B * 12), d_r = st.in(in->right0, B * 12), d_g = st.in(in->goal, B * 2);
    const auto d_t = st.out(out->target, B * K * 3, true), d_dp = st.out(out->desired_point, B * 2), d_ue = st.out(out->unicycle_end, B * 3);
    const auto d_n = st.out(out->n_steps, B), d_st = st.out(out->status, B);
    const auto d_fs = st.in(in->first_side, B);
    const auto d_sd = st.out(out->side, B * K, true);
    rc = st.upload(h->scratch);
    if (rc != WCQP_OK) return rc;
    const wcqp_unicycle_inputs din{st[d_l], st[d_r], st[d_g], st[d_fs]};
    const wcqp_unicycle_outputs dout{st[d_n], st[d_sd], st[d_t], st[d_st], st[d_dp], st[d_ue]};
    rc = wcqp_unicycle_plan_device(h, batch, &din, &dout, nullptr);
    return rc != WCQP_OK ? rc : st.download();
}

}  // extern "C"
