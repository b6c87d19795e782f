// The unicycle planner's per-robot body (include/wcqp.h: wcqp_unicycle_*, which states the planner), shared by unicycle_kernel
// (unicycle.hip: soles and goals from the caller's arrays) and goal_plan_kernel (tick_plan.hip: soles from a plan record of the tick
// handle) - and, in its timed form, by unicycle_timed_kernel and goal_plan_timed_kernel -, as prepare_device.h is shared by prepare.hip
// and position_tick.hip.  Internal, not ABI.
// A robot's plan is one serial chain of at most K x D RK4 steps, and the feasibility test rides on it: every sample is tested as it is
// reached, the state of the last feasible one stays in registers, and the unicycle rewinds to it when the D samples of a step are through -
// nothing is integrated twice and no path array exists.  The cosine and sine of a sample's heading serve its candidate, the first RK4 stage
// of the next sample and - when the candidate becomes a footprint - the stance frame of the next step.  Every lane walks the same K x D trip
// counts (a robot that has ended idles behind a predicate); a wave leaves the step loop when all of its robots have ended.
// TIMED (wcqp_unicycle_plan_timed_*): the candidates of a step are the samples min_step_ticks .. max_step_ticks, every feasible one is
// scored, and the state kept in registers is that of the best-scored feasible sample (the first of equals) instead of the last feasible
// one; the step's two durations are stored next to its target.  The untimed instantiation is the code it was before the flag.
#pragma once
#include "wcqp_internal.h"

namespace wcqp_unicycle {

struct UniPar {
    double dT, dx, dy, kd;                     // kd = unicycle_gain / d_x
    double g, vmax, wmax;
    double len_max, len_min, width_min, half_w, ang_max, ang_min;
    int D, K;
};

// TIMED only: the candidates' range and score (include/wcqp.h: wcqp_unicycle_timing), rho = r / (1 + r) of the switch-over-swing ratio r
struct UniTiming {
    int m_min, m_max;
    double inv_nom, time_w, pos_w, rho;        // inv_nom = 1 / (nominal_step_ticks dT)
    int32_t *ss_ticks, *ds_ticks;              // [B][K], the durations' rows (results, next to UniRows')
};

// what one robot's planning starts from: the entries of the two soles that are read (x, y, R00, R10), the goal, the swing foot
struct UniStart {
    double lx, ly, lc, ls, rx, ry, rc, rs, gx, gy;
    int sw;                                    // 0 left, 1 right
};

// where the results go: row i of each (desired_point / unicycle_end: or NULL)
struct UniRows {
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

// One lane's robot, planned from `in` into row i of `o`.  Called by every lane of the wave (the step loop votes); a lane that is not
// `live` repeats a live robot and stores nothing.
template <bool TIMED>
__device__ __forceinline__ void plan_robot_body(const UniPar& p, const UniTiming& tm, const UniStart& in, const UniRows& o, size_t i, bool live) {
    // ---- inputs, and whether all of this robot's are finite
    double lx = in.lx, ly = in.ly, lc = in.lc, ls = in.ls;
    double rx = in.rx, ry = in.ry, rc = in.rc, rs = in.rs;
    double gx = in.gx, gy = in.gy;
    int sw = in.sw;                                    // the swing foot: 0 left, 1 right
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
        [[maybe_unused]] double bcost = 0.0;           // TIMED: the score of candidate `best`
#pragma unroll 1
        for (int m = 1; m <= (TIMED ? tm.m_max : p.D); ++m) {
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
            if constexpr (TIMED) {
                // r_nom = (0, +-w): the lateral distance from it is rlat - sgn w
                const double dt = 1.0 / ((double)m * p.dT) - tm.inv_nom, dl = rlat - 2.0 * lat;
                const double cost = tm.time_w * (dt * dt) + tm.pos_w * (rlon * rlon + dl * dl);
                if (feasible && m >= tm.m_min && (best == 0 || cost < bcost)) {
                    best = m; bcost = cost; bx = x; by = y; bth = th; bc = c; bs = s; bcx = cx; bcy = cy;
                }
            } else {
                if (feasible) { best = m; bx = x; by = y; bth = th; bc = c; bs = s; bcx = cx; bcy = cy; }
            }
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
                        o.side[i * K + k] = (uint8_t)sw;
                        double* t = o.target + (i * K + k) * 3;
                        t[0] = bcx; t[1] = bcy; t[2] = dyaw;
                        if constexpr (TIMED) {
                            int ds = (int)floor((double)best * tm.rho + 0.5);
                            ds = ds > 1 ? ds : 1;
                            ds = ds < best - 1 ? ds : best - 1;
                            tm.ss_ticks[i * K + k] = best - ds;
                            tm.ds_ticks[i * K + k] = ds;
                        }
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
        o.side[i * K + k] = 0;
        double* t = o.target + (i * K + k) * 3;
        t[0] = 0.0; t[1] = 0.0; t[2] = 0.0;
        if constexpr (TIMED) { tm.ss_ticks[i * K + k] = 0; tm.ds_ticks[i * K + k] = 0; }
    }
    o.n_steps[i] = n_steps;
    o.status[i] = status;
    if (o.desired_point) { o.desired_point[i * 2] = bad ? 0.0 : px; o.desired_point[i * 2 + 1] = bad ? 0.0 : py; }
    if (o.unicycle_end) {
        o.unicycle_end[i * 3] = bad ? 0.0 : ux; o.unicycle_end[i * 3 + 1] = bad ? 0.0 : uy; o.unicycle_end[i * 3 + 2] = bad ? 0.0 : uth;
    }
}

__device__ __forceinline__ void plan_robot(const UniPar& p, const UniStart& in, const UniRows& o, size_t i, bool live) {
    plan_robot_body<false>(p, UniTiming{}, in, o, i, live);
}
__device__ __forceinline__ void plan_robot_timed(const UniPar& p, const UniTiming& tm, const UniStart& in, const UniRows& o, size_t i, bool live) {
    plan_robot_body<true>(p, tm, in, o, i, live);
}

}  // namespace wcqp_unicycle

namespace wcqp {
// unicycle.hip: the parameters a planner handle holds (NULL handle: NULL), for the kernels of other translation units
const wcqp_unicycle::UniPar* unicycle_par(wcqp_unicycle_t h);
// ... and the timed forms' validation of `tm` (what wcqp_unicycle_plan_timed_device refuses, it refuses), with the timing as a kernel takes
// it: the candidates' range and score, and the two duration rows (NULL rows are refused for a planner with max_steps > 0)
int unicycle_timing(wcqp_unicycle_t h, const wcqp_unicycle_timing* tm, int32_t* ss_ticks, int32_t* ds_ticks, wcqp_unicycle::UniTiming* out);
}  // namespace wcqp
