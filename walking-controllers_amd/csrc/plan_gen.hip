// Planned trajectories generated on the device from per-robot footstep lists (wcqp_tick_upload_footsteps).  include/wcqp.h defines the
// plan - timeline, swing, flags, ZMP, DCM reference, support-polygon sets - and tests/helpers/footstep_plan.py restates it in numpy; the
// record layout is tick_device.h's (kPlanRec).  Three kernels per upload, in stream order:
//   plan_prologue_kernel   one thread per robot, O(K): the footprint chain (plan_gen.h: kFpRec), the ZMP points, the set table
//   plan_dcm_kernel        one lane per (robot, axis), serial in the stage: the backward DCM recursion, tiles of stages through LDS
//   plan_record_kernel     one wave per (robot, 64 stages), one lane per stage: the 320-byte records, through LDS, as whole lines
// wcqp_tick_replan_footsteps runs the same three bodies with an origin (RP = true): robot i's plan is regenerated from stage M_i =
// origin[i] on - stage 0 of the rules moved to M_i, the start footprints taken from record M_i, the first double support's ZMP ramp started
// where the recursion arrives at the old ref_traj[M_i] - over a host-compacted list of robots (prologue, DCM pass) and of (robot, tile)
// pairs (record pass).  Nothing below M_i is stored: the DCM pass masks its tile write-out per stage, the record pass per 16-byte chunk.
// The timed calls (wcqp_tick_upload_footsteps_timed, wcqp_tick_replan_footsteps_timed) run the same bodies with TIMED = true: step k of a
// robot lasts its own ss_k + ds_k stages (plan_gen.h: PlanTimes), so no stage's step follows from a division.  The prologue writes the
// robot's start table - entry k the first stage s_k of step k's single support on the plan's own timeline, entry n the first standing
// stage -, the DCM pass walks a step index down it as its stage passes s_k, and the record pass copies the entries its tile touches into
// LDS next to the footprints and finds each lane's step by a search there.  The untimed instantiations are the code they were.
// The four forms - upload or replan, untimed or timed - are launched by one enqueue<RP, Arg> at the end of this file.  A plan uploaded with
// a swing profile (wcqp_tick_set_swing_profile) runs the record pass's SHAPED instantiations; prologue and DCM pass do not know the profile.
#include <cmath>
#include "plan_gen.h"

namespace {

using namespace wcqp_tick;

__device__ __forceinline__ void zmp_point(const double* pose, const double* dl, double* out) {
    out[0] = pose[0] + (pose[3] * dl[0] + pose[4] * dl[1]);
    out[1] = pose[1] + (pose[6] * dl[0] + pose[7] * dl[1]);
}

template <bool RP, bool TIMED>
__device__ __forceinline__ void plan_prologue(const PlanGenDev& g, const PlanTimes& tm) {
    const int slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= (RP ? g.n_robots : g.batch)) return;
    const int i = RP ? g.robots[slot] : slot;
    const int org = RP ? g.origin[i] : 0;
    const int n = g.n_steps[i], per = g.ss + g.ds;
    const size_t rec0 = (size_t)i * (size_t)g.traj_len;
    double fp[kFpPose];
    // desired left sole, desired right sole: of state0, or - a replan - of the record of the merge stage (read here, before the record pass)
    for (int k = 0; k < kFpPose; ++k) fp[k] = RP ? g.rec[(rec0 + (size_t)org) * kPlanRec + kPlanLeft + k] : g.state[(size_t)i * kStateLen + 24 + k];
    double* tab = g.table + (size_t)i * (size_t)(g.K + 1) * kFpRec;
    // set_base: the set the origin stage names - stage 0's own, built here, or the robot's last surviving one, which stays as it is
    int set = g.set_base[i];
    if (!RP) { g.set_at[set] = (long long)(rec0 * kPlanRec); g.set_code[set] = 2; }
    ++set;
    [[maybe_unused]] int s_next = g.first_ds;      // TIMED: s_k of the next step on the plan's own timeline, then the first standing stage
    for (int j = 0; j <= g.K; ++j) {
        if (j >= 1 && j <= n) {
            // step j - 1 lands: the swing foot's footprint becomes its target, rotated by the yaw increment about z
            const int k = j - 1, sw = g.side[(size_t)i * g.K + k];
            const double* tg = g.target + ((size_t)i * g.K + k) * 3;
            double* f = fp + 12 * sw;
            double sn, cs;
            sincos(tg[2], &sn, &cs);
            f[0] = tg[0]; f[1] = tg[1];
            for (int c = 0; c < 3; ++c) {
                const double r0 = f[3 + c], r1 = f[6 + c];
                f[3 + c] = cs * r0 - sn * r1;
                f[6 + c] = sn * r0 + cs * r1;
            }
            // its two changes of contact pair (the stance foot alone, both again), where a tick can reach them
            int s_k, ss_k;
            if constexpr (TIMED) {
                ss_k = tm.ss_k[(size_t)i * g.K + k];
                const int ds_k = k == n - 1 && tm.final_ds > 0 ? tm.final_ds : tm.ds_k[(size_t)i * g.K + k];
                tm.start[(size_t)i * (g.K + 1) + k] = s_next;
                s_k = org + s_next;
                s_next += ss_k + ds_k;
            } else {
                s_k = org + g.first_ds + k * per; ss_k = g.ss;
            }
            if (s_k <= g.max_ticks) { g.set_at[set] = (long long)((rec0 + s_k) * kPlanRec); g.set_code[set] = 1 - sw; ++set; }
            if (s_k + ss_k <= g.max_ticks) { g.set_at[set] = (long long)((rec0 + s_k + ss_k) * kPlanRec); g.set_code[set] = 2; ++set; }
        }
        if constexpr (TIMED) { if (j >= n) tm.start[(size_t)i * (g.K + 1) + j] = s_next; }
        double* t = tab + (size_t)j * kFpRec;
        for (int k = 0; k < kFpPose; ++k) t[k] = fp[k];
        zmp_point(fp, g.delta[0], t + 24);
        zmp_point(fp + 12, g.delta[1], t + 26);
    }
}

__global__ void plan_prologue_kernel(PlanGenDev g) { plan_prologue<false, false>(g, PlanTimes{}); }
__global__ void plan_prologue_replan_kernel(PlanGenDev g) { plan_prologue<true, false>(g, PlanTimes{}); }
__global__ void plan_prologue_timed_kernel(PlanGenTimedDev t) { plan_prologue<false, true>(t.g, t.tm); }
__global__ void plan_prologue_replan_timed_kernel(PlanGenTimedDev t) { plan_prologue<true, true>(t.g, t.tm); }

// ---- the DCM reference: xi_t = (xi_{t+1} - (1 - a) zmp_t) / a backwards from xi = zmp at the first standing stage
constexpr int kDcmRobots = 32, kDcmTile = 32, kDcmRow = 2 * kDcmTile + 2;

// RP: lane r of block x carries robot robots[32 x + r]; a lane computes and stores only stages >= its robot's origin, and the serial pass
// ends at the tile of the wave's lowest origin.  The first double support's ramp starts at the point that makes the recursion arrive at
// the old ref_traj[origin] (read before the pass stores over it): xi_M = X q^n - (1 - a) (za (S0 - S1) + zb S1), q = 1 / a, n = first_ds,
// S0 = sum_{j=1..n} q^j, S1 = sum_{j=1..n} j q^j / (n + 1), X the recursion's value at stage M + n - one division where the pass gets there.
// TIMED: the lane keeps the step its stage lies in (kc, from n - 1 down), that step's first stage and its two durations, and steps down
// when the stage passes below the step's first one; the last step's double support lasts final_ds, or - 0 - its own ds.
template <bool RP, bool TIMED>
__device__ __forceinline__ void plan_dcm(const PlanGenDev& g, const PlanTimes& tm) {
    __shared__ double t_xi[kDcmRobots * kDcmRow];
    __shared__ double t_vel[kDcmRobots * kDcmRow];
    const int lane = threadIdx.x, r = lane >> 1, ax = lane & 1;
    const int count = RP ? g.n_robots : g.batch;
    const int i_raw = blockIdx.x * kDcmRobots + r;
    const bool live = i_raw < count;
    const int i = RP ? g.robots[live ? i_raw : count - 1] : (live ? i_raw : g.batch - 1);
    const int org = RP ? g.origin[i] : 0;
    const int n = g.n_steps[i], per = g.ss + g.ds, T = g.traj_len;
    [[maybe_unused]] const int* start = TIMED ? tm.start + (size_t)i * (size_t)(g.K + 1) : nullptr;
    int s_end;                                                                                    // the first standing stage
    if constexpr (TIMED) s_end = org + start[n];
    else s_end = org + (n > 0 ? g.first_ds + n * per - g.ds + g.final_ds : g.first_ds);
    [[maybe_unused]] int kc = n - 1, kc_s = 0, kc_ss = 0, kc_ds = 0;
    if constexpr (TIMED) {
        if (n > 0) {
            kc_s = start[kc]; kc_ss = tm.ss_k[(size_t)i * g.K + kc];
            kc_ds = tm.final_ds > 0 ? tm.final_ds : tm.ds_k[(size_t)i * g.K + kc];
        }
    }
    const double* tab = g.table + (size_t)i * (size_t)(g.K + 1) * kFpRec;
    const unsigned char* side = g.side + (size_t)i * g.K;
    const double mid0 = 0.5 * (tab[24 + ax] + tab[26 + ax]);
    const double mid_n = 0.5 * (tab[(size_t)n * kFpRec + 24 + ax] + tab[(size_t)n * kFpRec + 26 + ax]);
    const double xi_org = RP ? g.ref[((size_t)i * (size_t)T + (size_t)org) * 2 + ax] : 0.0;
    int top = s_end > T ? s_end : T;
    for (int m = 1; m < 64; m <<= 1) { const int o = __shfl_xor(top, m); top = o > top ? o : top; }
    int bottom = 0;
    if (RP) {
        bottom = org;
        for (int m = 1; m < 64; m <<= 1) { const int o = __shfl_xor(bottom, m); bottom = o < bottom ? o : bottom; }
        bottom &= ~(kDcmTile - 1);
    }
    const double a = g.a, b1 = 1.0 - g.a;
    double xi = mid_n;
    int key = -2;                     // the segment za / zb belong to: -1 the first double support, 2 k single support of step k, 2 k + 1 the double support behind it
    double za = 0.0, zb = 0.0;
    for (int t = top - 1; t >= bottom; --t) {
        double z = 0.0;
        const int tr = t - org;       // the stage on the plan's own timeline
        if (RP && tr < 0) {
            // (below this lane's origin: nothing to compute, nothing of it is stored)
        } else if (t >= s_end) {
            z = mid_n; xi = mid_n;
        } else {
            if (tr < g.first_ds) {
                if (key != -1) {
                    key = -1; za = mid0; zb = n > 0 ? tab[24 + 2 * (1 - side[0]) + ax] : mid0;
                    if (RP) {
                        const double nn = (double)g.first_ds, q = 1.0 / a, qn = pow(q, nn);
                        const double S0 = q * (1.0 - qn) / (1.0 - q);
                        const double S1 = q * (1.0 - (nn + 1.0) * qn + nn * qn * q) / ((1.0 - q) * (1.0 - q) * (nn + 1.0));
                        za = (xi * qn - b1 * zb * S1 - xi_org) / (b1 * (S0 - S1));
                    }
                }
                z = za + ((double)(tr + 1) / (double)(g.first_ds + 1)) * (zb - za);
            } else {
                int k, u, ss_k;
                if constexpr (TIMED) {
                    while (kc > 0 && tr < kc_s) {
                        --kc;
                        kc_s = start[kc]; kc_ss = tm.ss_k[(size_t)i * g.K + kc]; kc_ds = tm.ds_k[(size_t)i * g.K + kc];
                    }
                    k = kc; u = tr - kc_s; ss_k = kc_ss;
                } else {
                    const int rr = tr - g.first_ds;
                    k = rr / per;
                    k = k < n - 1 ? k : n - 1;
                    u = rr - k * per;
                    ss_k = g.ss;
                }
                if (u < ss_k) {
                    if (key != 2 * k) { key = 2 * k; za = tab[(size_t)k * kFpRec + 24 + 2 * (1 - side[k]) + ax]; }
                    z = za;
                } else {
                    if (key != 2 * k + 1) {
                        key = 2 * k + 1;
                        const double* e = tab + (size_t)(k + 1) * kFpRec;
                        za = e[24 + 2 * (1 - side[k]) + ax];
                        zb = k < n - 1 ? e[24 + 2 * (1 - side[k + 1]) + ax] : 0.5 * (e[24 + ax] + e[26 + ax]);
                    }
                    const int nds = TIMED ? kc_ds : (k == n - 1 ? g.final_ds : g.ds);
                    z = za + ((double)(u - ss_k + 1) / (double)(nds + 1)) * (zb - za);
                }
            }
            xi = (xi - b1 * z) / a;
        }
        if (t >= T) continue;
        const int tt = t & (kDcmTile - 1);
        t_xi[r * kDcmRow + 2 * tt + ax] = xi;
        t_vel[r * kDcmRow + 2 * tt + ax] = g.omega * (xi - z);
        if (!RP && t == 0 && live) g.zmp0[2 * (size_t)i + ax] = z;
        if (tt != 0) continue;
        // stages [t, hi) of the block's robots: each robot's tile is contiguous in HBM, 32 lanes write it 16 bytes each
        __syncthreads();
        const int hi = t + kDcmTile < T ? t + kDcmTile : T;
        const int q = lane & 31;
        for (int r0 = 0; r0 < kDcmRobots; r0 += 2) {
            const int ro = r0 + (lane >> 5);
            const long so = (long)blockIdx.x * kDcmRobots + ro;
            if (so >= count || t + q >= hi) continue;
            const long io = RP ? (long)g.robots[so] : so;
            if (RP && t + q < g.origin[io]) continue;       // (the tile that straddles the robot's origin: only stages >= it)
            const size_t w = ((size_t)io * (size_t)T + (size_t)(t + q)) * 2;
            *reinterpret_cast<double2*>(g.ref + w) = make_double2(t_xi[ro * kDcmRow + 2 * q], t_xi[ro * kDcmRow + 2 * q + 1]);
            if (g.vel) *reinterpret_cast<double2*>(g.vel + w) = make_double2(t_vel[ro * kDcmRow + 2 * q], t_vel[ro * kDcmRow + 2 * q + 1]);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void plan_dcm_kernel(PlanGenDev g) { plan_dcm<false, false>(g, PlanTimes{}); }
__global__ __launch_bounds__(64) void plan_dcm_replan_kernel(PlanGenDev g) { plan_dcm<true, false>(g, PlanTimes{}); }
__global__ __launch_bounds__(64) void plan_dcm_timed_kernel(PlanGenTimedDev t) { plan_dcm<false, true>(t.g, t.tm); }
__global__ __launch_bounds__(64) void plan_dcm_replan_timed_kernel(PlanGenTimedDev t) { plan_dcm<true, true>(t.g, t.tm); }

// ---- the records.  A wave takes 64 consecutive stages of one robot - 20 KiB of records, contiguous in HBM and 64-byte aligned (a record
// is five lines): lane l computes stage s0 + l into row l of an LDS tile (rows of 41 doubles: the 8-byte LDS stores of 16 lanes fall on
// 16 different bank pairs), then the wave writes the tile out 16 bytes per lane, 1 KiB - sixteen whole lines - per store instruction.
// The robot's footprints come from its table, the entries the tile's stages touch copied into LDS first: a step lasts two stages or more,
// so 64 stages touch at most 34 entries.
constexpr int kRecTile = 64, kRecRow = kPlanRec + 1, kTabMax = kRecTile / 2 + 2;

// RP: block x takes entry x of the host's (robot, tile) list - the tiles at or above the robot's origin; in the tile that straddles it the
// lanes below the origin compute nothing and the write-out skips their records (a record is twenty 16-byte chunks, none shared with a
// neighbour).  Before the new plan's first single support the fixed-frame bit keeps the value of stage origin - 1, a record no replan
// of this origin writes.
// TIMED: the largest k of 0 .. n - 1 whose first stage start[k] is <= s, or -1 (n = 0, or s lies in the first double support)
__device__ __forceinline__ int step_at(const int* start, int n, int s) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (start[mid] <= s) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

// TIMED: the first stages and single-support lengths of steps j_lo .. j_hi - 1 sit in LDS next to the footprints (stl, ssl [kTabMax], the
// timed kernels' own: a step lasts two stages or more), and a lane finds its step by counting the first stages at or below its own.
// SHAPED: THE SHAPED SWING (include/wcqp.h; tests/helpers/swing_profile.py restates it) - the swing block gives the foot's height the
// two-branch smoothstep with its apex at x = apex and the landing term, pitches the foot about its own y axis (one more sincos per
// swinging lane, the nine rotation entries instead of six, two more of the twist) and a single-support stage's CoM height the quartic bump.
// Nothing else of the pass knows the profile (prof: the shaped kernels' second argument, unread otherwise): the tile, the tables in LDS and
// the write-out are the unshaped kernels'.
template <bool RP, bool TIMED, bool SHAPED>
__device__ __forceinline__ void plan_record(const PlanGenDev& g, const PlanTimes& tm, const PlanSwing& prof, int* stl, int* ssl) {
    __shared__ double tile[kRecTile * kRecRow];
    __shared__ double fpt[kTabMax * kFpPose];
    __shared__ double dyaw[kTabMax];
    __shared__ int swing[kTabMax];
    const int lane = threadIdx.x;
    const size_t i = RP ? (size_t)g.tiles[blockIdx.x].x : (size_t)blockIdx.y;
    const int org = RP ? g.origin[i] : 0;
    const int T = g.traj_len, s0 = (RP ? g.tiles[blockIdx.x].y : (int)blockIdx.x) * kRecTile;
    const int nvalid = T - s0 < kRecTile ? T - s0 : kRecTile;
    const int n = g.n_steps[i], per = g.ss + g.ds;
    // entries j_lo .. j_hi: from the step the first stage lies in (the last step's, once standing: its stance foot is the fixed frame) to the
    // footprints behind the step the last stage lies in (stages on the plan's own timeline: the origin is its stage 0)
    [[maybe_unused]] const int* start = TIMED ? tm.start + i * (size_t)(g.K + 1) : nullptr;
    auto step_of = [&](int s) {
        if constexpr (TIMED) { const int k = step_at(start, n, s); return k < 0 ? 0 : k; }
        else return s < g.first_ds ? 0 : (s - g.first_ds) / per;
    };
    const int last = n > 0 ? n - 1 : 0;
    int j_lo = step_of((RP && s0 < org ? org : s0) - org);
    j_lo = j_lo < last ? j_lo : last;
    int j_hi = step_of(s0 + nvalid - 1 - org) + 1;
    j_hi = j_hi < n ? j_hi : n;
    int cnt = j_hi - j_lo + 1;
    cnt = cnt < kTabMax ? cnt : kTabMax;
    const double* tab = g.table + (i * (size_t)(g.K + 1) + (size_t)j_lo) * kFpRec;
    for (int x = lane; x < cnt * kFpPose; x += kRecTile) fpt[x] = tab[(size_t)(x / kFpPose) * kFpRec + x % kFpPose];
    if (lane < cnt && j_lo + lane < n) {
        swing[lane] = g.side[i * g.K + j_lo + lane];
        dyaw[lane] = g.target[(i * g.K + j_lo + lane) * 3 + 2];
        if constexpr (TIMED) { stl[lane] = start[j_lo + lane]; ssl[lane] = tm.ss_k[i * g.K + j_lo + lane]; }
    }
    int fixed0 = 0;
    if (RP) fixed0 = ((int)g.rec[(i * (size_t)T + (size_t)(org - 1)) * kPlanRec + kPlanFlags] & 4) ? 0 : 1;
    __syncthreads();
    const int s = s0 + lane, sr = s - org;
    if (lane < nvalid && sr >= 0) {
        double* o = tile + lane * kRecRow;
        int k = -1, u = 0, ss_k = g.ss;
        // the steps in LDS: j_lo .. j_lo + nst - 1
        [[maybe_unused]] const int nst = (cnt < n - j_lo ? cnt : n - j_lo);
        if constexpr (TIMED) {
            if (sr >= g.first_ds && n > 0) {
                int x = 0;
                for (int y = 1; y < nst; ++y) x += stl[y] <= sr ? 1 : 0;
                k = j_lo + x; u = sr - stl[x]; ss_k = ssl[x];
            }
        } else {
            if (sr >= g.first_ds) { k = (sr - g.first_ds) / per; u = (sr - g.first_ds) - k * per; }
        }
        const bool swinging = k >= 0 && k < n && u < ss_k;
        // the footprints in force: after k + 1 landed steps, or - the swing foot still in the air - after k
        int j = k < 0 ? 0 : (k < n ? k + (swinging ? 0 : 1) : n);
        j = j - j_lo;
        j = j < 0 ? 0 : (j < cnt ? j : cnt - 1);
        const double* f = fpt + j * kFpPose;
        for (int e = 0; e < kFpPose; ++e) o[kPlanLeft + e] = f[e];
        for (int e = 0; e < 12; ++e) o[kPlanTwL + e] = 0.0;
        int flags = 3, fixed = fixed0;
        [[maybe_unused]] double bump = 0.0, dbump = 0.0;      // SHAPED: a single-support stage's CoM height over h0, and its velocity
        if (k >= 0 && n > 0) { const int kl = k < n ? k : n - 1; fixed = 1 - swing[kl - j_lo < cnt ? kl - j_lo : cnt - 1]; }
        if (swinging) {
            const int sw = swing[k - j_lo < cnt ? k - j_lo : cnt - 1];
            const double dy = dyaw[k - j_lo < cnt ? k - j_lo : cnt - 1];
            const double* p0 = f + 12 * sw;
            const double* p1 = f + (j + 1 < cnt ? kFpPose : 0) + 12 * sw;       // the target: the same foot after this step
            const double x = (double)(u + 1) / (double)ss_k, x1 = 1.0 - x;
            const double m = x * x * x * (10.0 - 15.0 * x + 6.0 * x * x), dm = 30.0 * x * x * x1 * x1;
            const double lz = 16.0 * x * x * x1 * x1, dlz = 32.0 * x * x1 * (1.0 - 2.0 * x);
            const double inv = 1.0 / ((double)ss_k * g.dT);
            double* op = o + kPlanLeft + 12 * sw;
            double* ot = o + kPlanTwL + 6 * sw;
            const double dx = p1[0] - p0[0], dyy = p1[1] - p0[1];
            op[0] = p0[0] + dx * m; op[1] = p0[1] + dyy * m; op[2] = p0[2] + g.lift * lz;
            double sn, cs;
            sincos(dy * m, &sn, &cs);
            for (int c = 0; c < 3; ++c) {
                const double r0 = p0[3 + c], r1 = p0[6 + c];
                op[3 + c] = cs * r0 - sn * r1;
                op[6 + c] = sn * r0 + cs * r1;
            }
            ot[0] = dx * dm * inv; ot[1] = dyy * dm * inv; ot[2] = g.lift * dlz * inv; ot[5] = dy * dm * inv;
            if constexpr (SHAPED) {
                // c0, its derivative in x, and the landing term with its derivative in TIME: v_land (3 y^2 - 2 y), exactly v_land at x = 1
                double c0 = lz, dc0 = dlz, land = 0.0, vland = 0.0;
                if (prof.apex > 0.0) {
                    if (x <= prof.apex) {
                        const double y = x / prof.apex;
                        c0 = y * y * (3.0 - 2.0 * y); dc0 = 6.0 * y * (1.0 - y) / prof.apex;
                    } else {
                        const double w = 1.0 - prof.apex, y = (x - prof.apex) / w;
                        c0 = 1.0 - y * y * (3.0 - 2.0 * y); dc0 = -6.0 * y * (1.0 - y) / w;
                        land = prof.v_land * w * ((double)ss_k * g.dT) * (y * y * y - y * y);
                        vland = prof.v_land * (3.0 * y * y - 2.0 * y);
                    }
                }
                op[2] = p0[2] + g.lift * c0 + land;
                ot[2] = g.lift * dc0 * inv + vland;
                // Rz(dyaw m) R is in place (its third row the footprint's own): the pitch rate turns about its second column, then Ry(theta)
                const double rate = prof.pitch * dc0 * inv;
                ot[3] = op[4] * rate; ot[4] = op[7] * rate; ot[5] += op[10] * rate;
                double sp, cp;
                sincos(prof.pitch * c0, &sp, &cp);
                for (int c = 3; c < 12; c += 3) {
                    const double a0 = op[c], a2 = op[c + 2];
                    op[c] = cp * a0 - sp * a2;
                    op[c + 2] = sp * a0 + cp * a2;
                }
                bump = prof.dh * lz; dbump = prof.dh * dlz * inv;
            }
            flags = sw == 1 ? 1 : 2;
        }
        o[kPlanFlags] = (double)(flags | (fixed == 0 ? 4 : 0));
        const double h0 = RP ? g.h0[i] : g.state[i * kStateLen + 68];
        o[kPlanHeight] = SHAPED ? h0 + bump : h0;
        o[kPlanHeightVel] = SHAPED ? dbump : 0.0;
        // the support-polygon set in force: the origin's, plus the changes of contact pair up to this stage that a tick can reach
        const int se = (s < g.max_ticks ? s : g.max_ticks) - org;
        int changes = 0;
        if constexpr (TIMED) {
            // (se <= s: its step is the lane's own or an earlier one of the tile - or, below the tile, found in the robot's table)
            if (se >= g.first_ds && n > 0) {
                int ke, s_ke, ss_ke;
                if (se >= stl[0]) {
                    int x = 0;
                    for (int y = 1; y < nst; ++y) x += stl[y] <= se ? 1 : 0;
                    ke = j_lo + x; s_ke = stl[x]; ss_ke = ssl[x];
                } else {
                    ke = step_at(start, n, se); s_ke = start[ke]; ss_ke = tm.ss_k[i * g.K + ke];
                }
                changes = 2 * ke + 1 + (se - s_ke >= ss_ke ? 1 : 0);
            }
        } else if (se >= g.first_ds) {
            const int ke = (se - g.first_ds) / per, ue = (se - g.first_ds) - ke * per;
            changes = ke < n ? 2 * ke + 1 + (ue >= g.ss ? 1 : 0) : 2 * n;
        }
        o[kPlanHull] = (double)(g.set_base[i] + changes);
    }
    __syncthreads();
    double* out = g.rec + (i * (size_t)T + (size_t)s0) * kPlanRec;
    const int total = nvalid * kPlanRec;
    for (int x = 2 * lane; x < total; x += 2 * kRecTile) {
        const int st = x / kPlanRec, e = x - st * kPlanRec;
        if (RP && s0 + st < org) continue;
        *reinterpret_cast<double2*>(out + x) = make_double2(tile[st * kRecRow + e], tile[st * kRecRow + e + 1]);
    }
}

__global__ __launch_bounds__(kRecTile) void plan_record_kernel(PlanGenDev g) { plan_record<false, false, false>(g, PlanTimes{}, PlanSwing{}, nullptr, nullptr); }
__global__ __launch_bounds__(kRecTile) void plan_record_replan_kernel(PlanGenDev g) { plan_record<true, false, false>(g, PlanTimes{}, PlanSwing{}, nullptr, nullptr); }
__global__ __launch_bounds__(kRecTile) void plan_record_timed_kernel(PlanGenTimedDev t) {
    __shared__ int stl[kTabMax], ssl[kTabMax];
    plan_record<false, true, false>(t.g, t.tm, PlanSwing{}, stl, ssl);
}
__global__ __launch_bounds__(kRecTile) void plan_record_replan_timed_kernel(PlanGenTimedDev t) {
    __shared__ int stl[kTabMax], ssl[kTabMax];
    plan_record<true, true, false>(t.g, t.tm, PlanSwing{}, stl, ssl);
}
// their shaped siblings: what a plan uploaded with a non-zero swing profile runs (enqueue<> chooses), the profile a second argument
__global__ __launch_bounds__(kRecTile) void plan_record_shaped_kernel(PlanGenDev g, PlanSwing sw) { plan_record<false, false, true>(g, PlanTimes{}, sw, nullptr, nullptr); }
__global__ __launch_bounds__(kRecTile) void plan_record_replan_shaped_kernel(PlanGenDev g, PlanSwing sw) { plan_record<true, false, true>(g, PlanTimes{}, sw, nullptr, nullptr); }
__global__ __launch_bounds__(kRecTile) void plan_record_timed_shaped_kernel(PlanGenTimedDev t, PlanSwing sw) {
    __shared__ int stl[kTabMax], ssl[kTabMax];
    plan_record<false, true, true>(t.g, t.tm, sw, stl, ssl);
}
__global__ __launch_bounds__(kRecTile) void plan_record_replan_timed_shaped_kernel(PlanGenTimedDev t, PlanSwing sw) {
    __shared__ int stl[kTabMax], ssl[kTabMax];
    plan_record<true, true, true>(t.g, t.tm, sw, stl, ssl);
}

// ---- the launch path: one implementation for the four forms - upload or replan (RP), untimed or timed (the argument's type)
// what differs by the argument: the PlanGenDev in it, the kernels that take it, the checks of its durations, and the rows a slab advances
const PlanGenDev& base(const PlanGenDev& g) { return g; }
const PlanGenDev& base(const PlanGenTimedDev& t) { return t.g; }

template <bool RP, class Arg> struct Passes;
template <> struct Passes<false, PlanGenDev> { static constexpr auto prologue = plan_prologue_kernel, dcm = plan_dcm_kernel, record = plan_record_kernel; static constexpr auto shaped = plan_record_shaped_kernel; };
template <> struct Passes<true, PlanGenDev> { static constexpr auto prologue = plan_prologue_replan_kernel, dcm = plan_dcm_replan_kernel, record = plan_record_replan_kernel; static constexpr auto shaped = plan_record_replan_shaped_kernel; };
template <> struct Passes<false, PlanGenTimedDev> { static constexpr auto prologue = plan_prologue_timed_kernel, dcm = plan_dcm_timed_kernel, record = plan_record_timed_kernel; static constexpr auto shaped = plan_record_timed_shaped_kernel; };
template <> struct Passes<true, PlanGenTimedDev> { static constexpr auto prologue = plan_prologue_replan_timed_kernel, dcm = plan_dcm_replan_timed_kernel, record = plan_record_replan_timed_kernel; static constexpr auto shaped = plan_record_replan_timed_shaped_kernel; };

// an untimed plan has one (ss, ds) and a resolved final_ds; a timed one its three rows, and a final_ds of 0 for each last step's own ds
bool durations_ok(const PlanGenDev& g) { return g.ss >= 1 && g.ds >= 1 && g.final_ds >= 1; }
bool durations_ok(const PlanGenTimedDev& t) { return t.tm.final_ds >= 0 && t.tm.start && (t.g.K == 0 || (t.tm.ss_k && t.tm.ds_k)); }

// the per-robot rows of the record pass moved on by i0 robots (its robot index is grid.y, which starts at 0 in every launch)
void advance(PlanGenDev& p, int i0) {
    p.n_steps += i0; p.side += (size_t)i0 * p.K; p.target += (size_t)i0 * p.K * 3; p.state += (size_t)i0 * kStateLen;
    p.set_base += i0; p.table += (size_t)i0 * (size_t)(p.K + 1) * kFpRec; p.rec += (size_t)i0 * (size_t)p.traj_len * kPlanRec;
}
void advance(PlanGenTimedDev& t, int i0) {
    advance(t.g, i0);
    t.tm.ss_k += (size_t)i0 * t.g.K; t.tm.ds_k += (size_t)i0 * t.g.K; t.tm.start += (size_t)i0 * (size_t)(t.g.K + 1);
}

// prologue, DCM pass and record pass in stream order.  An upload runs every robot, its record pass one launch per 65535 robots (they lie
// on grid.y) with rec0 / rec1 recorded around it; a replan runs the listed robots and tiles and records nothing.
template <bool RP, class Arg>
int enqueue(const Arg& a, const PlanSwing& sw, hipStream_t stream, hipEvent_t rec0, hipEvent_t rec1) {
    using P = Passes<RP, Arg>;
    const PlanGenDev& g = base(a);
    if (g.batch < 1 || g.traj_len < 1 || g.first_ds < 1 || g.K < 0 || !durations_ok(a)) return WCQP_E_INVALID;
    if (RP && (!g.origin || !g.robots || !g.tiles || !g.h0 || g.n_robots < 0 || g.n_tiles < 0)) return WCQP_E_INVALID;
    const int robots = RP ? g.n_robots : g.batch;
    if (robots == 0) return WCQP_OK;
    // the record pass of one grid: an all-zero profile takes the kernels that know none, with the one argument they always took
    auto record = [&](dim3 grid, const Arg& arg) {
        if (sw.shaped()) hipLaunchKernelGGL(P::shaped, grid, dim3(kRecTile), 0, stream, arg, sw);
        else hipLaunchKernelGGL(P::record, grid, dim3(kRecTile), 0, stream, arg);
    };
    hipLaunchKernelGGL(P::prologue, dim3((unsigned)((robots + 63) / 64)), dim3(64), 0, stream, a);
    hipLaunchKernelGGL(P::dcm, dim3((unsigned)((robots + kDcmRobots - 1) / kDcmRobots)), dim3(64), 0, stream, a);
    if (rec0) WCQP_HIP_TRY(hipEventRecord(rec0, stream));
    if (RP) {
        if (g.n_tiles > 0) record(dim3((unsigned)g.n_tiles), a);
    } else {
        constexpr int kSlab = 65535;
        for (int i0 = 0; i0 < g.batch; i0 += kSlab) {
            Arg slab = a;
            advance(slab, i0);
            const int nb = g.batch - i0 < kSlab ? g.batch - i0 : kSlab;
            record(dim3((unsigned)((g.traj_len + kRecTile - 1) / kRecTile), (unsigned)nb), slab);
        }
    }
    if (rec1) WCQP_HIP_TRY(hipEventRecord(rec1, stream));
    WCQP_HIP_TRY(hipGetLastError());
    return WCQP_OK;
}

}  // namespace

namespace wcqp {

int plan_gen_enqueue(const PlanGenDev& g, const PlanSwing& sw, hipStream_t stream, hipEvent_t rec0, hipEvent_t rec1) { return enqueue<false>(g, sw, stream, rec0, rec1); }
int plan_gen_enqueue(const PlanGenTimedDev& t, const PlanSwing& sw, hipStream_t stream, hipEvent_t rec0, hipEvent_t rec1) { return enqueue<false>(t, sw, stream, rec0, rec1); }
int plan_replan_enqueue(const PlanGenDev& g, const PlanSwing& sw, hipStream_t stream) { return enqueue<true>(g, sw, stream, nullptr, nullptr); }
int plan_replan_enqueue(const PlanGenTimedDev& t, const PlanSwing& sw, hipStream_t stream) { return enqueue<true>(t, sw, stream, nullptr, nullptr); }

}  // namespace wcqp
