// Stopped robots of a running fleet restarted on the device, per robot (wcqp_tick_restart_robots; include/wcqp.h states THE RESTARTED
// ROBOT, tests/helpers/plan_restart.py restates its plan in numpy).  The call lists robots - slot r is robot robots[r] - and two kernels
// run in stream order:
//   plan_restart_reset_kernel   one wave per slot: reads the robot's ik_fail, decides (ALWAYS, or IF_STOPPED: ik_fail > 0; or takes the
//                               decision a recover call's gate made, plan_recover.hip), writes the
//                               decision and ik_fail into the slot's result row and - for a robot that restarts - resets the state
//                               wcqp::upload_state sets (tick.hip: the one definition of "a robot at tick 0") from the slot's staged rows,
//                               and writes the slot's standing record (kPlanRec doubles), its ref_traj entry and the robot's entry of the
//                               set table plan_hull_sets_kernel reads behind the fill
//   plan_restart_fill_kernel    one wave per (slot, 64-stage tile) of the host's list, the tiles from S / 64 on: a tile is 2560
//                               contiguous doubles of ONE repeating 40-double pattern, so nothing goes through LDS - 64 % 20 = 4, so a
//                               lane's twenty 16-byte pieces cycle through five pieces of the pattern, which it loads once; each store
//                               instruction of the wave covers 1 KiB, sixteen whole lines.  The same wave stores the tile's ref_traj and
//                               dcm_vel entries, one 16-byte piece per lane.  Pieces of stages below S (the first tile) and at or above T
//                               (the last) are skipped; a slot the first kernel did not restart leaves its tiles untouched.
// Plain vector loads and stores, 64-bit row offsets (the records pass 4 GB), 32-bit piece indices inside a tile.
// wcqp_tick_reset_robots (THE RESET ROBOT: a streamed EXTERNAL handle) runs the same two kernels with tick_reset_extern_kernel between
// them, and without a resident plan the first of them alone with it (tick_reset_enqueue, below).
#include "plan_gen.h"

namespace {

using namespace wcqp_tick;

constexpr int kRecPieces = kPlanRec / 2;             // 20 pieces per record
constexpr int kTile = 64, kTilePieces = kTile * kRecPieces, kPerLane = kTilePieces / 64;
static_assert(kPlanRec == 40 && kPlanLeft == 3 && kPlanTwL == 27 && kPlanHull == 39, "the standing record below is written by entry");
static_assert(kPerLane == kRecPieces && (64 * 5) % kRecPieces == 0, "a lane's pieces repeat with period 5");

__global__ __launch_bounds__(64) void plan_restart_reset_kernel(PlanRestartDev g) {
    const int r = blockIdx.x, lane = threadIdx.x;
    const size_t i = (size_t)g.robots[r];
    const long long failed = g.ik_fail[i];            // (every lane: read before any lane resets it - the branch below waits for it)
    const bool go = g.decided ? g.decided[r] != 0 : (g.mode[r] == WCQP_TICK_RESTART_ALWAYS || failed > 0);
    __syncthreads();
    if (lane == 0) { g.restarted[r] = go ? 1 : 0; g.stopped[r] = go ? failed : 0; }
    if (!go) return;
    const double* st0 = g.state0 + (size_t)r * kStateLen;
    // the standing stage: both feet in contact, the left one the fixed frame, the two soles of state0, twists 0, height state0[68]
    for (int e = lane; e < kPlanRec; e += 64) {
        double v = 0.0;
        if (e == kPlanFlags) v = 7.0;
        else if (e == kPlanHeight) v = st0[68];
        else if (e >= kPlanLeft && e < kPlanTwL) v = st0[24 + (e - kPlanLeft)];
        else if (e == kPlanHull) v = (double)g.set_slot[r];
        g.pattern[(size_t)r * kPlanRec + e] = v;
    }
    for (int e = lane; e < kStateLen; e += 64) g.state[i * kStateLen + e] = st0[e];
    for (int e = lane; e < kDof; e += 64) { g.q_des[i * kDof + e] = g.q0[(size_t)r * kDof + e]; g.dq_prev[i * kDof + e] = 0.0; }
    if (lane < 2) {
#pragma clang fp contract(off)
        const int ax = lane;
        const double zl = zmp_point_ax(st0 + 24, g.delta[0], ax), zr = zmp_point_ax(st0 + 36, g.delta[1], ax);
        const double mid = 0.5 * (zl + zr);
        const double c0 = g.com0[(size_t)r * 2 + ax];
        const double xi0 = g.dcm0 ? g.dcm0[(size_t)r * 2 + ax] : mid, u0 = g.u0 ? g.u0[(size_t)r * 2 + ax] : mid;
        g.mid[(size_t)r * 2 + ax] = mid;
        if (g.mst) {      // c_ref, v_ref_prev, com, u_prev, p_star, v_star_prev, dcm, measured ZMP
            double* m = g.mst + (i * 2 + ax) * 8;
            m[0] = c0; m[1] = 0.0; m[2] = c0; m[3] = u0; m[4] = c0; m[5] = 0.0; m[6] = xi0; m[7] = u0;
        }
        const size_t w = i * 2 + ax;
        g.dcm[w] = xi0; g.com[w] = c0; g.c_ref[w] = c0; g.p_star[w] = c0; g.zmp_meas[w] = u0; g.u_prev[w] = u0;
        g.v_ref_prev[w] = 0.0; g.v_star_prev[w] = 0.0;
    }
    if (g.zs && lane >= 4 && lane < 8) g.zs[i * 4 + (lane - 4)] = 0.0;        // the gain smoother at rest at the stance gains
    if (lane == 8) {
        if (g.sel_built) g.sel_built[i] = -1;
        if (g.live_nc) g.live_nc[i] = 0;
        g.sel[i] = 2;
        if (g.com_h0) g.com_h0[i] = st0[68];
        g.mpc_fail[i] = 0; g.ik_fail[i] = 0; g.hot_try[i] = 0; g.hot_hit[i] = 0;
        g.ik_lo[i] = 0u; g.ik_up[i] = 0u;
        if (g.ik_iters) g.ik_iters[i] = 0;
        // the robot's standing set: built from record S - the fill below writes it first - in its next free slot
        const int slot = g.set_slot[r];
        g.set_at[slot] = (long long)((i * (size_t)g.traj_len + (size_t)g.stage) * kPlanRec);
        g.set_code[slot] = 2;
    }
}

__global__ __launch_bounds__(64) void plan_restart_fill_kernel(PlanRestartDev g) {
    const int lane = threadIdx.x;
    const int r = g.tiles[blockIdx.x].x, s0 = g.tiles[blockIdx.x].y * kTile;
    if (!g.restarted[r]) return;
    const size_t i = (size_t)g.robots[r];
    const int T = g.traj_len;
    // the pieces of this tile that belong to stages [S, T)
    const int lo = (g.stage > s0 ? g.stage - s0 : 0) * kRecPieces;
    const int hi = (T - s0 < kTile ? T - s0 : kTile) * kRecPieces;
    const double2* pat = reinterpret_cast<const double2*>(g.pattern + (size_t)r * kPlanRec);
    // (five named registers pairs, not an array: nothing for the compiler to move into LDS)
    const double2 v0 = pat[lane % kRecPieces], v1 = pat[(lane + 64) % kRecPieces], v2 = pat[(lane + 128) % kRecPieces],
                  v3 = pat[(lane + 192) % kRecPieces], v4 = pat[(lane + 256) % kRecPieces];
    double2* out = reinterpret_cast<double2*>(g.rec + (i * (size_t)T + (size_t)s0) * kPlanRec);
    auto put = [&](int u, const double2& val) {
        const int x = lane + 64 * u;
        if (x >= lo && x < hi) out[x] = val;
    };
#pragma unroll
    for (int k = 0; k < kPerLane; k += 5) { put(k, v0); put(k + 1, v1); put(k + 2, v2); put(k + 3, v3); put(k + 4, v4); }
    const int s = s0 + lane;
    if (s < g.stage || s >= T) return;
    const size_t w = i * (size_t)T + (size_t)s;
    reinterpret_cast<double2*>(g.ref)[w] = *reinterpret_cast<const double2*>(g.mid + (size_t)r * 2);
    if (g.vel) reinterpret_cast<double2*>(g.vel)[w] = make_double2(0.0, 0.0);
}

// wcqp_tick_reset_robots (include/wcqp.h: THE RESET ROBOT): behind plan_restart_reset_kernel, one wave per slot, what only a streamed EXTERNAL
// handle keeps of a robot that restarted - the measured joints at q0, no rejected reading, no stage and no pair in hand (the upload's:
// wcqp::reset_streamed_stage), the measured state a reading rejected at tick S keeps - (com0, dcm0, u_init), in the hand-off record of parity
// S - 1 where tick_feedback_kernel and tick_sensor_kernel read it -, and the filter record the next sensor call reads at rest by the
// upload's rule, marked fresh (sensors.h).  Plain vector loads and stores, 64-bit row offsets.
__global__ __launch_bounds__(64) void tick_reset_extern_kernel(TickResetDev e) {
    const int r = blockIdx.x, lane = threadIdx.x;
    if (!e.restarted[r]) return;
    const size_t i = (size_t)e.robots[r];
    for (int k = lane; k < kDof; k += 64) e.q_meas[i * kDof + k] = e.q0[(size_t)r * kDof + k];
    for (int k = lane; k < kPlanRec; k += 64) e.st_rec[i * kPlanRec + k] = 0.0;
    if (lane < 2) e.pair[i * 2 + lane] = -1;
    if (lane == 2) { e.feedback_fail[i] = 0; e.st_set_nc[i] = 0; }
    if (e.hand_prev && lane >= 4 && lane < 6) {
        const int ax = lane - 4;
        const size_t w = (size_t)r * 2 + ax;
        double* hd = e.hand_prev + i * kHandLen;
        hd[4 + ax] = e.com0[w]; hd[6 + ax] = e.dcm0 ? e.dcm0[w] : e.mid[w]; hd[10 + ax] = e.u0 ? e.u0[w] : e.mid[w];
    }
    if (e.filt) {
        // {u_prev, y_prev} of the CoM position filter at com0, everything else 0 (wcqp::upload_state), the mark set
        for (int k = lane; k < kFiltRec; k += 64) {
            double v = 0.0;
            if (k == kFiltCom || k == kFiltCom + 1) v = e.com0[(size_t)r * 2];
            else if (k == kFiltCom + 4 || k == kFiltCom + 5) v = e.com0[(size_t)r * 2 + 1];
            else if (k == kFiltFresh) v = 1.0;
            e.filt[i * kFiltRec + k] = v;
        }
    }
}

}  // namespace

namespace wcqp {

// what both enqueue functions ask of the record: every array the reset kernel touches, and - plan: the handle holds a plan to stand the
// robots on - the fill's arrays and bounds
static bool restart_dev_valid(const PlanRestartDev& g, bool plan) {
    if (!g.robots || (!g.mode && !g.decided) || !g.state0 || !g.q0 || !g.com0 || !g.set_slot || !g.pattern || !g.mid || !g.restarted || !g.stopped ||
        !g.set_at || !g.set_code)
        return false;
    if (!g.state || !g.q_des || !g.dq_prev || !g.dcm || !g.com || !g.c_ref || !g.p_star || !g.zmp_meas || !g.u_prev || !g.v_ref_prev || !g.v_star_prev ||
        !g.sel || !g.mpc_fail || !g.ik_fail || !g.hot_try || !g.hot_hit || !g.ik_lo || !g.ik_up)
        return false;
    if (g.n_robots < 1 || g.stage < 0) return false;
    // (stage S has a record, and every tile of the list lies within the T stages: the host builds it from S / 64 to (T - 1) / 64)
    return !plan || (g.tiles && g.rec && g.ref && g.n_tiles >= 1 && g.traj_len >= 1 && g.stage < g.traj_len);
}

int tick_reset_enqueue(const PlanRestartDev& g, const TickResetDev& e, hipStream_t stream) {
    if (!restart_dev_valid(g, g.rec != nullptr) || g.decided) return WCQP_E_INVALID;
    if (e.robots != g.robots || e.restarted != g.restarted || e.mid != g.mid || !e.q0 || !e.com0 || !e.q_meas || !e.feedback_fail || !e.pair || !e.st_rec ||
        !e.st_set_nc || e.n_robots != g.n_robots)
        return WCQP_E_INVALID;
    hipLaunchKernelGGL(plan_restart_reset_kernel, dim3((unsigned)g.n_robots), dim3(64), 0, stream, g);
    hipLaunchKernelGGL(tick_reset_extern_kernel, dim3((unsigned)g.n_robots), dim3(64), 0, stream, e);
    if (g.rec) hipLaunchKernelGGL(plan_restart_fill_kernel, dim3((unsigned)g.n_tiles), dim3(64), 0, stream, g);
    WCQP_HIP_TRY(hipGetLastError());
    return WCQP_OK;
}

int plan_restart_enqueue(const PlanRestartDev& g, hipStream_t stream) {
    if (!restart_dev_valid(g, true)) return WCQP_E_INVALID;
    hipLaunchKernelGGL(plan_restart_reset_kernel, dim3((unsigned)g.n_robots), dim3(64), 0, stream, g);
    hipLaunchKernelGGL(plan_restart_fill_kernel, dim3((unsigned)g.n_tiles), dim3(64), 0, stream, g);
    WCQP_HIP_TRY(hipGetLastError());
    return WCQP_OK;
}

}  // namespace wcqp
