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

}  // namespace

namespace wcqp {

int plan_restart_enqueue(const PlanRestartDev& g, hipStream_t stream) {
    if (!g.robots || (!g.mode && !g.decided) || !g.state0 || !g.q0 || !g.com0 || !g.set_slot || !g.tiles || !g.pattern || !g.mid || !g.restarted || !g.stopped ||
        !g.set_at || !g.set_code || !g.rec || !g.ref)
        return WCQP_E_INVALID;
    if (!g.state || !g.q_des || !g.dq_prev || !g.dcm || !g.com || !g.c_ref || !g.p_star || !g.zmp_meas || !g.u_prev || !g.v_ref_prev || !g.v_star_prev ||
        !g.sel || !g.mpc_fail || !g.ik_fail || !g.hot_try || !g.hot_hit || !g.ik_lo || !g.ik_up)
        return WCQP_E_INVALID;
    // (stage S has a record, and every tile of the list lies within the T stages: the host builds it from S / 64 to (T - 1) / 64)
    if (g.n_robots < 1 || g.n_tiles < 1 || g.traj_len < 1 || g.stage < 0 || g.stage >= g.traj_len) return WCQP_E_INVALID;
    hipLaunchKernelGGL(plan_restart_reset_kernel, dim3((unsigned)g.n_robots), dim3(64), 0, stream, g);
    hipLaunchKernelGGL(plan_restart_fill_kernel, dim3((unsigned)g.n_tiles), dim3(64), 0, stream, g);
    WCQP_HIP_TRY(hipGetLastError());
    return WCQP_OK;
}

}  // namespace wcqp
