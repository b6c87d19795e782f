// A running generated plan moved `shift` = R stages towards 0, in place (wcqp_tick_rebase_plan; include/wcqp.h states THE REBASED PLAN,
// tests/helpers/plan_rebase.py restates it in numpy).  Two kernels in stream order:
//   plan_rebase_prologue_kernel   one thread per robot: d_i - the slots the robot's sets move down by - out of its OLD record R, and the
//                                 ZMP of the new stage 0; thread 0 takes R off both copies of the tick index
//   plan_rebase_move_kernel       one wave per (robot, array): records, ref_traj, dcm_vel, the robot's set rows
// The move goes towards lower addresses inside a robot's row, so ONE wave owns the row and walks it in ascending chunks of kChunk 16-byte
// pieces: kLoads loads per lane, a wait for ALL of the wave's outstanding loads, then the stores.  When R stages are fewer bytes than a
// chunk, its source and destination overlap, and data dependence orders a store only behind its own load - hence the explicit wait.
// Chunk k + 1's source lies above everything chunk k stored (for any R >= 1), so ascending order needs nothing more between chunks.
// Stages [T - R, T) then become copies of the old stage T - 1, which the wave read before it moved anything.  Entry 39 of a record - the
// set it names - goes down by d_i in flight: the lane that holds piece 19 of a record (doubles 38, 39) subtracts it from the second.
// 64-bit row offsets (the records pass 4 GB), 32-bit piece indices inside a row.  No LDS.
#include <cmath>
#include "plan_gen.h"

namespace {

using namespace wcqp_tick;

constexpr int kLoads = 8, kChunk = 64 * kLoads;      // 16-byte pieces a wave keeps in flight: 8 KiB
constexpr int kRecPieces = kPlanRec / 2;             // 20 pieces per record
static_assert(kPlanRec == 40 && kPlanHull == 39, "piece 19 of a record holds entries 38 and 39");

// the ZMP of stage R from what the plan keeps of it (the generator's own value is gone): xi - vel / omega where the handle keeps the DCM
// velocity (vel = omega (xi - z)), else the recursion solved for z, (xi_{R+1} - a xi_R) / (1 - a).  Every operation rounded on its own,
// as numpy does
__device__ __forceinline__ double stage_zmp(const PlanRebaseDev& g, size_t w) {
#pragma clang fp contract(off)
    if (g.vel) return g.ref[w] - g.vel[w] / g.omega;
    const double p = g.a * g.ref[w];
    return (g.ref[w + 2] - p) / (1.0 - g.a);
}

__global__ __launch_bounds__(64) void plan_rebase_prologue_kernel(PlanRebaseDev g) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i == 0) { g.tick2[0] -= g.shift; g.tick2[1] -= g.shift; }
    if (i >= g.batch) return;
    const size_t st = (size_t)i * (size_t)g.traj_len + (size_t)g.shift;
    int d = (int)g.rec[st * kPlanRec + kPlanHull] - i * g.cap;
    d = d < 0 ? 0 : (d < g.cap ? d : g.cap - 1);      // (a record names one of its robot's slots: a row move never leaves them)
    g.d_out[i] = d;
    g.zmp0[2 * (size_t)i] = stage_zmp(g, st * 2);
    g.zmp0[2 * (size_t)i + 1] = stage_zmp(g, st * 2 + 1);
}

__device__ __forceinline__ void loads_returned() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// pieces [off, n) of `row` move to [0, n - off), ascending, read before write.  REC: the pieces are a record's, 20 each, and the second
// double of every 20th goes down by `sub`
template <bool REC, class P>
__device__ __forceinline__ void move_down(P* row, int n, int off, int lane, double sub) {
    const int n_move = n - off;
    for (int base = 0; base < n_move; base += kChunk) {
        P v[kLoads];
#pragma unroll
        for (int u = 0; u < kLoads; ++u) {
            // (past the end of the last chunk a lane repeats the last piece and stores nothing: no branch among the loads)
            const int x = base + u * 64 + lane;
            v[u] = row[(size_t)(x < n_move ? x : n_move - 1) + (size_t)off];
        }
        loads_returned();
#pragma unroll
        for (int u = 0; u < kLoads; ++u) {
            const int x = base + u * 64 + lane;
            P w = v[u];
            if constexpr (REC) w.y = x % kRecPieces == kRecPieces - 1 ? w.y - sub : w.y;
            if (x < n_move) row[x] = w;
        }
    }
}

// a row of T stages, `pp` pieces each: stages [R, T) move to [0, T - R), and the R stages behind them take `last` - the lane's piece
// (lane % pp) of the old stage T - 1, read by the caller before the move - 64 / pp whole stages per store instruction
template <bool REC>
__device__ __forceinline__ void rebase_row(double2* row, int T, int R, int pp, int lane, double sub) {
    double2 last = row[(size_t)(T - 1) * (size_t)pp + (size_t)(lane % pp)];
    if (REC && lane % pp == kRecPieces - 1) last.y -= sub;
    loads_returned();
    move_down<REC>(row, T * pp, R * pp, lane, sub);
    const int per = 64 / pp;                          // whole stages per store instruction
    if (lane >= per * pp) return;
    for (int s = T - R + lane / pp; s < T; s += per) row[(size_t)s * (size_t)pp + (size_t)(lane % pp)] = last;
}

__global__ __launch_bounds__(64) void plan_rebase_move_kernel(PlanRebaseDev g) {
    const int lane = threadIdx.x, role = blockIdx.y;
    const size_t i = blockIdx.x;
    const int T = g.traj_len, R = g.shift, d = g.d_out[i];
    if (role == 0) {
        rebase_row<true>(reinterpret_cast<double2*>(g.rec + i * (size_t)T * kPlanRec), T, R, kRecPieces, lane, (double)d);
    } else if (role == 1) {
        rebase_row<false>(reinterpret_cast<double2*>(g.ref + i * (size_t)T * 2), T, R, 1, lane, 0.0);
    } else if (role == 2) {
        if (g.vel) rebase_row<false>(reinterpret_cast<double2*>(g.vel + i * (size_t)T * 2), T, R, 1, lane, 0.0);
    } else if (d > 0) {
        // the robot's rows in slots >= i cap + d move down by d: A is eight pieces a slot, b four, nc one int
        const size_t s0 = i * (size_t)g.cap;
        move_down<false>(reinterpret_cast<double2*>(g.set_A + s0 * 16), g.cap * 8, d * 8, lane, 0.0);
        move_down<false>(reinterpret_cast<double2*>(g.set_b + s0 * 8), g.cap * 4, d * 4, lane, 0.0);
        move_down<false>(g.set_nc + s0, g.cap, d, lane, 0.0);
    }
}

}  // namespace

namespace wcqp {

int plan_rebase_enqueue(const PlanRebaseDev& g, hipStream_t stream) {
    if (!g.rec || !g.ref || !g.zmp0 || !g.set_A || !g.set_b || !g.set_nc || !g.tick2 || !g.d_out) return WCQP_E_INVALID;
    // (stage R and the stage behind it exist, and a row's piece indices are 32-bit)
    if (g.batch < 1 || g.cap < 1 || g.shift < 1 || g.shift > g.traj_len - 2 || (long long)g.traj_len * kRecPieces >= (1ll << 31)) return WCQP_E_INVALID;
    hipLaunchKernelGGL(plan_rebase_prologue_kernel, dim3((unsigned)((g.batch + 63) / 64)), dim3(64), 0, stream, g);
    hipLaunchKernelGGL(plan_rebase_move_kernel, dim3((unsigned)g.batch, 4u), dim3(64), 0, stream, g);
    WCQP_HIP_TRY(hipGetLastError());
    return WCQP_OK;
}

}  // namespace wcqp
