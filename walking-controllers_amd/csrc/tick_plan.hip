// The trajectories of a tick handle (tick_handle.h; tick.hip holds the rest of it): planned ones uploaded per stage (wcqp_tick_upload of a
// planned handle), walks generated from footsteps and replanned at a merge stage - from the caller's footsteps or from goals, planned here
// on the device (plan_gen.hip holds the plan kernels, unicycle_device.h the planner) -, the streamed stage of the next tick, and the plan read back.  See include/wcqp.h for the contract.
// Timed and untimed generated plans take one path: what the host decides on a plan's timeline - merge stages, set counts, spans, the bound
// on stage indices - is goal_merge.h's wcqp_goal::Timeline, built by GenPlan::timeline(i) (the plan in force) or list_timeline (a caller's list).
#include <cmath>
#include <cstring>
#include <vector>
#include "tick_handle.h"
#include "plan_gen.h"
#include "goal_merge.h"
#include "unicycle_device.h"
#include "prepare_rows.h"

namespace {

using namespace wcqp_tick;

// planned trajectories: the support-polygon rows of every contact change (tick_device.h: PlanDev), one thread per set - the corners of
// the feet in contact at the set's stage (its record's desired poses) hulled by the builder of hull.hip
struct PlanRect { double v[8]; };
PlanRect plan_rect(const wcqp_tick_s* h) {
    PlanRect r;
    for (int k = 0; k < 8; ++k) r.v[k] = h->p.foot_rect[k];
    return r;
}
// (the hull build below - foot_points of the feet in contact, then hull_rows - stands again in tick_desired_kernel: as one device function
// both kernels' instruction streams move - DESIGN §8.23)
__global__ void __launch_bounds__(128) plan_hull_sets_kernel(int n, PlanRect rect, const double* __restrict__ rec, const long long* __restrict__ at,
                                      const int* __restrict__ code, double* __restrict__ A, double* __restrict__ b, int* __restrict__ nc) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    if (code[g] < 0) return;        // (a slot no set of this call occupies: generated plans keep a fixed range of slots per robot)
    const double* r = rec + at[g];
    double px[8], py[8];
    int np = 0;
    if (code[g] == 0 || code[g] == 2) wcqp_hull::foot_points(rect.v, r + kPlanLeft, px, py, np);
    if (code[g] == 1 || code[g] == 2) wcqp_hull::foot_points(rect.v, r + kPlanRight, px, py, np);
    nc[g] = wcqp_hull::hull_rows(px, py, np, A + (size_t)g * 16, b + (size_t)g * 8);
}

// streamed trajectories (wcqp_tick_set_desired_*): the stage of the next tick - what WalkingModule::updateModule pops from the front of the
// planner's deques (WM/src/WalkingModule.cpp:509-511, 689-707, 1085-1165) - packed into the robot's record (tick_device.h: kPlanRec, ONE
// per robot) and validated by the rules of the planned upload.  16 lanes per robot: lane j carries entries j, 16 + j and 32 + j.
// A robot whose stage is invalid keeps its previous record and is stopped and counted like one whose sensor reading was rejected
// (sensors.hip).  pair: per robot the contact pair of the last stage a tick consumed and of the stage in hand (-1 after an upload); `first`:
// this is the first stage handed over since the last tick, so the pair in hand has been consumed.  When the new pair differs from the
// consumed one, lane 0 builds the robot's support-polygon rows from this stage's feet with the builder of hull_device.h - here, not in the
// tick kernel - into set i, which entry 39 names: the chain of tick t copies them into the live rows on seeing the change
// (tick_mpc_finish_from, ...PredictiveController.cpp:364-435); with no change the rows stay, whatever the feet do.
struct DesiredDev {
    const double *left_pose, *right_pose, *left_twist, *right_twist, *com_height, *com_height_vel;
    const unsigned char* contact;
    const double* h0;               // [B] TickDev::com_h0: the height of a stage without one
    double* rec; double* set_A; double* set_b; int* set_nc; int* pair;
    long long *ik_fail, *feedback_fail;
    int batch, first, build;        // build: the handle's controller reads hull rows (the MPC)
};
__global__ __launch_bounds__(64) void tick_desired_kernel(DesiredDev a, PlanRect rect) {
    const int lane = threadIdx.x, grp = lane >> 4, j = lane & 15;
    const long inst_raw = (long)blockIdx.x * 4 + grp;
    const bool live = inst_raw < a.batch;
    const size_t i = (size_t)(live ? inst_raw : (long)a.batch - 1);
    const unsigned f = a.contact[i];
    // entries j (flags, height, its velocity, the left pose and the first of the right), 16 + j, 32 + j (< 40: the twists' tail, the set)
    double v0, v1, v2 = 0.0;
    if (j == kPlanFlags) v0 = (double)f;
    else if (j == kPlanHeight) v0 = a.com_height ? a.com_height[i] : a.h0[i];
    else if (j == kPlanHeightVel) v0 = a.com_height_vel ? a.com_height_vel[i] : 0.0;
    else if (j < kPlanRight) v0 = a.left_pose[i * 12 + (j - kPlanLeft)];
    else v0 = a.right_pose[i * 12 + (j - kPlanRight)];
    const int k1 = 16 + j;
    v1 = k1 < kPlanTwL ? a.right_pose[i * 12 + (k1 - kPlanRight)] : a.left_twist[i * 6 + (k1 - kPlanTwL)];
    const int k2 = 32 + j;
    if (k2 < kPlanTwL + 6) v2 = a.left_twist[i * 6 + (k2 - kPlanTwL)];
    else if (k2 < kPlanHull) v2 = a.right_twist[i * 6 + (k2 - kPlanTwL - 6)];
    else if (k2 == kPlanHull) v2 = (double)i;
    const bool flags_bad = (f & 3u) == 0u || ((f & 4u) ? !(f & 1u) : !(f & 2u));       // no foot in contact / the fixed-frame foot is not
    const bool lane_bad = flags_bad || !(isfinite(v0) && isfinite(v1) && isfinite(v2));
    const bool bad = ((__ballot(lane_bad) >> (grp * 16)) & 0xffffull) != 0ull;
    if (!live) return;
    int* pr = a.pair + i * 2;
    const int consumed = a.first ? pr[1] : pr[0];
    if (bad) {
        if (j == 0) {
            pr[0] = consumed;
            a.feedback_fail[i] += 1;
            if (a.ik_fail[i] == 0) a.ik_fail[i] = 1;
        }
        return;
    }
    double* r = a.rec + i * kPlanRec;
    r[j] = v0; r[k1] = v1;
    if (k2 <= kPlanHull) r[k2] = v2;
    if (j != 0) return;
    const int code = (int)(f & 3u) - 1;
    pr[0] = consumed; pr[1] = code;
    if (a.build && code != consumed) {
        double px[8], py[8];
        int np = 0;
        if (code == 0 || code == 2) wcqp_hull::foot_points(rect.v, a.left_pose + i * 12, px, py, np);
        if (code == 1 || code == 2) wcqp_hull::foot_points(rect.v, a.right_pose + i * 12, px, py, np);
        a.set_nc[i] = wcqp_hull::hull_rows(px, py, np, a.set_A + i * 16, a.set_b + i * 8);
    }
}

// a resident plan (wcqp_tick_set_desired_from_plan): the stage of the next tick out of the plan the handle holds, in tick_desired_kernel's
// place and layout - 16 lanes per robot, four robots per wave, the dead slots of the last wave repeat the last robot and store nothing.
// t is the handle's tick index in device memory (TickDev::tick2, the copy the next launch reads).  Lane j copies entries j, 16 + j and
// 32 + j of plan record (i, t) into the robot's live record, whose entry 39 names the robot's own set i; lanes 0..7 copy the row set the
// plan's record names into that set, lane 0 its row count.  Nothing is validated (the upload did) and no hull is built: the rows exist,
// and the chain of tick t copies them into the live rows on a change of pair, as for every streamed handle.  pair / first: as above.
struct StageDev {
    wcqp::GPtr<const double> plan, set_A, set_b; wcqp::GPtr<const int> set_nc;      // the resident plan: [B][traj_len][kPlanRec], its sets
    wcqp::GPtr<const int> tick;
    wcqp::GPtr<double> rec, st_A, st_b; wcqp::GPtr<int> st_nc, pair;                // the live record and set of every robot, the pairs
    int batch, traj_len, first;
};
__global__ __launch_bounds__(64) void tick_stage_from_plan_kernel(StageDev a) {
    const int lane = threadIdx.x, grp = lane >> 4, j = lane & 15;
    const long inst_raw = (long)blockIdx.x * 4 + grp;
    const bool live = inst_raw < a.batch;
    const size_t i = (size_t)(live ? inst_raw : (long)a.batch - 1);
    const int t = *a.tick.get();
    const double* src = a.plan.get() + (i * (size_t)a.traj_len + (size_t)t) * (size_t)kPlanRec;       // (64-bit: the plan passes 4 GB)
    const double v0 = src[j], v1 = src[16 + j], v2 = j < 8 ? src[32 + j] : 0.0;
    const double flags = src[kPlanFlags];
    const size_t set = (size_t)src[kPlanHull];
    double2 rA = make_double2(0.0, 0.0);
    double rb = 0.0;
    if (j < WCQP_HULL_ROWS) {
        rA = reinterpret_cast<const double2*>(a.set_A.get())[set * WCQP_HULL_ROWS + j];
        rb = a.set_b.get()[set * WCQP_HULL_ROWS + j];
    }
    if (!live) return;
    double* r = a.rec.get() + i * kPlanRec;
    r[j] = v0; r[16 + j] = v1;
    if (j < 7) r[32 + j] = v2;
    if (j == 7) r[kPlanHull] = (double)i;
    if (j < WCQP_HULL_ROWS) {
        reinterpret_cast<double2*>(a.st_A.get())[i * WCQP_HULL_ROWS + j] = rA;
        a.st_b.get()[i * WCQP_HULL_ROWS + j] = rb;
    }
    if (j != 0) return;
    a.st_nc.get()[i] = a.set_nc.get()[set];
    int* pr = a.pair.get() + i * 2;
    const int consumed = a.first ? pr[1] : pr[0];
    pr[0] = consumed; pr[1] = ((int)flags & 3) - 1;
}

// A valid stage of one robot, for the planned upload and the streamed host form alike: a foot in contact, the fixed-frame foot in contact,
// finite poses [12], twists [6] and heights (height / height_vel: the stage's own entry, or NULL for none)
bool stage_valid(unsigned f, const double* left_pose, const double* right_pose, const double* left_twist, const double* right_twist,
                 const double* height, const double* height_vel) {
    if ((f & 3u) == 0u) return false;                          // neither foot in contact
    if ((f & 4u) ? !(f & 1u) : !(f & 2u)) return false;        // the fixed-frame foot is not in contact
    bool ok = true;
    for (int k = 0; k < 12; ++k) ok = ok && std::isfinite(left_pose[k]) && std::isfinite(right_pose[k]);
    for (int k = 0; k < 6; ++k) ok = ok && std::isfinite(left_twist[k]) && std::isfinite(right_twist[k]);
    if (height) ok = ok && std::isfinite(*height);
    if (height_vel) ok = ok && std::isfinite(*height_vel);
    return ok;
}

// A valid footstep list of robot i, for the upload and the replan alike: 0 <= n <= K steps, each with a side <= 1 and a finite target
bool footsteps_valid(size_t i, int K, const int32_t* n_steps, const uint8_t* side, const double* target) {
    const int n = n_steps[i];
    if (n < 0 || n > K) return false;
    for (int k = 0; k < n; ++k) {
        if (side[i * K + k] > 1) return false;
        for (int c = 0; c < 3; ++c) if (!std::isfinite(target[(i * K + k) * 3 + c])) return false;
    }
    return true;
}

// The timeline (goal_merge.h) of robot i's footstep list, n of at most K steps (a valid list: see above) from stage `origin` behind a first
// double support of first_ds stages: on the caller's per-step rows tm [B][K] (the timed calls), or - tm NULL - on the common (ss, ds)
wcqp_goal::Timeline list_timeline(size_t i, int K, int origin, int first_ds, int n, const wcqp_tick_step_timing* tm, int ss, int ds) {
    if (!tm) return wcqp_goal::Timeline::uniform(origin, first_ds, n, ss, ds);
    return wcqp_goal::Timeline::per_step(origin, first_ds, n, tm->ss_ticks + i * K, tm->ds_ticks + i * K, 1);
}

// What every pass of plan_gen.hip takes of a handle whose GenPlan scalars are in place, for lists of at most K steps per robot; the caller
// adds its own list pointers and first_ds (and a replan its origins, robots, tiles and h0)
PlanGenDev plan_gen_of(const wcqp_tick_s* h, int K) {
    const TickDev& d = h->d;
    const auto& gp = h->gp;
    PlanGenDev g{};
    g.state = d.state;
    g.rec = h->plan_rec; g.ref = const_cast<double*>(d.ref_traj.get());
    g.vel = (d.reactive || d.gain_sched) ? const_cast<double*>(d.dcm_vel.get()) : nullptr;
    g.zmp0 = h->gen_zmp0;
    g.batch = d.batch; g.K = K; g.traj_len = d.traj_len; g.max_ticks = h->p.max_ticks;
    g.ss = gp.ss; g.ds = gp.ds; g.final_ds = gp.final_ds;
    g.lift = gp.lift; g.dT = d.dT; g.omega = d.omega; g.a = std::exp(d.omega * d.dT);
    for (int k = 0; k < 2; ++k) { g.delta[0][k] = gp.delta[0][k]; g.delta[1][k] = gp.delta[1][k]; }
    return g;
}
// ... and the swing profile of the plan in force, the shaped record kernels' second argument (all zero: the launch path takes the others)
PlanSwing plan_swing_of(const wcqp_tick_s* h) {
    const wcqp_tick_swing_profile& s = h->gp.swing;
    return PlanSwing{s.apex_ratio, s.landing_velocity, s.pitch_delta, s.com_height_delta};
}

// the support-polygon row sets of a plan whose records are in place (in NULL-stream order): the previous upload's go, `ns` new ones are built
// on the device from the records of their stages (at: record offsets, code: contact pairs - device arrays), and the handle's kernels see them
int build_plan_sets(wcqp_tick_s* h, size_t ns, const long long* d_at, const int* d_code) {
    for (void* p : {(void*)h->set_A, (void*)h->set_b, (void*)h->set_nc}) if (p) (void)hipFree(p);
    h->set_A = nullptr; h->set_b = nullptr; h->set_nc = nullptr; h->n_sets = 0;
    if (hipMalloc(reinterpret_cast<void**>(&h->set_A), ns * 128) != hipSuccess || hipMalloc(reinterpret_cast<void**>(&h->set_b), ns * 64) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&h->set_nc), ns * 4) != hipSuccess)
        return WCQP_E_NOMEM;
    hipLaunchKernelGGL(plan_hull_sets_kernel, dim3((unsigned)((ns + 127) / 128)), dim3(128), 0, 0, (int)ns, plan_rect(h), h->plan_rec, d_at, d_code,
                       h->set_A, h->set_b, h->set_nc);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return WCQP_E_HIP;
    h->n_sets = ns;
    // a resident plan's sets stay behind the staging kernel (a launch argument): the tick's kernels keep the robots' own
    if (!h->planned) return WCQP_OK;
    // the kernels read the sets through the handle's TickDevPL in device memory
    h->pl.set_A = h->set_A; h->pl.set_b = h->set_b; h->pl.set_nc = h->set_nc;
    const TickDevPL g = h->dpl(h->d);
    WCQP_HIP_TRY(hipMemcpy(h->d_dev, &g, sizeof(TickDevPL), hipMemcpyHostToDevice));
    return WCQP_OK;
}
}  // namespace


// planned trajectories: the caller's per-stage arrays checked over the stages a run can reach (0 .. max_ticks), before anything of the
// handle changes
int wcqp::validate_plan(const wcqp_tick_s* h, const wcqp_tick_inputs* in) {
    const TickDev& d = h->d;
    const size_t B = (size_t)d.batch, T = (size_t)d.traj_len, reach = (size_t)h->p.max_ticks + 1;
    if (!in->left_traj || !in->right_traj || !in->left_twist || !in->right_twist || !in->contact) return WCQP_E_INVALID;
    for (size_t i = 0; i < B; ++i)
        for (size_t t = 0; t < reach; ++t) {
            const size_t w = i * T + t;
            if (!stage_valid(in->contact[w], in->left_traj + w * 12, in->right_traj + w * 12, in->left_twist + w * 6, in->right_twist + w * 6,
                             in->com_height_traj ? in->com_height_traj + w : nullptr, in->com_height_vel ? in->com_height_vel + w : nullptr))
                return WCQP_E_INVALID;
        }
    return WCQP_OK;
}

// ... repacked into the records (tick_device.h: kPlanRec), a slab of robots at a time, and the support-polygon row set of every change of
// contact pair (and of stage 0) built from its stage's desired feet; the records name the set in force
int wcqp::upload_plan(wcqp_tick_s* h, const wcqp_tick_inputs* in) {
    const TickDev& d = h->d;
    const size_t B = (size_t)d.batch, T = (size_t)d.traj_len, reach = (size_t)h->p.max_ticks + 1;
    std::vector<long long> set_at;       // record offset (doubles) of each set's stage
    std::vector<int> set_code;           // its contact pair (0 left, 1 right, 2 both)
    std::vector<double> set_of(B * T);   // the set in force at each stage
    for (size_t i = 0; i < B; ++i) {
        int prev = -1;
        for (size_t t = 0; t < T; ++t) {
            const int pair = (int)(in->contact[i * T + t] & 3u);
            if (t < reach && pair != prev) {       // (beyond the reach no tick changes the pair: the last set stays)
                set_at.push_back((long long)((i * T + t) * kPlanRec));
                set_code.push_back(pair - 1);
                prev = pair;
            }
            set_of[i * T + t] = (double)(set_at.size() - 1);
        }
    }
    const size_t slab = 256;
    std::vector<double> rec(slab * T * kPlanRec);
    for (size_t i0 = 0; i0 < B; i0 += slab) {
        const size_t n = B - i0 < slab ? B - i0 : slab;
        for (size_t i = i0; i < i0 + n; ++i) {
            const double h0 = in->state0[i * kStateLen + 68];
            for (size_t t = 0; t < T; ++t) {
                const size_t w = i * T + t;
                double* r = &rec[((i - i0) * T + t) * kPlanRec];
                r[kPlanFlags] = (double)in->contact[w];
                r[kPlanHeight] = in->com_height_traj ? in->com_height_traj[w] : h0;
                r[kPlanHeightVel] = in->com_height_vel ? in->com_height_vel[w] : 0.0;
                std::memcpy(r + kPlanLeft, in->left_traj + w * 12, 96); std::memcpy(r + kPlanRight, in->right_traj + w * 12, 96);
                std::memcpy(r + kPlanTwL, in->left_twist + w * 6, 48); std::memcpy(r + kPlanTwL + 6, in->right_twist + w * 6, 48);
                r[kPlanHull] = set_of[w];
            }
        }
        WCQP_HIP_TRY(hipMemcpy(h->plan_rec + i0 * T * kPlanRec, rec.data(), n * T * kPlanRec * 8, hipMemcpyHostToDevice));
    }
    // the row sets, built on the device from the records just copied
    const size_t ns = set_at.size();
    long long* d_at = nullptr; int* d_code = nullptr;
    int rc = WCQP_OK;
    if (hipMalloc(reinterpret_cast<void**>(&d_at), ns * 8) != hipSuccess || hipMalloc(reinterpret_cast<void**>(&d_code), ns * 4) != hipSuccess) rc = WCQP_E_NOMEM;
    if (rc == WCQP_OK && (hipMemcpy(d_at, set_at.data(), ns * 8, hipMemcpyHostToDevice) != hipSuccess ||
                          hipMemcpy(d_code, set_code.data(), ns * 4, hipMemcpyHostToDevice) != hipSuccess))
        rc = WCQP_E_HIP;
    if (rc == WCQP_OK) rc = build_plan_sets(h, ns, d_at, d_code);
    (void)hipFree(d_at); (void)hipFree(d_code);
    return rc;
}

namespace {

// Footsteps from goals for the robots a replan lists (wcqp_tick_replan_goals): one lane per listed robot, 64 per wave, one wave per
// workgroup, as unicycle_kernel - the same per-robot body (unicycle_device.h), a latency chain of K x D RK4 steps that wants no more
// than to stay clear of scratch.  Lane `slot` takes robot i = robots[slot]: the sole entries the planner reads of plan record M_i =
// origin[i] (a stage with both feet down), the flag word of record M_i - 1 (M_i >= 1) for a first_side of WCQP_TICK_SIDE_AUTO - the
// fixed-frame foot of that stage swings first: bit 2 set, the left one (0) -, and row i of the call's result rows, which the replan kernels
// behind it read as their footstep lists.  A robot that keeps its plan has no lane; dead lanes of the last wave repeat the last listed
// robot and store nothing.  Plain vector loads and stores, 64-bit offsets (the records pass 4 GB), no LDS.
struct GoalPlanDev {
    wcqp_unicycle::UniPar p;
    const double* rec;              // the plan records [B][traj_len][kPlanRec]
    const int* origin;              // [B] M_i of the listed robots
    const int* robots;              // [n_robots]
    const double* goal;             // [B][2]
    const unsigned char* side_in;   // [B] 0 / 1 / WCQP_TICK_SIDE_AUTO
    unsigned char* first_side;      // [B] the side taken
    wcqp_unicycle::UniRows out;
    int n_robots, traj_len;
};
// robot i's start: the soles of plan record M_i, the goal, and the side that swings first
__device__ __forceinline__ wcqp_unicycle::UniStart goal_start(const GoalPlanDev& a, size_t i) {
    const double* r = a.rec + (i * (size_t)a.traj_len + (size_t)a.origin[i]) * (size_t)kPlanRec;
    const unsigned flags = (unsigned)r[kPlanFlags - kPlanRec];
    int sw = a.side_in[i];
    if (sw == WCQP_TICK_SIDE_AUTO) sw = (flags & 4u) ? 0 : 1;
    const double *l = r + kPlanLeft, *q = r + kPlanRight;
    return {l[0], l[1], l[3], l[6], q[0], q[1], q[3], q[6], a.goal[i * 2], a.goal[i * 2 + 1], sw};
}
__global__ __launch_bounds__(64) void goal_plan_kernel(GoalPlanDev a) {
    const long raw = (long)blockIdx.x * 64 + threadIdx.x;
    const bool live = raw < a.n_robots;
    const size_t i = (size_t)a.robots[live ? raw : (long)a.n_robots - 1];
    const wcqp_unicycle::UniStart in = goal_start(a, i);
    if (live) a.first_side[i] = (unsigned char)in.sw;
    wcqp_unicycle::plan_robot(a.p, in, a.out, i, live);
}

// Its timed sibling (wcqp_tick_replan_goals_timed): the same lanes, loads and side rule, the timed body of unicycle_timed_kernel - every
// step's durations are chosen with its target and stored in rows i of tm.ss_ticks / tm.ds_ticks, which lie in the call's result rows next
// to a.out's and are the PlanTimes::ss_k / ds_k of the timed replan kernels behind it.
struct GoalPlanTimedDev {
    GoalPlanDev a;
    wcqp_unicycle::UniTiming tm;
};
__global__ __launch_bounds__(64) void goal_plan_timed_kernel(GoalPlanTimedDev t) {
    const GoalPlanDev& a = t.a;
    const long raw = (long)blockIdx.x * 64 + threadIdx.x;
    const bool live = raw < a.n_robots;
    const size_t i = (size_t)a.robots[live ? raw : (long)a.n_robots - 1];
    const wcqp_unicycle::UniStart in = goal_start(a, i);
    if (live) a.first_side[i] = (unsigned char)in.sw;
    wcqp_unicycle::plan_robot_timed(a.p, t.tm, in, a.out, i, live);
}

// the stage below which the enqueued ticks have consumed the plans in force (gp.timeline(i): settled by the caller): a resident plan's tick
// whose stage has been staged counts as enqueued, its live record holds that stage
int consumed_stages(const wcqp_tick_s* h) { return h->ticks_enqueued + (h->plan_staged ? 1 : 0); }

// What a replan needs of the host per call, for footsteps from the caller's lists and from goals alike: per robot the merge stage (-1: it
// keeps its plan), the compaction into robots and (robot, tile) pairs, and the sets that survive
struct ReplanCall {
    std::vector<int> merge, robots, keep, tiles;
    explicit ReplanCall(size_t B) : merge(B, -1), keep(B, 0) {}
};

// Robot i joins the call at merge stage M (already found allowed: wcqp_goal::merge_allowed).  fresh: the sets its new plan builds behind
// M where a tick can reach them - counted on the caller's list, or, where the device plans the steps, bounded by goal_sets_bound below.
// Its surviving sets are those of stages <= M (a set of stage M itself is built from the feet the new plan starts from); the new
// plan's sets follow them in the robot's `cap` slots, and a call whose sets would pass them is refused: plan_prologue writes its set
// table without a bound of its own.  cap (upload_footsteps) bounds the steps that START at a stage <= max_ticks for ANY stitched footstep
// list - an untimed step occupies ss + 1 stages or more, a timed one a stage of single and a stage of double support -, so for a robot
// that only ever walked the check never fires.  It fires for a robot that spent slots on restarts (wcqp_tick_restart_robots takes one
// per call, with no step behind it) since the last rebase: that robot is refused here until wcqp_tick_rebase_plan has freed them.
int replan_admit(const wcqp_tick_s* h, size_t i, int M, int fresh, ReplanCall& c) {
    const auto& gp = h->gp;
    const int c0 = gp.keep[i] + gp.timeline(i).sets_up_to(M < h->p.max_ticks ? M : h->p.max_ticks);
    if (c0 < 1 || c0 + fresh > gp.cap) return WCQP_E_INVALID;
    c.merge[i] = M; c.keep[i] = c0;
    c.robots.push_back((int)i);
    const int n_tile = (h->d.traj_len + 63) / 64;
    for (int tl = M / 64; tl < n_tile; ++tl) { c.tiles.push_back((int)i); c.tiles.push_back(tl); }
    return WCQP_OK;
}

// The sets a goal call's new plan can build, whatever steps the device chooses: at most K steps, the first at stage M + fd, each `spacing`
// stages or more behind the one before (an untimed plan: exactly ss + ds; a timed one: the planner's min_step_ticks, two at least), two
// sets for each that starts at a stage <= max_ticks.  With floor(M / L) steps landed by M at most (L = ss + 1, or 2) this stays within
// cap for every stitched list of steps: floor(M / L) + floor((max_ticks - M - 1) / L) + 1 <= (max_ticks + 1) / L + 1
int goal_sets_bound(int K, int M, int fd, long long spacing, int max_ticks) {
    const long long room = (long long)max_ticks - M - fd;
    if (room < 0 || K < 1) return 0;
    const long long n = room / (spacing < 2 ? 2 : spacing) + 1;
    return 2 * (int)(n < K ? n : K);
}

// where the footsteps of a replan come from: the caller's lists (wcqp_tick_replan_footsteps), or goals the device plans from
// (wcqp_tick_replan_goals: goal [B][2], first_side [B] or NULL for WCQP_TICK_SIDE_AUTO everywhere, the planner's parameters, the layout
// of the call's result rows)
struct ReplanSource {
    const wcqp_tick_replan* lists;
    const double* goal; const uint8_t* first_side; const wcqp_unicycle::UniPar* par;
    const wcqp_tick_s::GoalRows* rows;
    const wcqp_tick_step_timing* tm = nullptr;      // with lists, on a timed plan: the new steps' durations
    const wcqp_unicycle::UniTiming* utm = nullptr;  // with goals, on a timed plan: the timed planner's range and score (its rows: set here)
};

// Everything behind the checks, for a call that lists a robot at least: the call's device block - what the host hands over first (one
// copy, taken NOW, once the previous replan has left the block), then what the kernels write for each other -, the kernels on `st` behind
// the ticks already enqueued, the guard, and the plan in force of the listed robots.  The replan kernels read their footstep rows -
// n_steps, side, target, on a timed plan ss_k and ds_k - at `steps`: the caller's, staged in the block's front, or the result rows
// goal_plan_kernel (timed: goal_plan_timed_kernel) writes ahead of them.  Those travel back in one copy, with an event behind it, and
// the listed robots' step counts - and durations - are owed until then (tick_handle.h: GoalCall).  Synchronises with nothing but the
// block's own wait.
int replan_enqueue(wcqp_tick_s* h, const ReplanCall& c, int K, int fd, const ReplanSource& src, hipStream_t st) {
    const TickDev& d = h->d;
    auto& gp = h->gp;
    auto& gc = h->goal;
    const bool goals = src.lists == nullptr;
    const int cap = gp.cap;
    const size_t B = (size_t)d.batch, BK = B * (size_t)K, nr = c.robots.size(), nt = c.tiles.size() / 2, nslots = B * (size_t)cap;
    const wcqp_tick_s::GoalRows gr = goals ? *src.rows : wcqp_tick_s::GoalRows{};
    size_t off = 0;
    auto carve = [&off](size_t bytes) { const size_t at = off; off += (bytes + 255) & ~(size_t)255; return at; };
    const size_t o_org = carve(B * 4), o_base = carve(B * 4), o_rob = carve(nr * 4), o_tile = carve(nt * 8);
    struct StepRows { size_t n, side, target, ss, ds; } steps{};
    if (!goals) { steps.n = carve(B * 4); steps.side = carve(BK); steps.target = carve(BK * 24); }
    const size_t o_goal = goals ? carve(B * 16) : 0, o_fsin = goals ? carve(B) : 0;
    if (src.tm) { steps.ss = carve(BK * 4); steps.ds = carve(BK * 4); }
    const size_t front = off;
    const size_t o_res = goals ? carve(gr.bytes) : 0;
    if (goals) steps = StepRows{o_res + gr.n, o_res + gr.side, o_res + gr.target, o_res + gr.ss, o_res + gr.ds};
    const size_t o_tab = carve(B * (size_t)(K + 1) * kFpRec * 8), o_at = carve(nslots * 8), o_code = carve(nslots * 4);
    size_t o_start = 0;
    if (gp.timed) o_start = carve(B * (size_t)(K + 1) * 4);       // (PlanTimes::start)
    std::vector<char> blob(front, 0);
    {
        int* org = reinterpret_cast<int*>(blob.data() + o_org); int* base = reinterpret_cast<int*>(blob.data() + o_base);
        for (size_t i = 0; i < B; ++i) {
            const bool on = c.merge[i] != -1;
            org[i] = on ? c.merge[i] : -1;
            base[i] = (int)(i * (size_t)cap) + (on ? c.keep[i] - 1 : 0);
        }
        std::memcpy(blob.data() + o_rob, c.robots.data(), nr * 4); std::memcpy(blob.data() + o_tile, c.tiles.data(), nt * 8);
        if (!goals) {
            int* nn = reinterpret_cast<int*>(blob.data() + steps.n);
            for (size_t i = 0; i < B; ++i) nn[i] = c.merge[i] != -1 ? src.lists->n_steps[i] : 0;
            if (BK > 0) { std::memcpy(blob.data() + steps.side, src.lists->side, BK); std::memcpy(blob.data() + steps.target, src.lists->target, BK * 24); }
            if (src.tm && BK > 0) { std::memcpy(blob.data() + steps.ss, src.tm->ss_ticks, BK * 4); std::memcpy(blob.data() + steps.ds, src.tm->ds_ticks, BK * 4); }
        } else {
            // (a goal of a robot that keeps its plan may be anything, a NaN too: its row is zero here and no lane reads it)
            double* gl = reinterpret_cast<double*>(blob.data() + o_goal);
            for (int i : c.robots) { gl[(size_t)i * 2] = src.goal[(size_t)i * 2]; gl[(size_t)i * 2 + 1] = src.goal[(size_t)i * 2 + 1]; }
            unsigned char* fs = reinterpret_cast<unsigned char*>(blob.data() + o_fsin);
            for (size_t i = 0; i < B; ++i) fs[i] = src.first_side ? src.first_side[i] : (unsigned char)WCQP_TICK_SIDE_AUTO;
        }
    }
    if (goals) {      // the pinned rows the results come back into (the previous call's have been folded in: the caller settled)
        if (!gc.ev) WCQP_HIP_TRY(hipEventCreateWithFlags(&gc.ev, hipEventDisableTiming));
        if (gc.host_cap < gr.bytes) {
            if (gc.host) (void)hipHostFree(gc.host);
            gc.host = nullptr; gc.host_cap = 0;
            if (hipHostMalloc(reinterpret_cast<void**>(&gc.host), gr.bytes, hipHostMallocDefault) != hipSuccess) return WCQP_E_NOMEM;
            gc.host_cap = gr.bytes;
        }
    }
    if (const int rc = h->rp.take(h->copy_stream, blob.data(), front, off); rc != WCQP_OK) return rc;
    char* buf = static_cast<char*>(h->rp.mem.ptr);
    char* res = buf + o_res;
    PlanGenDev g = plan_gen_of(h, K);
    g.origin = reinterpret_cast<const int*>(buf + o_org);
    g.set_base = reinterpret_cast<const int*>(buf + o_base); g.robots = reinterpret_cast<const int*>(buf + o_rob);
    g.tiles = reinterpret_cast<const int2*>(buf + o_tile);
    g.n_steps = reinterpret_cast<const int*>(buf + steps.n);
    g.side = reinterpret_cast<const unsigned char*>(buf + steps.side);
    g.target = reinterpret_cast<const double*>(buf + steps.target);
    g.table = reinterpret_cast<double*>(buf + o_tab);
    g.set_at = reinterpret_cast<long long*>(buf + o_at); g.set_code = reinterpret_cast<int*>(buf + o_code);
    g.h0 = d.com_h0.get(); g.n_robots = (int)nr; g.n_tiles = (int)nt; g.first_ds = fd;
    // in the caller's stream order, behind the ticks already enqueued: no pointer a tick or a captured graph holds changes, and the set
    // slots written are those past each robot's surviving ones, which no stage below its merge stage names
    if (goals) {
        WCQP_HIP_TRY(hipMemsetAsync(res, 0, gr.bytes, st));      // (the rows of robots without a lane read back as zeros)
        GoalPlanDev a{};
        a.p = *src.par; a.rec = h->plan_rec; a.origin = g.origin; a.robots = g.robots;
        a.goal = reinterpret_cast<const double*>(buf + o_goal); a.side_in = reinterpret_cast<const unsigned char*>(buf + o_fsin);
        a.first_side = gr.at<unsigned char>(res, gr.fs);
        a.out = wcqp_unicycle::UniRows{gr.at<int32_t>(res, gr.n), gr.at<int32_t>(res, gr.status), gr.at<uint8_t>(res, gr.side),
                                       gr.at<double>(res, gr.target), gr.at<double>(res, gr.dp), gr.at<double>(res, gr.ue)};
        a.n_robots = (int)nr; a.traj_len = d.traj_len;
        if (src.utm) {
            GoalPlanTimedDev t{a, *src.utm};
            t.tm.ss_ticks = gr.at<int32_t>(res, gr.ss); t.tm.ds_ticks = gr.at<int32_t>(res, gr.ds);
            hipLaunchKernelGGL(goal_plan_timed_kernel, dim3((unsigned)((nr + 63) / 64)), dim3(64), 0, st, t);
        } else {
            hipLaunchKernelGGL(goal_plan_kernel, dim3((unsigned)((nr + 63) / 64)), dim3(64), 0, st, a);
        }
        WCQP_HIP_TRY(hipGetLastError());
    }
    WCQP_HIP_TRY(hipMemsetAsync(g.set_code, 0xff, nslots * 4, st));
    if (gp.timed) {
        const PlanGenTimedDev t{g, PlanTimes{reinterpret_cast<const int*>(buf + steps.ss), reinterpret_cast<const int*>(buf + steps.ds),
                                             reinterpret_cast<int*>(buf + o_start), gp.final_ds}};
        if (const int rc = wcqp::plan_replan_enqueue(t, plan_swing_of(h), st); rc != WCQP_OK) return rc;
    } else if (const int rc = wcqp::plan_replan_enqueue(g, plan_swing_of(h), st); rc != WCQP_OK) return rc;
    hipLaunchKernelGGL(plan_hull_sets_kernel, dim3((unsigned)((nslots + 127) / 128)), dim3(128), 0, st, (int)nslots, plan_rect(h), h->plan_rec, g.set_at, g.set_code,
                       h->set_A, h->set_b, h->set_nc);
    WCQP_HIP_TRY(hipGetLastError());
    if (goals) {
        WCQP_HIP_TRY(hipMemcpyAsync(gc.host, res, gr.bytes, hipMemcpyDeviceToHost, st));
        WCQP_HIP_TRY(hipEventRecord(gc.ev, st));
    }
    if (const int rc = h->rp.guard(st); rc != WCQP_OK) return rc;
    for (int i : c.robots) {
        gp.origin[i] = c.merge[i]; gp.first_ds[i] = fd; gp.keep[i] = c.keep[i];
        if (!goals) gp.set_steps((size_t)i, src.lists->n_steps[i], src.tm ? src.tm->ss_ticks + (size_t)i * K : nullptr, src.tm ? src.tm->ds_ticks + (size_t)i * K : nullptr);
    }
    if (goals) { gc.pending = true; gc.owed = c.robots; gc.rows = gr; }
    return WCQP_OK;
}

// what both replans ask of the handle before they look at a robot
int replan_ready(const wcqp_tick_s* h) {
    if (!h->holds_plan()) return WCQP_E_UNSUPPORTED;
    if (!h->uploaded) return WCQP_E_INVALID;
    if (!h->generated) return WCQP_E_UNSUPPORTED;        // (a classically uploaded plan has no known timeline)
    return WCQP_OK;
}

// wcqp_tick_upload_footsteps (tm NULL) and wcqp_tick_upload_footsteps_timed
int upload_footsteps(wcqp_tick_t h, const wcqp_tick_inputs* in, const wcqp_tick_footsteps* steps, const wcqp_tick_step_timing* tm) {
    if (!h || !in || !steps) return WCQP_E_INVALID;
    if (!h->holds_plan()) return WCQP_E_UNSUPPORTED;
    TickDev& d = h->d;
    const size_t B = (size_t)d.batch;
    const int K = steps->max_steps;
    // everything is checked before anything of the handle changes (a handle uploaded before keeps that upload)
    if (!in->state0 || !in->q0 || !in->com0 || !steps->n_steps || K < 0 || (K > 0 && (!steps->side || !steps->target))) return WCQP_E_INVALID;
    if (steps->first_ds_ticks < 1 || (!tm && (steps->ss_ticks < 1 || steps->ds_ticks < 1)) || steps->final_ds_ticks < 0) return WCQP_E_INVALID;
    if (tm && K > 0 && (!tm->ss_ticks || !tm->ds_ticks)) return WCQP_E_INVALID;
    // (a timed plan keeps the caller's final_ds_ticks: 0 stands for every robot's own last ds)
    const int final_ds = tm || steps->final_ds_ticks > 0 ? steps->final_ds_ticks : steps->ds_ticks;
    const long long per = (long long)steps->ss_ticks + steps->ds_ticks;
    if (!tm && !wcqp_goal::stages_fit(steps->first_ds_ticks, wcqp_goal::span_bound(K, per, final_ds))) return WCQP_E_INVALID;
    auto finite = [](const double* a, size_t n) { bool ok = true; for (size_t k = 0; k < n; ++k) ok = ok && std::isfinite(a[k]); return ok; };
    if (!std::isfinite(steps->lift) || !finite(steps->zmp_delta_left, 2) || !finite(steps->zmp_delta_right, 2)) return WCQP_E_INVALID;
    if (!finite(in->q0, B * kDof) || !finite(in->com0, B * 2) || (in->dcm0 && !finite(in->dcm0, B * 2)) || (in->u_init && !finite(in->u_init, B * 2)))
        return WCQP_E_INVALID;
    // the support-polygon sets: every robot owns `cap` slots - stage 0's set, then two per step (the stance foot alone, both again) where a
    // tick can reach them.  A step occupies ss + 1 stages or more, so at most (max_ticks + 1) / (ss + 1) + 1 steps start at a stage
    // <= max_ticks, whatever wcqp_tick_replan_footsteps later stitches together: the range never has to grow, and no set ever moves
    // (a timed step: a stage of single and a stage of double support or more)
    const int cap = 1 + 2 * ((h->p.max_ticks + 1) / (tm ? 2 : steps->ss_ticks + 1) + 1);
    std::vector<int> set_base(B);
    const size_t ns = B * (size_t)cap;
    for (size_t i = 0; i < B; ++i) {
        if (!footsteps_valid(i, K, steps->n_steps, steps->side, steps->target)) return WCQP_E_INVALID;
        // (the timed plan's own durations and stage indices; an untimed plan's were bounded above, for any list of K steps)
        const wcqp_goal::Timeline tl = list_timeline(i, K, 0, steps->first_ds_ticks, steps->n_steps[i], tm, steps->ss_ticks, steps->ds_ticks);
        if (tm && (!tl.durations_valid() || !wcqp_goal::stages_fit(tl.first_step(), tl.span(final_ds)))) return WCQP_E_INVALID;
        if (!finite(in->state0 + i * kStateLen + 24, 24) || !std::isfinite(in->state0[i * kStateLen + 68])) return WCQP_E_INVALID;
        set_base[i] = (int)(i * (size_t)cap);
    }
    if (ns > (size_t)1 << 30) return WCQP_E_UNSUPPORTED;
    // from here on the device state changes: a call that fails on the way leaves the handle unrunnable until the next good upload
    h->uploaded = false;
    WCQP_HIP_TRY(hipDeviceSynchronize());
    if (!h->gen_zmp0) { const int rca = dev_alloc(h, &h->gen_zmp0, B * 2); if (rca != WCQP_OK) return rca; }
    {   // wcqp_tick_rebase_plan's row of d_i, on the device and pinned, and the event behind its copy
        auto& rb = h->rebase;
        if (!rb.dev) { const int rca = dev_alloc(h, &rb.dev, B); if (rca != WCQP_OK) return rca; }
        if (!rb.host && hipHostMalloc(reinterpret_cast<void**>(&rb.host), B * 4, hipHostMallocDefault) != hipSuccess) return WCQP_E_NOMEM;
        if (!rb.ev) WCQP_HIP_TRY(hipEventCreateWithFlags(&rb.ev, hipEventDisableTiming));
    }
    {   // what this plan fixes for the handle, and a replan needs to know of it (wcqp_tick_replan_footsteps)
        auto& gp = h->gp;
        gp.ss = tm ? 0 : steps->ss_ticks; gp.ds = tm ? 0 : steps->ds_ticks; gp.final_ds = final_ds; gp.cap = cap; gp.lift = steps->lift;
        gp.timed = tm != nullptr;
        gp.swing = h->swing_pending;
        for (int k = 0; k < 2; ++k) { gp.delta[0][k] = steps->zmp_delta_left[k]; gp.delta[1][k] = steps->zmp_delta_right[k]; }
    }
    // the footsteps, the table and the set table: device memory of this call
    struct Scratch {
        std::vector<void*> p;
        ~Scratch() { for (void* q : p) (void)hipFree(q); }
        void* get(size_t bytes) { void* q = nullptr; if (hipMalloc(&q, bytes > 0 ? bytes : 1) != hipSuccess) return nullptr; p.push_back(q); return q; }
    } scratch;
    PlanGenDev g = plan_gen_of(h, K);
    const size_t BK = B * (size_t)K;
    int* d_n = static_cast<int*>(scratch.get(B * 4)); int* d_base = static_cast<int*>(scratch.get(B * 4));
    unsigned char* d_side = static_cast<unsigned char*>(scratch.get(BK)); double* d_tg = static_cast<double*>(scratch.get(BK * 24));
    double* d_tab = static_cast<double*>(scratch.get(B * (size_t)(K + 1) * kFpRec * 8));
    long long* d_at = static_cast<long long*>(scratch.get(ns * 8)); int* d_code = static_cast<int*>(scratch.get(ns * 4));
    if (!d_n || !d_base || !d_side || !d_tg || !d_tab || !d_at || !d_code) return WCQP_E_NOMEM;
    int *d_ssk = nullptr, *d_dsk = nullptr, *d_start = nullptr;
    if (tm) {
        d_ssk = static_cast<int*>(scratch.get(BK * 4)); d_dsk = static_cast<int*>(scratch.get(BK * 4));
        d_start = static_cast<int*>(scratch.get(B * (size_t)(K + 1) * 4));
        if (!d_ssk || !d_dsk || !d_start) return WCQP_E_NOMEM;
        if (BK > 0) {
            WCQP_HIP_TRY(hipMemcpy(d_ssk, tm->ss_ticks, BK * 4, hipMemcpyHostToDevice));
            WCQP_HIP_TRY(hipMemcpy(d_dsk, tm->ds_ticks, BK * 4, hipMemcpyHostToDevice));
        }
    }
    WCQP_HIP_TRY(hipMemset(d_code, 0xff, ns * 4));      // (-1: a slot without a set; the prologue enters the ones in use)
    WCQP_HIP_TRY(hipMemcpy(d_n, steps->n_steps, B * 4, hipMemcpyHostToDevice));
    WCQP_HIP_TRY(hipMemcpy(d_base, set_base.data(), B * 4, hipMemcpyHostToDevice));
    if (BK > 0) {
        WCQP_HIP_TRY(hipMemcpy(d_side, steps->side, BK, hipMemcpyHostToDevice));
        WCQP_HIP_TRY(hipMemcpy(d_tg, steps->target, BK * 24, hipMemcpyHostToDevice));
    }
    WCQP_HIP_TRY(hipMemcpy(d.state, in->state0, B * kStateLen * 8, hipMemcpyHostToDevice));      // (the initial footprints and the CoM height)
    g.n_steps = d_n; g.side = d_side; g.target = d_tg; g.set_base = d_base; g.table = d_tab; g.set_at = d_at; g.set_code = d_code;
    g.first_ds = steps->first_ds_ticks;
    for (hipEvent_t& e : h->gen_ev) if (!e) WCQP_HIP_TRY(hipEventCreate(&e));
    int rc = tm ? wcqp::plan_gen_enqueue(PlanGenTimedDev{g, PlanTimes{d_ssk, d_dsk, d_start, final_ds}}, plan_swing_of(h), nullptr, h->gen_ev[0], h->gen_ev[1])
                : wcqp::plan_gen_enqueue(g, plan_swing_of(h), nullptr, h->gen_ev[0], h->gen_ev[1]);
    if (rc == WCQP_OK) rc = build_plan_sets(h, ns, d_at, d_code);      // (synchronises)
    if (rc != WCQP_OK) return rc;
    WCQP_HIP_TRY(hipEventElapsedTime(&h->gen_record_ms, h->gen_ev[0], h->gen_ev[1]));
    h->vel_explicit = g.vel != nullptr;       // (the generated velocities, where the handle keeps any: the splice has no tail for them)
    h->generated = true;
    {   // per robot the plan in force
        auto& gp = h->gp;
        gp.origin.assign(B, 0); gp.first_ds.assign(B, steps->first_ds_ticks); gp.keep.assign(B, 1);
        gp.n_steps.assign(B, 0); gp.dur.assign(tm ? B : 0, std::vector<int>());
        for (size_t i = 0; i < B; ++i) gp.set_steps(i, steps->n_steps[i], tm ? tm->ss_ticks + i * K : nullptr, tm ? tm->ds_ticks + i * K : nullptr);
        h->rp.pending = false; h->goal.pending = false; h->goal.owed.clear(); h->rebase.pending = false;      // (the device was synchronised above)
        h->restart.pending = false; h->restart.owed.clear(); h->restart.called = false;
    }
    WCQP_HIP_TRY(hipMemset(const_cast<int*>(d.phase0.get()), 0, B * 4));
    WCQP_HIP_TRY(hipMemset(const_cast<double*>(d.swing_twist.get()), 0, B * 48));
    if (h->streamed) { const int rcs = wcqp::reset_streamed_stage(h); if (rcs != WCQP_OK) return rcs; }
    // dcm0 / u_init NULL: the generated DCM reference and ZMP of stage 0
    std::vector<double> dcm0, u0;
    wcqp_tick_inputs eff = *in;
    if (!in->dcm0) {
        dcm0.resize(B * 2);
        WCQP_HIP_TRY(hipMemcpy2D(dcm0.data(), 16, d.ref_traj.get(), (size_t)d.traj_len * 16, 16, B, hipMemcpyDeviceToHost));
        eff.dcm0 = dcm0.data();
    }
    if (!in->u_init) {
        u0.resize(B * 2);
        WCQP_HIP_TRY(hipMemcpy(u0.data(), h->gen_zmp0, B * 16, hipMemcpyDeviceToHost));
        eff.u_init = u0.data();
    }
    return wcqp::upload_state(h, &eff, 2);
}

// wcqp_tick_replan_footsteps (tm NULL, an untimed plan) and wcqp_tick_replan_footsteps_timed (tm: the new steps' durations, a timed one)
int replan_footsteps(wcqp_tick_t h, const wcqp_tick_replan* rp, const wcqp_tick_step_timing* tm, void* stream) {
    if (!h || !rp) return WCQP_E_INVALID;
    if (const int rc = replan_ready(h); rc != WCQP_OK) return rc;
    const auto& gp = h->gp;
    if (gp.timed != (tm != nullptr)) return WCQP_E_UNSUPPORTED;           // (a plan is timed or not from its upload on)
    const size_t B = (size_t)h->d.batch;
    const int K = rp->max_steps, T = h->d.traj_len, fd = rp->first_ds_ticks;
    // everything is checked here, on the host, before anything changes: a refused call leaves the handle exactly as it was
    if (!rp->merge_stage || !rp->n_steps || K < 0 || (K > 0 && (!rp->side || !rp->target)) || fd < 1) return WCQP_E_INVALID;
    if (tm && K > 0 && (!tm->ss_ticks || !tm->ds_ticks)) return WCQP_E_INVALID;
    const long long last = (long long)T + fd;       // (no new plan starts its steps later)
    if (!tm && !wcqp_goal::stages_fit(last, wcqp_goal::span_bound(K, (long long)gp.ss + gp.ds, gp.final_ds))) return WCQP_E_INVALID;
    if (const int rc = h->settle(); rc != WCQP_OK) return rc;       // (the step counts, and on a timed plan the durations, a goal call still owes)
    ReplanCall c(B);
    for (size_t i = 0; i < B; ++i) {
        const int M = rp->merge_stage[i];
        if (M == -1) continue;                            // (the robot keeps its plan: nothing of its rows is read)
        // stage 0 is the initial state's, stages the enqueued ticks have consumed stay (within one wcqp_tick_run call the kernel reads a stage
        // ahead, between calls nothing is ahead), a plan is cut only behind its own origin, and the merge stage has both feet in contact in
        // the plan in force: not inside one of its single supports
        if (!wcqp_goal::merge_allowed(gp.timeline(i), M, consumed_stages(h), T)) return WCQP_E_INVALID;
        if (!footsteps_valid(i, K, rp->n_steps, rp->side, rp->target)) return WCQP_E_INVALID;
        const wcqp_goal::Timeline fresh = list_timeline(i, K, M, fd, rp->n_steps[i], tm, gp.ss, gp.ds);
        if (tm && (!fresh.durations_valid() || !wcqp_goal::stages_fit(last, fresh.span(gp.final_ds)))) return WCQP_E_INVALID;
        if (const int rc = replan_admit(h, i, M, fresh.sets_up_to(h->p.max_ticks), c); rc != WCQP_OK) return rc;
    }
    if (c.robots.empty()) return WCQP_OK;
    return replan_enqueue(h, c, K, fd, ReplanSource{rp, nullptr, nullptr, nullptr, nullptr, tm}, (hipStream_t)stream);
}

// wcqp_tick_replan_goals (tm NULL, an untimed plan) and wcqp_tick_replan_goals_timed (tm: the timed planner's range and score, a timed one)
int replan_goals(wcqp_tick_t h, wcqp_unicycle_t planner, const wcqp_unicycle_timing* tm, const wcqp_tick_goals* gl, void* stream) {
    if (!h || !planner || !gl || !gl->goal) return WCQP_E_INVALID;
    if (const int rc = replan_ready(h); rc != WCQP_OK) return rc;
    const auto& gp = h->gp;
    // (a plan is timed or not from its upload on: the untimed planner kernel knows one common timing, the timed one none)
    if (gp.timed != (tm != nullptr)) return WCQP_E_UNSUPPORTED;
    const wcqp_unicycle::UniPar* par = wcqp::unicycle_par(planner);
    const size_t B = (size_t)h->d.batch;
    const int K = par->K, T = h->d.traj_len, fd = gl->first_ds_ticks;
    wcqp_unicycle::UniTiming utm{};
    if (tm) {      // (the planner's own validation of tm; the duration rows are the call's, set where they are carved)
        int32_t rows = 0;
        if (const int rc = wcqp::unicycle_timing(planner, tm, &rows, &rows, &utm); rc != WCQP_OK) return rc;
        utm.ss_ticks = nullptr; utm.ds_ticks = nullptr;
    }
    if (fd < 1 || gl->min_lead_ticks < 0) return WCQP_E_INVALID;
    // (the steps are the device's to choose: an untimed one lasts ss + ds stages, a timed one max_step_ticks at most, and its
    // ds <= m - 1 covers a final_ds of 0)
    const long long longest = tm ? (long long)tm->max_step_ticks : (long long)gp.ss + gp.ds;
    if (!wcqp_goal::stages_fit((long long)T + fd, wcqp_goal::span_bound(K, longest, gp.final_ds))) return WCQP_E_INVALID;
    if (const int rc = h->settle(); rc != WCQP_OK) return rc;       // (AUTO and the checks read the step counts - and durations - of the plans in force)
    ReplanCall c(B);
    std::vector<int> taken(B, 0), decided(B, 0);
    const int t0 = consumed_stages(h);
    for (size_t i = 0; i < B; ++i) {
        int M = gl->merge_stage ? gl->merge_stage[i] : WCQP_TICK_MERGE_AUTO;
        if (M == WCQP_TICK_MERGE_KEEP) { decided[i] = WCQP_GOAL_KEPT; continue; }      // (none of its rows is read)
        if (M < WCQP_TICK_MERGE_AUTO || M == 0) return WCQP_E_INVALID;
        const uint8_t fs = gl->first_side ? gl->first_side[i] : (uint8_t)WCQP_TICK_SIDE_AUTO;
        if (fs > 1 && fs != WCQP_TICK_SIDE_AUTO) return WCQP_E_INVALID;
        if (!std::isfinite(gl->goal[i * 2]) || !std::isfinite(gl->goal[i * 2 + 1])) return WCQP_E_INVALID;
        const wcqp_goal::Timeline in_force = gp.timeline(i);
        if (M == WCQP_TICK_MERGE_AUTO) {
            M = wcqp_goal::merge_auto(in_force, t0, gl->min_lead_ticks, T);
            if (M == wcqp_goal::kTooLate) { decided[i] = WCQP_GOAL_TOO_LATE; continue; }
        } else if (!wcqp_goal::merge_allowed(in_force, M, t0, T)) {
            return WCQP_E_INVALID;
        }
        // (the new plan's steps are the device's: their sets are bounded, not counted)
        const int fresh = goal_sets_bound(K, M, fd, tm ? (long long)tm->min_step_ticks : (long long)gp.ss + gp.ds, h->p.max_ticks);
        if (const int rc = replan_admit(h, i, M, fresh, c); rc != WCQP_OK) return rc;
        taken[i] = M;
    }
    const auto rows = wcqp_tick_s::GoalRows::of(B, (size_t)K, tm != nullptr);
    if (!c.robots.empty())
        if (const int rc = replan_enqueue(h, c, K, fd, ReplanSource{nullptr, gl->goal, gl->first_side, par, &rows, nullptr, tm ? &utm : nullptr}, (hipStream_t)stream); rc != WCQP_OK)
            return rc;
    auto& gc = h->goal;
    gc.called = true; gc.rows = rows; gc.merge.swap(taken); gc.decided.swap(decided);
    return WCQP_OK;
}

}  // namespace

extern "C" {

int wcqp_tick_upload_footsteps(wcqp_tick_t h, const wcqp_tick_inputs* in, const wcqp_tick_footsteps* steps) {
    return upload_footsteps(h, in, steps, nullptr);
}

int wcqp_tick_upload_footsteps_timed(wcqp_tick_t h, const wcqp_tick_inputs* in, const wcqp_tick_footsteps* steps, const wcqp_tick_step_timing* tm) {
    if (!tm) return WCQP_E_INVALID;
    return upload_footsteps(h, in, steps, tm);
}

int wcqp_tick_replan_footsteps(wcqp_tick_t h, const wcqp_tick_replan* rp, void* stream) { return replan_footsteps(h, rp, nullptr, stream); }

int wcqp_tick_replan_footsteps_timed(wcqp_tick_t h, const wcqp_tick_replan* rp, const wcqp_tick_step_timing* tm, void* stream) {
    if (!tm) return WCQP_E_INVALID;
    return replan_footsteps(h, rp, tm, stream);
}

int wcqp_tick_replan_goals(wcqp_tick_t h, wcqp_unicycle_t planner, const wcqp_tick_goals* gl, void* stream) {
    return replan_goals(h, planner, nullptr, gl, stream);
}

int wcqp_tick_replan_goals_timed(wcqp_tick_t h, wcqp_unicycle_t planner, const wcqp_unicycle_timing* tm, const wcqp_tick_goals* gl, void* stream) {
    if (!tm) return WCQP_E_INVALID;
    return replan_goals(h, planner, tm, gl, stream);
}

// THE SHAPED SWING (include/wcqp.h): host only.  The profile waits on the handle for the next wcqp_tick_upload_footsteps*
int wcqp_tick_set_swing_profile(wcqp_tick_t h, const wcqp_tick_swing_profile* p) {
    if (!h || !p) return WCQP_E_INVALID;
    if (!h->holds_plan()) return WCQP_E_UNSUPPORTED;
    if (!std::isfinite(p->apex_ratio) || !std::isfinite(p->landing_velocity) || !std::isfinite(p->pitch_delta) || !std::isfinite(p->com_height_delta))
        return WCQP_E_INVALID;
    if (p->apex_ratio < 0.0 || p->apex_ratio >= 1.0 || p->landing_velocity > 0.0) return WCQP_E_INVALID;
    if (p->landing_velocity != 0.0 && p->apex_ratio == 0.0) return WCQP_E_INVALID;      // (the quartic has no landing branch)
    if (std::fabs(p->pitch_delta) > 0.78539816339744830962) return WCQP_E_INVALID;
    h->swing_pending = *p;
    return WCQP_OK;
}

int wcqp_tick_get_swing_profile(wcqp_tick_t h, wcqp_tick_swing_profile* out) {
    if (!h || !out) return WCQP_E_INVALID;
    if (!h->holds_plan()) return WCQP_E_UNSUPPORTED;
    const bool in_force = h->uploaded && h->generated;      // (a classically uploaded plan has none)
    *out = in_force ? h->gp.swing : wcqp_tick_swing_profile{0.0, 0.0, 0.0, 0.0};
    return WCQP_OK;
}

// THE REBASED PLAN (include/wcqp.h).  The host decides - on the timelines of the plans in force, settled first - and keeps its own
// books: origins and the tick count go down by the shift at once, each robot's `keep` by d_i once the row has come back (RebaseCall)
int wcqp_tick_rebase_plan(wcqp_tick_t h, int32_t shift, void* stream) {
    if (!h) return WCQP_E_INVALID;
    if (const int rc = replan_ready(h); rc != WCQP_OK) return rc;
    // (the internal plant's disturbance is a hash of the tick index: a rewound index would repeat its stream)
    if (!h->external && h->p.noise != 0.0) return WCQP_E_UNSUPPORTED;
    const TickDev& d = h->d;
    auto& gp = h->gp;
    auto& rb = h->rebase;
    const size_t B = (size_t)d.batch;
    const int R = shift == WCQP_TICK_REBASE_AUTO ? wcqp_goal::rebase_auto(h->ticks_enqueued) : shift;
    if (const int rc = h->settle(); rc != WCQP_OK) return rc;       // (the rule reads timelines; and the previous rebase's row has come back)
    for (size_t i = 0; i < B; ++i)
        if (!wcqp_goal::rebase_allowed(gp.timeline(i), R, h->ticks_enqueued, h->p.max_ticks, gp.final_ds)) return WCQP_E_INVALID;
    if (!rb.dev || !rb.host || !rb.ev) return WCQP_E_INVALID;       // (cannot happen: every generated upload allocates them)
    PlanRebaseDev g{};
    g.rec = h->plan_rec; g.ref = const_cast<double*>(d.ref_traj.get());
    g.vel = (d.reactive || d.gain_sched) ? const_cast<double*>(d.dcm_vel.get()) : nullptr;
    g.zmp0 = h->gen_zmp0;
    g.set_A = h->set_A; g.set_b = h->set_b; g.set_nc = h->set_nc;
    g.tick2 = d.tick2.p; g.d_out = rb.dev;
    g.batch = d.batch; g.traj_len = d.traj_len; g.shift = R; g.cap = gp.cap;
    g.omega = d.omega; g.a = std::exp(d.omega * d.dT);
    const hipStream_t st = (hipStream_t)stream;
    if (const int rc = wcqp::plan_rebase_enqueue(g, st); rc != WCQP_OK) return rc;
    WCQP_HIP_TRY(hipMemcpyAsync(rb.host, rb.dev, B * 4, hipMemcpyDeviceToHost, st));
    WCQP_HIP_TRY(hipEventRecord(rb.ev, st));
    rb.pending = true;
    // (an origin 2^30 stages back belongs to a plan that ended before stage 0 - stages_fit bounds its span -: it may stay there)
    for (size_t i = 0; i < B; ++i) if (gp.origin[i] > -(1 << 30)) gp.origin[i] -= R;
    h->ticks_enqueued -= R;
    h->plan_shift += R;
    return WCQP_OK;
}

// the standing ZMP of the two soles of a state0 row on the host, operation for operation plan_restart_reset_kernel's (zmp_point_ax)
static double standing_zmp_host(const double* st0, const double (*delta)[2], int ax) {
#pragma clang fp contract(off)
    const double* L = st0 + 24;
    const double* R = st0 + 36;
    const double rl = L[3 + 3 * ax] * delta[0][0] + L[4 + 3 * ax] * delta[0][1], rr = R[3 + 3 * ax] * delta[1][0] + R[4 + 3 * ax] * delta[1][1];
    const double zl = L[ax] + rl, zr = R[ax] + rr;
    return 0.5 * (zl + zr);
}

// THE RESTARTED ROBOT and THE RECOVERED ROBOT (include/wcqp.h), one path.  The host checks everything and compacts the listed robots' rows
// into the call's block, one row per SLOT, so a kept robot's rows are never read.  A restart call (rs) brings the posture rows and the
// device decides IF_STOPPED; a recover call (rv, prep) brings targets, and the device decides, solves the posture of the slots that go on
// and restarts those that end SOLVED (plan_recover.hip around prepare.hip's kernel).  The host's own books: tick_handle.h, RestartCall.
// THE RESET ROBOT (`reset`: wcqp_tick_reset_robots, a restart call's rows on a streamed EXTERNAL handle) takes the same path: `plan` says
// whether the handle holds a plan to stand the robot on - a resident one -, and what only such a handle keeps is reset behind the restart's
// first kernel (plan_restart.hip)
static int restart_call(wcqp_tick_t h, const wcqp_tick_restart* rs, wcqp_prepare_t prep, const wcqp_tick_recover* rv, void* stream, bool reset = false) {
    const bool recover = rv != nullptr;
    if (!h || (!rs && !rv)) return WCQP_E_INVALID;
    if (reset) {
        // (a POSITION handle's non-linear IK keeps state of its own; the synthetic-gait EXTERNAL handle has no stage to start from)
        if (!h->streamed || !h->external || h->position) return WCQP_E_UNSUPPORTED;
        if (h->resident) { if (const int rc = replan_ready(h); rc != WCQP_OK) return rc; }
        else if (!h->uploaded) return WCQP_E_INVALID;
    } else {
        if (!h->holds_plan()) return WCQP_E_UNSUPPORTED;
        // (the caller's plant is the state there: wcqp_tick_reset_robots resets it with the handle's rows)
        if (h->external || h->resident || h->streamed) return WCQP_E_UNSUPPORTED;
        if (const int rc = replan_ready(h); rc != WCQP_OK) return rc;
    }
    const bool plan = !reset || h->resident;
    const uint8_t* mode = recover ? rv->mode : rs->mode;
    const double* dcm0 = recover ? rv->dcm0 : rs->dcm0;
    const double* u_init = recover ? rv->u_init : rs->u_init;
    if (!mode) return WCQP_E_INVALID;
    if (!recover && (!rs->state0 || !rs->q0 || !rs->com0)) return WCQP_E_INVALID;
    if (recover) {
        if (!prep || (rv->left_d == nullptr) != (rv->right_d == nullptr)) return WCQP_E_INVALID;
        // the IK must walk the tree the handle's ticks walk: the joints it reads and writes are theirs
        std::vector<double> tab; int rounds = 0;
        if (!h->kin || !wcqp::kin_fused_tables(h->kin, tab, &rounds)) return WCQP_E_INVALID;
        const std::vector<double>& mine = wcqp::prepare_model_table(prep);
        if (mine.size() != tab.size() || std::memcmp(mine.data(), tab.data(), tab.size() * sizeof(double)) != 0) return WCQP_E_INVALID;
    }
    // (the call comes first in tick S's sequence: a stage or a feedback in hand was made for the robot as it was)
    if (reset && (h->desired_set || h->feedback_set)) return WCQP_E_INVALID;
    const TickDev& d = h->d;
    auto& gp = h->gp;
    auto& rc_ = h->restart;
    const size_t B = (size_t)d.batch;
    const int T = d.traj_len, cap = gp.cap;
    if (const int rc = h->settle(); rc != WCQP_OK) return rc;       // (the slot counts and timelines goal, rebase and restart calls still owe)
    const int S = consumed_stages(h);
    if (S > h->p.max_ticks) return WCQP_E_INVALID;
    // the caller's rows by kind: where they lie, how long a robot's row is, and (below) where the slot rows go in the block
    struct In { const double* host; size_t len; size_t at; };
    In in[7] = {{recover ? rv->left_d : rs->state0, recover ? (size_t)12 : (size_t)kStateLen, 0}, {recover ? rv->right_d : rs->q0, recover ? (size_t)12 : (size_t)kDof, 0},
                {recover ? rv->com_d : rs->com0, recover ? (size_t)3 : (size_t)2, 0}, {recover ? rv->Rd_neck : nullptr, 9, 0},
                {recover ? rv->q_guess : nullptr, (size_t)kDof, 0}, {dcm0, 2, 0}, {u_init, 2, 0}};
    auto finite = [](const double* a, size_t n) { bool ok = true; for (size_t k = 0; k < n; ++k) ok = ok && std::isfinite(a[k]); return ok; };
    std::vector<int> robots, keep_new;
    for (size_t i = 0; i < B; ++i) {
        const uint8_t m = mode[i];
        if (m == WCQP_TICK_RESTART_KEEP) continue;            // (none of its rows is read)
        if (m > WCQP_TICK_RESTART_IF_STOPPED) return WCQP_E_INVALID;
        for (const In& a : in)
            if (a.host && !finite(a.host + i * a.len, a.len)) return WCQP_E_INVALID;
        // the robot's slots in use by sets of stages < S - no stage >= S keeps its record, so the sets they alone name are free -, and one
        // more for the standing set (a robot the device decides: counted as if it restarted)
        const int used = plan ? gp.keep[i] + gp.timeline(i).sets_up_to((S - 1 < h->p.max_ticks ? S - 1 : h->p.max_ticks)) : 0;
        if (plan && (used < 1 || used + 1 > cap)) return WCQP_E_INVALID;
        robots.push_back((int)i); keep_new.push_back(used + 1);
    }
    if (robots.empty()) {      // (nothing is enqueued: the result is "nobody, at stage S")
        if (const int rc = rc_.wait(); rc != WCQP_OK) return rc;
        rc_.robots.clear(); rc_.keep_new.clear(); rc_.owed.clear();
        rc_.called = true; rc_.recover = recover; rc_.stage = S;
        return WCQP_OK;
    }
    // (a handle without a plan: no tile, and the first kernel's set table has one entry per slot of the call, which nothing reads)
    const size_t nr = robots.size(), n_tile = (size_t)((T + 63) / 64), t0 = (size_t)(S / 64), nt = plan ? nr * (n_tile - t0) : 0, nslots = plan ? B * (size_t)cap : nr;
    const size_t res_bytes = nr * wcqp_tick_s::RestartCall::row_bytes(recover);
    size_t off = 0;
    auto carve = [&off](size_t bytes) { const size_t at = off; off += (bytes + 255) & ~(size_t)255; return at; };
    const size_t o_rob = carve(nr * 4), o_mode = carve(nr), o_slot = carve(nr * 4), o_tile = carve(nt * 8), o_cnt = carve(recover ? 4 : 0);
    for (In& a : in) a.at = carve(a.host ? nr * a.len * 8 : 0);
    const size_t front = off;
    const size_t o_pat = carve(nr * kPlanRec * 8), o_mid = carve(nr * 16), o_res = carve(res_bytes), o_at = carve(nslots * 8), o_code = carve(nslots * 4);
    // a recover call: the restart's rows, which its gate writes; the slots' packed rows; the packed rows the IK reads and writes
    size_t o_st = in[0].at, o_q = in[1].at, o_com = in[2].at, o_dec = 0, o_pos = 0, o_pk[5] = {0, 0, 0, 0, 0}, o_ik[5] = {0, 0, 0, 0, 0};
    if (recover) {
        o_st = carve(nr * kStateLen * 8); o_q = carve(nr * kDof * 8); o_com = carve(nr * 16); o_dec = carve(nr * 4); o_pos = carve(nr * 4);
        const size_t pk[5] = {12, 12, 3, 9, (size_t)kDof}, ik[5] = {(size_t)kDof * 8, (size_t)kStateLen * 8, 16, 4, 4};
        for (int k = 0; k < 5; ++k) { o_pk[k] = carve(nr * pk[k] * 8); o_ik[k] = carve(nr * ik[k]); }
    }
    std::vector<char> blob(front, 0);       // (a recover call's counter starts at 0)
    {
        std::memcpy(blob.data() + o_rob, robots.data(), nr * 4);
        int* slot = reinterpret_cast<int*>(blob.data() + o_slot); int* tile = reinterpret_cast<int*>(blob.data() + o_tile);
        for (size_t r = 0; r < nr; ++r) {
            const size_t i = (size_t)robots[r];
            blob[o_mode + r] = (char)mode[i];
            slot[r] = plan ? (int)(i * (size_t)cap) + keep_new[r] - 1 : (int)r;
            for (size_t tl = t0; plan && tl < n_tile; ++tl) { *tile++ = (int)r; *tile++ = (int)tl; }
            for (const In& a : in)
                if (a.host) std::memcpy(blob.data() + a.at + r * a.len * 8, a.host + i * a.len, a.len * 8);
        }
    }
    if (!rc_.ev) WCQP_HIP_TRY(hipEventCreateWithFlags(&rc_.ev, hipEventDisableTiming));
    if (const int rc = rc_.wait(); rc != WCQP_OK) return rc;       // (the previous call's rows, before this one's take their place)
    if (rc_.host_cap < res_bytes) {
        if (rc_.host) (void)hipHostFree(rc_.host);
        rc_.host = nullptr; rc_.host_cap = 0;
        if (hipHostMalloc(reinterpret_cast<void**>(&rc_.host), res_bytes, hipHostMallocDefault) != hipSuccess) return WCQP_E_NOMEM;
        rc_.host_cap = res_bytes;
    }
    if (const int rc = h->rp.take(h->copy_stream, blob.data(), front, off); rc != WCQP_OK) return rc;
    char* buf = static_cast<char*>(h->rp.mem.ptr);
    auto dbl = [buf](size_t at) { return reinterpret_cast<double*>(buf + at); };
    auto i32 = [buf](size_t at) { return reinterpret_cast<int*>(buf + at); };
    PlanRestartDev g{};
    g.robots = i32(o_rob); g.mode = reinterpret_cast<const unsigned char*>(buf + o_mode);
    g.decided = recover ? i32(o_dec) : nullptr;
    g.state0 = dbl(o_st); g.q0 = dbl(o_q); g.com0 = dbl(o_com);
    g.dcm0 = dcm0 ? dbl(in[5].at) : nullptr; g.u0 = u_init ? dbl(in[6].at) : nullptr;
    g.set_slot = i32(o_slot); g.tiles = reinterpret_cast<const int2*>(buf + o_tile);
    g.pattern = dbl(o_pat); g.mid = dbl(o_mid);
    // the result rows, in the order RestartCall reads them
    g.stopped = reinterpret_cast<long long*>(buf + o_res); g.restarted = i32(o_res + nr * (recover ? 24 : 8));
    g.set_at = reinterpret_cast<long long*>(buf + o_at); g.set_code = i32(o_code);
    g.rec = plan ? h->plan_rec : nullptr; g.ref = plan ? const_cast<double*>(d.ref_traj.get()) : nullptr;
    g.vel = plan && (d.reactive || d.gain_sched) ? const_cast<double*>(d.dcm_vel.get()) : nullptr;
    g.mst = d.skew ? d.mst.p : nullptr; g.state = d.state.p; g.q_des = d.q_des.p; g.dq_prev = d.dq_prev.p;
    g.dcm = d.dcm.p; g.com = d.com.p; g.c_ref = d.c_ref.p; g.p_star = d.p_star.p; g.zmp_meas = d.zmp_meas.p; g.u_prev = d.u_prev.p;
    g.v_ref_prev = d.v_ref_prev.p; g.v_star_prev = d.v_star_prev.p;
    g.zs = d.gain_sched ? h->zg.zs.p : nullptr;
    g.com_h0 = h->kin ? const_cast<double*>(d.com_h0.get()) : nullptr;
    g.sel_built = d.skew ? d.sel_built.p : nullptr; g.live_nc = d.skew ? d.live_nc.p : nullptr; g.sel = d.sel.p;
    g.mpc_fail = d.mpc_fail.p; g.ik_fail = d.ik_fail.p; g.hot_try = d.hot_try.p; g.hot_hit = d.hot_hit.p;
    g.ik_iters = h->position ? h->pos.ik_iters : nullptr;
    g.ik_lo = h->ik_lo; g.ik_up = h->ik_up;
    g.n_robots = (int)nr; g.n_tiles = (int)nt; g.traj_len = T; g.stage = S;
    for (int k = 0; k < 2; ++k) { g.delta[0][k] = gp.delta[0][k]; g.delta[1][k] = gp.delta[1][k]; }
    // in the caller's stream order, behind the ticks already enqueued: no pointer a tick or a captured graph holds changes, and the set
    // slot written is one no stage below S names
    const hipStream_t st = (hipStream_t)stream;
    if (recover) {
        PlanRecoverDev v{};
        v.robots = g.robots; v.mode = g.mode;
        v.left_in = rv->left_d ? dbl(in[0].at) : nullptr; v.right_in = rv->right_d ? dbl(in[1].at) : nullptr;
        v.com_in = rv->com_d ? dbl(in[2].at) : nullptr; v.neck_in = rv->Rd_neck ? dbl(in[3].at) : nullptr; v.q_in = rv->q_guess ? dbl(in[4].at) : nullptr;
        v.ik_fail = d.ik_fail.p; v.q_des = d.q_des.p; v.rec = h->plan_rec;
        v.pos = i32(o_pos); v.count = i32(o_cnt);
        v.p_left = dbl(o_pk[0]); v.p_right = dbl(o_pk[1]); v.p_com = dbl(o_pk[2]); v.p_neck = dbl(o_pk[3]); v.p_q = dbl(o_pk[4]);
        v.o_q = dbl(o_ik[0]); v.o_state = dbl(o_ik[1]); v.o_res = dbl(o_ik[2]); v.o_status = i32(o_ik[3]); v.o_iters = i32(o_ik[4]);
        v.state0 = dbl(o_st); v.q0 = dbl(o_q); v.com0 = dbl(o_com); v.decided = i32(o_dec);
        v.residual = dbl(o_res + nr * 8); v.status = g.restarted + nr; v.iters = g.restarted + 2 * nr;
        v.n_robots = (int)nr; v.traj_len = T; v.stage = S;
        for (int k = 0; k < 2; ++k) { v.delta[0][k] = gp.delta[0][k]; v.delta[1][k] = gp.delta[1][k]; }
        wcqp::PrepareRows pr{};
        pr.max_rows = (int)nr; pr.n_rows = v.count;
        pr.left_d = v.p_left; pr.right_d = v.p_right; pr.com_d = v.p_com; pr.Rd_neck = rv->Rd_neck ? v.p_neck : nullptr; pr.q_guess = v.p_q;
        pr.q = dbl(o_ik[0]); pr.state = dbl(o_ik[1]); pr.residual = dbl(o_ik[2]); pr.status = i32(o_ik[3]); pr.iters = i32(o_ik[4]);
        if (const int rc = wcqp::plan_recover_gather_enqueue(v, st); rc != WCQP_OK) return rc;
        if (const int rc = wcqp::prepare_enqueue_rows(prep, pr, st); rc != WCQP_OK) return rc;
        if (const int rc = wcqp::plan_recover_gate_enqueue(v, st); rc != WCQP_OK) return rc;
    }
    WCQP_HIP_TRY(hipMemsetAsync(g.set_code, 0xff, nslots * 4, st));
    const int t_hand = h->ticks_for_handoff();
    if (reset) {
        TickResetDev e{};
        e.robots = g.robots; e.restarted = g.restarted; e.q0 = g.q0; e.com0 = g.com0; e.dcm0 = g.dcm0; e.u0 = g.u0; e.mid = g.mid;
        e.q_meas = h->q_meas; e.feedback_fail = h->feedback_fail; e.pair = h->st_pair; e.st_rec = h->st_rec; e.st_set_nc = h->st_set_nc;
        // THE RULE for a reading rejected at tick S: it keeps the hand-off record of parity S - 1 (tick.hip, sensors.hip), so the reset rows go there
        e.hand_prev = t_hand > 0 ? d.hand.p + (size_t)((t_hand - 1) & 1) * B * kHandLen : nullptr;
        // (no feedback is in hand, so no sensor call's write is pending: slot filt_cur is the one the next sensor call reads)
        e.filt = h->filt_state ? h->filt_state + (size_t)h->filt_cur * B * kFiltRec : nullptr;
        e.n_robots = (int)nr;
        if (const int rc = wcqp::tick_reset_enqueue(g, e, st); rc != WCQP_OK) return rc;
    } else if (const int rc = wcqp::plan_restart_enqueue(g, st); rc != WCQP_OK) return rc;
    if (plan) {
        hipLaunchKernelGGL(plan_hull_sets_kernel, dim3((unsigned)((nslots + 127) / 128)), dim3(128), 0, st, (int)nslots, plan_rect(h), h->plan_rec, g.set_at, g.set_code,
                           h->set_A, h->set_b, h->set_nc);
        WCQP_HIP_TRY(hipGetLastError());
    }
    WCQP_HIP_TRY(hipMemcpyAsync(rc_.host, buf + o_res, res_bytes, hipMemcpyDeviceToHost, st));
    WCQP_HIP_TRY(hipEventRecord(rc_.ev, st));
    if (const int rc = h->rp.guard(st); rc != WCQP_OK) return rc;
    rc_.called = true; rc_.recover = recover; rc_.stage = S; rc_.pending = true; rc_.owed.clear();
    for (size_t r = 0; plan && r < nr; ++r) {
        if (!recover && mode[robots[r]] == WCQP_TICK_RESTART_ALWAYS) h->stand_from((size_t)robots[r], S, keep_new[r]);
        else rc_.owed.push_back((int)r);
    }
    if (reset) {
        // the HOST forms of tick S's stage and feedback work on the NULL stream behind the last run's event: from here on behind this call
        if (h->run.done) { if (const int rc = h->run.guard(st); rc != WCQP_OK) return rc; }
        // before any tick wcqp_tick_download reports the uploaded measured state from the host's rows: the reset robots' are the call's
        // (ALWAYS only: no robot is stopped there, so IF_STOPPED resets none)
        for (size_t r = 0; t_hand == 0 && r < nr; ++r) {
            const size_t i = (size_t)robots[r];
            if (mode[i] != WCQP_TICK_RESTART_ALWAYS || h->meas0.size() != B * 6) continue;
            for (int ax = 0; ax < 2; ++ax) {
                const double mid = standing_zmp_host(rs->state0 + i * kStateLen, gp.delta, ax);
                h->meas0[i * 6 + ax] = dcm0 ? dcm0[2 * i + ax] : mid; h->meas0[i * 6 + 2 + ax] = rs->com0[2 * i + ax];
                h->meas0[i * 6 + 4 + ax] = u_init ? u_init[2 * i + ax] : mid;
            }
        }
    }
    rc_.robots.swap(robots); rc_.keep_new.swap(keep_new);
    return WCQP_OK;
}

int wcqp_tick_restart_robots(wcqp_tick_t h, const wcqp_tick_restart* rs, void* stream) {
    if (!rs) return WCQP_E_INVALID;
    return restart_call(h, rs, nullptr, nullptr, stream);
}

int wcqp_tick_reset_robots(wcqp_tick_t h, const wcqp_tick_restart* rs, void* stream) {
    if (!rs) return WCQP_E_INVALID;
    return restart_call(h, rs, nullptr, nullptr, stream, true);
}

int wcqp_tick_recover_robots(wcqp_tick_t h, wcqp_prepare_t prepare, const wcqp_tick_recover* rv, void* stream) {
    if (!rv) return WCQP_E_INVALID;
    return restart_call(h, nullptr, prepare, rv, stream);
}

int wcqp_tick_get_restart_result(wcqp_tick_t h, const wcqp_tick_restart_result* out) {
    if (!h || !out) return WCQP_E_INVALID;
    auto& rc_ = h->restart;
    if (!rc_.called) return WCQP_E_INVALID;
    if (const int rc = rc_.wait(); rc != WCQP_OK) return rc;       // (that call's own event, not the stream or the device)
    const size_t B = (size_t)h->d.batch;
    if (out->restarted) std::memset(out->restarted, 0, B);
    if (out->stopped_ticks) std::memset(out->stopped_ticks, 0, B * 8);
    for (size_t r = 0; r < rc_.robots.size(); ++r) {
        if (out->restarted) out->restarted[rc_.robots[r]] = (uint8_t)rc_.restarted()[r];
        if (out->stopped_ticks) out->stopped_ticks[rc_.robots[r]] = rc_.stopped()[r];
    }
    if (out->stage) *out->stage = rc_.stage;
    return WCQP_OK;
}

int wcqp_tick_get_recover_result(wcqp_tick_t h, const wcqp_tick_recover_result* out) {
    if (!h || !out) return WCQP_E_INVALID;
    auto& rc_ = h->restart;
    if (!rc_.called || !rc_.recover) return WCQP_E_INVALID;
    const wcqp_tick_restart_result shared{out->restarted, out->stopped_ticks, out->stage};
    if (const int rc = wcqp_tick_get_restart_result(h, &shared); rc != WCQP_OK) return rc;
    const size_t B = (size_t)h->d.batch;
    for (size_t i = 0; i < B; ++i) {
        if (out->status) out->status[i] = WCQP_RECOVER_KEPT;
        if (out->iters) out->iters[i] = 0;
        if (out->residual) { out->residual[2 * i] = 0.0; out->residual[2 * i + 1] = 0.0; }
    }
    for (size_t r = 0; r < rc_.robots.size(); ++r) {
        const size_t i = (size_t)rc_.robots[r];
        if (out->status) out->status[i] = rc_.status()[r];
        if (out->iters) out->iters[i] = rc_.iters()[r];
        if (out->residual) { out->residual[2 * i] = rc_.residual()[2 * r]; out->residual[2 * i + 1] = rc_.residual()[2 * r + 1]; }
    }
    return WCQP_OK;
}

int wcqp_tick_get_goal_result(wcqp_tick_t h, const wcqp_tick_goal_result* out) {
    if (!h || !out) return WCQP_E_INVALID;
    auto& gc = h->goal;
    if (!gc.called) return WCQP_E_INVALID;
    if (const int rc = h->settle(); rc != WCQP_OK) return rc;       // (waits for that call's own event, not for the stream or the device)
    const auto& at = gc.rows;
    const size_t B = (size_t)h->d.batch, K = at.K;
    for (size_t i = 0; i < B; ++i) {
        const bool dev = gc.decided[i] == 0;              // (a robot that had a lane: its rows came back)
        const char* r = gc.host;
        if (out->merge_stage) out->merge_stage[i] = gc.merge[i];
        if (out->first_side) out->first_side[i] = dev ? (uint8_t)r[at.fs + i] : 0;
        if (out->status) out->status[i] = dev ? at.at<int32_t>(r, at.status)[i] : gc.decided[i];
        if (out->n_steps) out->n_steps[i] = dev ? at.at<int32_t>(r, at.n)[i] : 0;
        if (out->side && K > 0) { if (dev) std::memcpy(out->side + i * K, r + at.side + i * K, K); else std::memset(out->side + i * K, 0, K); }
        if (out->target && K > 0) { if (dev) std::memcpy(out->target + i * K * 3, r + at.target + i * K * 24, K * 24); else std::memset(out->target + i * K * 3, 0, K * 24); }
        if (out->desired_point) { if (dev) std::memcpy(out->desired_point + i * 2, r + at.dp + i * 16, 16); else std::memset(out->desired_point + i * 2, 0, 16); }
        if (out->unicycle_end) { if (dev) std::memcpy(out->unicycle_end + i * 3, r + at.ue + i * 24, 24); else std::memset(out->unicycle_end + i * 3, 0, 24); }
    }
    return WCQP_OK;
}

int wcqp_tick_get_goal_timing(wcqp_tick_t h, int32_t* ss_ticks, int32_t* ds_ticks) {
    if (!h) return WCQP_E_INVALID;
    auto& gc = h->goal;
    if (!gc.called || !gc.rows.timed) return WCQP_E_INVALID;
    if (const int rc = h->settle(); rc != WCQP_OK) return rc;       // (waits for that call's own event, as wcqp_tick_get_goal_result)
    const auto& at = gc.rows;
    const size_t B = (size_t)h->d.batch, K = at.K;
    for (size_t i = 0; i < B && K > 0; ++i) {
        const bool dev = gc.decided[i] == 0;
        for (int which = 0; which < 2; ++which) {
            int32_t* dst = which ? ds_ticks : ss_ticks;
            if (!dst) continue;
            if (dev) std::memcpy(dst + i * K, gc.host + (which ? at.ds : at.ss) + i * K * 4, K * 4); else std::memset(dst + i * K, 0, K * 4);
        }
    }
    return WCQP_OK;
}

int wcqp_tick_get_plan(wcqp_tick_t h, int32_t robot0, int32_t n, int32_t stage0, int32_t m, const wcqp_tick_plan_window* out) {
    if (!h || !out) return WCQP_E_INVALID;
    if (!h->holds_plan()) return WCQP_E_UNSUPPORTED;
    const TickDev& d = h->d;
    if (!h->uploaded || robot0 < 0 || n < 1 || stage0 < 0 || m < 1 || (long long)robot0 + n > d.batch || (long long)stage0 + m > d.traj_len) return WCQP_E_INVALID;
    const bool has_vel = d.reactive || d.gain_sched;
    if ((out->dcm_vel_traj && !has_vel) || (out->u_init && !h->generated)) return WCQP_E_UNSUPPORTED;
    WCQP_HIP_TRY(hipDeviceSynchronize());
    const size_t N = (size_t)n, M = (size_t)m, T = (size_t)d.traj_len, R0 = (size_t)robot0, S0 = (size_t)stage0;
    for (int which = 0; which < 2; ++which) {
        double* dst = which ? out->dcm_vel_traj : out->ref_traj;
        const double* src = which ? d.dcm_vel.get() : d.ref_traj.get();
        if (dst) WCQP_HIP_TRY(hipMemcpy2D(dst, M * 16, src + (R0 * T + S0) * 2, T * 16, M * 16, N, hipMemcpyDeviceToHost));
    }
    if (out->u_init) WCQP_HIP_TRY(hipMemcpy(out->u_init, h->gen_zmp0 + R0 * 2, N * 16, hipMemcpyDeviceToHost));
    const bool hull = out->hull_A || out->hull_b || out->hull_nc;
    std::vector<double> sA, sb; std::vector<int> snc;
    if (hull) {
        sA.resize(h->n_sets * 16); sb.resize(h->n_sets * 8); snc.resize(h->n_sets);
        WCQP_HIP_TRY(hipMemcpy(sA.data(), h->set_A, h->n_sets * 128, hipMemcpyDeviceToHost));
        WCQP_HIP_TRY(hipMemcpy(sb.data(), h->set_b, h->n_sets * 64, hipMemcpyDeviceToHost));
        WCQP_HIP_TRY(hipMemcpy(snc.data(), h->set_nc, h->n_sets * 4, hipMemcpyDeviceToHost));
    }
    if (!hull && !out->contact && !out->com_height && !out->com_height_vel && !out->left_traj && !out->right_traj && !out->left_twist && !out->right_twist)
        return WCQP_OK;
    // the records of the window, a slab of robots at a time (64 MiB of host memory at most, one robot at least), unpacked on the host
    size_t slab = ((size_t)64 << 20) / (M * kPlanRec * 8);
    slab = slab < 1 ? 1 : (slab > N ? N : slab);
    std::vector<double> rec(slab * M * kPlanRec);
    for (size_t i0 = 0; i0 < N; i0 += slab) {
        const size_t nn = N - i0 < slab ? N - i0 : slab;
        WCQP_HIP_TRY(hipMemcpy2D(rec.data(), M * kPlanRec * 8, h->plan_rec + ((R0 + i0) * T + S0) * kPlanRec, T * kPlanRec * 8, M * kPlanRec * 8, nn,
                                 hipMemcpyDeviceToHost));
        for (size_t w0 = 0; w0 < nn * M; ++w0) {
            const double* r = &rec[w0 * kPlanRec];
            const size_t w = i0 * M + w0;
            if (out->contact) out->contact[w] = (uint8_t)r[kPlanFlags];
            if (out->com_height) out->com_height[w] = r[kPlanHeight];
            if (out->com_height_vel) out->com_height_vel[w] = r[kPlanHeightVel];
            if (out->left_traj) std::memcpy(out->left_traj + w * 12, r + kPlanLeft, 96);
            if (out->right_traj) std::memcpy(out->right_traj + w * 12, r + kPlanRight, 96);
            if (out->left_twist) std::memcpy(out->left_twist + w * 6, r + kPlanTwL, 48);
            if (out->right_twist) std::memcpy(out->right_twist + w * 6, r + kPlanTwL + 6, 48);
            if (hull) {
                const size_t set = (size_t)r[kPlanHull];
                if (set >= h->n_sets) return WCQP_E_HIP;
                if (out->hull_A) std::memcpy(out->hull_A + w * 16, &sA[set * 16], 128);
                if (out->hull_b) std::memcpy(out->hull_b + w * 8, &sb[set * 8], 64);
                if (out->hull_nc) out->hull_nc[w] = snc[set];
            }
        }
    }
    return WCQP_OK;
}

// what both forms of wcqp_tick_set_desired_* ask before they touch anything
static int desired_ready(const wcqp_tick_s* h, const wcqp_tick_desired* des) {
    if (!h || !des) return WCQP_E_INVALID;
    if (!h->streamed) return WCQP_E_UNSUPPORTED;
    if (!h->uploaded || !des->left_pose || !des->right_pose || !des->left_twist || !des->right_twist || !des->contact) return WCQP_E_INVALID;
    return WCQP_OK;
}

int wcqp_tick_set_desired_device(wcqp_tick_t h, const wcqp_tick_desired* des, void* stream) {
    if (const int rc = desired_ready(h, des); rc != WCQP_OK) return rc;
    const TickDev& d = h->d;
    DesiredDev a{};
    a.left_pose = des->left_pose; a.right_pose = des->right_pose; a.left_twist = des->left_twist; a.right_twist = des->right_twist;
    a.com_height = des->com_height; a.com_height_vel = des->com_height_vel; a.contact = des->contact; a.h0 = d.com_h0;
    a.rec = h->st_rec; a.set_A = h->st_set_A; a.set_b = h->st_set_b; a.set_nc = h->st_set_nc; a.pair = h->st_pair;
    a.ik_fail = d.ik_fail; a.feedback_fail = h->feedback_fail;
    a.batch = d.batch; a.first = h->desired_set ? 0 : 1; a.build = d.reactive ? 0 : 1;
    hipLaunchKernelGGL(tick_desired_kernel, dim3((unsigned)((d.batch + 3) / 4)), dim3(64), 0, (hipStream_t)stream, a, plan_rect(h));
    WCQP_HIP_TRY(hipGetLastError());
    h->desired_set = true; h->plan_staged = false;
    return WCQP_OK;
}

int wcqp_tick_set_desired_from_plan(wcqp_tick_t h, void* stream) {
    if (!h) return WCQP_E_INVALID;
    if (!h->resident) return WCQP_E_UNSUPPORTED;
    // (every upload of such a handle brings a plan; stage t = ticks_enqueued is one a tick may run: within the records, and validated)
    if (!h->uploaded || h->ticks_enqueued >= h->p.max_ticks) return WCQP_E_INVALID;
    const TickDev& d = h->d;
    StageDev a{};
    a.plan = h->plan_rec; a.set_A = h->set_A; a.set_b = h->set_b; a.set_nc = h->set_nc;
    a.tick = d.tick2.p + h->phase;
    a.rec = h->st_rec; a.st_A = h->st_set_A; a.st_b = h->st_set_b; a.st_nc = h->st_set_nc; a.pair = h->st_pair;
    a.batch = d.batch; a.traj_len = d.traj_len; a.first = h->desired_set ? 0 : 1;
    hipLaunchKernelGGL(tick_stage_from_plan_kernel, dim3((unsigned)((d.batch + 3) / 4)), dim3(64), 0, (hipStream_t)stream, a);
    WCQP_HIP_TRY(hipGetLastError());
    h->desired_set = true; h->plan_staged = true;
    return WCQP_OK;
}

// wcqp_tick_set_desired_host's staging rows, each array named once (the call's layout, and the capacity wcqp_tick_create gives the block)
struct DesiredStage {
    wcqp::HostStage st;
    wcqp::StageSlot<double> lp, rp, lt, rt, ch, chv;
    wcqp::StageSlot<uint8_t> contact;
    DesiredStage(size_t B, const wcqp_tick_desired& des)
        : lp(st.in(des.left_pose, B * 12)), rp(st.in(des.right_pose, B * 12)), lt(st.in(des.left_twist, B * 6)), rt(st.in(des.right_twist, B * 6)),
          ch(st.in(des.com_height, B, /*the handle's constant height without it*/ true)), chv(st.in(des.com_height_vel, B, true)),
          contact(st.in(des.contact, B)) {}
};

int wcqp_tick_set_desired_host(wcqp_tick_t h, const wcqp_tick_desired* des) {
    if (const int rc = desired_ready(h, des); rc != WCQP_OK) return rc;
    const size_t B = (size_t)h->d.batch;
    // the stage rule of the planned upload: an invalid stage leaves the handle as it was
    for (size_t i = 0; i < B; ++i)
        if (!stage_valid(des->contact[i], des->left_pose + i * 12, des->right_pose + i * 12, des->left_twist + i * 6, des->right_twist + i * 6,
                         des->com_height ? des->com_height + i : nullptr, des->com_height_vel ? des->com_height_vel + i : nullptr))
            return WCQP_E_INVALID;
    // the last run may have been enqueued on a non-blocking stream, which the NULL stream below does not wait for: wait for its end
    if (const int rc = h->run.wait(); rc != WCQP_OK) return rc;
    DesiredStage s(B, *des);
    int rc = s.st.upload(h->des_stage.ptr, h->des_stage.cap);
    if (rc != WCQP_OK) return rc;
    wcqp_tick_desired dv{};
    dv.left_pose = s.st[s.lp]; dv.right_pose = s.st[s.rp]; dv.left_twist = s.st[s.lt]; dv.right_twist = s.st[s.rt];
    dv.com_height = s.st[s.ch]; dv.com_height_vel = s.st[s.chv]; dv.contact = s.st[s.contact];
    rc = wcqp_tick_set_desired_device(h, &dv, nullptr);
    if (rc != WCQP_OK) return rc;
    // in place when this call returns: the tick may be enqueued on any stream, and the staging rows are free for the next call
    WCQP_HIP_TRY(hipStreamSynchronize(nullptr));
    return WCQP_OK;
}

}  // extern "C"

namespace wcqp {
// no stage yet (every tick's comes through wcqp_tick_set_desired_*): zero records, no rows, no pair - a robot whose very first stage is
// rejected runs stopped on a record that holds nothing
int reset_streamed_stage(wcqp_tick_s* h) {
    const size_t B = (size_t)h->d.batch;
    WCQP_HIP_TRY(hipMemset(h->st_rec, 0, B * kPlanRec * 8)); WCQP_HIP_TRY(hipMemset(h->st_set_nc, 0, B * 4));
    WCQP_HIP_TRY(hipMemset(h->st_pair, 0xff, B * 8));
    return WCQP_OK;
}
size_t desired_stage_bytes(size_t batch) {
    const double* const d = stage_sizing<double>();
    const wcqp_tick_desired all{d, d, d, d, stage_sizing<uint8_t>(), d, d};
    return DesiredStage(batch, all).st.total;
}
}  // namespace wcqp
