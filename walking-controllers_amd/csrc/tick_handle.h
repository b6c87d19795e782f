// The tick handle (wcqp_tick_t) and what its two translation units share: tick.hip (create / destroy, upload, run, splice, feedback,
// download) and tick_plan.hip (planned, generated, replanned and streamed trajectories).  Internal, not ABI.
#pragma once
#include <vector>
#include "wcqp_internal.h"
#include "tick_device.h"
#include "ik_common.h"
#include "position_tick.h"
#include "goal_merge.h"

// how a tick is launched: the skewed base-eliminated kernel (ONE launch), MPC + the 16-lane kernel with glue and post fused in
// (two), or MPC, glue, IK and post (four; any other IK kernel, and what the fused forms are tested against)
enum class TickForm { SKEWED, MPC_IK16, FOUR_LAUNCH };

// A device block that takes the caller's HOST arrays at call time and is then read in the caller's stream order, behind ticks that may
// still run for a long time: it only grows, and an event recorded behind its consumer guards it for the next call.  Without a block
// (`mem` unused) it is that guard alone.
struct StagedBlock {
    wcqp::DeviceScratch mem;
    hipEvent_t done = nullptr;
    bool pending = false;
    // the previous consumer has left
    int wait() {
        if (pending) { WCQP_HIP_TRY(hipEventSynchronize(done)); pending = false; }
        return WCQP_OK;
    }
    // a block of `bytes` whose first `n` are the caller's `host` rows, taken NOW: copied on a copy stream of the handle's own (made here
    // when there is none yet) and waited for before this returns
    int take(hipStream_t& copy_stream, const void* host, size_t n, size_t bytes) {
        if (!copy_stream) WCQP_HIP_TRY(hipStreamCreateWithFlags(&copy_stream, hipStreamNonBlocking));
        if (!done) WCQP_HIP_TRY(hipEventCreateWithFlags(&done, hipEventDisableTiming));
        int rc = wait();
        if (rc == WCQP_OK) rc = mem.reserve(bytes);
        if (rc != WCQP_OK) return rc;
        WCQP_HIP_TRY(hipMemcpyAsync(mem.ptr, host, n, hipMemcpyHostToDevice, copy_stream));
        WCQP_HIP_TRY(hipStreamSynchronize(copy_stream));
        return WCQP_OK;
    }
    // the consumer is everything enqueued on `s` so far
    int guard(hipStream_t s) {
        WCQP_HIP_TRY(hipEventRecord(done, s));
        pending = true;
        return WCQP_OK;
    }
    void release() {
        mem.release();
        if (done) (void)hipEventDestroy(done);
        done = nullptr; pending = false;
    }
};

// A device block of fixed capacity that takes a host form's arrays (wcqp::HostStage::upload(ptr, cap)): wcqp_tick_create sizes it by the
// stage's own layout with every optional array present, so a call's layout always fits - and one that did not would be refused, not written
struct FixedStage {
    char* ptr = nullptr;
    size_t cap = 0;
};

struct wcqp_tick_s {
    wcqp_tick_params p{};
    wcqp_mpc_t mpc = nullptr;
    wcqp_ik_t ik = nullptr;
    wcqp_tick::TickDev d{};
    wcqp_tick::TickDev* d_dev = nullptr;     // skewed tick: a TickDevPL of `d` in device memory (the fused kernels read it from there, see ik4_device.h)
    wcqp_ik::TickVariant variant{};   // skewed tick: the kernels this handle runs (wcqp_tick_create)
    std::vector<void*> allocs;
    double *J_left = nullptr, *J_right = nullptr, *J_neck = nullptr, *J_com = nullptr;
    unsigned* mpc_active = nullptr; double* mpc_margin = nullptr;
    unsigned *ik_lo = nullptr, *ik_up = nullptr;
    hipGraph_t graph = nullptr;
    hipGraphExec_t graph_exec = nullptr;
    hipStream_t graph_stream = nullptr;
    bool uploaded = false;
    int ticks_enqueued = 0;  // since the last upload, less what wcqp_tick_rebase_plan took off (plan_shift): the stage of the next tick
    long long plan_shift = 0;     // stages rebased since the last upload, summed (WCQP_TICK_OPT_PLAN_SHIFT)
    // the tick count for what only asks whether a tick has run since the upload and for its parity (the hand-off record of the last tick,
    // the feedback kernels' first-tick rule): a rebase takes an even count off ticks_enqueued, perhaps all of it, and no tick back
    int ticks_for_handoff() const { return ticks_enqueued == 0 && plan_shift > 0 ? 2 : ticks_enqueued; }
    double* log_ferr = nullptr;   // logger rows with dense Jacobians: where the IK kernel forms the foot errors
    TickForm form = TickForm::FOUR_LAUNCH;   // from the IK handle's route (wcqp_tick_create)
    wcqp_kin_t kin = nullptr;     // use_kinematics: Jacobians, actual poses and hull rows are rebuilt every tick
    wcqp_tick::KinTick kt{};
    int phase = 0;                // which copy of the tick index the next launch reads (TickDev::tick2): toggles per LAUNCH
    int ticks_per_launch = 1;     // > 1 only for the skewed tick without a kinematics launch: the ticks one launch walks through
    // wcqp_tick_splice_reference: the caller's host rows are staged HERE at call time (a copy stream of the handle's own, waited
    // for before the call returns), the strided device-to-device copy then runs in the caller's stream order
    StagedBlock splice;
    hipStream_t copy_stream = nullptr;
    bool vel_explicit = false;    // uploaded with an explicit dcm_vel_traj (reactive controller): the splice has no velocity tail
    bool external = false, feedback_set = false;     // wcqp_tick_params.plant = EXTERNAL: one tick per run call, each behind a set_feedback
    double* q_meas = nullptr;
    FixedStage fb_stage;          // wcqp_tick_set_feedback_host's staging rows (FeedbackStage, tick.hip)
    // sensor feedback (EXTERNAL with kinematics, wcqp_tick_set_sensor_feedback_*): the host form's staging rows (SensorStage, tick.hip),
    // the rejection counter, and the guard each run records on its stream (no block: the host forms wait for it before they stage)
    FixedStage sens_stage;
    long long* feedback_fail = nullptr;
    StagedBlock run;
    // the sensor form's low-pass filters (wcqp_tick_params.*_cut_frequency; sensors.h): two slots of per-robot state [2][B][kFiltRec].  A
    // sensor call reads slot filt_cur - what the last RUN tick left - and writes the other one; wcqp_tick_run commits it (filt_pending)
    // when it consumes the tick, so a replaced call advances nothing and a tick fed by the plain form holds the state.  A robot's FRESH mark
    // (sensors.h: kFiltFresh; wcqp_tick_reset_robots writes it into slot filt_cur) lies in its record and is double-buffered with it
    double* filt_state = nullptr;
    int filt_mask = 0, filt_cur = 0;
    bool filt_started = false, filt_pending = false;
    double filt_fb[3] = {0.0, 0.0, 0.0}, filt_fa[3] = {0.0, 0.0, 0.0};
    std::vector<double> meas0;    // EXTERNAL: dcm0, com0, u_init of the last upload ([B][6]: wcqp_tick_outputs.measured before any tick)
    wcqp_tick::ZmpSched zg{};     // zmp_gain_scheduling (d.gain_sched): the stance gains, the smoother, its per-robot state
    // the handle's TickDev with the scheduling record behind it (what the scheduled kernels take)
    wcqp_tick::TickDevGS dgs(const wcqp_tick::TickDev& base) const { wcqp_tick::TickDevGS g; static_cast<wcqp_tick::TickDev&>(g) = base; g.zg = zg; return g; }
    // planned_trajectories: the per-stage records and what the planned kernels take (the scheduling record behind it, used or not)
    bool planned = false;
    wcqp_tick::PlanDev pl{};
    double* set_A = nullptr; double* set_b = nullptr; int* set_nc = nullptr;     // the row sets of the last upload (PlanDev::set_*)
    size_t n_sets = 0;            // how many (wcqp_tick_get_plan reads them back)
    // wcqp_tick_upload_footsteps: the generated ZMP of stage 0 [B][2] (allocated by the first such upload), and whether the plan in place was generated
    double* gen_zmp0 = nullptr; bool generated = false;
    hipEvent_t gen_ev[2] = {nullptr, nullptr}; float gen_record_ms = 0.0f;     // the record pass of the last such upload, timed (wcqp_tick_info.plan_record_ms)
    // wcqp_tick_replan_footsteps: what the last wcqp_tick_upload_footsteps fixed for the handle - the timings, lift and deltas, and `cap`, the
    // slots of the set arrays each robot owns (robot i: [i cap, (i + 1) cap)) - and per robot the plan in force: the stage it was generated
    // from, its first double support and step count, and `keep`, the robot's slots in use by sets of stages <= that origin
    struct GenPlan {
        int ss = 0, ds = 0, final_ds = 0, cap = 0;
        double lift = 0.0, delta[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
        // THE SHAPED SWING: the profile the upload took (the handle's swing_pending at that call); every replan of the plan keeps it
        wcqp_tick_swing_profile swing{0.0, 0.0, 0.0, 0.0};
        bool shaped() const { return swing.apex_ratio != 0.0 || swing.landing_velocity != 0.0 || swing.pitch_delta != 0.0 || swing.com_height_delta != 0.0; }
        std::vector<int> origin, first_ds, n_steps, keep;
        // a TIMED plan (wcqp_tick_upload_footsteps_timed): ss and ds are unused, final_ds is the upload's own value (0: a last step's own
        // ds), cap counts a step as two stages, and dur[i] holds the durations of robot i's plan in force, ss_k then ds_k per step
        bool timed = false;
        std::vector<std::vector<int>> dur;
        // robot i's plan in force on its own timeline (goal_merge.h) - the one place that knows which kind of plan the handle holds
        wcqp_goal::Timeline timeline(size_t i) const {
            return timed ? wcqp_goal::Timeline::per_step(origin[i], first_ds[i], n_steps[i], dur[i].data(), dur[i].data() + 1, 2)
                         : wcqp_goal::Timeline::uniform(origin[i], first_ds[i], n_steps[i], ss, ds);
        }
        // robot i takes n steps from now on: on a timed plan with the durations ss_k / ds_k [n] (unread on an untimed one)
        void set_steps(size_t i, int n, const int32_t* ss_k, const int32_t* ds_k) {
            n_steps[i] = n;
            if (!timed) return;
            dur[i].resize(2 * (size_t)n);
            for (int k = 0; k < n; ++k) { dur[i][2 * k] = ss_k[k]; dur[i][2 * k + 1] = ds_k[k]; }
        }
    } gp;
    // wcqp_tick_set_swing_profile: what the NEXT wcqp_tick_upload_footsteps* copies into gp.swing (a running plan never sees it)
    wcqp_tick_swing_profile swing_pending{0.0, 0.0, 0.0, 0.0};
    // its per-call device memory (footsteps, robot and tile lists, footprint tables, set table), guarded behind the call's kernels
    StagedBlock rp;
    // The result rows of a goal call (wcqp_tick_replan_goals*), one contiguous run of B robots' rows for a planner of K steps - doubles,
    // then the 32-bit rows, then the bytes -: the kernels write them in device memory, one copy brings them into GoalCall::host, and every
    // reader finds a row at the offset stated HERE.  A timed call has the two duration rows [B][K]; an untimed one gives them no room.
    struct GoalRows {
        size_t K = 0; bool timed = false;
        size_t target = 0, dp = 0, ue = 0, n = 0, status = 0, ss = 0, ds = 0, side = 0, fs = 0, bytes = 0;
        static GoalRows of(size_t B, size_t K, bool timed) {
            GoalRows r;
            const size_t BK = B * K, dur = timed ? BK * 4 : 0;
            r.K = K; r.timed = timed;
            r.target = 0; r.dp = r.target + BK * 24; r.ue = r.dp + B * 16;
            r.n = r.ue + B * 24; r.status = r.n + B * 4; r.ss = r.status + B * 4; r.ds = r.ss + dur;
            r.side = r.ds + dur; r.fs = r.side + BK; r.bytes = r.fs + B;
            return r;
        }
        template <class T> T* at(char* base, size_t off) const { return reinterpret_cast<T*>(base + off); }
        template <class T> const T* at(const char* base, size_t off) const { return reinterpret_cast<const T*>(base + off); }
    };
    // wcqp_tick_replan_goals: the footsteps are planned on the device, so a goal-replanned robot's gp.n_steps is known only once the
    // call's result rows have come back into `host` (pinned; one copy behind the call's kernels, `ev` recorded behind it).  Until then the
    // robot is `owed`: whatever reads gp.n_steps calls settle() first, which waits for that event alone and folds the values in.  The
    // rows stay for wcqp_tick_get_goal_result, with what the host decided per robot at the call: the merge stage taken (0: none) and
    // WCQP_GOAL_KEPT / WCQP_GOAL_TOO_LATE (0: the device's status row holds).  A TIMED goal call (wcqp_tick_replan_goals_timed) owes the
    // robot's durations too, and settle() folds them into gp.dur next to the step counts - every reader of a timeline (the merge rule,
    // replan_admit, AUTO of a later goal call) sits behind a settle()
    struct GoalCall {
        char* host = nullptr; size_t host_cap = 0;
        hipEvent_t ev = nullptr;
        bool called = false, pending = false;
        GoalRows rows;                                    // of the last call: the planner's max_steps, timed or not, where its rows lie in `host`
        std::vector<int> owed, merge, decided;
        int wait() {
            if (pending) { WCQP_HIP_TRY(hipEventSynchronize(ev)); pending = false; }
            return WCQP_OK;
        }
        void release() {
            if (host) (void)hipHostFree(host);
            if (ev) (void)hipEventDestroy(ev);
            host = nullptr; host_cap = 0; ev = nullptr; pending = false; called = false; owed.clear();
        }
    } goal;
    // wcqp_tick_rebase_plan owes the same way: d_i, the slots robot i's sets moved down by, is read on the device (plan_rebase.hip) and
    // comes back into `host` (pinned, [B]) behind `ev`; until then every gp.keep is owed d_i, and settle() takes it off.  A call settles
    // before it enqueues, so one row is in flight at most.  dev / host: allocated by the first wcqp_tick_upload_footsteps*
    struct RebaseCall {
        int* dev = nullptr; int* host = nullptr;
        hipEvent_t ev = nullptr;
        bool pending = false;
        void release() {
            if (host) (void)hipHostFree(host);
            if (ev) (void)hipEventDestroy(ev);
            host = nullptr; ev = nullptr; pending = false;
        }
    } rebase;
    // wcqp_tick_restart_robots and wcqp_tick_recover_robots: one row per LISTED robot (slot r of the call: robot robots[r]) comes back into
    // `host` (pinned) behind `ev`: the ik_fail rows [n] as int64, a recover call's residual rows [n][2] as doubles, the decisions [n] as
    // int32, a recover call's status and iters rows [n] as int32.  THE RULE, for both calls: a robot whose restart the HOST decides - one
    // listed ALWAYS in a restart call - is on its standing plan in gp at once; a robot the DEVICE decides - IF_STOPPED, and every listed
    // robot of a recover call, whose IK must end SOLVED - is `owed`, and settle() puts it on the standing plan (origin `stage`, no steps,
    // `keep_new` slots in use) if its row says it restarted.  The rows stay for wcqp_tick_get_restart_result / _recover_result.
    // wcqp_tick_reset_robots (a streamed EXTERNAL handle) is a restart call here; without a resident plan no robot is ever owed
    struct RestartCall {
        char* host = nullptr; size_t host_cap = 0;
        hipEvent_t ev = nullptr;
        bool called = false, pending = false;           // pending: the rows are still on their way
        bool recover = false;                           // the last call was a recover call: the rows hold its three more columns
        int stage = 0;
        std::vector<int> robots, keep_new, owed;        // by slot: the robot, its slot count if it restarts; the slots still owed
        static size_t row_bytes(bool recover) { return recover ? 36 : 12; }
        const long long* stopped() const { return reinterpret_cast<const long long*>(host); }
        const double* residual() const { return reinterpret_cast<const double*>(host + robots.size() * 8); }
        const int* restarted() const { return reinterpret_cast<const int*>(host + robots.size() * (recover ? 24 : 8)); }
        const int* status() const { return restarted() + robots.size(); }
        const int* iters() const { return restarted() + 2 * robots.size(); }
        int wait() {
            if (pending) { WCQP_HIP_TRY(hipEventSynchronize(ev)); pending = false; }
            return WCQP_OK;
        }
        void release() {
            if (host) (void)hipHostFree(host);
            if (ev) (void)hipEventDestroy(ev);
            host = nullptr; host_cap = 0; ev = nullptr; pending = false; called = false; recover = false; owed.clear();
        }
    } restart;
    // robot i stands from stage S on: the plan in force wcqp_tick_restart_robots leaves
    void stand_from(size_t i, int S, int keep_new) {
        gp.origin[i] = S; gp.first_ds[i] = 0; gp.keep[i] = keep_new;
        gp.set_steps(i, 0, nullptr, nullptr);
    }
    int settle() {
        if (!restart.owed.empty()) {
            if (const int rc = restart.wait(); rc != WCQP_OK) return rc;
            for (int r : restart.owed)
                if (restart.restarted()[r]) stand_from((size_t)restart.robots[r], restart.stage, restart.keep_new[r]);
            restart.owed.clear();
        }
        if (const int rc = goal.wait(); rc != WCQP_OK) return rc;
        if (!goal.owed.empty()) {
            const GoalRows& r = goal.rows;
            const int32_t* n = r.at<int32_t>(goal.host, r.n);
            for (int i : goal.owed) gp.set_steps((size_t)i, n[i], r.at<int32_t>(goal.host, r.ss) + (size_t)i * r.K, r.at<int32_t>(goal.host, r.ds) + (size_t)i * r.K);
            goal.owed.clear();
        }
        if (rebase.pending) {
            WCQP_HIP_TRY(hipEventSynchronize(rebase.ev));
            rebase.pending = false;
            for (size_t i = 0; i < gp.keep.size(); ++i) gp.keep[i] -= rebase.host[i];
        }
        return WCQP_OK;
    }
    // streamed_trajectories (an EXTERNAL handle): pl.rec holds ONE record per robot, the stage wcqp_tick_set_desired_* handed over for the next
    // tick, pl.set_* one row set per robot; `planned` stays false (the splice of the DCM reference keeps working)
    bool streamed = false, desired_set = false;
    double* st_rec = nullptr; double* st_set_A = nullptr; double* st_set_b = nullptr; int* st_set_nc = nullptr;
    int* st_pair = nullptr;       // [B][2] contact pair of the last consumed stage / of the stage in hand (tick_desired_kernel)
    FixedStage des_stage;         // wcqp_tick_set_desired_host's staging rows (DesiredStage, tick_plan.hip)
    // resident_plan (a streamed handle): it also holds a plan - records and row sets as a planned handle's - which the kernels of the tick never
    // see (pl keeps pointing at the live record and the robots' own sets); wcqp_tick_set_desired_from_plan copies stage t out of it.
    // plan_rec: the records [B][traj_len][kPlanRec] of whichever handle holds a plan (a planned handle: pl.rec), what the plan generator,
    // the replan, the set builder and wcqp_tick_get_plan take.  plan_staged: the stage in hand came from the plan (the replan rule)
    bool resident = false, plan_staged = false;
    double* plan_rec = nullptr;
    bool holds_plan() const { return planned || resident; }
    wcqp_tick::TickDevPL dpl(const wcqp_tick::TickDev& base) const { wcqp_tick::TickDevPL g; static_cast<wcqp_tick::TickDevGS&>(g) = dgs(base); g.pl = pl; return g; }
    // ik_mode = POSITION (a planned handle): the non-linear IK runs every tick in position_tick_kernel, which takes `pos` beside the
    // handle's TickDevPL in device memory; the chain's state, hand-off rows and live hull rows are the skewed handle's, but nothing is
    // skewed - no prime launch, no tick ahead.  With WCQP_TICK_OPT_POSITION_STREAMED the handle is a streamed one instead (`streamed`,
    // `external`, perhaps `resident`, with everything such a handle allocates) and position_tick_external_kernel runs its one tick per call
    bool position = false;
    wcqp::PosTickDev pos{};
};

template <typename T>
int dev_alloc(wcqp_tick_s* h, T** out, size_t count) {
    void* p = nullptr;
    if (hipMalloc(&p, (count > 0 ? count : 1) * sizeof(T)) != hipSuccess) return WCQP_E_NOMEM;
    h->allocs.push_back(p);              // owned from here on: wcqp_tick_destroy frees it whatever happens next
    if (hipMemset(p, 0, (count > 0 ? count : 1) * sizeof(T)) != hipSuccess) return WCQP_E_HIP;
    *out = static_cast<T*>(p);
    return WCQP_OK;
}

template <typename T>
int dev_alloc(wcqp_tick_s* h, wcqp::GPtr<T>* out, size_t count) { return dev_alloc(h, &out->p, count); }

namespace wcqp {
// tick_plan.hip, for wcqp_tick_upload of a planned handle: the caller's per-stage arrays checked before anything of the handle changes,
// then repacked into the records with their support-polygon row sets
int validate_plan(const wcqp_tick_s* h, const wcqp_tick_inputs* in);
int upload_plan(wcqp_tick_s* h, const wcqp_tick_inputs* in);
// tick_plan.hip, for both uploads of a streamed handle: no stage in hand - zero records, no rows, no pair
int reset_streamed_stage(wcqp_tick_s* h);
// tick.hip, the tail wcqp_tick_upload and wcqp_tick_upload_footsteps share once the trajectories are in place (pair0 >= 0: the contact
// pair of stage 0 where `in` holds no contact array)
int upload_state(wcqp_tick_s* h, const wcqp_tick_inputs* in, int pair0);
// tick_plan.hip, for wcqp_tick_create: the bytes of wcqp_tick_set_desired_host's staging rows with every optional array present
size_t desired_stage_bytes(size_t batch);
}  // namespace wcqp
