// Planned trajectories generated on the device from per-robot footstep lists (wcqp_tick_upload_footsteps, include/wcqp.h, which
// defines the plan; plan_gen.hip holds the kernels).  Internal, not ABI.
#pragma once
#include "wcqp_internal.h"
#include "tick_device.h"
#include "sensors.h"

namespace wcqp_tick {

// One robot's footprint table, [K + 1] entries of kFpRec doubles: entry j holds both feet's footprints after j steps have landed -
// left sole (p 3 | R 9 row-major) at 0, right sole at 12 - and the two feet's ZMP points (p_xy + R_2x2 delta) at 24 / 26.  Entries past the
// robot's own n_steps repeat the last one.
constexpr int kFpRec = 28, kFpPose = 24;

struct PlanGenDev {
    // the footsteps (device copies of wcqp_tick_footsteps) and the desired-foot / height entries of state0
    const int* n_steps;             // [B]
    const unsigned char* side;      // [B][K]
    const double* target;           // [B][K][3]
    const double* state;            // [B][kStateLen]
    const int* set_base;            // [B] index of the support-polygon set the plan's first stage names: an upload's stage-0 set, which the prologue
                                    // enters, or - a replan - the robot's last surviving set; the plan's own sets follow it (tick_plan.hip: a fixed range of
                                    // slots per robot)
    double* table;                  // [B][K + 1][kFpRec], written by the prologue
    long long* set_at;              // [sets] record offset (doubles) of each set's stage
    int* set_code;                  // [sets] its contact pair (0 left, 1 right, 2 both)
    double* rec;                    // PlanDev::rec
    double* ref;                    // TickDev::ref_traj
    double* vel;                    // TickDev::dcm_vel, or NULL on a handle that keeps none
    double* zmp0;                   // [B][2] the ZMP of stage 0
    int batch, K, traj_len, max_ticks;
    int first_ds, ss, ds, final_ds; // stages (final_ds already resolved: never 0)
    double lift, dT, omega, a;      // a = exp(omega dT)
    double delta[2][2];             // zmp_delta_left / zmp_delta_right
    // wcqp_tick_replan_footsteps only (plan_replan_enqueue; NULL / 0 in an upload): first_ds is then the double support from the merge stage
    const int* origin;              // [B] the stage M_i robot i's plan is regenerated from (its timeline's stage 0); unread for a robot not listed
    const int* robots;              // [n_robots] the robots regenerated
    const int2* tiles;              // [n_tiles] (robot, 64-stage tile) of the record pass: the tiles at or above the robot's origin
    const double* h0;               // [B] TickDev::com_h0, the CoM height of every stage
    int n_robots, n_tiles;
};

// THE SHAPED SWING (wcqp_tick_swing_profile, as the upload took it): a kernel argument of its own, behind PlanGenDev / PlanGenTimedDev, of
// the shaped record kernels only - with every field zero the launch path takes the kernels that do not know it, with the arguments they
// always took
struct PlanSwing {
    double apex, v_land, pitch, dh;
    bool shaped() const { return apex != 0.0 || v_land != 0.0 || pitch != 0.0 || dh != 0.0; }
};

// The timed calls' per-step durations (wcqp_tick_step_timing's device copies) and the start table the prologue writes from them
struct PlanTimes {
    const int* ss_k;                // [B][K] single-support stages of step k
    const int* ds_k;                // [B][K] double-support stages behind step k (the last step's: see final_ds)
    int* start;                     // [B][K + 1] entry k < n: the first stage s_k of step k's single support on the plan's own timeline (s_0 = first_ds);
                                    // entries n .. K: the first standing stage
    int final_ds;                   // the last step's double support, or 0 for its own ds_k
};
// what the timed kernels take: PlanGenDev as the untimed ones do (ss, ds and final_ds of it are not read), and the durations
struct PlanGenTimedDev {
    PlanGenDev g;
    PlanTimes tm;
};

// wcqp_tick_rebase_plan (plan_rebase.hip): a generated plan and everything indexed by its stages moved `shift` stages towards 0, in place
struct PlanRebaseDev {
    double* rec;                    // [B][traj_len][kPlanRec]
    double* ref;                    // TickDev::ref_traj
    double* vel;                    // TickDev::dcm_vel, or NULL on a handle that keeps none
    double* zmp0;                   // [B][2] the generated ZMP of stage 0
    double* set_A; double* set_b; int* set_nc;      // the row sets: robot i owns slots [i cap, (i + 1) cap)
    int* tick2;                     // TickDev::tick2: both copies of the tick index go down by shift
    int* d_out;                     // [B] d_i, the slots robot i's sets move down by: entry 39 of its old record `shift`, less i cap
    int batch, traj_len, shift, cap;
    double omega, a;                // a = exp(omega dT)
};

// wcqp_tick_restart_robots (plan_restart.hip): the listed robots - slot r of the call is robot robots[r] - decided on the device, and those
// that restart reset to the staged rows and put on a standing plan from stage S on.  The staged rows are compact, one per SLOT
struct PlanRestartDev {
    const int* robots;              // [n_robots]
    const unsigned char* mode;      // [n_robots] WCQP_TICK_RESTART_ALWAYS / _IF_STOPPED
    const int* decided;             // NULL, or [n_robots] the decision, made elsewhere on the device (plan_recover.hip: nonzero restarts); mode is then unread
    const double* state0;           // [n_robots][kStateLen]
    const double* q0;               // [n_robots][kDof]
    const double* com0;             // [n_robots][2]
    const double* dcm0;             // [n_robots][2], or NULL: the standing stage's ZMP
    const double* u0;               // [n_robots][2], or NULL: the same
    const int* set_slot;            // [n_robots] the robot's next free slot of the row sets: where its standing set goes
    const int2* tiles;              // [n_tiles] (slot, 64-stage tile): the tiles at or above S / 64
    // what the first kernel writes per slot for the second, and for the host
    double* pattern;                // [n_robots][kPlanRec] the standing record
    double* mid;                    // [n_robots][2] its ref_traj entry, the ZMP
    int* restarted;                 // [n_robots] 1: the robot restarts
    long long* stopped;             // [n_robots] its ik_fail just before (0 if it does not)
    long long* set_at; int* set_code;               // plan_hull_sets_kernel's table, indexed by set slot (memset to -1 ahead of the kernels)
    double* rec; double* ref; double* vel;          // the plan, as in PlanRebaseDev
    // the state wcqp::upload_state sets (tick.hip), every array indexed by ROBOT; NULL where the handle keeps none
    double *mst, *state, *q_des, *dq_prev, *dcm, *com, *c_ref, *p_star, *zmp_meas, *u_prev, *v_ref_prev, *v_star_prev, *zs, *com_h0;
    int *sel_built, *live_nc, *sel;
    long long *mpc_fail, *ik_fail, *hot_try, *hot_hit, *ik_iters;
    unsigned *ik_lo, *ik_up;
    int n_robots, n_tiles, traj_len, stage;         // stage: S
    double delta[2][2];             // zmp_delta_left / zmp_delta_right
};

// wcqp_tick_reset_robots (plan_restart.hip): what only a streamed EXTERNAL handle keeps per robot, reset behind plan_restart_reset_kernel for
// the slots it restarted - the rows of PlanRestartDev it reads are that call's.  Every array is indexed by ROBOT
struct TickResetDev {
    const int* robots;              // [n_robots] PlanRestartDev's
    const int* restarted;           // [n_robots] written by plan_restart_reset_kernel ahead of this kernel
    const double* q0;               // [n_robots][kDof]
    const double* com0;             // [n_robots][2]
    const double* dcm0;             // [n_robots][2], or NULL: `mid`
    const double* u0;               // [n_robots][2], or NULL: `mid`
    const double* mid;              // [n_robots][2] the standing ZMP plan_restart_reset_kernel wrote
    double* q_meas;                 // [B][kDof]
    long long* feedback_fail;       // [B]
    int* pair;                      // [B][2] st_pair: -1, -1 as after an upload
    double* st_rec; int* st_set_nc; // the live record [B][kPlanRec] and the row count of the robot's own set: 0 as after an upload
    double* hand_prev;              // the hand-off records [B][kHandLen] of parity S - 1, where a reading rejected at tick S finds the measured
                                    // state to keep; NULL at tick 0 (the host keeps the rows: wcqp_tick_s::meas0)
    double* filt;                   // the filter slot the next sensor call reads [B][kFiltRec], or NULL on a handle without filters
    int n_robots;
};

// a foot's ZMP point p_xy + R_2x2 delta of the sole `pose` (p 3 | R 9 row-major), every operation rounded on its own, as numpy does
__device__ __forceinline__ double zmp_point_ax(const double* pose, const double* dl, int ax) {
#pragma clang fp contract(off)
    const double r = pose[3 + 3 * ax] * dl[0] + pose[4 + 3 * ax] * dl[1];
    return pose[ax] + r;
}

// wcqp_tick_recover_robots (plan_recover.hip): around the non-linear IK of prepare.hip, the kernel that decides per slot and packs the rows
// of the slots that go on, and the gate that turns the IK's status into PlanRestartDev::decided and hands its rows to the restart
struct PlanRecoverDev {
    const int* robots;              // [n_robots]
    const unsigned char* mode;      // [n_robots] WCQP_TICK_RESTART_ALWAYS / _IF_STOPPED
    // the caller's rows, one per SLOT; NULL: left / right the soles of record S (both or neither), com the standing ZMP of the soles and the
    // height of record S, q the robot's q_des; neck: no neck target
    const double *left_in, *right_in, *com_in, *neck_in, *q_in;
    const long long* ik_fail;       // [B]
    const double* q_des;            // [B][kDof]
    const double* rec;              // the plan's records
    // what the gather kernel writes: per slot its packed row (>= 0) or WCQP_RECOVER_NOT_STOPPED / _NOT_STANDING; the rows of the slots that
    // go on, packed to the front in no particular order, as prepare_kernel reads them; and their number
    int* pos;                       // [n_robots]
    int* count;                     // zero when the kernel starts
    double *p_left, *p_right, *p_com, *p_neck, *p_q;
    // what the IK leaves per packed row, and what the gate makes of it per slot: the restart's rows and decision, the result rows
    const double *o_q, *o_state, *o_res;
    const int *o_status, *o_iters;
    double *state0, *q0, *com0;     // PlanRestartDev's
    int* decided;
    int *status, *iters; double* residual;
    int n_robots, traj_len, stage;
    double delta[2][2];
};

}  // namespace wcqp_tick

namespace wcqp {
// plan_recover.hip: the two kernels either side of the IK, each enqueue-only
int plan_recover_gather_enqueue(const wcqp_tick::PlanRecoverDev& g, hipStream_t stream);
int plan_recover_gate_enqueue(const wcqp_tick::PlanRecoverDev& g, hipStream_t stream);
// its two kernels in stream order: decide-and-reset over the slots, then the fill over the tiles.  Enqueue-only
int plan_restart_enqueue(const wcqp_tick::PlanRestartDev& g, hipStream_t stream);
// wcqp_tick_reset_robots: plan_restart_reset_kernel, the reset of what only an EXTERNAL handle keeps, and - g.rec set: a resident plan - the
// fill.  Enqueue-only
int tick_reset_enqueue(const wcqp_tick::PlanRestartDev& g, const wcqp_tick::TickResetDev& e, hipStream_t stream);
// its two kernels in stream order: d_i, the ZMP of the new stage 0 and the tick index first, then the rows.  Enqueue-only
int plan_rebase_enqueue(const wcqp_tick::PlanRebaseDev& g, hipStream_t stream);
// prologue, DCM pass and record pass of one upload, in stream order (plan_gen.hip); rec0 / rec1 (or NULL): events recorded around the record
// pass.  An untimed plan (ss, ds, final_ds >= 1), or a timed one (wcqp_tick_upload_footsteps_timed: final_ds >= 0 and the three rows).
// sw: the plan's swing profile (all zero: none)
int plan_gen_enqueue(const wcqp_tick::PlanGenDev& g, const wcqp_tick::PlanSwing& sw, hipStream_t stream, hipEvent_t rec0, hipEvent_t rec1);
int plan_gen_enqueue(const wcqp_tick::PlanGenTimedDev& t, const wcqp_tick::PlanSwing& sw, hipStream_t stream, hipEvent_t rec0, hipEvent_t rec1);
// the same three passes from per-robot origins, over the listed robots and tiles only (wcqp_tick_replan_footsteps*); enqueue-only
int plan_replan_enqueue(const wcqp_tick::PlanGenDev& g, const wcqp_tick::PlanSwing& sw, hipStream_t stream);
int plan_replan_enqueue(const wcqp_tick::PlanGenTimedDev& t, const wcqp_tick::PlanSwing& sw, hipStream_t stream);
}  // namespace wcqp
