// Planned trajectories generated on the device from per-robot footstep lists (wcqp_tick_upload_footsteps, include/wcqp.h, which
// defines the plan; plan_gen.hip holds the kernels).  Internal, not ABI.
#pragma once
#include "wcqp_internal.h"
#include "tick_device.h"

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
    const int* set_base;            // [B] index of the robot's first support-polygon set (sets are numbered robot by robot, stage by stage)
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
};

}  // namespace wcqp_tick

namespace wcqp {
// prologue, DCM pass and record pass of one upload, in stream order (plan_gen.hip); rec0 / rec1 (or NULL): events recorded around the record pass
int plan_gen_enqueue(const wcqp_tick::PlanGenDev& g, hipStream_t stream, hipEvent_t rec0, hipEvent_t rec1);
}  // namespace wcqp
