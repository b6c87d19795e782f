// Sensor feedback of the tick pipeline (wcqp_tick_set_sensor_feedback_*, include/wcqp.h): the measured CoM, DCM and ZMP of every
// robot from its joint encoders and the two feet's force / torque wrenches, evaluated on the device (sensors.hip).  Internal, not ABI.
#pragma once
#include "wcqp_internal.h"
#include "tick_device.h"

namespace wcqp_tick {

// what the sensor kernel reads and writes: the caller's sensor arrays and the handle's state
struct SensorDev {
    const double* q;              // [B][kDof] measured joint positions (rad)
    const double* dq;             // [B][kDof] measured joint velocities (rad/s)
    const double* wl;             // [B][6] left sole wrench fx fy fz tx ty tz, in the sole frame
    const double* wr;             // [B][6] right sole wrench
    const double* q_des;          // [B][kDof] TickDev::q_des (a rejected robot's measured joints at tick 0)
    const double* state;          // [B][kStateLen] the desired sole poses at 24 (left) / 36 (right): p 3 | R 9
    const int* phase0;            // [B] gait offset: the stance side of tick t
    const double* kin_tab;        // TickDev::kin_tab, the fused kinematics' model table
    double* mst;                  // TickDev::mst: com [2], dcm [6], measured ZMP [7] of each axis' record
    const double* hand;           // TickDev::hand: com / dcm / measured ZMP of the previous tick (a rejected robot keeps them)
    double* q_meas;               // TickDev::q_meas
    long long* ik_fail;           // TickDev::ik_fail: > 0 stops the robot (tick_robot_stopped)
    long long* feedback_fail;     // [B] rejected sensor ticks
    int batch, t, step_ticks, kin_rounds;
    double omega;                 // sqrt(gravity / com_height)
    const double* rec;            // streamed trajectories: [B][kPlanRec] the stage of tick t (stance side and anchor pose); else NULL
    // the low-pass filters (wcqp_tick_params.*_cut_frequency; read by the FILT kernels only): the state of the last RUN tick, where this
    // tick's goes (the host commits it when wcqp_tick_run consumes the tick), y = fb (u + u_prev) + fa y_prev per filter
    const double* filt_src;       // [B][kFiltRec]
    double* filt_dst;             // [B][kFiltRec], the handle's other slot
    double fb[3], fa[3];          // joint velocity, wrench, CoM: Ts / (2 tau + Ts), (2 tau - Ts) / (2 tau + Ts)
    int filt_mask;                // bit 0 joint velocity, bit 1 wrench, bit 2 CoM (wcqp_tick_info.sensor_filters)
    int filt_first;               // the first sensor reading since the upload: the joint-velocity and wrench filters start AT it
};

// One robot's filter record (doubles), {u_prev, y_prev} pairs: joint velocity j at 2 j; the wrench components the ZMP reads - fz tx ty of the
// left sole, then of the right - at kFiltWrench + 2 c; axis a of the CoM at kFiltCom + 4 a (position pair, velocity pair).  At kFiltFresh
// the robot's FRESH mark (0.0 / 1.0; wcqp_tick_reset_robots sets it, every upload clears it): the joint-velocity and wrench filters start
// AT the robot's next accepted reading, as every robot's do at the first reading after an upload (SensorDev::filt_first).  It lies in the
// record, so it is double-buffered with it: a rejected reading carries it over, an accepted one clears it.  544 bytes.
constexpr int kFiltWrench = 46, kFiltCom = 58, kFiltFresh = 66, kFiltRec = 68;
static_assert(kFiltWrench == 2 * kDof && kFiltFresh == kFiltCom + 8 && (kFiltRec * 8) % 16 == 0, "filter record layout");

}  // namespace wcqp_tick

namespace wcqp {
// enqueues the sensor kernel for tick a.t of every robot on `stream` (sensors.hip); a.filt_mask != 0: the filtering one
int sensor_feedback_enqueue(const wcqp_tick::SensorDev& a, hipStream_t stream);
// The first-order low-pass 1 / (1 + s tau), tau = 1 / (2 pi cut_hz), discretised with the bilinear transform at the sample time Ts:
// y_k = (Ts (u_k + u_{k-1}) - (Ts - 2 tau) y_{k-1}) / (2 tau + Ts) = fb (u_k + u_{k-1}) + fa y_{k-1}
void lowpass_coeffs(double cut_hz, double Ts, double* fb, double* fa);
}  // namespace wcqp
