// Sensor feedback of the tick pipeline (wcqp_tick_set_sensor_feedback_*, include/wcqp.h): the measured CoM, DCM and ZMP of every
// robot from its joint encoders and the two feet's force / torque wrenches, evaluated on the device (sensors.hip).  Internal, not ABI.
#pragma once
#include "wcqp_internal.h"

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
};

}  // namespace wcqp_tick

namespace wcqp {
// enqueues the sensor kernel for tick a.t of every robot on `stream` (sensors.hip)
int sensor_feedback_enqueue(const wcqp_tick::SensorDev& a, hipStream_t stream);
}  // namespace wcqp
