// Support-polygon rows from foot poses.  One thread per robot instance: the
// hull of at most 8 points is a few dozen flops, the kernel is a pure streaming pass
// (2 x 96 B in, 200 B out per instance).
//
// Reference: WalkingController::setConvexHullConstraint / buildConvexHull
//            src/WalkingDCMModelPredictiveController.cpp:364-489 (iDynTree ConvexHullHelpers upstream).
#include <cmath>
#include "wcqp_internal.h"
#include "hull_device.h"

namespace {

__global__ void __launch_bounds__(128) hull_from_feet_kernel(int batch, const double* __restrict__ rect,
                                      const double* __restrict__ left_T, const double* __restrict__ right_T,
                                      const unsigned char* __restrict__ contact,
                                      double* __restrict__ hull_A, double* __restrict__ hull_b, int* __restrict__ hull_nc) {
    const int inst = blockIdx.x * blockDim.x + threadIdx.x;
    if (inst >= batch) return;
    double px[8], py[8];
    int np = 0;
    const unsigned c = contact[inst];
    for (int f = 0; f < 2; ++f) {
        if (!((c >> f) & 1u)) continue;
        // foot-frame corner (x, y, 0) -> world, projected on the XY plane through the origin
        wcqp_hull::foot_points(rect, (f == 0 ? left_T : right_T) + (size_t)inst * 12, px, py, np);
    }
    hull_nc[inst] = wcqp_hull::hull_rows(px, py, np, hull_A + (size_t)inst * 16, hull_b + (size_t)inst * 8);
}

// The tick pipeline with per-tick kinematics: the three row sets (left foot, right foot, both in contact) of every robot
// from the DESIRED foot poses in its pose block (entries 24..35 left, 36..47 right).  One thread per (robot, contact pair).
struct RectArg { double v[8]; };
__global__ void __launch_bounds__(128) hull_tables_kernel(int batch, RectArg rect, const double* __restrict__ state, int state_len,
                                   double* __restrict__ tab_A, double* __restrict__ tab_b, int* __restrict__ tab_nc) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= batch * 3) return;
    const int inst = g / 3, code = g % 3;
    const double* sd = state + (size_t)inst * state_len;
    double px[8], py[8];
    int np = 0;
    if (code == 0 || code == 2) wcqp_hull::foot_points(rect.v, sd + 24, px, py, np);
    if (code == 1 || code == 2) wcqp_hull::foot_points(rect.v, sd + 36, px, py, np);
    tab_nc[g] = wcqp_hull::hull_rows(px, py, np, tab_A + (size_t)g * 16, tab_b + (size_t)g * 8);
}

}  // namespace

namespace wcqp {
int hull_tables_from_state(int batch, const double* foot_rect_host, const double* state_dev, int state_len,
                           double* tab_A, double* tab_b, int* tab_nc, hipStream_t stream) {
    if (batch < 1 || !foot_rect_host || !state_dev || !tab_A || !tab_b || !tab_nc) return WCQP_E_INVALID;
    RectArg r;
    for (int k = 0; k < 8; ++k) r.v[k] = foot_rect_host[k];
    hipLaunchKernelGGL(hull_tables_kernel, dim3((batch * 3 + 127) / 128), dim3(128), 0, stream, batch, r, state_dev, state_len, tab_A, tab_b, tab_nc);
    WCQP_HIP_TRY(hipGetLastError());
    return WCQP_OK;
}
}  // namespace wcqp

extern "C" {

// what both forms refuse before they look for a device
static int check_call(int32_t batch, const double* foot_rect, const double* left_T, const double* right_T,
                      const uint8_t* contact, const double* hull_A, const double* hull_b, const int32_t* hull_nc) {
    return batch < 0 || !foot_rect || !left_T || !right_T || !contact || !hull_A || !hull_b || !hull_nc ? WCQP_E_INVALID : WCQP_OK;
}

int wcqp_hull_from_feet_device(int32_t batch, const double* foot_rect, const double* left_T, const double* right_T,
                               const uint8_t* contact, double* hull_A, double* hull_b, int32_t* hull_nc, void* stream) {
    const int rc = check_call(batch, foot_rect, left_T, right_T, contact, hull_A, hull_b, hull_nc);
    if (rc != WCQP_OK || batch == 0) return rc;
    hipLaunchKernelGGL(hull_from_feet_kernel, dim3((batch + 127) / 128), dim3(128), 0, (hipStream_t)stream,
                       batch, foot_rect, left_T, right_T, contact, hull_A, hull_b, hull_nc);
    WCQP_HIP_TRY(hipGetLastError());
    return WCQP_OK;
}

int wcqp_hull_from_feet_host(int32_t batch, const double* foot_rect, const double* left_T, const double* right_T,
                             const uint8_t* contact, double* hull_A, double* hull_b, int32_t* hull_nc) {
    int rc = check_call(batch, foot_rect, left_T, right_T, contact, hull_A, hull_b, hull_nc);
    if (rc != WCQP_OK || batch == 0) return rc;
    rc = wcqp::require_device("hull builder");
    if (rc != WCQP_OK) return rc;
    const size_t B = (size_t)batch;
    wcqp::HostStage st;
    const auto d_rect = st.in(foot_rect, 8), d_l = st.in(left_T, B * 12), d_r = st.in(right_T, B * 12);
    const auto d_A = st.out(hull_A, B * 16), d_b = st.out(hull_b, B * 8);
    const auto d_n = st.out(hull_nc, B);
    const auto d_c = st.in(contact, B);
    // no handle: a block of the call's own, released on every way out; a copy that fails is WCQP_E_HIP
    wcqp::DeviceScratch block;
    rc = st.upload(block);
    if (rc == WCQP_OK) rc = wcqp_hull_from_feet_device(batch, st[d_rect], st[d_l], st[d_r], st[d_c], st[d_A], st[d_b], st[d_n], nullptr);
    if (rc == WCQP_OK) rc = st.download();
    block.release();
    return rc;
}

}  // extern "C"
