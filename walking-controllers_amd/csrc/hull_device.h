// Device side of the support-polygon builder, shared by hull.hip and the tick pipeline's
// kinematics kernel.  Internal, not ABI.
// Reference: WalkingController::setConvexHullConstraint / buildConvexHull
//            src/WalkingDCMModelPredictiveController.cpp:364-489 (iDynTree ConvexHullHelpers upstream).
#pragma once
#include "wcqp_internal.h"

namespace wcqp_hull {

#if defined(__HIPCC__)
// Corners of the foot rectangle `rect` (x, y) x 4 through the foot-to-world transform T (position 3, row-major
// rotation 9), projected on the XY plane; appended to (px, py).
__device__ __forceinline__ void foot_points(const double* rect, const double* T, double* px, double* py, int& np) {
    for (int k = 0; k < 4; ++k) {
        const double x = rect[2 * k], y = rect[2 * k + 1];
        px[np] = T[3] * x + T[4] * y + T[0];
        py[np] = T[6] * x + T[7] * y + T[1];
        ++np;
    }
}

// Rows A u <= b of the convex hull of np <= 8 points (CCW, unit outward normals, padded to 8 rows with
// 0.u <= 1e30); returns the row count (0 when fewer than 3 points).  One thread.  Sorts px / py in place.
// The row count is not a function of the polygon alone: with collinear corners (parallel feet) the orientation test decides on
// rounding, and a corner kept on an edge gives that edge twice (wcqp.h, hull section).
__device__ __forceinline__ int hull_rows(double* px, double* py, int np, double* A, double* b) {
    for (int k = 0; k < 8; ++k) { A[2 * k] = 0.0; A[2 * k + 1] = 0.0; b[k] = 1e30; }
    if (np < 3) return 0;
    // insertion sort by (x, y), then Andrew's monotone chain (collinear points dropped, up to the rounding of the orientation test)
    for (int i = 1; i < np; ++i) {
        const double x = px[i], y = py[i];
        int j = i - 1;
        while (j >= 0 && (px[j] > x || (px[j] == x && py[j] > y))) { px[j + 1] = px[j]; py[j + 1] = py[j]; --j; }
        px[j + 1] = x; py[j + 1] = y;
    }
    // Coincident corners (two feet at one pose) are one corner: the sort left them adjacent, and both passes take the first of each run
    // only.  Taken twice, a repeated point's orientation test is dx * dy - dy * dx - fused, the rounding error of one product, positive
    // half the time - and the point stays as a vertex with an edge of length 0: a NaN row made from finite inputs.  Nothing changes for a
    // set without exactly equal points.
    double hx[16], hy[16];
    int k = 0, last = 0;                                            // last: the lower hull's last point, where the upper hull starts
    for (int i = 0; i < np; ++i) {                                  // lower hull
        if (i > 0 && px[i] == px[i - 1] && py[i] == py[i - 1]) continue;
        while (k >= 2 && (hx[k - 1] - hx[k - 2]) * (py[i] - hy[k - 2]) - (hy[k - 1] - hy[k - 2]) * (px[i] - hx[k - 2]) <= 0) --k;
        hx[k] = px[i]; hy[k] = py[i]; ++k;
        last = i;
    }
    const int lower = k + 1;
    for (int i = np - 2; i >= 0; --i) {                             // upper hull
        if (i >= last || (i > 0 && px[i] == px[i - 1] && py[i] == py[i - 1])) continue;
        while (k >= lower && (hx[k - 1] - hx[k - 2]) * (py[i] - hy[k - 2]) - (hy[k - 1] - hy[k - 2]) * (px[i] - hx[k - 2]) <= 0) --k;
        hx[k] = px[i]; hy[k] = py[i]; ++k;
    }
    // every corner at one point: no direction - two edges of length 0, whose rows are NaN (wcqp.h)
    if (k == 1) { hx[1] = hx[0]; hy[1] = hy[0]; hx[2] = hx[0]; hy[2] = hy[0]; k = 3; }
    // more vertices than the 8 rows hold: only when every corner lies on one line to rounding (feet of no width in tandem), where both
    // passes may keep every point - the set is the segment between the first and the last point of the sort
    if (k - 1 > 8) { hx[1] = px[np - 1]; hy[1] = py[np - 1]; hx[2] = hx[0]; hy[2] = hy[0]; k = 3; }
    const int nc = k - 1;                                           // last point == first point
    for (int e = 0; e < nc; ++e) {
        const double dx = hx[e + 1] - hx[e], dy = hy[e + 1] - hy[e];
        const double len = sqrt(dx * dx + dy * dy);
        const double ax = dy / len, ay = -dx / len;                 // outward normal of a CCW edge
        A[2 * e] = ax; A[2 * e + 1] = ay;
        b[e] = ax * hx[e] + ay * hy[e];
    }
    return nc;
}
#endif

}  // namespace wcqp_hull
