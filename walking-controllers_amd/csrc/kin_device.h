// Kinematic-tree model in the form the device code reads, and the forward-kinematics walk of the device code, stated once:
//  - the small 3-D helpers and the per-slot leaves (a frame in LDS, one pointer-jumping composition, an attached frame, the base pose
//    from the anchor sole, a frame from base to world): used by the stand-alone kinematics kernel (kin.hip, one joint per lane), by the
//    kinematics phase fused into the tick kernels (ik4_device.h, JSRC = 2) and by the sensor-feedback kernel (sensors.hip);
//  - the walk over 16 lanes per robot with lane j owning joints j and 16 + j (walk_*), built from those leaves and read from the model
//    table in LDS (kKinTab*): the fused phase at the desired joints and the sensor kernel at the measured ones are the SAME functions,
//    each with its own LDS map - frame stride, number of attached frames and the places of frames and prefix sums are parameters.
// Internal, not ABI.
#pragma once
#include "wcqp_internal.h"

namespace wcqp_kin {

constexpr int kMaxDof = WCQP_KIN_MAX_DOF;     // 32
constexpr int kMaxRounds = 5;                 // pointer jumping covers 2^5 = 32 >= kMaxDof levels

struct KinDev {
    int dof, n_rounds, dfs_contig;
    int up[kMaxRounds][kMaxDof];              // up[0] = parent, up[r + 1][j] = up[r][up[r][j]] (-1: above the root)
    int sub_end[kMaxDof];                     // last joint of j's subtree when the subtrees are index ranges (dfs_contig)
    unsigned desc_mask[kMaxDof];              // joints moved by joint j (itself included)
    unsigned path_mask[3];                    // joints on the path root -> frame f
    double R0[kMaxDof][9], p0[kMaxDof][3], axis[kMaxDof][3], mass[kMaxDof], com[kMaxDof][3];
    double root_mass, root_com[3], total_mass;
    int frame_joint[3];
    double frame_R[3][9], frame_p[3][3];
};

#if defined(__HIPCC__)
__device__ __forceinline__ void mat3_mul(const double* A, const double* B, double* C) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) C[3 * r + c] = A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c];
}
__device__ __forceinline__ void mat3_vec(const double* A, const double* v, double* o) {
#pragma unroll
    for (int r = 0; r < 3; ++r) o[r] = A[3 * r] * v[0] + A[3 * r + 1] * v[1] + A[3 * r + 2] * v[2];
}
__device__ __forceinline__ void cross3(const double* a, const double* b, double* o) {
    o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}
// (Ro, po) = (Ra, pa) o (Rb, pb)
__device__ __forceinline__ void frame_mul(const double* Ra, const double* pa, const double* Rb, const double* pb, double* Ro, double* po) {
    mat3_mul(Ra, Rb, Ro);
    double d[3];
    mat3_vec(Ra, pb, d);
#pragma unroll
    for (int k = 0; k < 3; ++k) po[k] = pa[k] + d[k];
}
// local frame of a revolute joint: R0 * Rot(axis, q)   (Rodrigues)
// sin and cos of a joint angle: Cody-Waite reduction by pi/2 in two FMA steps and the fdlibm kernels on |r| <= pi/4 (their
// published minimax coefficients; < 1 ulp each).  Joint angles are a few radians at most: the reduction's error is
// |k| x 2^-107, nothing the Payne-Hanek branch of ocml's sincos (154 VALU instructions and two branches per call) would add to.
__device__ __forceinline__ void joint_sincos(double x, double& sn, double& cs) {
    const double k = rint(x * 6.36619772367581382433e-01);
    double r = fma(-k, 1.57079632679489655800e+00, x);
    r = fma(-k, 6.12323399573676603587e-17, r);
    const double z = r * r;
    const double ps = fma(z, fma(z, fma(z, fma(z, 1.58969099521155010221e-10, -2.50507602534068634195e-08), 2.75573137070700676789e-06), -1.98412698298579493134e-04), 8.33333333332248946124e-03);
    const double s = fma(z * r, fma(z, ps, -1.66666666666666324348e-01), r);
    const double pc = z * fma(z, fma(z, fma(z, fma(z, fma(z, -1.13596475577881948265e-11, 2.08757232129817482790e-09), -2.75573143513906633035e-07), 2.48015872894767294178e-05), -1.38888888888741095749e-03), 4.16666666666666019037e-02);
    const double hz = 0.5 * z, w = 1.0 - hz;
    const double c = w + (((1.0 - w) - hz) + z * pc);
    const int n = (int)k & 3;
    const double a = (n & 1) ? c : s, b = (n & 1) ? s : c;
    sn = (n & 2) ? -a : a;
    cs = ((n + 1) & 2) ? -b : b;
}
__device__ __forceinline__ void joint_rotation(const double* R0, const double* ax, double q, double* Ra) {
    double sn, cs;
    joint_sincos(q, sn, cs);
    const double v = 1.0 - cs;
    const double Rq[9] = {cs + v * ax[0] * ax[0],         v * ax[0] * ax[1] - sn * ax[2], v * ax[0] * ax[2] + sn * ax[1],
                          v * ax[1] * ax[0] + sn * ax[2], cs + v * ax[1] * ax[1],         v * ax[1] * ax[2] - sn * ax[0],
                          v * ax[2] * ax[0] - sn * ax[1], v * ax[2] * ax[1] + sn * ax[0], cs + v * ax[2] * ax[2]};
    mat3_mul(R0, Rq, Ra);
}
// lane i of a DPP row receives lane i - N (0 below the row start)
template <int N>
__device__ __forceinline__ double row_shr0(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x110 + N, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x110 + N, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
// inclusive prefix sum over each 16-lane DPP row
__device__ __forceinline__ double row_scan(double v) {
    v += row_shr0<1>(v);
    v += row_shr0<2>(v);
    v += row_shr0<4>(v);
    v += row_shr0<8>(v);
    return v;
}

__device__ __forceinline__ void st2(double* p, double a, double b) { *reinterpret_cast<double2*>(p) = make_double2(a, b); }
__device__ __forceinline__ double2 ld2(const double* p) { return *reinterpret_cast<const double2*>(p); }

// ---- per-slot leaves: a frame in LDS is 12 doubles, R (9, row-major) | p (3), at a 16-byte boundary
__device__ __forceinline__ void frame_store(double* T, const double* R, const double* p) {
#pragma unroll
    for (int k = 0; k < 8; k += 2) st2(T + k, R[k], R[k + 1]);
    st2(T + 8, R[8], p[0]); st2(T + 10, p[1], p[2]);
}
__device__ __forceinline__ void frame_load(const double* T, double* R, double* p) {
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = T[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = T[9 + k];
}
// one pointer-jumping composition: (R, p) <- T o (R, p), T the frame of the ancestor the round jumps to
__device__ __forceinline__ void frame_jump(const double* T, double* R, double* p) {
    double Rp[9], pp[3], Rn[9], pn[3];
    frame_load(T, Rp, pp);
    frame_mul(Rp, pp, R, p, Rn, pn);
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = Rn[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = pn[k];
}
// an attached frame (fR, fp: its constant pose in its joint's frame) from its joint's frame T
__device__ __forceinline__ void attached_frame(const double* T, const double* fR, const double* fp, double* Rf, double* pf) {
    double Rj[9], pj[3], Rc[9], pc[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) { Rj[k] = T[k]; Rc[k] = fR[k]; }
#pragma unroll
    for (int k = 0; k < 3; ++k) { pj[k] = T[9 + k]; pc[k] = fp[k]; }
    frame_mul(Rj, pj, Rc, pc, Rf, pf);
}
// base pose from the anchor sole: world_T_base = world_T_sole,desired * (base_T_sole)^-1.  sdp, sdR: the sole's desired pose, as the
// caller has read it; Fs: the sole's frame in base coordinates
__device__ __forceinline__ void base_from_anchor(const double* sdp, const double* sdR, const double* Fs, double* Rb, double* pb) {
    double Rs[9], ps[3], d3[3];
    frame_load(Fs, Rs, ps);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) Rb[3 * r + c] = sdR[3 * r] * Rs[3 * c] + sdR[3 * r + 1] * Rs[3 * c + 1] + sdR[3 * r + 2] * Rs[3 * c + 2];
    mat3_vec(Rb, ps, d3);
#pragma unroll
    for (int k = 0; k < 3; ++k) pb[k] = sdp[k] - d3[k];
}
// a frame given in base coordinates, in world coordinates at F
__device__ __forceinline__ void frame_to_world(const double* Rb, const double* pb, const double* R, const double* p, double* F) {
    double Rg[9], pg[3];
    frame_mul(Rb, pb, R, p, Rg, pg);
#pragma unroll
    for (int k = 0; k < 9; ++k) F[k] = Rg[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) F[9 + k] = pg[k];
}
#endif

// ---- the model as one table of doubles, as the 16-lane walk reads it from LDS (built by wcqp::kin_fused_tables, kin.hip):
// [kWalkDof][22] = R0 9 | p0 3 | axis 3 | com 3 | mass | four ints: the joint's pointer-jumping links of rounds 0..2, the last joint of its
// subtree | pad; then [3][12] attached frames R 9 | p 3; then root_com 3, root_mass, three ints: the joints the frames are attached to.
constexpr int kWalkDof = 23;                  // joints of the robot the walk is laid out for: lane j owns joints j and 16 + j
constexpr int kKinTabJoint = 22, kKinTabInts = 19, kKinTabFrames = kKinTabJoint * kWalkDof, kKinTabRoot = kKinTabFrames + 36, kKinTabSize = kKinTabRoot + 6;

#if defined(__HIPCC__)
// ---- the walk: 16 lanes per robot (one DPP row), lane j owns joint cs[0] = j and, when var1, joint cs[1] = 16 + j (else cs[1] = 0, a
// slot that computes along and stores nothing).  FS: stride of the joint frames at TW; NF: attached frames, on lanes 0 .. NF - 1.
// One function per step; the steps are fenced (wcqp::wave_lds_fence) where the next one reads what other lanes stored.

// the lane's pointer-jumping links and subtree ends, and (lanes 0 .. NF - 1) the joint its attached frame sits on
template <int NF>
__device__ __forceinline__ int walk_links(const double* kmodel, int j, const int (&cs)[2], int (&kup)[2][3], int (&ksub)[2]) {
#pragma unroll
    for (int s_ = 0; s_ < 2; ++s_) {
        const int* ip = reinterpret_cast<const int*>(kmodel + cs[s_] * kKinTabJoint + kKinTabInts);
        kup[s_][0] = ip[0]; kup[s_][1] = ip[1]; kup[s_][2] = ip[2]; ksub[s_] = ip[3];
    }
    return reinterpret_cast<const int*>(kmodel + kKinTabRoot + 4)[j < NF ? j : 0];
}
// local joint frames (R0 Rot(axis, q), p0), relative to the parent's
__device__ __forceinline__ void walk_local_frames(const double* kmodel, const int (&cs)[2], double q0, double q1, double (&Ra)[2][9], double (&pa)[2][3]) {
#pragma unroll
    for (int s_ = 0; s_ < 2; ++s_) {
        const double* mt = kmodel + cs[s_] * kKinTabJoint;
        double R0[9], axl[3];
#pragma unroll
        for (int k = 0; k < 9; ++k) R0[k] = mt[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) { pa[s_][k] = mt[9 + k]; axl[k] = mt[12 + k]; }
        joint_rotation(R0, axl, s_ == 0 ? q0 : q1, Ra[s_]);
    }
}
// the tree in base coordinates by pointer jumping: after round r a frame is relative to its 2^(r+1)-th ancestor; the frames end at TW
template <int FS>
__device__ __forceinline__ void walk_tree_to_base(double* TW, const int (&cs)[2], bool var1, const int (&kup)[2][3], int n_rounds, double (&Ra)[2][9], double (&pa)[2][3]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        if (r >= n_rounds) break;
#pragma unroll
        for (int s_ = 0; s_ < 2; ++s_)
            if (s_ == 0 || var1) frame_store(TW + cs[s_] * FS, Ra[s_], pa[s_]);
        wcqp::wave_lds_fence();
#pragma unroll
        for (int s_ = 0; s_ < 2; ++s_) {
            const int u = kup[s_][r];
            if (u >= 0 && (s_ == 0 || var1)) frame_jump(TW + u * FS, Ra[s_], pa[s_]);
        }
        wcqp::wave_lds_fence();
    }
#pragma unroll
    for (int s_ = 0; s_ < 2; ++s_)
        if (s_ == 0 || var1) frame_store(TW + cs[s_] * FS, Ra[s_], pa[s_]);
    wcqp::wave_lds_fence();
}
// attached frames in base coordinates: lane j < NF computes frame j (the others frame 0, unused) and stores it at FRB [NF][12]
template <int FS, int NF>
__device__ __forceinline__ void walk_attached_frames(const double* kmodel, const double* TW, double* FRB, int j, int kfj, double* Rf, double* pf) {
    const double* ft = kmodel + kKinTabFrames + (j < NF ? j : 0) * 12;
    attached_frame(TW + kfj * FS, ft, ft + 9, Rf, pf);
    if (j < NF) {
        double* F = FRB + j * 12;
#pragma unroll
        for (int k = 0; k < 9; ++k) F[k] = Rf[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) F[9 + k] = pf[k];
    }
    wcqp::wave_lds_fence();
}
// own joints in world coordinates (back from TW: not held in registers across the steps in between), their axes, link first moments {m c, m}
template <int FS>
__device__ __forceinline__ void walk_joints_to_world(const double* kmodel, const double* TW, const int (&cs)[2], bool var1, const double* Rb, const double* pb,
                                                     double (&pw)[2][3], double (&aw)[2][3], double (&e4)[2][4]) {
#pragma unroll
    for (int s_ = 0; s_ < 2; ++s_) {
        const double* mt = kmodel + cs[s_] * kKinTabJoint;
        double Rw[9], cl[3], Rl[9], pl[3];
        frame_load(TW + cs[s_] * FS, Rl, pl);
        frame_mul(Rb, pb, Rl, pl, Rw, pw[s_]);
        const double axl[3] = {mt[12], mt[13], mt[14]};
        mat3_vec(Rw, axl, aw[s_]);
        const double cj[3] = {mt[15], mt[16], mt[17]};
        const double mj = (s_ == 0 || var1) ? mt[18] : 0.0;
        mat3_vec(Rw, cj, cl);
#pragma unroll
        for (int k = 0; k < 3; ++k) e4[s_][k] = mj * (pw[s_][k] + cl[k]);
        e4[s_][3] = mj;
    }
}
// subtree first moments: the joint numbering is depth-first, a subtree is an index range; inclusive prefix sums over joints 0..15
// (slot 0, a DPP row scan) and 16.. (slot 1, offset by the row's total) at PS [32][4]
__device__ __forceinline__ void walk_prefix_sums(double* PS, int j, const double (&e4)[2][4]) {
    double p0s[4], p1s[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { p0s[k] = row_scan(e4[0][k]); p1s[k] = row_scan(e4[1][k]); }
    st2(PS + j * 4, p0s[0], p0s[1]); st2(PS + j * 4 + 2, p0s[2], p0s[3]);
    wcqp::wave_lds_fence();
    const double2 t01 = ld2(PS + 15 * 4), t23 = ld2(PS + 15 * 4 + 2);
    st2(PS + (16 + j) * 4, p1s[0] + t01.x, p1s[1] + t01.y); st2(PS + (16 + j) * 4 + 2, p1s[2] + t23.x, p1s[3] + t23.y);
    wcqp::wave_lds_fence();
}
// the robot's first moment and mass with the root link's (tot), its CoM (ctot) and 1 / M
__device__ __forceinline__ void walk_com_total(const double* kmodel, const double* PS, const double* Rb, const double* pb, double (&tot)[4], double (&ctot)[3], double& iM) {
    const double* rt = kmodel + kKinTabRoot;
    const double rootc[3] = {rt[0], rt[1], rt[2]};
    const double root_mass = rt[3];
    double cr[3];
    mat3_vec(Rb, rootc, cr);
    const double* Pt = PS + (kWalkDof - 1) * 4;
#pragma unroll
    for (int k = 0; k < 3; ++k) tot[k] = Pt[k] + root_mass * (pb[k] + cr[k]);
    tot[3] = Pt[3] + root_mass;
    iM = 1.0 / tot[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) ctot[k] = tot[k] * iM;
}
// the CoM column of joint c (subtree c .. sub_end, joint position pw, axis aw): a_c x (c_sub - p_c) m_sub / M
__device__ __forceinline__ void walk_com_column(const double* PS, int c, int sub_end, const double* pw, const double* aw, double iM, double* lin) {
    const double* Pe = PS + sub_end * 4;
    const double* Pb = PS + (c > 0 ? c - 1 : 0) * 4;
    const double z = c > 0 ? 1.0 : 0.0;
    const double ms = Pe[3] - z * Pb[3];
    const double d3[3] = {(Pe[0] - z * Pb[0] - ms * pw[0]) * iM, (Pe[1] - z * Pb[1] - ms * pw[1]) * iM, (Pe[2] - z * Pb[2] - ms * pw[2]) * iM};
    cross3(aw, d3, lin);
}
#endif

}  // namespace wcqp_kin
