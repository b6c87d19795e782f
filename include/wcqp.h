/*
 * wcqp.h — C ABI of the MI355X-native batched QP solve path that replaces the
 * osqp-eigen / qpOASES calls behind the reference's WalkingController
 * (DCM-MPC) and WalkingQPIK (Jacobian QP-IK) solver interfaces.
 *
 * Citations are relative to /root/reference/modules/Walking_module ("WM/").
 *
 * The reference has no FFI: its boundary is two C++ class surfaces
 * (WM/include/WalkingDCMModelPredictiveController.hpp:190-250 with
 * WM/include/MPCSolver.hpp:57-138, and WM/include/WalkingQPInverseKinematics.hpp:81-208).
 * Every entry point below names the reference call(s) it stands in for.  Batch = 1
 * reproduces the per-robot call; batch = B solves B independent robot instances.
 *
 * Conventions
 *   - plain C, no exceptions cross the ABI; every function returns WCQP_OK (0) or
 *     a negative WCQP_E_* code; per-instance results carry a WCQP_STATUS_* code
 *     (the batch analogue of the reference's `bool` returns).
 *   - all arithmetic is IEEE fp64 like the reference.
 *   - `*_device` entry points take DEVICE pointers and a hipStream_t (as void*); they
 *     enqueue work and return without synchronising (graph-capturable: no
 *     allocation, no sync inside).  `*_host` entry points take HOST pointers,
 *     stage through the handle's own device buffers and synchronise.
 *   - the handle owns every buffer it allocates; the caller owns inputs/outputs.
 *     A solver handle (wcqp_mpc_t, wcqp_ik_t, wcqp_kin_t) and wcqp_qp_enqueue_steps retain no caller pointer past a
 *     call.  Two objects DO, by design: a wcqp_qp_plan_t keeps the device pointers of every record it was created
 *     from, and both solver handles, until wcqp_qp_plan_destroy (the caller keeps those arrays and handles alive and
 *     their addresses unchanged for as long as the plan may be enqueued); a wcqp_tick_t owns its whole robot state on
 *     the device and copies HOST inputs at the call that receives them (wcqp_tick_upload,
 *     wcqp_tick_splice_reference: the host array may be released when the call returns).  On the HOST side a handle is single-caller
 *     (like the reference's solvers, which are only touched under WalkingModule's m_mutex,
 *     WM/src/WalkingModule.cpp:429): one thread at a time calls into it.  On the DEVICE
 *     side the work a `*_device` call (or wcqp_qp_enqueue_steps) enqueues only READS the
 *     handle's device state (constants uploaded at create / wcqp_ik_set_posture), so solves
 *     of one wcqp_mpc_t / wcqp_ik_t pair enqueued on several streams may run concurrently -
 *     the caller keeps their input / output arrays apart.  (wcqp_ik_set_posture and the
 *     `*_host` entry points synchronise the device first; a wcqp_tick_t owns its state and
 *     takes one stream at a time.)
 *
 * Non-finite inputs
 *   A NaN or an Inf in one instance's inputs never aborts the batch, never comes back WCQP_STATUS_SOLVED and never reaches a documented
 *   output; what the instance reports does not depend on the instances next to it, and they do not notice it (their results are bit for
 *   bit those of a batch in which the value is finite).  Each entry point below says what it returns for such an instance.  (Finite inputs
 *   so large that the arithmetic overflows are treated the same way.)
 *
 * Size limits (32-bit addressing)
 *   The solve kernels reach row i of a per-instance array as base + a 32-bit BYTE offset, so every such array must end within 2^32 bytes
 *   of its start: count x row_bytes <= 2^32, checked by every entry point from its arguments alone - before it looks for a device,
 *   allocates or launches, and without reading the arrays - and answered with WCQP_E_UNSUPPORTED.  The rows, per entry point (the widest
 *   one decides):
 *     wcqp_mpc_solve_device / _host    ref: ref_len x 16 B (batch <= 2^32 / (16 ref_len) = 2^28 / ref_len); hull_A: 128 B; the rest narrower.
 *                                      (The stand-alone kernel itself forms 64-bit addresses; the limit is kept so that a batch one route
 *                                      takes is a batch every route takes.)
 *     wcqp_ik_solve_device / _host     J_left, J_right: 6 x 29 x 8 = 1392 B (batch <= 3085465); J_neck, J_com, state: 696 B; q, dq: 184 B
 *     wcqp_qp_enqueue_steps            both of the above, per record (the code of the first call that refuses)
 *     wcqp_qp_plan_create              both of the above for every record that has the part
 *     wcqp_qp_step_from_slabs          both of the above for the layout's batch and ref_len
 *     wcqp_tick_create                 ref_traj, dcm_vel_traj: (max_ticks + horizon + 1) x 16 B; the two MPC -> IK hand-off records:
 *                                      2 x batch rows of 112 B; the IK's arrays as above (1392 B).  From the parameters alone, before the
 *                                      device is looked for.  The planned-trajectory records use 64-bit offsets and set no limit.
 *     wcqp_kin_jacobians_*, wcqp_hull_from_feet_*   64-bit addresses throughout: no limit beyond int32 batch.
 *     wcqp_unicycle_plan_device / _host   target: max_steps x 24 B; the soles: 96 B.  (The kernel forms 64-bit addresses; the limit is
 *                                      kept for the reason given for the MPC.)  wcqp_unicycle_plan_timed_device / _host: the same.
 */
#ifndef WCQP_H
#define WCQP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WCQP_VERSION 400

/* return codes */
#define WCQP_OK              0
#define WCQP_E_INVALID      (-1)   /* bad argument / NULL pointer                      */
#define WCQP_E_UNSUPPORTED  (-2)   /* size outside what the kernels are built for      */
#define WCQP_E_NUMERIC      (-3)   /* host-side constant precomputation failed         */
#define WCQP_E_HIP          (-4)   /* HIP runtime error (no device, launch failure...) */
#define WCQP_E_NOMEM        (-5)

/* per-instance status */
#define WCQP_STATUS_SOLVED        0
#define WCQP_STATUS_MAX_ITER      1   /* active-set iteration budget exhausted            */
#define WCQP_STATUS_INFEASIBLE    2   /* constraints admit no point                       */
#define WCQP_STATUS_OUTSIDE_HULL  3   /* MPC: margin(u0) < -convex_hull_tolerance
                                         (WM/src/WalkingDCMModelPredictiveController.cpp:513-517) */
#define WCQP_STATUS_NUMERIC       4   /* non-positive pivot (KKT not regular), or a NaN / Inf
                                         among the instance's inputs (see "Non-finite inputs") */
#define WCQP_STATUS_STRUCTURE     5   /* IK: handle created with WCQP_IK_JAC_MIXED, but this instance's Jacobians do
                                         not have MIXED-representation base blocks          */

#define WCQP_HULL_ROWS   8            /* hull rows are padded to 8 per instance           */
#define WCQP_MAX_DOF     32
#define WCQP_IK_STATE_LEN 87          /* doubles in the packed per-instance pose block    */

const char* wcqp_strerror(int code);
int wcqp_version(void);
/* number of visible HIP devices (0 on a CPU-only host; never initialises a context) */
int wcqp_device_count(void);
/* HIP streams for hosts that reach this library through an FFI and have no HIP binding of their own (ctypes, cgo, JNI):
 * what the `stream` argument of the `*_device` entry points takes.  Non-blocking streams of the current device;
 * wcqp_stream_synchronize(NULL) waits for the whole device.  (The reference has no counterpart: its solvers are synchronous.) */
int wcqp_stream_create(void** out);
int wcqp_stream_destroy(void* stream);
int wcqp_stream_synchronize(void* stream);

/* =====================================================================================
 * DCM-MPC  — replaces  WalkingController::{initialize, setConvexHullConstraint,
 *            setFeedback, setReferenceSignal, solve, getControllerOutput}
 *            (WM/src/WalkingDCMModelPredictiveController.cpp:311-535) and the
 *            MPCSolver / OsqpEigen::Solver object they drive (WM/src/MPCSolver.cpp:16-322).
 * ===================================================================================== */
typedef struct wcqp_mpc_params {
    int32_t horizon;              /* N = round(controllerHorizon / sampling_time), cpp:182-187 */
    double  sampling_time;        /* cpp:182                                                   */
    double  com_height;           /* cpp:224-229                                               */
    double  gravity;              /* cpp:230 (default 9.81)                                    */
    double  Q[4];                 /* state weight, row-major 2x2 (stateWeightTriplets)         */
    double  R[4];                 /* input weight, row-major 2x2 (inputWeightTriplets)         */
    double  convex_hull_tolerance;/* cpp:306                                                   */
    double  feas_tol;             /* feasibility slack of a candidate vertex; 0 -> 1e-10       */
} wcqp_mpc_params;

typedef struct wcqp_mpc_s* wcqp_mpc_t;

/* WalkingController::initialize/initializeMatrices (cpp:170-243, 311-362): builds P,
 * A_eq and the gradient sub-matrix, then condenses the batch-constant equality KKT
 * once on the host (u0 = sum_i Gr_i r_i + Gx x0 + Gu u_prev - Sigma0 A_h' mu). */
int wcqp_mpc_create(const wcqp_mpc_params* params, wcqp_mpc_t* out);
int wcqp_mpc_destroy(wcqp_mpc_t h);

/* Host-side introspection of the condensed constants (tests):
 * Gr[(N+1)*4], Gx[4], Gu[4], Sigma0[4], all row-major 2x2 blocks. */
int wcqp_mpc_get_condensed(wcqp_mpc_t h, double* Gr, double* Gx, double* Gu, double* Sigma0);
/* Dense copies of the reference's constant blocks for parity checks against
 * initializeMatrices: P[n*n], A_eq[n_x*n], grad_sub[n_u*2]; n = 4N+2. */
int wcqp_mpc_get_matrices(wcqp_mpc_t h, double* P, double* A_eq, double* grad_sub);

/*
 * One MPC tick for `batch` instances — the contents of the reference's "MPC" profiler
 * bracket (WM/src/WalkingModule.cpp:604-636):
 *   hull_A[B][8][2], hull_b[B][8], hull_nc[B]  <- setConvexHullConstraint / MPCSolver::setConstraintsMatrix
 *                                                 + the hull part of setBounds (MPCSolver.cpp:76-123,149-153);
 *                                                 rows >= hull_nc[i] are ignored
 *   x0[B][2]                                   <- setFeedback / setBounds rows 0..1 (MPCSolver.cpp:143-146)
 *   ref[B][ref_len][2], ref_len >= 1           <- setReferenceSignal / setGradient (MPCSolver.cpp:183-239);
 *                                                 stages >= ref_len repeat the last one (:200-214)
 *   u_prev[B][2]                               <- m_output fed back as previousControllerOutput (:244-245)
 * outputs
 *   u0[B][2]      first input = desired ZMP    -> getControllerOutput (cpp:510-511, 523-535)
 *   status[B]     WCQP_STATUS_*                -> the bool of solve() (cpp:491-521)
 *   active[B]     bit e set <=> hull row e is in the optimal active set       (may be NULL)
 *   margin[B]     signed distance of u0 to the hull boundary, + inside         (may be NULL)
 * Non-finite inputs: a NaN or +-Inf in x0, in u_prev, in a stage of ref the horizon reads (stages 0 .. min(N, ref_len - 1)) or in a hull
 * row below hull_nc gives status = WCQP_STATUS_NUMERIC, u0 = (0, 0), active = 0, margin = -inf.  Hull rows at or above hull_nc and ref
 * stages beyond the horizon are never looked at: a non-finite value there changes nothing.  The same holds for the MPC part of
 * wcqp_qp_enqueue_steps and of a plan.  (The tick keeps such values out of its state: wcqp_tick_upload and wcqp_tick_splice_reference
 * refuse them, wcqp_tick_set_feedback_* rejects the robot.)
 */
int wcqp_mpc_solve_device(wcqp_mpc_t h, int32_t batch,
                          const double* x0, const double* ref, int32_t ref_len,
                          const double* u_prev,
                          const double* hull_A, const double* hull_b, const int32_t* hull_nc,
                          double* u0, int32_t* status, uint32_t* active, double* margin,
                          void* stream);
int wcqp_mpc_solve_host(wcqp_mpc_t h, int32_t batch,
                        const double* x0, const double* ref, int32_t ref_len,
                        const double* u_prev,
                        const double* hull_A, const double* hull_b, const int32_t* hull_nc,
                        double* u0, int32_t* status, uint32_t* active, double* margin);

/* =====================================================================================
 * Support polygon rows from foot poses — the batch analogue of
 * WalkingController::setConvexHullConstraint -> buildConvexHull
 * (WM/src/WalkingDCMModelPredictiveController.cpp:364-489): feet rectangles
 * (foot_size, cpp:295-303) transformed by the foot poses, projected on the XY plane, 2-D
 * convex hull.  iDynTree's row order / normalisation is upstream and unpinned, so the
 * convention is this library's own: CCW hull, unit outward normals,
 * rows a.u <= b, padded to 8 rows with 0.u <= 1e30.
 *   foot_rect[8]            corners (x, y) x 4 of the foot rectangle in the foot frame
 *   left_T / right_T[B][12] foot-to-world transforms: position (3) + row-major rotation (9)
 *   contact[B]              bit 0 = left foot in contact, bit 1 = right foot in contact
 * outputs hull_A[B][8][2], hull_b[B][8], hull_nc[B] (0 when no foot is in contact — the
 * reference refuses that case, cpp:406-410; the MPC kernel then reports the unconstrained u0).
 * The rows are the polygon; their COUNT is not a function of the polygon alone.  When corners are
 * collinear (parallel feet side by side or in tandem: four corners on one line) the builder's
 * orientation test decides on rounding errors, a corner within an ulp of an edge may be kept as a
 * vertex, and that edge is then delivered twice: consecutive rows that agree to ~1e-15.  Compare
 * rows as sets, not index by index; the MPC takes such rows as they are.
 * Coincident corners are merged: two feet at one pose give that foot's polygon.
 * A set with no area: corners on one segment (a foot rolled by pi/2 projects on a line) give
 * hull_nc = 2, the finite rows +-n.u <= +-n.a of the segment's line, which do not bound it along
 * the segment (more than two distinct corners on a line: 2 to 8 such rows, by the rounding above,
 * never more); corners that all coincide (a zero foot_rect) have no direction and give hull_nc = 2
 * with both rows NaN, which the MPC answers with WCQP_STATUS_NUMERIC.
 * ===================================================================================== */
int wcqp_hull_from_feet_device(int32_t batch, const double* foot_rect,
                               const double* left_T, const double* right_T, const uint8_t* contact,
                               double* hull_A, double* hull_b, int32_t* hull_nc, void* stream);
int wcqp_hull_from_feet_host(int32_t batch, const double* foot_rect,
                             const double* left_T, const double* right_T, const uint8_t* contact,
                             double* hull_A, double* hull_b, int32_t* hull_nc);

/* =====================================================================================
 * QP-IK — replaces WalkingQPIK_osqp::solve / WalkingQPIK_qpOASES::solve and the
 *         OsqpEigen::Solver / qpOASES::SQProblem objects behind them
 *         (WM/src/WalkingQPInverseKinematics_osqp.cpp:340-428,
 *          WM/src/WalkingQPInverseKinematics_qpOASES.cpp:284-362).
 * ===================================================================================== */
#define WCQP_IK_FORM_QPOASES 0   /* bounds enforced, kappa = 1, feet always corrected        */
#define WCQP_IK_ALG_DEFAULT   0
#define WCQP_IK_ALG_SWEEP     1        /* round-1 A/B baseline; diagnostic builds only (-DWCQP_DIAG_KERNELS), else WCQP_E_UNSUPPORTED */
#define WCQP_IK_ALG_NULLSPACE 2        /* null-space kernel, reduced Hessian on the fp64 VALU                 */
#define WCQP_IK_ALG_NULLSPACE_MFMA 3   /* same, reduced-Hessian Gram product as one v_mfma_f64_16x16x4 tile per
                                          instance: ~5 % faster than 2 in interleaved A/B runs;
                                          needs use_com_as_constraint (one 16x16 tile), else runs as 2        */
#define WCQP_IK_ALG_NULLSPACE_16L 4    /* null-space kernel on 16 lanes per instance, 4 instances per wave
                                          (csrc/ik3.hip): 1.6x the throughput of 3 on a full chip; the fall-back of
                                          algorithm 5 for Jacobians without the MIXED pattern and the kernel of
                                          WCQP_IK_JAC_GENERAL; needs use_com_as_constraint, else runs as 2          */
#define WCQP_IK_ALG_BASE_ELIM 5        /* base unknowns eliminated in closed form through the left-foot rows, 23-variable
                                          QP in range space (csrc/ik4.hip): what the default resolves to when the CoM is a
                                          constraint, every joint weight is > 0 and the neck weight is positive definite;
                                          otherwise runs as 4.  See `jacobian_structure`.                        */
/* jacobian_structure: what the caller promises about the base blocks (columns 0..5) of the four Jacobians.
 * The reference always passes iDynTree free-floating Jacobians in MIXED representation
 * (WM/src/WalkingForwardKinematics.cpp:33, 436-454): J_left/J_right = [I B; 0 I | .], J_com = [I B | .],
 * J_neck (angular rows) = [0 I | .].  Algorithm 5 relies on that pattern and CHECKS it per instance: for each of the six base
 * columns the absolute deviations of its identity / zero entries from 1.0 / 0.0, summed over the four Jacobians, must not exceed
 * WCQP_IK_MIXED_TOL (a producer that forms the blocks through rotation products hands over 0.9999999999999999; such entries are
 * then TREATED as exact, which moves the solution by at most WCQP_IK_MIXED_TOL x |base velocity|).  Beyond the tolerance - or with
 * a NaN in a base block - the instance does not have the pattern. */
#define WCQP_IK_MIXED_TOL 1e-12
#define WCQP_IK_JAC_AUTO    0    /* default: instances without the pattern are re-solved by the general kernel (one
                                    more, nearly empty, launch per call)                                          */
#define WCQP_IK_JAC_MIXED   1    /* instances without the pattern come back WCQP_STATUS_STRUCTURE (dq = 0); one launch */
#define WCQP_IK_JAC_GENERAL 2    /* arbitrary Jacobians: the general kernel (algorithm 4) only                     */
#define WCQP_IK_FORM_OSQP    1   /* joint-limit rows are zero rows (never bind), extra
                                    k_attFoot on the neck gradient term, zero-twist rule
                                                               */

typedef struct wcqp_ik_params {
    int32_t dof;                         /* actuated DoF (23 on iCub); n = dof + 6            */
    int32_t use_com_as_constraint;       /* qpInverseKinematics.ini:2                          */
    int32_t form;                        /* WCQP_IK_FORM_*                                     */
    int32_t max_iter;                    /* active-set changes budget; 0 -> 100 (nWSR, qp.cpp:312) */
    double  com_weight[9];               /* row-major 3x3, used when !use_com_as_constraint    */
    double  neck_weight[9];              /* row-major 3x3                                      */
    double  joint_reg_weights[WCQP_MAX_DOF];
    double  joint_reg_gains[WCQP_MAX_DOF];
    double  joint_reg_rad[WCQP_MAX_DOF]; /* jointRegularization already in rad (osqp.cpp:101-102) */
    double  v_min[WCQP_MAX_DOF];         /* joint velocity limits (WalkingModule.cpp:237-243)  */
    double  v_max[WCQP_MAX_DOF];         /* any v_min[j] <= v_max[j] (else WCQP_E_INVALID): v_min need not be -v_max, an interval may
                                            exclude zero, v_min[j] == v_max[j] pins joint j (dq[j] is that value exactly), +-1e30 leaves
                                            a side open; an empty feasible set is WCQP_STATUS_INFEASIBLE per instance                 */
    double  k_pos_com, k_pos_foot, k_att_foot, k_neck;
    double  rho;                         /* weight of the A'A term that regularises H; 0 -> 1  */
    double  tol;                         /* bound-violation tolerance; 0 -> 1e-12              */
    int32_t algorithm;                   /* WCQP_IK_ALG_*: 0 -> default (5; 2 for CoM-as-cost), 1 = sweep on H + rho A'A (csrc/ik.hip),
                                            2 / 3 = null-space (csrc/ik2.hip) without / with MFMA, 4 = null-space on
                                            16 lanes per instance (csrc/ik3.hip), 5 = base elimination + range space
                                            (csrc/ik4.hip); same optimum */
    int32_t jacobian_structure;          /* WCQP_IK_JAC_* (algorithms 0 / 5 only)               */
} wcqp_ik_params;

typedef struct wcqp_ik_s* wcqp_ik_t;

/* WalkingQPIK_*::initialize + WalkingQPIK::initializeMatrices
 * (osqp.cpp:54-133, qp.cpp:53-133, WalkingQPInverseKinematics.cpp:25-116). */
int wcqp_ik_create(const wcqp_ik_params* params, wcqp_ik_t* out);
int wcqp_ik_destroy(wcqp_ik_t h);
/* WalkingQPIK::setDesiredJointPosition (WalkingQPInverseKinematics.cpp:246-256): replaces the regularisation posture
 * (rad, `dof` entries) that enters the gradient of every later solve (osqp.cpp:185, qp.cpp:166).  Synchronises the
 * device; not graph-capturable. */
int wcqp_ik_set_posture(wcqp_ik_t h, const double* joint_reg_rad);

/*
 * One IK tick for `batch` instances — the solver part of the reference's "IK" bracket
 * (WM/src/WalkingModule.cpp:367-425, 721-740).  n = dof + 6, all matrices row-major:
 *   J_left[B][6][n], J_right[B][6][n]   <- setLeftFootJacobian / setRightFootJacobian
 *   J_neck[B][3][n]                     <- rows 3..5 of the 6 x n neck Jacobian, as kept by
 *                                          setNeckJacobian (WalkingQPInverseKinematics.cpp:214-215)
 *   J_com[B][3][n]                      <- setCoMJacobian
 *   q[B][dof]                           <- setRobotState joint positions
 *   state[B][87]                        <- setRobotState / setDesired* poses, packed:
 *        p_left 0..2 | R_left 3..11 | p_right 12..14 | R_right 15..23
 *        pd_left 24..26 | Rd_left 27..35 | pd_right 36..38 | Rd_right 39..47
 *        R_neck 48..56 | Rd_neck 57..65 (already multiplied by additional_rotation, cpp:143-146)
 *        com 66..68 | com_des 69..71 | com_vel_des 72..74 | twist_left 75..80 | twist_right 81..86
 * outputs
 *   dq[B][dof]                          -> getSolution (osqp.cpp:410-428, qp.cpp:341-362)
 *   status[B]                           -> the bool of solve()
 *   active_lower[B], active_upper[B]    bit i set <=> joint i sits on its lower/upper velocity
 *                                       limit with a positive multiplier          (may be NULL)
 *   foot_err[B][12]                     -> getLeftFootError | getRightFootError
 *                                          (osqp.cpp:430-454, qp.cpp:364-401)     (may be NULL)
 *   iters[B]                            active-set changes performed              (may be NULL)
 * Non-finite inputs: a NaN or +-Inf in a joint column (6 .. n-1) of any of the four Jacobians, in q or in an entry of `state` the form
 * reads gives status = WCQP_STATUS_NUMERIC, dq = 0, active_lower = active_upper = 0 and iters <= max_iter - whichever kernel the handle
 * runs, and through wcqp_qp_enqueue_steps and the plans as well.  Both forms read every entry of `state`, with one exception: under
 * WCQP_IK_FORM_OSQP a foot whose desired twist has twist[0] == twist[1] == 0 gets no pose correction (the zero-twist rule, osqp.cpp:286-306),
 * so that foot's actual and desired pose entries (left 0..11, 24..35; right 12..23, 36..47) are not read and a non-finite value there
 * changes nothing.  One in a base block (columns 0 .. 5) keeps the meaning given under
 * jacobian_structure: WCQP_STATUS_STRUCTURE with WCQP_IK_JAC_MIXED; with WCQP_IK_JAC_AUTO the general kernel re-solves the instance, which
 * then ends WCQP_STATUS_NUMERIC with dq = 0.  foot_err of such an instance is unspecified (it may hold NaN).
 */
int wcqp_ik_solve_device(wcqp_ik_t h, int32_t batch,
                         const double* J_left, const double* J_right,
                         const double* J_neck, const double* J_com,
                         const double* q, const double* state,
                         double* dq, int32_t* status,
                         uint32_t* active_lower, uint32_t* active_upper,
                         double* foot_err, int32_t* iters,
                         void* stream);
int wcqp_ik_solve_host(wcqp_ik_t h, int32_t batch,
                       const double* J_left, const double* J_right,
                       const double* J_neck, const double* J_com,
                       const double* q, const double* state,
                       double* dq, int32_t* status,
                       uint32_t* active_lower, uint32_t* active_upper,
                       double* foot_err, int32_t* iters);

/* =====================================================================================
 * Several solve calls in one host call.  A robot-tick batch at the BASELINE size is two kernels of
 * about 5 and 15 us, which is what their two launches cost a host that reaches this library through
 * an FFI (ctypes, cgo, JNI): wcqp_qp_enqueue_steps takes an array of argument records and makes, for
 * each record in order, exactly the calls
 *     wcqp_mpc_solve_device(mpc, batch, <the record's MPC arguments>, mpc_stream)
 *     wcqp_ik_solve_device (ik,  batch, <the record's IK arguments>,  ik_stream)
 * (a record whose x0 is NULL skips the MPC call, one whose J_left is NULL the IK call).  Same
 * streams, same results; a record whose two calls name the SAME stream is enqueued as one launch
 * whose workgroups split between the two problems (the IK handle's default kernel permitting) - the
 * MPC waves then run in the slots the IK waves leave idle while they wait for their inputs.  The
 * first failing call's code is returned and *n_done (may be NULL) says how many records were
 * enqueued completely.
 */
typedef struct wcqp_qp_step {
    /* wcqp_mpc_solve_device */
    const double* x0; const double* ref; int32_t ref_len; const double* u_prev;
    const double* hull_A; const double* hull_b; const int32_t* hull_nc;
    double* u0; int32_t* mpc_status; uint32_t* mpc_active; double* mpc_margin; void* mpc_stream;
    /* wcqp_ik_solve_device */
    const double* J_left; const double* J_right; const double* J_neck; const double* J_com;
    const double* q; const double* state;
    double* dq; int32_t* ik_status; uint32_t* active_lower; uint32_t* active_upper;
    double* foot_err; int32_t* iters; void* ik_stream;
} wcqp_qp_step;
int wcqp_qp_enqueue_steps(wcqp_mpc_t mpc, wcqp_ik_t ik, int32_t batch,
                          int32_t n_steps, const wcqp_qp_step* steps, int32_t* n_done);

/* A PLAN of steps: the records of wcqp_qp_enqueue_steps, uploaded once and replayed as ONE launch.  Consecutive steps of the
 * BASELINE workload are independent cold-start batches, so nothing has to order them on the device: a wavefront owns four
 * robots and walks through the records on its own - no launch, ramp-up or tail per step, the MPC of a record solved on the
 * IK's lanes while its Jacobians are in flight - and `ways` wavefronts share a robot group, way w taking records w, w + ways,
 * ... (two ways fill both wave slots of every SIMD at the BASELINE batch of 4096).  Records of DIFFERENT ways run
 * concurrently: they must not share output arrays (give each way its own, like the pipelines of separate streams).
 * ways = WCQP_PLAN_WAYS_AUTO picks the number of ways (enough workgroups for the hardware's dispatcher to even out the launch's ends: 16 at
 * 4096 robots, 4 from 16384 on, never more than one per record); every record then needs output arrays of its own.
 * ways = 0 is the WORK-QUEUE form: the launch has as many wavefronts as are resident at once (2 per SIMD), and each takes the
 * next (record, robot group) unit - robot-group-major - from a device-side queue when it is done with one, so that no wave slot
 * idles while another wavefront still has records left (the tail of the fixed ways).  Any two records may then be in flight
 * together and in any order: NO two records of the plan may share an output array.  The queue is re-armed by the launch itself;
 * launches of ONE plan must be ordered (one stream at a time), different plans are independent.
 * A plan in which NO record has an IK part (J_left == NULL in every record; `ik` may then be NULL, ways >= 1) is an MPC-only plan -
 * BASELINE config 2 on its own: one launch walks through the DCM-MPC batches; one in which NO record has an MPC part (x0 == NULL in
 * every record) is an IK-only plan - config 3 on its own.  Otherwise every
 * record needs both parts; the stream fields of the records are ignored (wcqp_qp_plan_enqueue names the stream).
 * WCQP_E_UNSUPPORTED unless the IK handle runs its default kernel with jacobian_structure = WCQP_IK_JAC_MIXED: use
 * wcqp_qp_enqueue_steps then.  Same results as the single calls, bit for bit.  The arrays the
 * records point to must stay valid while the plan is used; the handles must outlive the plan. */
#define WCQP_PLAN_WAYS_AUTO (-1)
typedef struct wcqp_qp_plan_s* wcqp_qp_plan_t;
int wcqp_qp_plan_create(wcqp_mpc_t mpc, wcqp_ik_t ik, int32_t batch, int32_t n_steps, const wcqp_qp_step* steps, int32_t ways,
                        wcqp_qp_plan_t* out);
int wcqp_qp_plan_enqueue(wcqp_qp_plan_t plan, void* stream);      /* enqueue only; graph-capturable */
int wcqp_qp_plan_destroy(wcqp_qp_plan_t plan);

/* =====================================================================================
 * Shard slabs: the exchange format of the multi-GPU path (rank 0 scatters the inputs of every rank's block of
 * robots, the ranks solve, rank 0 gathers the solutions).  All input arrays of a block live in ONE contiguous device buffer -
 *     [x0 | ref | u_prev | hull_A | hull_b | hull_nc | J_left | J_right | J_neck | J_com | q | state]
 * each in the layout of wcqp_mpc_solve_device / wcqp_ik_solve_device, every array starting on a 256-byte boundary - and all
 * outputs in another - [u0 | mpc_margin | dq | mpc_status | mpc_active | ik_status | active_lower | active_upper | iters] - so
 * that ONE ncclScatter (ncclSend / ncclRecv per peer) and ONE ncclGather move a step's data whatever the backend, and the solve
 * kernels read the received bytes where they landed: wcqp_qp_step_from_slabs fills a step record with pointers INTO the two
 * slabs (no unpack, no copy).  The reference has no counterpart (one robot per process, WM/include/WalkingModule.hpp:65-77).
 * Pure host arithmetic: no device call, usable from any host language next to RCCL. */
#define WCQP_SLAB_IN_ARRAYS  12
#define WCQP_SLAB_OUT_ARRAYS 9
typedef struct wcqp_slab_layout {
    int32_t batch, ref_len;
    int64_t in_offset[WCQP_SLAB_IN_ARRAYS];    /* byte offsets, in the order listed above */
    int64_t in_bytes;                          /* size of an input slab (a multiple of 256)  */
    int64_t out_offset[WCQP_SLAB_OUT_ARRAYS];
    int64_t out_bytes;
} wcqp_slab_layout;
int wcqp_slab_layout_for(int32_t batch, int32_t ref_len, wcqp_slab_layout* out);
/* step <- pointers into the slabs (streams NULL; foot_err NULL).  in_slab / out_slab: device addresses of buffers of at least
 * in_bytes / out_bytes, at least 16-byte aligned (every hipMalloc is 256-byte aligned). */
int wcqp_qp_step_from_slabs(const wcqp_slab_layout* layout, const void* in_slab, void* out_slab, wcqp_qp_step* step);

/* =====================================================================================
 * Batched kinematics: forward kinematics of a kinematic tree and the free-floating
 * Jacobians in MIXED representation that the QP-IK consumes - what the reference obtains from
 * iDynTree::KinDynComputations through WalkingFK:
 *   setInternalRobotState        WM/src/WalkingForwardKinematics.cpp:258-276
 *   get{Left,Right}FootToWorldTransform, getNeckOrientation, getCoMPosition   :312-340, 354-366, 402-405
 *   get{Left,Right}FootJacobian, getNeckJacobian, getCoMJacobian              :436-454 (MIXED, :33)
 * The robot model of the reference is an external URDF (WalkingModule.cpp:107) that is not in the
 * repository: the tree comes in as a table.  Joint j has a parent joint (-1 = root link, always < j), a
 * fixed transform (R0, p0) from the parent joint frame to its own frame at q = 0, a unit axis in its own
 * frame and carries one link; three frames are attached: left sole, right sole, neck.
 * Generalised velocity: (v of the base origin in world, omega of the base in world, dq).
 * Outputs use the batch layouts of wcqp_ik_solve_*: J_left/J_right [B][6][6+dof] (linear rows, then
 * angular), J_neck [B][3][6+dof] (angular rows), J_com [B][3][6+dof]; if `state` is given, the ACTUAL
 * poses are written into the packed pose block (foot positions/rotations, neck rotation, CoM position:
 * offsets 0..23, 48..56, 66..68), the desired entries are left alone.
 * ===================================================================================== */
#define WCQP_KIN_MAX_DOF 32
typedef struct wcqp_kin_params {
    int32_t dof;                        /* 6 + dof <= 32                                          */
    int32_t parent[WCQP_KIN_MAX_DOF];   /* parent joint, -1 = root link; parent[j] < j             */
    double  R0[WCQP_KIN_MAX_DOF][9];    /* row-major                                               */
    double  p0[WCQP_KIN_MAX_DOF][3];
    double  axis[WCQP_KIN_MAX_DOF][3];  /* in the joint's own frame; normalised at create          */
    double  mass[WCQP_KIN_MAX_DOF];     /* link carried by joint j                                 */
    double  com[WCQP_KIN_MAX_DOF][3];   /* its centre of mass in the joint frame                   */
    double  root_mass, root_com[3];
    int32_t frame_joint[3];             /* left sole, right sole, neck: joint the frame is fixed to */
    double  frame_R[3][9], frame_p[3][3];
} wcqp_kin_params;

typedef struct wcqp_kin_s* wcqp_kin_t;

/* Needs no device.  Any tree with parent[j] < j is taken (whatever its numbering, depth or the joints its frames sit on).
 * WCQP_E_UNSUPPORTED for a dof outside 1 .. 26; WCQP_E_INVALID for a NULL pointer, a parent[j] >= j or < -1, a negative or NaN mass or
 * root_mass, a robot without mass, an axis of length zero or with a NaN, a frame_joint outside 0 .. dof - 1.  *out is written on
 * success only. */
int wcqp_kin_create(const wcqp_kin_params* params, wcqp_kin_t* out);
int wcqp_kin_destroy(wcqp_kin_t h);
/* base [B][12] = position, row-major rotation of the root link; q [B][dof].  DEVICE pointers. */
int wcqp_kin_jacobians_device(wcqp_kin_t h, int32_t batch, const double* base, const double* q,
                              double* J_left, double* J_right, double* J_neck, double* J_com,
                              double* state /* [B][87] or NULL */, void* stream);
/* same with HOST pointers (copies in and out; `state` is read-modify-write) */
int wcqp_kin_jacobians_host(wcqp_kin_t h, int32_t batch, const double* base, const double* q,
                            double* J_left, double* J_right, double* J_neck, double* J_com, double* state);

/* =====================================================================================
 * Batched non-linear inverse kinematics (SURVEY.md component #11): the posture a robot's walk starts from - what
 * WalkingModule::prepareRobot (WM/src/WalkingModule.cpp:880-1005; the targets and the neck rule :944-984) obtains from
 * WalkingIK::computeIK (WM/src/WalkingInverseKinematics.cpp:239-305, 346-424), an iDynTree / IPOPT non-linear IK with the left sole as
 * the fixed base, the right sole and the CoM as full constraints, a joint regularisation and a neck rotation target as costs and the
 * model's joint limits as bounds.  iDynTree's InverseKinematics and IPOPT are upstream of the reference: THE PROBLEM AND THE ITERATION
 * ARE THIS BUILD'S OWN DEFINITION, stated here (tests/helpers/prepare_spec.py restates them in numpy).
 *
 * The problem, per robot.  Unknowns: the joints q [dof].  The base is no unknown: the left sole is anchored at its desired pose T_L
 * (world_T_base = T_L * (base_T_leftsole(q))^-1, as the tick's kinematics anchor the stance foot).
 *     minimise    w_q/2 |q - q_reg|^2  +  w_n/2 |log(R_neck(q) Rd_neck^T)|^2
 *     subject to  p_right(q) = pd_right,   log(R_right(q) Rd_right^T) = 0,   com(q) = com_d (x, y and height),   q_min <= q <= q_max
 * log is the rotation vector of a rotation matrix.  The gradient of the neck term with respect to a world angular velocity is taken to
 * be that vector itself (exact to first order in it), so the cost gradient is w_q (q - q_reg) + w_n Jn^T phi_n with Jn the anchored
 * neck Jacobian (angular rows).  w_n = 0 switches the neck target off (no `additional_frame`); q_min / q_max NULL: no limits.
 *
 * The iteration (the contract is the optimum it stops at, not its path).  With the left sole anchored every MIXED Jacobian is reduced
 * to the joints: J~ = J[:, 6:] - J[:, :6] (J_left[:, :6])^-1 J_left[:, 6:].  The guess is first clipped into the limits.  One
 * iteration solves exactly this QP for dq:
 *     minimise  1/2 dq^T H dq + g^T dq,   H = w_q I + w_n Jn~^T Jn~,   g = w_q (q - q_reg) + w_n Jn~^T phi_n
 *     s. t.     [JR~; Jc~] dq = -c   (nine rows: c = p_right - pd_right | log(R_right Rd_right^T) | com - com_d)
 *               q_min - q <= dq <= q_max - q
 * and steps q += min(1, step_cap / max|dq|) dq.  The step cap is no part of the QP (far from the target it would make it infeasible).
 * A robot stops WCQP_STATUS_SOLVED when max|dq| < tol_step and max|c| < tol_constraint; a QP whose equality rows and active bounds are
 * dependent ends WCQP_STATUS_INFEASIBLE, one whose Hessian is not positive definite WCQP_STATUS_NUMERIC, max_iter iterations spent
 * WCQP_STATUS_MAX_ITER.  For every status other than SOLVED q comes back as the CLIPPED GUESS, never a half-converged iterate.
 * Non-finite inputs (the header's contract): a NaN or an Inf in a robot's targets or guess gives WCQP_STATUS_NUMERIC, q = the guess with
 * every non-finite entry replaced by 0 and clipped, iters = 0, residual = +inf; the other robots do not notice.
 *
 * DEVIATIONS from the reference, all upstream of it and unpinned: iDynTree's roll-pitch-yaw parametrisation of the rotation targets,
 * its internal cost scaling and IPOPT's path are not reproduced; the reference's 1e-4 tolerances are parameters here (1e-4 is a legal
 * setting); the CoM weight 100 of setCOMTarget has no effect on a hard constraint and is not taken; the reference expresses everything in
 * the left-sole frame, here the same problem is stated in the world frame with the sole anchored.
 * ===================================================================================== */
typedef struct wcqp_prepare_params {  /* every value is taken as given (no 0 -> default; capi.PrepareSolver holds the defaults) */
    double  w_q;                         /* joint_regularization_weight (inverseKinematics.ini), reference 0.5; > 0                 */
    double  w_n;                         /* weight of the neck rotation target, reference 1.0; 0 = off; >= 0                        */
    double  step_cap;                    /* largest joint step of an iteration [rad], default 0.3; > 0                              */
    double  tol_step;                    /* default 1e-12; >= 0                                                                     */
    double  tol_constraint;              /* default 1e-10; >= 0                                                                     */
    int32_t max_iter;                    /* default 100; >= 1                                                                       */
    const double* q_reg;                 /* [dof] jointRegularization, rad; HOST pointer, copied at create                          */
    const double* q_min;                 /* [dof] joint limits, HOST pointers copied at create; both NULL: no limits                */
    const double* q_max;
} wcqp_prepare_params;

typedef struct wcqp_prepare_s* wcqp_prepare_t;

/* WalkingIK::initialize (WM/src/WalkingInverseKinematics.cpp:25-237).  The handle copies the model out of `kin` (which may be destroyed
 * afterwards).  WCQP_E_INVALID for a NULL kin, params, q_reg or out, a non-finite weight, tolerance or step cap or one outside the ranges
 * above, a non-finite q_reg, only one of q_min / q_max, q_min > q_max or a NaN limit, max_iter < 1; WCQP_E_UNSUPPORTED for a tree the 16-lane walk of the tick's
 * fused kinematics cannot run (wcqp_tick_params.kin_handoff: 23 joints, depth-first numbering, depth <= 8, every joint on the path of at
 * most one attached frame).  Needs no device. */
int wcqp_prepare_create(wcqp_kin_t kin, const wcqp_prepare_params* params, wcqp_prepare_t* out);
int wcqp_prepare_destroy(wcqp_prepare_t h);
/* WalkingIK::computeIK (WM/src/WalkingInverseKinematics.cpp:346-424) as WalkingModule::prepareRobot calls it (WM/src/WalkingModule.cpp:944-984),
 * for `batch` robots, ALL ITERATIONS IN ONE LAUNCH.  DEVICE pointers; enqueue only (no allocation, no synchronisation):
 *   left_d, right_d [B][12]   desired sole poses: p 3 | R 9 row-major (the left one is the anchor)
 *   com_d [B][3]              desired CoM
 *   Rd_neck [B][9] or NULL    desired neck orientation (already multiplied by additional_rotation); NULL: no neck target (as w_n = 0)
 *   q_guess [B][dof]
 * outputs
 *   q [B][dof]                the optimum (SOLVED) or the clipped guess
 *   base [B][12]              world pose of the root link at q: p 3 | R 9 (the `base` of wcqp_kin_jacobians_*)
 *   state [B][87]             the packed pose block of wcqp_ik_solve_*, ready to be wcqp_tick_inputs.state0: the ACTUAL poses at q
 *                             (0..23, 48..56, 66..68), the desired entries = the targets (24..47 the two soles, 57..65 Rd_neck - the
 *                             actual neck orientation without a neck target -, 69..71 com_d), velocities and twists 0
 *   status [B], iters [B]     WCQP_STATUS_*; iterations (QPs solved)
 *   residual [B][2]           max |c| and max |stationarity| - the infinity norm of H-free g + [JR~; Jc~]^T lambda + mu, with lambda
 *                             and mu the multipliers of the last QP - at the returned q of a SOLVED robot; +inf otherwise
 * Any output pointer but q and status may be NULL.  Rows: state 696 B - a batch whose arrays pass the 4 GB rule above (batch x 696 > 2^32)
 * gets WCQP_E_UNSUPPORTED before anything is looked for or allocated. */
int wcqp_prepare_solve_device(wcqp_prepare_t h, int32_t batch, const double* left_d, const double* right_d, const double* com_d,
                              const double* Rd_neck, const double* q_guess,
                              double* q, double* base, double* state, int32_t* status, int32_t* iters, double* residual, void* stream);
/* same with HOST pointers: staged through the handle's own device buffer, synchronises */
int wcqp_prepare_solve_host(wcqp_prepare_t h, int32_t batch, const double* left_d, const double* right_d, const double* com_d,
                            const double* Rd_neck, const double* q_guess,
                            double* q, double* base, double* state, int32_t* status, int32_t* iters, double* residual);

/* =====================================================================================
 * Device-resident tick pipeline — BASELINE configs 4/5 and SURVEY.md §8f-1/2: the call
 * order of WalkingModule::updateModule around the two solvers (WM/src/WalkingModule.cpp:
 * 578-745) for a batch of synthetic robots, kept entirely on the GPU:
 *   MPC   hull rows of this tick's contact pair (= setConvexHullConstraint; the kernel indexes one
 *         of the three precomputed row sets, so a contact change costs nothing),
 *         window [t, t+N] of the per-instance DCM reference trajectory (the deque that
 *         advances one stage per tick, WalkingModule.cpp:35-96), x0 = measured DCM,
 *         u_prev = previous output (MPCSolver.cpp:244-245)
 *   glue  LIPM reference (StableDCMModel.cpp:63-90), ZMP-CoM law + integrator
 *         (WalkingZMPController.cpp:146-173) -> desired CoM position /
 *         velocity into the IK pose block (WalkingModule.cpp:686-695); synthetic LIPM plant
 *   IK    joint velocities
 *   post  q <- Integrator(dq) (WalkingModule.cpp:741-744), contact pair of the next tick, tick += 1
 * With the default IK kernel (base elimination) a tick is ONE kernel - forward kinematics (use_kinematics), the MPC chain, the glue,
 * the IK and the post step on the 16 lanes a robot's IK runs on - and, the robots of a wavefront depending on no other wavefront's,
 * a launch walks through ALL the ticks of a wcqp_tick_run call (ticks_per_launch).  The MPC -> ZMP-CoM law -> plant chain does not
 * depend on the IK, so the tick is SKEWED inside a call: the kernel solves IK(t) and, in the shadow of its loads, the MPC chain of
 * tick t + 1 (a call starts with the MPC of its first tick alone and its last tick runs no MPC ahead: between calls nothing is
 * ahead of anything).  Same results as the in-order forms that remain for the other IK algorithms: the general 16-lane kernel
 * (algorithm 4) takes an MPC launch and an IK launch per tick, an explicit 32-lane / sweep IK algorithm or the CoM-as-cost
 * variant four (stand-alone glue / post kernels); for those, and with ticks_per_launch = 1, `use_graph` replays hipGraphs of 8
 * ticks each (captured ONCE: the tick index lives in device memory), remaining ticks go as plain launches.
 * ===================================================================================== */
#define WCQP_KIN_HANDOFF_FUSED   0
#define WCQP_KIN_HANDOFF_DENSE   1
#define WCQP_KIN_HANDOFF_COMPACT 2
typedef struct wcqp_tick_params {
    int32_t batch;              /* instances on this device                                   */
    int32_t first;              /* global index of instance 0 (disturbance stream)             */
    int32_t max_ticks;          /* trajectories hold max_ticks + horizon + 1 stages            */
    int32_t log_ticks;          /* > 0: keep u0/dq of the first log_ticks ticks for parity     */
    int32_t step_ticks, ds_ticks;
    double  k_com, k_zmp;       /* zmpControllerParams.ini:7-8                                 */
    double  noise;              /* amplitude of the bounded DCM disturbance                    */
    uint64_t seed;
    wcqp_mpc_params mpc;
    wcqp_ik_params ik;
    /* Per-tick kinematics (SURVEY.md 8f-4 inside the tick, WM/src/WalkingModule.cpp:715, 396-410): when set, every tick
     * first evaluates the forward kinematics of `kin` at the integrated joint positions q_des with the floating base
     * anchored at the stance foot of the current step (world_T_base = desired sole pose x inverse of the sole's pose in
     * the base frame: WalkingFK::evaluateWorldToBaseTransformation, WM/src/WalkingForwardKinematics.cpp:160-256) and gives
     * the IK of the tick the four MIXED Jacobians and the actual foot / neck poses and CoM (`kin_handoff` says how); the
     * support-polygon rows of the three contact pairs are built from the DESIRED foot poses (state0 entries 24..47,
     * `foot_rect`) when those are uploaded, and a tick selects by its contact pair (setConvexHullConstraint,
     * ...PredictiveController.cpp:364-435, switches rows only when the pair changes).  The J_* and hull_tab_* inputs are
     * then ignored (may be NULL). */
    /* IK hot start (SQProblem::hotstart, WM/src/WalkingQPInverseKinematics_qpOASES.cpp:312-335): by default every tick
     * first tries the previous tick's active joint-velocity bounds of the robot (added in one step, accepted when all
     * their multipliers are positive) and falls back to the cold active-set walk otherwise; 1 = always cold.
     * Same optimum either way (the QP is strictly convex); base-eliminated kernel only. */
    int32_t ik_cold_start_only;
    int32_t use_kinematics;
    wcqp_kin_params kin;
    double  foot_rect[8];       /* corners (x, y) x 4 of the foot rectangle in the foot frame (foot_size, cpp:295-303) */
    /* How the per-tick kinematics reach the IK of the same tick (WCQP_KIN_HANDOFF_*; same results):
     * FUSED (0, default)  no hand-off at all: the wavefront that solves a robot's IK first evaluates its forward kinematics and
     *           its Jacobian columns (16 lanes per robot, two joints per lane) - one launch per tick, or many ticks per launch
     *           (ticks_per_launch).  Needs a tree whose joints each lie on the path of at most ONE of the three frames (left sole,
     *           right sole, neck: a humanoid whose legs and torso branch at the root link), depth-first joint numbering, depth
     *           <= 8 and an MPC horizon <= 55; otherwise COMPACT is taken.
     * DENSE (1)   a kinematics launch per tick writes the four dense Jacobians (the layouts of wcqp_kin_jacobians_* /
     *           wcqp_ik_solve_*), 4.4 KB per robot of which ~70 % are structural zeros.
     * COMPACT (2) a kinematics launch per tick writes, per joint, its CoM column and its column of the ONE frame Jacobian
     *           it is on the path of, plus the three vectors p_frame - p_base that make up the base blocks [I -S(p); 0 I]:
     *           1.4 KB per robot (same condition on the tree as FUSED, else DENSE). */
    int32_t kin_handoff;
    /* Ticks per launch of the fused kernel (default IK kernel; constant Jacobians or FUSED kinematics): the robots of a wavefront depend on
     * no other wavefront's, so a wave walks through the ticks of a wcqp_tick_run call on its own - no launch, ramp-up or tail
     * per tick, and a wave whose robots walk a long active set falls behind without holding anybody up.
     * 0 -> all the ticks of a wcqp_tick_run call in one launch; k > 0: at most k per launch; 1 = one launch per tick (what
     * `use_graph` then replays from a hipGraph of 8 ticks).  Same results whatever the value. */
    int32_t ticks_per_launch;
    /* > 0: keep, for the first logger_ticks ticks, the row WalkingModule hands its logger per tick (WM/src/WalkingModule.cpp:800-810;
     * the 53 values behind "record" of the column list :1231-1250), per robot: wcqp_tick_outputs.logger.  Columns:
     *   0-1 dcm (measured)   2-3 dcm_des   4-5 dcm_des_d (finite difference of the uploaded reference: the planner's DCM velocity is
     *   not an input of this pipeline)   6-7 zmp (measured = the previous command)   8-9 zmp_des (the MPC's u0)   10-12 com (measured:
     *   the kinematics' CoM with use_kinematics, else the plant's)   13-14 com_des   15-16 com_des_d   17-19 lf position   20-22 lf
     *   roll pitch yaw (iDynTree::Rotation::asRPY)   23-28 rf   29-34 lf_des   35-40 rf_des   41-46 lf_err   47-52 rf_err (the IK's
     *   getLeftFootError / getRightFootError; with kinematics in the tick the dense Jacobians they are formed with do not exist and
     *   the twelve - residuals of equality constraints, O(1e-15) in the reference too - are logged as zeros).
     * Runs a logging build of the tick kernel (the default IK kernel only); a debugging aid like the reference's dumpData. */
    int32_t logger_ticks;
    /* Where a tick's MEASURED state comes from (WCQP_TICK_PLANT_*).  INTERNAL (0, default): the synthetic LIPM plant of the harness
     * (measured DCM follows xi+ = a xi + b u0 + w, measured CoM c+ = c + dT (-omega (c - xi)), measured ZMP = the previous command,
     * measured joints = the desired ones).  EXTERNAL: the caller's - B robots simulated or measured by something else - handed over on
     * the device before every tick with wcqp_tick_set_feedback_device; what the reference reads from the robot every tick:
     * setFeedback(measuredDCM) WM/src/WalkingModule.cpp:612, WalkingZMPController::setFeedback(measuredZMP, measuredCoM) :665, the
     * measured joint positions of WalkingQPIK::setRobotState :373.  A tick then cannot run ahead of its feedback: wcqp_tick_run takes
     * exactly ONE tick per call, in order (MPC(t), then IK(t): 2 launches + the feedback copy).  Default IK kernel only. */
    int32_t plant;
    /* The DCM controller of the tick (WCQP_TICK_DCM_*).  MPC (0, default): the DCM-MPC above (WalkingModule.cpp:604-636, the
     * reference's `use_mpc 1`).  REACTIVE (1): WalkingDCMReactiveController (WM/src/WalkingDCMReactiveController.cpp:63-82, the
     * reference's default `use_mpc 0`, WalkingModule.cpp:124, 188-211, 638-656), closed form per axis:
     *     zmp_des = dcm_des - dcm_des_dot / omega - k_dcm (dcm_des - dcm_measured),   omega = sqrt(gravity / com_height)
     * with dcm_des the reference stage of the tick and dcm_des_dot wcqp_tick_inputs.dcm_vel_traj (NULL: the forward difference
     * (ref[t+1] - ref[t]) / dT).  Everything after it is what the MPC tick does: ZMP-CoM law, IK, joint integration, plant.
     * With REACTIVE:
     *   - the MPC's Q, R and hull inputs are ignored; the hull tables may be NULL when there are no kinematics;
     *   - mpc.horizon still sets the length of the trajectory buffers (max_ticks + horizon + 1 stages), and sampling_time,
     *     com_height and gravity keep their meaning;
     *   - mpc_fail stays 0;
     *   - u0_log and logger columns 8-9 hold the reactive output zmp_des; logger columns 4-5 the velocity actually used;
     *   - the fused kinematics hand-off is taken at any horizon (the MPC's needs horizon < 55);
     *   - wcqp_tick_splice_reference on a handle uploaded with an explicit dcm_vel_traj returns WCQP_E_UNSUPPORTED (the splice
     *     has no velocity tail); with NULL velocities it works as with the MPC.
     * wcqp_tick_create returns WCQP_E_INVALID for an unknown controller, and for REACTIVE with a k_dcm that is not finite. */
    int32_t dcm_controller;
    double k_dcm;               /* kDCM of DCM_REACTIVE_CONTROLLER (app/robots/<robot>/dcmReactiveControllerParams.ini:1) */
    /* ZMP-CoM gain scheduling (0 = off: the fixed gains k_com / k_zmp on every tick).  On (the reference's `useGainScheduling 1`,
     * app/robots/<robot>/zmpControllerParams.ini, set for all three shipped robots), k_com / k_zmp are the *_walking values and every
     * tick t, before the ZMP-CoM law, does what WM/src/WalkingModule.cpp:657-662 and WM/src/WalkingZMPController.cpp:29-125 do:
     *   - stance = sqrt(vx * vx + vy * vy) < 0.001, with (vx, vy) the DCM velocity of tick t: wcqp_tick_inputs.dcm_vel_traj, or (NULL)
     *     the forward difference of ref_traj - MPC handles then read the velocity too;
     *   - both gains' smoothers advance one step towards the stance gains (stance) or the walking ones; the gains of tick t are their
     *     outputs after the step (tick 0 already uses the output after one step);
     *   - wcqp_tick_upload puts both at rest at the stance gains (WalkingZMPController::initialize); their state carries across
     *     wcqp_tick_run calls and splices;
     *   - wcqp_tick_splice_reference on a handle uploaded with an explicit dcm_vel_traj returns WCQP_E_UNSUPPORTED, as with REACTIVE.
     * The smoother (iCub::ctrl::minJerkTrajGen upstream, which is not part of the reference) is this project's restatement: the
     * third-order minimum-jerk approximation H(s) = (150/T^3) / (s^3 + (9/T) s^2 + (60/T^2) s + 150/T^3), T = zmp_smoothing_time,
     * discretised with the bilinear (Tustin) transform at mpc.sampling_time.  Both smoothers are this linear filter of unit DC gain,
     * both start at rest at the stance gains, so the tick runs ONE filter s(t) of the 0 / 1 walking indicator per robot and uses
     * k = k_stance + (k_walking - k_stance) s(t).
     * wcqp_tick_create returns WCQP_E_INVALID with scheduling on when a stance gain is not finite or zmp_smoothing_time is not a
     * finite number > 0. */
    int32_t zmp_gain_scheduling;
    double k_com_stance, k_zmp_stance;   /* kCoM_stance / kZMP_stance of zmpControllerParams.ini                                   */
    double zmp_smoothing_time;           /* smoothingTime of zmpControllerParams.ini [s]                                           */
    /* Planned-trajectory mode (0 = off: the synthetic gait of step_ticks / ds_ticks / phase0 / swing_twist).  On, every tick t takes
     * from stage t of the planner's trajectories (wcqp_tick_inputs.left_traj ... com_height_vel) what WalkingModule::updateTrajectories
     * (WM/src/WalkingModule.cpp:1085-1145) pulls from TrajectoryGenerator:
     *   - the IK's desired foot poses (state 24..47) and twists (75..86), the desired CoM height and its velocity (71, 74);
     *   - the desired neck orientation (57..65) = RotZ(atan2(sin yL + sin yR, cos yL + cos yR)) * neck_additional_rotation, with each
     *     foot's yaw atan2(R10, R00) (WalkingModule.cpp:697-707, :383; WalkingQPInverseKinematics.cpp:143-146);
     *   - the floating-base anchor of the forward kinematics: the desired pose of the foot the fixed-frame bit names (:1147-1165);
     *   - the contact pair; on a change of pair the MPC's support-polygon rows are rebuilt from that tick's desired foot poses and
     *     foot_rect (...PredictiveController.cpp:364-435), with no change they stay.
     * Everything else is what the tick does without it.  phase0, step_ticks (beyond the range check), ds_ticks, swing_twist, hull_tab_*
     * and the desired-pose / Rd_neck entries of state0 are ignored.  Runs with per-tick kinematics and the FUSED hand-off in the skewed
     * kernel of the default IK algorithm, either DCM controller, with or without gain scheduling, any ticks_per_launch and use_graph.
     * wcqp_tick_create returns WCQP_E_UNSUPPORTED, before any device allocation, for the mode with constant Jacobians, with the DENSE or
     * COMPACT hand-off (or wherever FUSED would not be taken: an MPC horizon of 56 or more, a tree FUSED cannot run), logger_ticks > 0,
     * the EXTERNAL plant or an IK algorithm other than the default; wcqp_tick_splice_reference returns WCQP_E_UNSUPPORTED on such a
     * handle (there is no tail for the feet).  WCQP_E_INVALID for a value other than 0 / 1 or a non-finite neck_additional_rotation. */
    int32_t planned_trajectories;
    double neck_additional_rotation[9];  /* additional_rotation of qpInverseKinematics.ini, row-major                              */
    /* Streamed trajectories (0 = off: the handle behaves as before, bit for bit).  A capability of the EXTERNAL plant: on, every tick t
     * takes its desired stage - the FRONT of the planner's deques, what WalkingModule::updateModule consumes per tick
     * (WM/src/WalkingModule.cpp:509-511, 689-707, 1085-1165) - from the wcqp_tick_set_desired_* call that preceded it, instead of the
     * synthetic gait.  The stage supplies what planned_trajectories lists above: the IK's desired feet (state 24..47) and twists (75..86),
     * the CoM height and its velocity (71, 74), the desired neck orientation RotZ(meanYaw) * neck_additional_rotation (57..65), the
     * floating-base anchor = the desired pose of the fixed-frame foot, the contact pair, and on a change of pair (and at tick 0) the MPC's
     * support-polygon rows rebuilt from that stage's feet and foot_rect; with no change of pair the rows stay, whatever the feet do
     * (...PredictiveController.cpp:364-435).  Nothing is uploaded per stage ([B][T] arrays do not exist), and replanning the feet needs no
     * merge call: the caller hands over stages of the new plan from the next tick on (the DCM reference's tail still goes through
     * wcqp_tick_splice_reference, which works on such a handle as on any EXTERNAL one).
     * phase0, swing_twist, hull_tab_* (may be NULL) and the desired-pose / Rd_neck entries of state0 are ignored at upload.
     * wcqp_tick_create returns WCQP_E_INVALID for a value other than 0 / 1 or a non-finite neck_additional_rotation, and
     * WCQP_E_UNSUPPORTED, before anything touches the device, unless plant = EXTERNAL, use_kinematics with the FUSED hand-off actually
     * taken (an MPC horizon below 56; REACTIVE any), the default / base-eliminated IK algorithm, logger_ticks = 0 and
     * planned_trajectories = 0. */
    int32_t streamed_trajectories;
    /* Low-pass filters of the sensor form (wcqp_tick_set_sensor_feedback_*, which says what they do), cut frequencies in Hz; 0 = that
     * filter off (the reference's use_* 0; all three 0: the handle behaves as before, bit for bit):
     *   joint_velocity_cut_frequency   use_joint_velocity_filter / joint_velocity_cut_frequency   (robotControl.ini)
     *   wrench_cut_frequency           use_wrench_filter / wrench_cut_frequency                   (robotControl.ini)
     *   com_cut_frequency              use_filters / cut_frequency                                (forwardKinematics.ini)
     * wcqp_tick_create returns WCQP_E_INVALID for a negative or non-finite value and WCQP_E_UNSUPPORTED, before anything touches the
     * device, for a value > 0 on a handle without a sensor form: the internal plant, or use_kinematics = 0. */
    double joint_velocity_cut_frequency;
    double wrench_cut_frequency;
    double com_cut_frequency;
    /* The inverse kinematics of the tick (WCQP_TICK_IK_*).  VELOCITY (0, default: the handle behaves as before, bit for bit): the Jacobian
     * QP-IK gives joint velocities, which are integrated - the reference's `use_QP-IK 1` (WM/src/WalkingModule.cpp:709-744).  POSITION (1):
     * the reference's `use_QP-IK 0` (:745-769) - WalkingIK::computeIK(m_leftTrajectory.front(), m_rightTrajectory.front(),
     * desiredCoMPosition, m_qDesired) gives the joint POSITIONS of the tick directly: every tick's joints are an optimum of the position
     * problem of wcqp_prepare_* above, so the soles sit on their planned poses to the solver's tolerance on every tick, with no drift from
     * an integration.  A mode of a planned handle (planned_trajectories = 1).  Tick t of a POSITION handle:
     *   1. The chain, exactly as the planned velocity tick runs it: the stage t record, the LIPM reference, the MPC or the reactive law, the
     *      gain schedule where set, the ZMP-CoM law and its integrator, the internal plant.  It reads nothing the IK writes and keeps
     *      running for a stopped robot.
     *   2. The targets: left_d, right_d = the desired soles of record t; com_d = (p_star x, p_star y, the desired CoM height of record t);
     *      Rd_neck = RotZ(meanYaw) * neck_additional_rotation, as the planned tick forms it.
     *   3. The problem and the iteration of wcqp_prepare_*, unchanged: the left sole anchored at left_d, the right sole and the CoM as
     *      equality rows, the joint regularisation and the neck target as costs, the joint limits as bounds.
     *   4. The guess is q_des of tick t - 1 (tick 0: q0), clipped into the limits; the budget is position_ik.max_iter iterations PER TICK.
     *   5. WCQP_STATUS_SOLVED: q_des takes the optimum.
     *   6. Any other status: ik_fail counts the tick and the robot is stopped, as in the velocity tick - q_des keeps its value (at tick 0:
     *      the clipped q0), no further IK is run for that robot and every later tick also counts.
     * `position_ik` holds the problem's parameters: its HOST pointers are copied at create, every value is taken as given (no 0 -> default;
     * capi.TickPipeline holds the defaults).  `ik` is ignored on such a handle apart from `dof` and the refusal of an `algorithm` below.
     * DEVIATIONS from the reference: the fixed-frame bit of the record does not move the anchor - WalkingIK always uses the left foot as its
     * base; the neck target is the planned tick's own, not yawRotation^-1 * inertial_R_world (WalkingModule.cpp:703-707); the upstream
     * deviations listed for wcqp_prepare_* apply; the CoM velocity and the twists of the record are not read.
     * wcqp_tick_create, before anything touches the device: WCQP_E_INVALID for an unknown ik_mode and, with POSITION, for any position_ik
     * value wcqp_prepare_create refuses; WCQP_E_UNSUPPORTED for POSITION without planned_trajectories, and together with the EXTERNAL plant,
     * streamed_trajectories (the last two unless WCQP_TICK_OPT_POSITION_STREAMED asks for them, wcqp_tick_create_opts below), logger_ticks > 0
     * or an IK algorithm other than the default.  Every refusal of planned_trajectories applies
     * unchanged (the FUSED hand-off actually taken, the tree).  On a POSITION handle wcqp_tick_upload, wcqp_tick_upload_footsteps,
     * wcqp_tick_replan_footsteps, wcqp_tick_get_plan and wcqp_tick_run (any n_ticks, ticks_per_launch, use_graph, stream) work as on any
     * planned handle; one launch of its kernel walks the ticks of a run call, and nothing runs ahead between ticks (no skew). */
    int32_t ik_mode;
    wcqp_prepare_params position_ik;
} wcqp_tick_params;
#define WCQP_TICK_PLANT_INTERNAL 0
#define WCQP_TICK_PLANT_EXTERNAL 1
#define WCQP_TICK_DCM_MPC        0
#define WCQP_TICK_DCM_REACTIVE   1
#define WCQP_TICK_IK_VELOCITY    0
#define WCQP_TICK_IK_POSITION    1

typedef struct wcqp_tick_inputs {   /* HOST pointers, copied at upload */
    const double* ref_traj;     /* [B][max_ticks+N+1][2]                                      */
    const double* hull_tab_A;   /* [B][3][8][2]  rows for {left, right, both} in contact       */
    const double* hull_tab_b;   /* [B][3][8]                                                   */
    const int32_t* hull_tab_nc; /* [B][3]                                                      */
    const int32_t* phase0;      /* [B] offset into the step cycle                              */
    const double* J_left; const double* J_right; const double* J_neck; const double* J_com;
    const double* state0;       /* [B][87] poses; CoM entries and twists are rewritten per tick */
    const double* swing_twist;  /* [B][6] desired twist of whichever foot is in the air        */
    const double* q0;           /* [B][dof]                                                    */
    const double* dcm0; const double* com0; const double* u_init;   /* [B][2] each             */
    const double* dcm_vel_traj; /* [B][max_ticks+N+1][2] or NULL: the planner's DCM velocity (WalkingModule.cpp:641-642), read by
                                 * the REACTIVE controller and by ZMP gain scheduling (NULL: the forward difference of ref_traj);
                                 * MPC handles without gain scheduling ignore it */
    /* planned_trajectories only (ignored otherwise; required then, except the two CoM height arrays): T = max_ticks + N + 1 stages,
     * stage t what the planner's deques hold at front() on tick t.  wcqp_tick_upload returns WCQP_E_INVALID when a required array is
     * NULL, or when a stage a run can reach (0 .. max_ticks) has neither foot in contact, a fixed-frame foot that is not in contact or
     * a non-finite value - checked before anything of the handle changes (a handle uploaded before keeps that upload).  The upload also
     * builds the support-polygon rows of every change of contact pair from that stage's desired feet and foot_rect. */
    const double* left_traj;    /* [B][T][12] left sole: position 3, rotation 9 row-major (m_leftTrajectory)                 */
    const double* right_traj;   /* [B][T][12] right sole (m_rightTrajectory)                                                  */
    const double* left_twist;   /* [B][T][6]  m_leftTwistTrajectory                                                           */
    const double* right_twist;  /* [B][T][6]  m_rightTwistTrajectory                                                          */
    const uint8_t* contact;     /* [B][T] bit 0 left in contact, bit 1 right in contact, bit 2 left is the fixed frame        */
    const double* com_height_traj;  /* [B][T] or NULL: state0 entry 68 (m_comHeightTrajectory)                               */
    const double* com_height_vel;   /* [B][T] or NULL: 0 (m_comHeightVelocity)                                               */
} wcqp_tick_inputs;

typedef struct wcqp_tick_outputs {  /* HOST pointers, any may be NULL */
    double* u0_log;             /* [log_ticks][B][2]                                           */
    double* dq_log;             /* [log_ticks][B][dof]                                         */
    double* q_des;              /* [B][dof]                                                    */
    double* dcm; double* com;   /* [B][2]                                                      */
    int64_t* mpc_fail; int64_t* ik_fail;   /* [B] ticks whose QP did not end SOLVED; a robot whose IK failed once is
                                              stopped (the reference's updateModule returns false, WalkingModule.cpp:723-739):
                                              dq = 0 from then on and every further tick counts                      */
    int64_t* hot_try; int64_t* hot_hit;    /* [B] ticks on which the previous active set was tried / accepted (IK hot start) */
    int32_t* tick;              /* ticks executed so far                                       */
    double* logger;             /* [logger_ticks][B][53] logger rows (wcqp_tick_params.logger_ticks)   */
    uint32_t* active_lower; uint32_t* active_upper;   /* [B] the IK's active joint-velocity bounds of the LAST tick (bit i = joint i):
                                                         what the next tick's hot start begins from                               */
    double* zmp_gains;          /* [B][2] kCoM, kZMP the last executed tick used (zmp_gain_scheduling; without it k_com, k_zmp;
                                   after an upload, before any tick: the stance gains)                                            */
    double* measured;           /* [B][6] EXTERNAL plant only: dcm xy, com xy, ZMP xy the last executed tick used as its measured state,
                                   whichever feedback form set it (after an upload, before any tick: dcm0, com0, u_init).  Any other
                                   handle: WCQP_E_UNSUPPORTED when non-NULL                                                       */
    int64_t* feedback_fail;     /* [B] EXTERNAL plant only: ticks whose feedback was rejected - by wcqp_tick_set_sensor_feedback_*, by
                                   wcqp_tick_set_feedback_* (a non-finite value) or by wcqp_tick_set_desired_* - since the last
                                   upload.  Any other handle: WCQP_E_UNSUPPORTED when non-NULL                                      */
    double* q_log;              /* [log_ticks][B][dof] POSITION handles only (wcqp_tick_params.ik_mode): the joints tick t commanded.  On
                                   such a handle dq_log must be NULL (WCQP_E_UNSUPPORTED otherwise: no velocity exists), hot_try and hot_hit
                                   read 0, and active_lower / active_upper are the JOINT LIMITS active in the last QP of the last executed
                                   tick (0 for a robot whose last tick did not end SOLVED).  Any other handle: WCQP_E_UNSUPPORTED when
                                   non-NULL                                                                                         */
    int64_t* ik_iters;          /* [B] POSITION handles only: Gauss-Newton iterations spent since the last upload.  Any other handle:
                                   WCQP_E_UNSUPPORTED when non-NULL                                                                 */
} wcqp_tick_outputs;

typedef struct wcqp_tick_s* wcqp_tick_t;
int wcqp_tick_create(const wcqp_tick_params* params, wcqp_tick_t* out);
/* Parameters added after wcqp_tick_params was closed (its layout, last fields included, is pinned): they travel in a struct of their own
 * that only grows at its end, beside the unchanged wcqp_tick_params.  wcqp_tick_create(p, out) is wcqp_tick_create_ext(p, NULL, out).
 *
 * resident_plan (0 = off: every handle behaves as before, bit for bit).  A capability of a streamed handle (streamed_trajectories = 1,
 * hence the EXTERNAL plant): the handle additionally HOLDS the plan arrays of a planned handle - the records [B][T][40] (320 B per robot
 * and stage, T = max_ticks + horizon + 1), the plan's support-polygon row sets, and ref_traj / dcm_vel as it does already - and
 * wcqp_tick_set_desired_from_plan stages tick t's stage out of them on the device, in the place of a wcqp_tick_set_desired_* call.  The
 * tick, its prime launch and the sensor form run what they run on any streamed handle: they read the robot's one live record.
 *   - wcqp_tick_upload_footsteps, wcqp_tick_upload WITH the planned arrays (left_traj ... com_height_vel; required on such a handle, by
 *     the rules of a planned handle's upload), wcqp_tick_replan_footsteps and wcqp_tick_get_plan work as on a planned handle, through
 *     the same code; without resident_plan they stay refused on a streamed handle (WCQP_E_UNSUPPORTED).
 *   - Order per tick: wcqp_tick_set_desired_from_plan (it counts as a wcqp_tick_set_desired_*) -> wcqp_tick_set_sensor_feedback_* or
 *     wcqp_tick_set_feedback_* -> wcqp_tick_run(h, 1, ...).  A later wcqp_tick_set_desired_* before the run replaces the stage, as a
 *     second one does today; a second wcqp_tick_set_desired_from_plan restages it.
 *   - Replan rule: a tick whose stage has been staged from the plan counts as enqueued - wcqp_tick_replan_footsteps after tick t was
 *     staged needs merge_stage[i] >= t + 1 (WCQP_E_INVALID otherwise, the handle unchanged).
 * wcqp_tick_create_ext returns WCQP_E_INVALID for a value other than 0 / 1 and WCQP_E_UNSUPPORTED, before anything touches the device, for
 * resident_plan = 1 without streamed_trajectories; every refusal of a streamed handle stays (planned_trajectories = 1 with the EXTERNAL
 * plant or together with streamed_trajectories among them). */
typedef struct wcqp_tick_params_ext {
    int32_t resident_plan;
} wcqp_tick_params_ext;
int wcqp_tick_create_ext(const wcqp_tick_params* params, const wcqp_tick_params_ext* ext, wcqp_tick_t* out);      /* ext NULL: all zero */
/* Capabilities added after both structs were closed travel as an OPTION LIST: a later capability is one more key, not one more struct or
 * field.  wcqp_tick_create_ext(p, ext, out) is wcqp_tick_create_opts with the one option {WCQP_TICK_OPT_RESIDENT_PLAN, ext->resident_plan}
 * (ext NULL: 0), and the three entry points share one body: a parameter block gets the same answer through each of them.  A key that is
 * absent is 0; every key so far is a switch.  wcqp_tick_create_opts returns WCQP_E_INVALID, before anything touches the device, for a NULL
 * params or out, n_opts < 0, a NULL opts with n_opts > 0, an unknown key, a key given twice and a value other than 0 / 1.
 * wcqp_tick_get_option reports the value the handle took (WCQP_E_INVALID for an unknown key or a NULL argument).
 *
 * WCQP_TICK_OPT_RESIDENT_PLAN: wcqp_tick_params_ext.resident_plan, above.
 *
 * WCQP_TICK_OPT_POSITION_STREAMED = 1: ik_mode = WCQP_TICK_IK_POSITION on a STREAMED handle - the position tick closed on the measured
 * robot (the reference closes both of its IK paths on getFeedbacks / updateFKSolver / evaluateCoM, DCM, ZMP, WM/src/WalkingModule.cpp:546-575).
 * The caller's order per tick is the streamed handle's: wcqp_tick_set_desired_* or wcqp_tick_set_desired_from_plan, then
 * wcqp_tick_set_feedback_* or wcqp_tick_set_sensor_feedback_*, then wcqp_tick_run(h, 1, ...).  Tick t then
 *   1. runs the chain exactly as the streamed velocity tick runs it, on the measured DCM, CoM and ZMP and on the robot's live record: the
 *      MPC or the reactive law, gain scheduling where set, the ZMP-CoM law, the hull rows of the robot's own set on a change of contact pair;
 *   2. forms the targets of the POSITION mode (wcqp_tick_params.ik_mode) from the live record: both soles, (p_star x, p_star y, the
 *      record's CoM height), RotZ(meanYaw) * neck_additional_rotation;
 *   3. solves the non-linear IK of wcqp_prepare_* from q_des of tick t - 1 (tick 0: the uploaded q0), clipped into the limits, within
 *      position_ik.max_iter iterations;
 *   4. WCQP_STATUS_SOLVED: q_des takes the optimum.  Any other status: ik_fail counts the tick, q_des keeps its value and the robot is
 *      stopped, as on the planned POSITION handle.
 * The hot start is the previous RESULT, not the encoders - the reference's own rule (m_guess = m_qResult,
 * WM/src/WalkingInverseKinematics.cpp:389, 421); setFullModelFeedBack only places joints that are not optimised, and all dof joints are:
 * q_meas is validated as on every EXTERNAL handle (a non-finite value rejects the robot) but the IK does not read it.  A robot rejected by
 * either feedback form or by wcqp_tick_set_desired_device is stopped like a robot whose IK failed: its ik_fail and feedback_fail are those
 * of a streamed VELOCITY handle given the same stages and the same feed.  The deviations of the POSITION mode carry over (the anchor foot,
 * the neck target, the twists and the CoM-height velocity of the record are not read).  wcqp_tick_download gives q_log, ik_iters,
 * measured and feedback_fail (dq_log: WCQP_E_UNSUPPORTED).
 * The option needs, WCQP_E_UNSUPPORTED otherwise and before anything touches the device: ik_mode = POSITION; streamed_trajectories = 1
 * (hence plant = EXTERNAL); use_kinematics with the FUSED hand-off; the default IK algorithm; logger_ticks = 0; with the MPC a horizon
 * below 56, as on every streamed handle.  Every position_ik check applies unchanged.  It combines with WCQP_TICK_OPT_RESIDENT_PLAN = 1.
 * WITHOUT the option POSITION with streamed_trajectories or the EXTERNAL plant stays WCQP_E_UNSUPPORTED through all three entry points. */
typedef struct wcqp_tick_option {
    int32_t key;                   /* WCQP_TICK_OPT_* */
    int32_t value;
} wcqp_tick_option;
#define WCQP_TICK_OPT_RESIDENT_PLAN      1   /* = wcqp_tick_params_ext.resident_plan */
#define WCQP_TICK_OPT_POSITION_STREAMED  2   /* 1: ik_mode POSITION on a streamed (EXTERNAL) handle */
#define WCQP_TICK_OPT_PLAN_TIMED         3   /* REPORTED ONLY (wcqp_tick_get_option; wcqp_tick_create_opts refuses it as an unknown key): 1 while the plan in
                                              * place came from wcqp_tick_upload_footsteps_timed (per-step timings), 0 otherwise.  wcqp_tick_info_ext is
                                              * closed like the structs before it, so the flag travels by key */
#define WCQP_TICK_OPT_PLAN_SHIFT         4   /* REPORTED ONLY, like WCQP_TICK_OPT_PLAN_TIMED: the stages wcqp_tick_rebase_plan has taken since the last upload,
                                              * summed (0 after every upload; saturates at INT32_MAX) */
#define WCQP_TICK_OPT_SWING_PROFILE      5   /* REPORTED ONLY, like WCQP_TICK_OPT_PLAN_TIMED: 1 while the plan in force was generated with a non-zero
                                              * swing profile (wcqp_tick_set_swing_profile, below), 0 otherwise */
int wcqp_tick_create_opts(const wcqp_tick_params* params, const wcqp_tick_option* opts, int32_t n_opts, wcqp_tick_t* out);
int wcqp_tick_get_option(wcqp_tick_t h, int32_t key, int32_t* value);
int wcqp_tick_destroy(wcqp_tick_t h);
/* also rewinds to tick 0.  Non-finite inputs: WCQP_E_INVALID, before anything of the handle changes, for a NaN or an Inf in ref_traj,
 * dcm_vel_traj (where it is read), dcm0, com0, u_init or q0 - of any robot: such a value would enter that robot's state on the first tick
 * and never leave.  wcqp_tick_splice_reference refuses a non-finite ref_tail the same way. */
int wcqp_tick_upload(wcqp_tick_t h, const wcqp_tick_inputs* in);
/* Planned trajectories generated on the device from footsteps.  wcqp_tick_upload_footsteps is wcqp_tick_upload for a handle with
 * planned_trajectories whose stages the device expands itself, from a few footsteps per robot: it fills the arrays the classic upload
 * fills (records, DCM reference and velocity, support-polygon sets), rewinds to tick 0 and resets what an upload resets.  The planner
 * library upstream is not part of the reference: like the minimum-jerk smoother and the low-pass filters, THE PLAN IS THIS BUILD'S OWN
 * DEFINITION, stated here (tests/helpers/footstep_plan.py restates it in numpy; synth.synth_planned_walk_batch is a special case).
 *   dT = mpc.sampling_time, omega = sqrt(gravity / com_height), T = max_ticks + N + 1 stages.
 *   Timeline  stages [0, first_ds) are double support; step k occupies the next ss + ds stages - ss of single support, then ds of double
 *             support - the last step's double support lasting final_ds stages instead; after that the robot stands.
 *   Swing     at stage s of the single support, x = (s + 1) / ss, m = 10 x^3 - 15 x^4 + 6 x^5, m' = 30 x^2 (1 - x)^2:
 *             position = p + (target - p) m + lift 16 x^2 (1 - x)^2 z (the target's z is the foot's own), rotation = Rz(dyaw m) R,
 *             twist = the analytic derivative / (ss dT), angular part about z only.  The foot lands on the last single-support stage;
 *             its footprint from the next stage on is exactly the target with rotation Rz(dyaw) R.  A foot may swing twice in a row.
 *   Flags     bits 0 / 1: left / right in contact; bit 2: the left foot is the fixed frame - the stance foot of the latest single
 *             support, the left one before the first.
 *   ZMP       single support: the stance foot's point p_xy + R_2x2 delta.  Double support of n stages, stage u (0-based):
 *             a + (u + 1) / (n + 1) (b - a), a the previous stance foot's point (the midpoint of both feet's points before the first
 *             step), b the next stance foot's (the midpoint after the last step).  Standing: the midpoint.
 *   DCM       xi_t = (xi_{t+1} - (1 - a) zmp_t) / a, a = exp(omega dT), backwards from xi = zmp at the first standing stage - over the
 *             whole plan, also where it ends past T (a plan cut off by T is simply truncated); dcm_vel = omega (xi - zmp).
 *   Height    state0[68], velocity 0 (with a swing profile: THE SHAPED SWING, below, which also shapes the swing foot).  The desired neck orientation is derived per tick, as in every planned handle.
 *   Sets      the support-polygon rows by the rule of the classic upload: one set at stage 0 and one at every change of contact pair at
 *             a stage <= max_ticks, built from that stage's desired feet and foot_rect; later stages name the last set.
 * From `in` it reads state0 (the initial footprints are its desired-foot entries 24..47, the CoM height entry 68), q0, com0 and -
 * optionally - dcm0 and u_init (NULL: the generated DCM reference and ZMP of stage 0); every trajectory pointer is ignored and may be NULL.
 * WCQP_E_UNSUPPORTED on a handle without planned_trajectories.  WCQP_E_INVALID, with the handle unchanged (a handle uploaded before keeps
 * that upload), for a NULL required pointer, n_steps outside 0..K, a side other than 0 / 1, a non-finite value (of a step the robot
 * takes, of the state0 entries read, q0, com0, dcm0, u_init, lift or the deltas), a tick count below 1 or final_ds_ticks below 0.
 * The call always rewinds to tick 0; wcqp_tick_replan_footsteps below regenerates a running plan from a later stage.  In this call step
 * timings are common to the batch and to all steps (per-step timings: wcqp_tick_upload_footsteps_timed, below).  Not offered, and
 * refused by construction rather than silently ignored: device-pointer footsteps (of a running walk, wcqp_tick_replan_goals plans the
 * footsteps on the device and keeps them there). */
typedef struct wcqp_tick_footsteps {      /* HOST pointers, copied at the call */
    int32_t max_steps;                    /* K: row length of the per-step arrays, >= 0 */
    const int32_t* n_steps;               /* [B] 0..K steps robot i takes */
    const uint8_t* side;                  /* [B][K] foot that swings in step k: 0 left, 1 right */
    const double*  target;                /* [B][K][3] x, y of the sole's new footprint (world), yaw INCREMENT of the foot [rad] */
    int32_t first_ds_ticks, ss_ticks, ds_ticks, final_ds_ticks;   /* stages; final_ds_ticks 0 -> ds_ticks */
    double  lift;                         /* apex height of the swing foot [m] */
    double  zmp_delta_left[2], zmp_delta_right[2];   /* plannerParams.ini leftZMPDelta / rightZMPDelta, foot frame */
} wcqp_tick_footsteps;
int wcqp_tick_upload_footsteps(wcqp_tick_t h, const wcqp_tick_inputs* in, const wcqp_tick_footsteps* steps);
/* A new goal for a walk that is running (WalkingModule::setPlannerInput / askNewTrajectories / updateTrajectories,
 * WM/src/WalkingModule.cpp:1059-1145, 1263-1308: the planner restarts at a merge point inside a double support from the old trajectory's DCM
 * there, and everything from the merge point on is replaced).  Robot i's generated plan is regenerated on the device from stage M_i =
 * merge_stage[i] on, from new footsteps; a robot with merge_stage -1 keeps its plan, and none of its rows is read.  ss_ticks, ds_ticks,
 * final_ds_ticks, lift and the ZMP deltas are those of the handle's last wcqp_tick_upload_footsteps (the reference's planner parameters
 * are fixed for a run too).  THE REPLANNED PLAN, this build's own definition as the one above (tests/helpers/footstep_replan.py restates it):
 *   Below M_i   every stage of robot i stays bit for bit: records, ref_traj, dcm_vel, and the support-polygon sets those stages name.
 *   Footprints  the two desired sole poses of the current plan's record M_i - a stage with both feet in contact.
 *   Timeline    stages [M_i, M_i + first_ds_ticks) are double support; from there on timeline, swing, flags, ZMP of single and double supports,
 *               height and neck follow the rules above with stage 0 moved to M_i.
 *   Fixed frame before the new plan's first single support (for n_steps = 0: everywhere) bit 2 keeps the value of stage M_i - 1.
 *   DCM         the backward recursion above, from the new plan's first standing stage down to M_i + first_ds_ticks, where its value is X.
 *               The first double support's ZMP is z_u = a + (u + 1) / (n + 1) (b - a), n = first_ds_ticks, b the first new stance foot's point
 *               (n_steps = 0: the midpoint of both feet's points) and a - per axis - the point for which the recursion arrives at xi_{M_i} = the
 *               old plan's ref_traj[M_i] (the reference's setDCMInitialState, for the position): with q = exp(-omega dT),
 *               S0 = sum_{j=1..n} q^j, S1 = sum_{j=1..n} j q^j / (n + 1):   xi_{M_i} = X q^n + (exp(omega dT) - 1) (a (S0 - S1) + b S1).
 *               dcm_vel = omega (xi - zmp) as above.  DEVIATION: the reference also hands the planner the old DCM VELOCITY at the merge
 *               point; here the velocity at M_i follows from a and is not matched.
 *   Sets        the classic rule on the stitched plan: stage M_i changes no contact pair, so the records from M_i to the next change name the
 *               robot's last surviving set (the last one of a stage <= M_i); every later change of pair at a stage <= max_ticks gets a set
 *               built from that stage's feet.
 * Enqueue-only, like wcqp_tick_splice_reference: the HOST arrays are staged into device memory of the handle before the call returns, the
 * kernels run on `stream` behind the ticks already enqueued; no counter, state record, filter or tick index changes, no pointer a tick or
 * a captured graph holds moves, and no set a stage below M_i names is rewritten.  Valid between wcqp_tick_run calls.
 * WCQP_E_UNSUPPORTED on a handle without planned_trajectories, or whose plan was not generated (wcqp_tick_info.plan_generated = 0: such a
 * plan has no known timeline).  WCQP_E_INVALID - checked on the host before anything changes, the handle exactly as it was - for a handle
 * that is not uploaded, a NULL pointer, first_ds_ticks < 1, and for a robot that replans: n_steps outside 0..K', a side above 1 or a
 * non-finite target of a step it takes, M_i = 0 or < -1, M_i < the ticks enqueued so far (within one wcqp_tick_run call the kernel reads a
 * stage ahead, between calls nothing is ahead), M_i >= T, M_i below the stage its current plan was generated from, or a stage M_i that
 * lies in a single support of its current plan; also for a robot whose support-polygon set slots cannot take the new plan's sets - two
 * per step that starts at a stage <= max_ticks -, which happens only after wcqp_tick_restart_robots calls (each takes a slot with no
 * step behind it) and until wcqp_tick_rebase_plan frees the slots of past stages.  WCQP_E_UNSUPPORTED on a TIMED plan (wcqp_tick_replan_footsteps_timed, below, replans
 * those).  Not offered: replanning a classically uploaded plan, device pointers (the goal form below, wcqp_tick_replan_goals, keeps the
 * footsteps on the device: they are planned there and never visit the host). */
typedef struct wcqp_tick_replan {         /* HOST pointers, copied before the call returns */
    const int32_t* merge_stage;           /* [B] M_i >= 1: robot i's plan is regenerated from stage M_i on; -1: robot i keeps its plan */
    int32_t max_steps;                    /* K': row length of the per-step arrays, >= 0 */
    const int32_t* n_steps;               /* [B] 0..K' (0 = come to a stop) */
    const uint8_t* side;                  /* [B][K'] */
    const double*  target;                /* [B][K'][3] x, y, yaw increment */
    int32_t first_ds_ticks;               /* >= 1: stages of double support from M_i before the first new step */
} wcqp_tick_replan;
int wcqp_tick_replan_footsteps(wcqp_tick_t h, const wcqp_tick_replan* rp, void* stream);
/* A walk that outlasts max_ticks (WalkingModule::advanceReferenceSignals, WM/src/WalkingModule.cpp:35-..., called at :816, pops the front of
 * every trajectory deque and pushes the last element back, for as long as the module runs).  wcqp_tick_rebase_plan moves a GENERATED plan
 * and everything indexed by its stages R = shift stages towards 0 on the device: stage R becomes stage 0, the tick index goes down by R,
 * the robots' state is not touched, and ticks and replans go on as if nothing had happened - with R more ticks of room.
 * shift = WCQP_TICK_REBASE_AUTO: the largest even shift <= the ticks enqueued.  THE REBASED PLAN, with T stages
 * (tests/helpers/plan_rebase.py restates it on the windows wcqp_tick_get_plan returns):
 *   Stages [0, T - R)  of every robot are the old stages [R, T), bit for bit: record entries 0..38, ref_traj, dcm_vel, and the support-polygon
 *               rows a stage names, as wcqp_tick_get_plan returns them.
 *   Stages [T - R, T)  are copies of the old stage T - 1 (the reference's push-back of the last element).  The admission rule makes that a
 *               standing stage - twists 0, dcm_vel 0, ref_traj equal to its ZMP -, so the copy is what the generator would have produced there.
 *   Tick index  both device copies go down by R, and so does the host's count of enqueued ticks: wcqp_tick_run has R more ticks of room,
 *               merge stages and wcqp_tick_splice_reference's from_tick are stages of the REBASED plan.
 *   Plan in force  every robot's plan keeps its first double support, steps and durations; the stage it was generated from goes down by R
 *               and may become negative.  A pending wcqp_tick_replan_goals* is settled first (the rule below reads timelines).
 *   State       no state record, counter, filter, gain smoother, live hull row, hand-off record or joint array is read or written.
 *   Logs        u0_log, dq_log, q_log and the logger rows are indexed by the tick index, which this call rewinds: the ticks that follow
 *               write over rows R stages back.  A caller who wants the rows of the ticks so far downloads before rebasing.
 *   ZMP of stage 0  wcqp_tick_plan_window.u_init becomes the ZMP of the new stage 0, recovered from what the plan keeps of old stage R:
 *               ref_traj[R] - dcm_vel[R] / omega on a handle that keeps the DCM velocity (reactive controller, gain scheduling), else the
 *               recursion solved for it, (ref_traj[R + 1] - a ref_traj[R]) / (1 - a), a = exp(omega dT) - each operation rounded on its
 *               own.  It agrees with the generator's value to rounding, not bit for bit.
 *   Set slots   robot i owns slots [i cap, (i + 1) cap) of the row sets and entry 39 of a record names one.  With d_i = (entry 39 of the old
 *               record R) - i cap, the robot's rows in slots >= i cap + d_i move down by d_i and entry 39 of every record of the robot goes
 *               down by d_i: the sets of stages that are gone free their slots, so replans never run out of them.
 * Enqueue-only: two kernels on `stream` behind the ticks already enqueued, and one 4-byte row per robot (d_i) that travels back behind
 * an event of its own, which the next call that needs it waits for (as for the step counts of wcqp_tick_replan_goals).  No pointer a tick
 * or a captured graph holds moves.  On a handle with resident_plan a stage in hand (wcqp_tick_set_desired_from_plan) stays in hand.
 * Valid between wcqp_tick_run calls.  Everything is checked on the host before anything changes; a refused call leaves the handle as it was.
 * WCQP_E_UNSUPPORTED: a handle that holds no plan, or whose plan was not generated (wcqp_tick_info.plan_generated = 0: no known timeline);
 * plant = INTERNAL with noise != 0 (the disturbance is a hash of the tick index, and a rewound index would repeat its stream).
 * WCQP_E_INVALID: not uploaded; shift odd (the MPC -> IK hand-off record is addressed by the tick's parity), shift < 2 - also AUTO with
 * fewer than two ticks enqueued -, shift > the ticks enqueued; any robot whose plan in force does not STAND from a stage <= max_ticks
 * on, that is first_ds_ticks + its steps' durations (the last double support as the plan resolves it), counted from the stage the plan
 * was generated from, exceed max_ticks.  That rule guarantees that every change of contact pair of the plan has its row set - sets are
 * built for stages <= max_ticks only - and that stage T - 1 stands.  A robot on a plan cut off by T is first replanned to one that ends.
 * SIZING: max_ticks must hold the longest plan a robot is ever given from its merge stage to standing, plus the ticks between two
 * rebases: with plans of at most P stages, merged at most L stages ahead, and a rebase every E ticks, max_ticks >= E + L + P.
 * Not offered: rebasing a classically uploaded plan, per-robot shifts, a tick offset inside the kernels (noise, logs). */
#define WCQP_TICK_REBASE_AUTO (-1)
int wcqp_tick_rebase_plan(wcqp_tick_t h, int32_t shift, void* stream);
/* Stopped robots of a running fleet restarted per robot (the reference leaves that state per robot: stopWalking -> prepareRobot ->
 * startWalking, WM/src/WalkingModule.cpp).  A robot whose IK fails once is stopped for good - ik_fail[i] > 0, dq = 0 from then on - and
 * wcqp_tick_upload* rewinds EVERY robot of the handle.  wcqp_tick_restart_robots applies the upload's rules to the listed robots alone, at
 * the stage S the next tick will read (the ticks enqueued so far), on the device.  mode [B]: KEEP - the robot keeps state and plan, none
 * of its rows is read (they may hold NaN) -, ALWAYS, or IF_STOPPED - the DEVICE decides: the robot restarts iff ik_fail[i] > 0 when the
 * call's kernels run, behind the ticks already enqueued.  THE RESTARTED ROBOT (tests/helpers/plan_restart.py restates its plan on the
 * windows wcqp_tick_get_plan returns):
 *   Plan        stages below S stay bit for bit: records, ref_traj, dcm_vel and the row sets those stages name.  Every stage >= S is the
 *               same STANDING stage: both feet in contact, the fixed-frame bit = left, the two soles of state0 (entries 24..47), twists 0,
 *               CoM height state0[68] with velocity 0, ref_traj = the ZMP = the midpoint of the two feet's points p_xy + R_2x2 delta
 *               (zmp_delta_* of the upload; each operation rounded on its own), dcm_vel 0, and entry 39 names ONE new support-polygon
 *               set, built from these feet by the classic rule in the robot's next free slot.  A standing stage has no swing, so a swing
 *               profile in force changes nothing of it; timed and untimed plans alike.
 *   Plan in force  "generated from S, no steps": wcqp_tick_replan_footsteps* and wcqp_tick_replan_goals* with M_i >= S send the robot
 *               walking again (they read the soles of record M_i, as always), and wcqp_tick_rebase_plan admits it, because it stands.
 *   State       what wcqp_tick_upload_footsteps does for every robot, for this one: the MPC chain's records, the live hull rows marked
 *               unbuilt (the first tick builds them), the contact pair "both", the desired CoM height, the pose block (= the row of
 *               state0), q_des = q0, DCM = dcm0, CoM = com0 (and its references), measured ZMP and previous command = u_init, previous
 *               velocities 0, the gain smoother at rest at the stance gains, and mpc_fail, ik_fail, hot_try, hot_hit, the previous
 *               active set and (POSITION) ik_iters at 0.  dcm0 / u_init NULL: the standing stage's ZMP above, for every listed robot.
 *               NOT touched: the tick index (the robot goes on at tick S with the fleet: u0_log, dq_log, q_log rows below S stay), the
 *               logs, any other robot's row, any pointer a tick or a captured graph holds.  Between wcqp_tick_run calls nothing is ahead
 *               of anything: the next call primes its own first tick and rewrites the whole MPC -> IK hand-off record of parity S & 1.
 * Enqueue-only: the host rows of the LISTED robots are staged before the call returns (the block a replan stages through; a kept robot's
 * rows are not even copied), three kernels run on `stream` behind the ticks already enqueued, and one small row per listed robot -
 * restarted or not, and its ik_fail just before - travels back behind an event of its own.  With IF_STOPPED the host does not know who
 * restarted until then: the robot's plan in force is OWED, as a goal call owes step counts, and the next call that reads a timeline or a
 * slot count waits for THAT event first, nothing else.  A robot listed ALWAYS owes nothing.  Pending goal and rebase calls are settled
 * first.  Valid between wcqp_tick_run calls.  A call that lists no robot returns WCQP_OK and enqueues nothing.
 * Everything is checked on the host before anything changes; a refused call leaves the handle as it was.
 * WCQP_E_UNSUPPORTED: a handle that holds no plan; plant = EXTERNAL or a resident plan (the caller's plant is the state there); a plan that
 * was not generated (wcqp_tick_info.plan_generated = 0).  WCQP_E_INVALID: not uploaded; mode, state0, q0 or com0 NULL; a mode above 2; a
 * non-finite value in state0, q0, com0, dcm0 or u_init of a robot whose mode is not KEEP; S > max_ticks; a listed robot whose set slots
 * cannot take one more set (IF_STOPPED counts as if it restarted) - wcqp_tick_rebase_plan frees the slots of past stages.
 * SLOTS: a restart takes one of the robot's set slots with no step behind it, so it also takes room from the replans that follow: a
 * footstep or goal replan whose new sets would not fit returns WCQP_E_INVALID (see there) until a rebase.  cap has room for one step
 * more than can start within max_ticks, so a robot restarted over and over without a rebase between runs out.
 * Rows that never visit the host: wcqp_tick_recover_robots below runs the posture IK on the device and restarts from its result.
 * Not offered: a restart at a stage other than S, a per-robot tick index.  EXTERNAL and resident handles: wcqp_tick_reset_robots below. */
#define WCQP_TICK_RESTART_KEEP        0
#define WCQP_TICK_RESTART_ALWAYS      1
#define WCQP_TICK_RESTART_IF_STOPPED  2
typedef struct wcqp_tick_restart {        /* HOST pointers, staged before the call returns */
    const uint8_t* mode;                  /* [B] WCQP_TICK_RESTART_* */
    const double*  state0;                /* [B][87]: entries 24..47 (the two soles) and 68 (CoM height) make the plan, the row becomes the pose block */
    const double*  q0;                    /* [B][dof] */
    const double*  com0;                  /* [B][2] */
    const double*  dcm0;                  /* [B][2] or NULL: the standing stage's ZMP */
    const double*  u_init;                /* [B][2] or NULL: the same */
} wcqp_tick_restart;
int wcqp_tick_restart_robots(wcqp_tick_t h, const wcqp_tick_restart* r, void* stream);
typedef struct wcqp_tick_restart_result { /* HOST pointers, any may be NULL */
    uint8_t* restarted;                   /* [B] 1: the robot was restarted by the last call */
    int64_t* stopped_ticks;               /* [B] its ik_fail just before (0 if not restarted) */
    int32_t* stage;                       /* the stage S of the last call */
} wcqp_tick_restart_result;
int wcqp_tick_get_restart_result(wcqp_tick_t h, const wcqp_tick_restart_result* out);   /* waits for that call's event only */
/* Stopped robots stood up on the device: posture IK and restart in one enqueue-only call (the reference's Stopped -> prepareRobot ->
 * startWalking, WM/src/WalkingModule.cpp:882, 944-984, 1223, whose IK starts from the measured joints, :944).  wcqp_tick_restart_robots
 * takes the posture as host rows, so its caller downloads (to learn who stopped, and where their joints are), solves, and restarts: two
 * synchronisations.  wcqp_tick_recover_robots does the three steps on the device, on `stream`, behind the ticks already enqueued; the
 * posture never visits the host.  S is the stage the next tick reads, as for a restart.  THE RECOVERED ROBOT - a listed robot (mode is not
 * KEEP; tests/helpers/plan_recover.py restates the targets and the host composition the call equals):
 *   Decision    ALWAYS: the robot goes on.  IF_STOPPED: it goes on iff ik_fail[i] > 0 when the call's kernels run; otherwise its status is
 *               WCQP_RECOVER_NOT_STOPPED.  With soles taken from the plan (left_d and right_d NULL) a robot that would go on does so only
 *               if bits 0 and 1 of record S's flags are both set - a double support or standing: both soles lie on the ground at landed
 *               poses -; otherwise its status is WCQP_RECOVER_NOT_STANDING.  A robot that does not go on is not touched and costs no IK
 *               iteration.
 *   Posture     the problem and iteration of wcqp_prepare_solve_* with `prepare`'s parameters.  left_d / right_d: the caller's rows, or
 *               the left and right sole of record S.  com_d: the caller's row, or x, y = the midpoint of the two feet's ZMP points
 *               p_xy + R_2x2 delta of THESE soles (zmp_delta_* of the upload, each operation rounded on its own: the ZMP of THE RESTARTED
 *               ROBOT's standing stage) and z = the CoM height of record S.  Rd_neck: the caller's row, or no neck target.  q_guess: the
 *               caller's row, or the robot's q_des as the device holds it when the kernels run - the joints it stopped at.  The rows q,
 *               state, status, iters, residual are bit for bit what wcqp_prepare_solve_host returns for these inputs: the same kernel runs,
 *               over the rows of the robots that go on alone.
 *   Restart     a robot whose IK ended WCQP_STATUS_SOLVED is THE RESTARTED ROBOT of wcqp_tick_restart_robots, bit for bit, with
 *               state0 = the pose block of the IK, q0 = its q, com0 = entries 66, 67 of that block (the CoM at the solved posture), and
 *               dcm0 / u_init as given: the same kernels and the same set builder produce it.  Any other status leaves the robot exactly
 *               as it was: state, plan, and an ik_fail that keeps counting.
 * Every listed robot is decided by the device - ALWAYS too: the SOLVED gate applies to it -, so every listed robot's plan in force is OWED
 * as an IF_STOPPED robot's of a restart call is: one result row per listed robot comes back behind an event of the call's own, and the
 * next call that reads a timeline or a slot count waits for that event first.  Slots are counted as if every listed robot restarted.  A
 * recover call is the handle's last restart call: wcqp_tick_get_restart_result reports its restarted / stopped_ticks / stage too.
 * Pending goal, rebase and restart calls are settled first.  Valid between wcqp_tick_run calls.  A call that lists nobody returns WCQP_OK
 * and enqueues nothing.  The host rows of the LISTED robots are staged before the call returns.  (The first solve of a wcqp_prepare_t,
 * here or in wcqp_prepare_solve_*, copies its tables to the device and waits for that copy alone.)
 * Everything is checked on the host before anything changes; a refused call leaves the handle and the last result as they were.
 * WCQP_E_UNSUPPORTED: exactly where wcqp_tick_restart_robots returns it.  WCQP_E_INVALID: as for a restart - not uploaded, mode NULL, a
 * mode above 2, S > max_ticks, a listed robot without a free set slot -, and: `prepare` or the struct NULL; exactly one of left_d /
 * right_d NULL; a `prepare` whose model table is not byte for byte that of the handle's kinematics (or a handle without kinematics); a
 * non-finite value in a given left_d, right_d, com_d, Rd_neck, q_guess, dcm0 or u_init row of a listed robot - rows of KEPT robots are
 * never read and may hold NaN.
 * wcqp_tick_get_recover_result: WCQP_E_INVALID before any recover call, and when the handle's last restart call was not one.
 * Not offered: a restart at a stage other than S, a per-robot tick index.  EXTERNAL and resident handles: wcqp_tick_reset_robots below. */
#define WCQP_RECOVER_KEPT          (-1)   /* mode KEEP: not listed                                          */
#define WCQP_RECOVER_NOT_STOPPED   (-2)   /* IF_STOPPED and ik_fail == 0 when the call's kernels ran         */
#define WCQP_RECOVER_NOT_STANDING  (-3)   /* soles from the plan, and record S is not a double support       */
typedef struct wcqp_tick_recover {        /* HOST pointers, staged before the call returns */
    const uint8_t* mode;      /* [B] WCQP_TICK_RESTART_KEEP / _ALWAYS / _IF_STOPPED, as wcqp_tick_restart.mode      */
    const double*  left_d;    /* [B][12] p 3 | R 9, the anchor; NULL together with right_d: the soles of plan record S */
    const double*  right_d;   /* [B][12]                                                                           */
    const double*  com_d;     /* [B][3] or NULL: x, y = the standing ZMP of these soles, z = the CoM height of record S */
    const double*  Rd_neck;   /* [B][9] or NULL: no neck target                                                    */
    const double*  q_guess;   /* [B][dof] or NULL: the robot's own joints on the device (q_des), read by the call's kernels */
    const double*  dcm0;      /* [B][2] or NULL, as wcqp_tick_restart.dcm0                                          */
    const double*  u_init;    /* [B][2] or NULL, as wcqp_tick_restart.u_init                                        */
} wcqp_tick_recover;
int wcqp_tick_recover_robots(wcqp_tick_t h, wcqp_prepare_t prepare, const wcqp_tick_recover* r, void* stream);
typedef struct wcqp_tick_recover_result { /* HOST pointers, any may be NULL */
    uint8_t* restarted; int64_t* stopped_ticks;  /* [B], as wcqp_tick_restart_result                       */
    int32_t* status;   /* [B] WCQP_STATUS_* of the robot's IK, or WCQP_RECOVER_*                            */
    int32_t* iters;    /* [B] 0 for a robot whose IK did not run                                            */
    double*  residual; /* [B][2] as wcqp_prepare_solve_*; 0 for a robot whose IK did not run                 */
    int32_t* stage;
} wcqp_tick_recover_result;
int wcqp_tick_get_recover_result(wcqp_tick_t h, const wcqp_tick_recover_result* out);  /* waits for that call's event only */
/* Robots of a sensor-fed fleet reset per robot: the caller's simulator put a robot back - it fell, or its episode ended -, and the
 * controller follows.  On a streamed EXTERNAL handle a robot stops for good after one rejected reading or stage, and wcqp_tick_upload*
 * rewinds every robot and synchronises the device.  wcqp_tick_reset_robots takes wcqp_tick_restart - mode, state0, q0, com0, dcm0, u_init,
 * HOST rows, KEEP / ALWAYS / IF_STOPPED as there - at the stage S the next tick reads (the ticks enqueued so far).  THE RESET ROBOT - a
 * listed robot that goes on (ALWAYS, or IF_STOPPED and ik_fail[i] > 0 when the call's kernels run; tests/helpers/tick_reset.py restates it):
 *   State       THE RESTARTED ROBOT's, written by the same kernel from the call's rows.  dcm0 / u_init NULL: the standing ZMP of the two
 *               soles of state0 with the restart's rounding rule (a handle without a resident plan knows no zmp_delta_*: the deltas are
 *               0 there, the ZMP is the midpoint of the two sole origins).
 *   EXTERNAL    the measured joints = q0; feedback_fail = 0; no stage and no contact pair in hand, as after an upload: the robot's next
 *               stage rebuilds or copies its support-polygon rows.  A REJECTED READING at tick S: the robot keeps (com0, dcm0, u_init)
 *               as its measured state and q0 as its measured joints, exactly as a robot rejected on tick 0 keeps the uploaded state, and
 *               is stopped and counted again.  THE RULE stays one: a robot rejected at tick t > 0 keeps the hand-off record of parity
 *               t - 1, and the call writes the three rows into that record (before any tick: into the rows wcqp_tick_download reports as
 *               `measured`, which therefore shows the reset rows when S = 0).
 *   Filters     (sensor filters on) the upload's rule for this robot: the CoM position filter at com0, its velocity filter at 0, and the
 *               joint-velocity and wrench filters start AT the robot's next accepted reading - a per-robot FRESH mark in the filter
 *               record, double-buffered with it: a second sensor call for the same tick starts from the same state, a rejected reading
 *               leaves the robot fresh, an accepted one clears the mark.  Every upload clears every mark.
 *   Plan        (resident_plan only) THE RESTARTED ROBOT's, word for word: stages below S bit for bit, every stage >= S the standing
 *               stage of state0's soles with one new set in the robot's next free slot, plan in force "generated from S, no steps" -
 *               the same fill kernel, set builder, slot accounting and owed bookkeeping.  Without a resident plan there is no plan
 *               part: the caller's next wcqp_tick_set_desired_* is the robot's stage.
 *   NOT touched the tick index, the logs below S, any other robot's row, any pointer a tick or a captured graph holds.
 * ORDER: the call comes first in tick S's sequence, reset_robots -> set_desired_* / set_desired_from_plan -> set_*feedback_* -> run(1); with
 * a stage or a feedback already in hand it returns WCQP_E_INVALID.  Enqueue-only on `stream`: the listed robots' rows are staged before it
 * returns, a kept robot's rows are never read.  The HOST forms of the stage and the feedback wait for the call's kernels, whatever the
 * stream.  Pending goal, rebase and restart calls are settled first; IF_STOPPED owes the plan in force as a restart does.  It is the
 * handle's last restart call: wcqp_tick_get_restart_result reports it, wcqp_tick_get_recover_result returns WCQP_E_INVALID after it.  A
 * call that lists nobody returns WCQP_OK and enqueues nothing.  Everything is checked on the host before anything changes.
 * WCQP_E_UNSUPPORTED: a handle that is not streamed (internal plant, planned handles, the synthetic-gait EXTERNAL handle); a POSITION handle;
 * a resident plan that was not generated.  WCQP_E_INVALID: not uploaded; the struct, mode, state0, q0 or com0 NULL; a mode above 2; a
 * non-finite value in a listed robot's rows; S > max_ticks; a stage or a feedback in hand; on a resident handle a listed robot without a
 * free set slot (wcqp_tick_rebase_plan frees the slots of past stages).
 * Not offered: wcqp_tick_recover_robots on these handles (the caller's plant holds the posture), POSITION streamed handles, a reset at a
 * stage other than S, soles taken from the measured feet. */
int wcqp_tick_reset_robots(wcqp_tick_t h, const wcqp_tick_restart* r, void* stream);
/* Per-step timings: every footstep carries its own durations (the reference's planner gives every step its own, between minStepDuration
 * and maxStepDuration; wcqp_unicycle_plan_timed_* below chooses them and fills exactly these two arrays).  THE TIMED PLAN is the plan
 * wcqp_tick_upload_footsteps defines (tests/helpers/footstep_plan_timed.py restates it), with four changes:
 *   - step k of robot i occupies ss[i][k] + ds[i][k] stages: ss of single support, then ds of double support;
 *   - the last step's double support lasts steps->final_ds_ticks stages if that is > 0, else ds[i][n - 1];
 *   - steps->ss_ticks / ds_ticks are ignored;
 *   - the swing phase is x = (s + 1) / ss_k, the twist is divided by ss_k dT, and a double support's ZMP ramp uses that step's own n.
 * Flags, fixed frame, ZMP points, the backward DCM recursion from the first standing stage, height and the set rule keep their wording.
 * THE TIMED REPLAN is the replanned plan above on the per-step timeline: "a single support of its current plan" refers to the plan in
 * force with its own durations, `tm` gives the NEW steps' durations, and the last step's double support again falls back to the
 * final_ds_ticks of the upload, or to its own ds.
 * A plan is timed or not from its upload on (wcqp_tick_get_option with WCQP_TICK_OPT_PLAN_TIMED): wcqp_tick_replan_footsteps on a timed plan and
 * wcqp_tick_replan_footsteps_timed on an untimed one return WCQP_E_UNSUPPORTED, and so does wcqp_tick_replan_goals on a timed plan (its
 * merge-point rule and planner kernel know one common timing: wcqp_tick_replan_goals_timed below is the call for a timed plan) - each
 * before anything changes.
 * wcqp_tick_get_plan, the POSITION tick and the resident plans of streamed handles take a timed plan as any other.
 * Refusals, on the host, with the handle unchanged: every refusal of the untimed call (its ss_ticks / ds_ticks rule aside), and
 * WCQP_E_INVALID for a NULL tm or a NULL pointer inside it (K > 0), ss < 1 or ds < 1 of a step the robot takes, or a timeline - of any
 * robot, the first double support and, in a replan, the T stages in front included - that passes 2^30 stages. */
typedef struct wcqp_tick_step_timing {   /* HOST pointers, copied at the call */
    const int32_t* ss_ticks;             /* [B][K] single-support stages of step k, >= 1 for a step the robot takes */
    const int32_t* ds_ticks;             /* [B][K] double-support stages behind step k, >= 1 */
} wcqp_tick_step_timing;
int wcqp_tick_upload_footsteps_timed(wcqp_tick_t h, const wcqp_tick_inputs* in, const wcqp_tick_footsteps* steps, const wcqp_tick_step_timing* tm);
int wcqp_tick_replan_footsteps_timed(wcqp_tick_t h, const wcqp_tick_replan* rp, const wcqp_tick_step_timing* tm, void* stream);
/* The shape of a step (plannerParams.ini footApexTime, stepLandingVelocity, pitchDelta, comHeightDelta, which the reference hands its
 * planner at WM/src/TrajectoryGenerator.cpp:94-111; the shipped set is 0.8, 0.0, 0.0 - in DEGREES there, radians here - and 0.01).
 * wcqp_tick_set_swing_profile stores a profile on the handle - host only, nothing is launched -; the next wcqp_tick_upload_footsteps or
 * wcqp_tick_upload_footsteps_timed copies it into the plan it generates, next to lift and the ZMP deltas, and every replan of that plan
 * (wcqp_tick_replan_footsteps*, wcqp_tick_replan_goals*) keeps it: the reference's planner parameters are fixed for a run too.  A later
 * wcqp_tick_set_swing_profile does not touch a running plan, nor does wcqp_tick_rebase_plan touch the profile.  An all-zero profile - and
 * a handle never given one - is THE PLAN above, bit for bit, by the same kernels.  THE SHAPED SWING, this build's own definition like
 * THE PLAN (tests/helpers/swing_profile.py restates it): step k with ss_k single-support stages, at stage u; x = (u + 1) / ss_k; m, m' the
 * plan's quintic; D = ss_k dT; r = apex_ratio; h(y) = 3 y^2 - 2 y^3.
 *   Shape     c0(x) and its derivative in x:  r = 0: 16 x^2 (1 - x)^2, as in THE PLAN;  r > 0 and x <= r: h(x / r);  r > 0 and x > r:
 *             1 - h(y), y = (x - r) / (1 - r).  C1 at x = r (both branches give 1 with slope 0 there).
 *   Height of the swing foot   z = p_z + lift c0(x) + landing_velocity (1 - r) D (y^3 - y^2), the last term for r > 0 and x > r only.
 *             Vertical twist = the analytic derivative in time, lift c0'(x) / D + landing_velocity (3 y^2 - 2 y).  At x = 1 - the landing
 *             stage - z = p_z and the vertical twist is exactly landing_velocity.  The landing term is C1 at x = r as well (y = 0).
 *             The descent is monotone if and only if |landing_velocity| (1 - r) D <= 3 lift.  That is NOT checked: durations chosen on
 *             the device (wcqp_tick_replan_goals_timed) are not known to the host.
 *   Pitch     theta = pitch_delta c0(x) about the foot's own y axis: rotation = Rz(dyaw m) R Ry(theta), angular twist (world frame) =
 *             z dyaw m' / D + (Rz(dyaw m) R)[:, 1] pitch_delta c0'(x) / D.  theta = 0 at x = 1: the footprint from the next stage on is
 *             still exactly the target.
 *   CoM height  in a single-support stage: com_height = h0 + com_height_delta 16 x^2 (1 - x)^2, com_height_vel = its derivative / D; in
 *             every other stage h0 and 0.  h0 = state0[68] in an upload, the handle's constant height in a replan; merge stages lie in
 *             double supports, where the bump is 0, so a replanned plan stays continuous.
 *   Unchanged   the swing foot's x, y and yaw increment, flags, ZMP, DCM reference and velocity, the timeline, the support-polygon sets (built
 *             at changes of contact pair, where the landing foot has theta = 0 and z = p_z) and the rules of wcqp_tick_replan_* and
 *             wcqp_tick_rebase_plan (the stage T - 1 it copies stands, so its height is h0).
 * wcqp_tick_get_swing_profile returns the profile of the plan IN FORCE (all zero without a generated plan), not the pending one;
 * wcqp_tick_get_option(WCQP_TICK_OPT_SWING_PROFILE) says whether it is non-zero.
 * Refusals, on the host, the handle unchanged: WCQP_E_UNSUPPORTED on a handle that holds no plan (neither planned_trajectories nor
 * resident_plan).  WCQP_E_INVALID for a NULL pointer, a non-finite value, apex_ratio < 0 or >= 1, landing_velocity > 0,
 * landing_velocity != 0 with apex_ratio = 0 (the quartic has no landing branch), |pitch_delta| > pi / 4.
 * Not offered: useMinimumJerkFootTrajectory (x and y already follow the quintic), per-robot profiles, changing the profile of a running
 * plan, a natural frequency that follows the CoM height (the reference keeps omega constant too). */
typedef struct wcqp_tick_swing_profile {
    double apex_ratio;        /* footApexTime: 0 = the symmetric quartic of THE PLAN; else in (0, 1) */
    double landing_velocity;  /* stepLandingVelocity [m/s]: <= 0; != 0 needs apex_ratio > 0 */
    double pitch_delta;       /* pitchDelta, RADIANS here: |.| <= pi / 4 */
    double com_height_delta;  /* comHeightDelta [m] */
} wcqp_tick_swing_profile;
int wcqp_tick_set_swing_profile(wcqp_tick_t h, const wcqp_tick_swing_profile* p);      /* host only, nothing launched */
int wcqp_tick_get_swing_profile(wcqp_tick_t h, wcqp_tick_swing_profile* out);          /* the one of the plan in force */

typedef struct wcqp_unicycle_s* wcqp_unicycle_t;       /* the unicycle planner's handle, stated at the end of this header */

/* "Robot i, go there" for a walk that is running, on the device and enqueue-only: the reference's setGoal(x, y) -
 * WalkingModule::setPlannerInput, askNewTrajectories and updateTrajectories (WM/src/WalkingModule.cpp:500-535, 1059-1145, 1263-1308).
 * For every robot that replans, ONE kernel (goal_plan_kernel) plans footsteps with the unicycle planner stated below from the two
 * desired soles of plan record M_i towards goal[i]; the three kernels of wcqp_tick_replan_footsteps then regenerate the plan from M_i
 * from those footsteps - THE REPLANNED PLAN is the one defined above, with K' = the planner's max_steps -, the set builder follows, and
 * one copy brings the result rows back into pinned memory of the handle, with an event behind it.  All of it is enqueued on `stream`
 * behind the ticks already enqueued; the call synchronises with nothing but the previous replan's hold on the handle's staging block,
 * and the footsteps never visit the host.  `planner` is read at the call only.  Valid between wcqp_tick_run calls, on every handle
 * that holds a generated plan: planned handles, the POSITION tick, resident plans of streamed handles.
 *   Merge stage  merge_stage[i] = WCQP_TICK_MERGE_KEEP: robot i keeps its plan, none of its rows is read (its goal may be a NaN).
 *               M_i >= 1: taken as given and checked exactly as wcqp_tick_replan_footsteps checks it.  WCQP_TICK_MERGE_AUTO: with the plan in
 *               force of robot i generated from stage O with a first double support of fo stages and n steps, per = ss + ds, step k's
 *               single support starts at s_k = O + fo + k per; the plan's MERGE POINTS are s_k + ss for k = 0 .. n - 2 - the first stage of
 *               each inner double support - and every stage >= L, L = s_{n-1} + ss (n = 0: L = O): the last double support and standing.
 *               t0 = the ticks enqueued so far, plus 1 when a resident plan's stage has been staged (the term of the replan rule).
 *               M_i = the smallest merge point >= max(t0 + min_lead_ticks, 1, O).  M_i >= T: the robot keeps its plan, status
 *               WCQP_GOAL_TOO_LATE.  (csrc/goal_merge.h is the rule, tests/helpers/goal_merge.py restates it.)
 *               This is the three-way rule of setPlannerInput (WalkingModule.cpp:1263-1308), whose merge points are the same stages
 *               counted from the current tick, with a lead of 20: the front merge point if it is > 20 ticks away; with the front one <= 20
 *               and more than one merge point, the second; otherwise 20 ticks on.  The two rules coincide while per > min_lead_ticks: the
 *               second merge point is per stages behind the first and so beyond the lead, and "otherwise" is the last double support or
 *               standing, where every stage is a merge point here.  They differ for per <= min_lead_ticks: the reference then takes the
 *               second merge point although it is nearer than the lead, this rule goes on to the first one the lead allows.  They also
 *               differ by one stage at the boundary (a merge point exactly min_lead_ticks away is taken here, passed over there).
 *   First side   first_side[i] = 0 / 1: the foot that swings first.  WCQP_TICK_SIDE_AUTO: the fixed-frame foot of record M_i - 1 - bit 2 of its
 *               flags set: the left foot, 0; clear: the right, 1 - and the feet keep alternating across the merge, the reference's
 *               askNewTrajectories(..., !m_isLeftFixedFrame.front(), ...).  The host keeps no sides: the kernel reads the record.
 *   Degenerate   a robot whose desired point overflows ends WCQP_UNICYCLE_INVALID_INPUT on the device (the host cannot see it: the soles
 *               are there): it regenerates with n_steps = 0 and comes to a stop at M_i.  WCQP_UNICYCLE_STUCK and _TRUNCATED keep the steps
 *               found so far, as the host composition of plan_host and wcqp_tick_replan_footsteps does.
 * Refusals, all checked on the host before anything changes, the handle exactly as it was: WCQP_E_UNSUPPORTED as
 * wcqp_tick_replan_footsteps (no planned_trajectories or resident plan, a plan that was not generated); WCQP_E_INVALID for a NULL handle,
 * planner, struct or goal, a handle that is not uploaded, first_ds_ticks < 1, min_lead_ticks < 0, and for a robot that does not KEEP: a
 * merge_stage below -2 or an explicit one that breaks the rules of wcqp_tick_replan_footsteps, a first_side other than 0, 1 or 255, a
 * non-finite goal; also for a robot whose set slots cannot take the sets of the steps the device MAY choose - two for each of at most K
 * steps that can start at a stage <= max_ticks, the first at M_i + first_ds_ticks, the others ss + ds stages apart (a timed plan:
 * min_step_ticks) - which, as for wcqp_tick_replan_footsteps, happens only to a robot that spent slots on wcqp_tick_restart_robots
 * calls since the last rebase.  Every robot KEEP or TOO_LATE: WCQP_OK, nothing enqueued.
 * The step count of a goal-replanned robot is known to the host only when the rows are back: every later call that needs it
 * (wcqp_tick_replan_footsteps, wcqp_tick_replan_goals, wcqp_tick_get_goal_result) first waits for THAT call's event, nothing else. */
#define WCQP_TICK_MERGE_KEEP  (-1)   /* robot keeps its plan; none of its rows is read */
#define WCQP_TICK_MERGE_AUTO  (-2)   /* the rule above chooses M_i                      */
#define WCQP_TICK_SIDE_AUTO   255    /* the fixed-frame foot of stage M_i - 1 swings first */
#define WCQP_GOAL_KEPT        (-1)   /* status of a robot that was not asked to replan  */
#define WCQP_GOAL_TOO_LATE    (-2)   /* AUTO found no merge stage below T: plan kept    */
typedef struct wcqp_tick_goals {     /* HOST pointers, copied before the call returns */
    const double*  goal;             /* [B][2], the argument of setGoal, unicycle frame   */
    const int32_t* merge_stage;      /* [B] KEEP / AUTO / M_i >= 1; NULL = AUTO for all   */
    const uint8_t* first_side;       /* [B] 0 / 1 / SIDE_AUTO;      NULL = SIDE_AUTO for all */
    int32_t first_ds_ticks;          /* >= 1, as wcqp_tick_replan.first_ds_ticks          */
    int32_t min_lead_ticks;          /* AUTO only, >= 0; the reference's 20               */
} wcqp_tick_goals;
int wcqp_tick_replan_goals(wcqp_tick_t h, wcqp_unicycle_t planner, const wcqp_tick_goals* g, void* stream);
/* What the last wcqp_tick_replan_goals call decided and planned: waits for that call's event only (not for the stream, not for the
 * device).  merge_stage, first_side and status are the values TAKEN; status is the planner's WCQP_UNICYCLE_* for a robot that
 * replanned, WCQP_GOAL_KEPT / WCQP_GOAL_TOO_LATE for one that did not, and every row of such a robot is zero.  K' = the max_steps of
 * the planner of that call.  WCQP_E_INVALID for a NULL handle or struct, or before any such call. */
typedef struct wcqp_tick_goal_result { /* HOST pointers, any may be NULL; rows of KEPT / TOO_LATE robots zero */
    int32_t* merge_stage; uint8_t* first_side; int32_t* status;    /* [B] the values TAKEN; status: WCQP_UNICYCLE_* or WCQP_GOAL_* */
    int32_t* n_steps; uint8_t* side; double* target;               /* [B], [B][K'], [B][K'][3], K' = the planner's max_steps */
    double* desired_point; double* unicycle_end;                   /* [B][2], [B][3] */
} wcqp_tick_goal_result;
int wcqp_tick_get_goal_result(wcqp_tick_t h, const wcqp_tick_goal_result* out);   /* waits for the last replan_goals call only */
/* The same for a TIMED plan (wcqp_tick_upload_footsteps_timed): wcqp_tick_replan_goals on the per-step timeline, with the same
 * wcqp_tick_goals - KEEP / AUTO / explicit M_i, first_side 0 / 1 / WCQP_TICK_SIDE_AUTO, first_ds_ticks, min_lead_ticks.  ONE kernel
 * (goal_plan_timed_kernel) runs the timed planner of wcqp_unicycle_plan_timed_* (the same `tm`; the planner's step_ticks is not read) from
 * the two desired soles of plan record M_i: it plans every listed robot's steps AND their durations; the three timed replan kernels then
 * regenerate the plan from those rows - THE TIMED REPLAN as wcqp_tick_replan_footsteps_timed defines it, with K' = the planner's
 * max_steps -, the set builder follows, and one copy brings the result rows, the two duration rows among them, back into the handle's
 * pinned block with an event behind it.  Enqueued on `stream` behind the ticks already enqueued; nothing is waited for but the previous
 * replan's hold on the staging block; neither footsteps nor durations visit the host.  Valid wherever the untimed call is.
 *   Merge stage  as above on robot i's own timeline: s_0 = O + fo, s_{k+1} = s_k + ss_k + ds_k with the durations of its plan in force; the
 *               MERGE POINTS are s_k + ss_k for k = 0 .. n - 2 and every stage >= L = s_{n-1} + ss_{n-1} (n = 0: L = O); M_i = the smallest
 *               merge point >= max(t0 + min_lead_ticks, 1, O); M_i >= T: WCQP_GOAL_TOO_LATE.  With equal durations this is the untimed
 *               rule.  An explicit M_i is checked exactly as wcqp_tick_replan_footsteps_timed checks it.  (csrc/goal_merge.h is the
 *               rule, tests/helpers/goal_merge_timed.py restates it.)
 *   Degenerate   as above: WCQP_UNICYCLE_INVALID_INPUT found on the device gives n_steps = 0 and a stop at M_i; WCQP_UNICYCLE_STUCK and
 *               _TRUNCATED keep the steps found so far, with their durations.
 * Refusals, all on the host before anything changes, the handle exactly as it was: every refusal of wcqp_tick_replan_goals;
 * WCQP_E_UNSUPPORTED on an untimed plan (a plan is timed or not from its upload on); WCQP_E_INVALID for a NULL tm, for a tm that
 * wcqp_unicycle_plan_timed_device refuses, and when T + first_ds_ticks + K' max_step_ticks + final_ds passes 2^30 stages (a step of m
 * ticks has ds <= m - 1, so a final_ds of 0 is covered).  Every robot KEEP or TOO_LATE: WCQP_OK, nothing enqueued.
 * Both the step count and the durations of a goal-replanned robot are known to the host only when the rows are back: every later call
 * that needs them (the replans, the result getters) first waits for THAT call's event, nothing else.
 * wcqp_tick_get_goal_result works after this call exactly as after the untimed one (wcqp_tick_goal_result keeps its fields: callers
 * pass it with their own sizeof); the durations come through wcqp_tick_get_goal_timing: ss_ticks / ds_ticks [B][K'] (HOST pointers,
 * either may be NULL), zero for KEPT / TOO_LATE robots and for steps not taken.  It waits for that call's event only, and returns
 * WCQP_E_INVALID for a NULL handle, before any goal call, or when the last goal call was the untimed one. */
struct wcqp_unicycle_timing;        /* the timed planner's candidates and score, stated at the end of this header */
int wcqp_tick_replan_goals_timed(wcqp_tick_t h, wcqp_unicycle_t planner, const struct wcqp_unicycle_timing* tm,
                                 const wcqp_tick_goals* g, void* stream);
int wcqp_tick_get_goal_timing(wcqp_tick_t h, int32_t* ss_ticks, int32_t* ds_ticks);   /* [B][K'] each, either may be NULL */
/* The plan a planned handle holds, however it was uploaded: n robots from robot0, m stages from stage0, stage-major per robot.
 * Synchronises.  Every pointer but two works on any planned handle, however it was uploaded.  The two: a non-NULL dcm_vel_traj makes
 * the call return WCQP_E_UNSUPPORTED on a handle that keeps no velocity (neither the reactive controller nor gain scheduling), and a
 * non-NULL u_init - this pointer alone - makes it return WCQP_E_UNSUPPORTED on a handle whose plan was uploaded with wcqp_tick_upload
 * (wcqp_tick_info.plan_generated says which).  WCQP_E_UNSUPPORTED also on a handle without planned_trajectories; WCQP_E_INVALID before
 * an upload and for a window outside the batch or the T stages.  Only what is asked for is copied: a call without a record-derived
 * pointer (the feet, twists, contact, heights, hull rows) does not read the records. */
typedef struct wcqp_tick_plan_window {    /* HOST pointers, any may be NULL */
    double* left_traj; double* right_traj;     /* [n][m][12] */
    double* left_twist; double* right_twist;   /* [n][m][6]  */
    uint8_t* contact;                          /* [n][m]     */
    double* com_height; double* com_height_vel;   /* [n][m]  */
    double* ref_traj; double* dcm_vel_traj;    /* [n][m][2]  */
    double* hull_A; double* hull_b; int32_t* hull_nc;   /* [n][m][8][2], [n][m][8], [n][m]: the support-polygon rows in force at each stage */
    double* u_init;                            /* [n][2] a generated plan's ZMP of stage 0 (what a NULL u_init of wcqp_tick_upload_footsteps stands for) */
} wcqp_tick_plan_window;
int wcqp_tick_get_plan(wcqp_tick_t h, int32_t robot0, int32_t n, int32_t stage0, int32_t m, const wcqp_tick_plan_window* out);
/* enqueue only; use_graph: hipGraph replays of 8 ticks each, remainder as plain launches - IGNORED (no graph is built) whenever
 * the fused kernel runs several ticks per launch, i.e. for every wcqp_tick_params.ticks_per_launch != 1 including the default 0,
 * which makes a whole call ONE launch: a caller that needs the device back within a bound (another stream's work, a watchdog)
 * caps it - ticks_per_launch = 256 keeps a launch of 8192 robots under 5 ms at no measurable cost.  WCQP_E_INVALID when the
 * ticks enqueued since the last upload + n_ticks would exceed max_ticks (the trajectories end there).  A call that fails AFTER
 * it has started to enqueue leaves the handle without a defined state: it then refuses to run until the next wcqp_tick_upload. */
int wcqp_tick_run(wcqp_tick_t h, int32_t n_ticks, int32_t use_graph, void* stream);
/* Trajectory merge (WM/src/WalkingModule.cpp:500-535, 1263-1308: a newly planned trajectory is spliced into the deques at a
 * merge point - 20 ticks ahead in the shipped configuration - and `resetTrajectory` is raised for exactly one tick): replaces
 * stages [from_tick, from_tick + n_stages) of every instance's DCM reference trajectory with ref_tail[B][n_stages][2] (HOST
 * pointer; its rows are staged into device memory of the handle BEFORE the call returns - the caller may release or reuse
 * ref_tail at once, whatever is still running on `stream`), in stream order behind the ticks already enqueued, while everything
 * else of the pipeline stays as it is; later
 * ticks see the new stages through their windows [t, t + N].  from_tick >= the ticks enqueued so far, from_tick + n_stages <=
 * max_ticks + N + 1.  The reset flag itself has no counterpart: it makes MPCSolver::setGradient rebuild the gradient instead of
 * shifting it (MPCSolver.cpp:188-239), and this library always evaluates the gradient's contribution from the current window.
 * Valid between wcqp_tick_run calls (a call leaves nothing running ahead); captured graphs stay valid - the trajectory
 * buffer does not move. */
int wcqp_tick_splice_reference(wcqp_tick_t h, int32_t from_tick, int32_t n_stages, const double* ref_tail, void* stream);
/* External feedback (wcqp_tick_params.plant = WCQP_TICK_PLANT_EXTERNAL): the measured state the NEXT tick is to use - DEVICE
 * pointers, dcm_meas / com_meas / zmp_meas [B][2], q_meas [B][dof] or NULL (= the desired joint positions, as with the internal
 * plant).  Enqueues one small copy kernel on `stream`: the arrays may be reused once it has run (stream order), nothing is
 * retained.  Required before every wcqp_tick_run call of such a handle (which then takes n_ticks = 1: WCQP_E_INVALID otherwise,
 * or when no feedback has been set since the last tick); WCQP_E_UNSUPPORTED on a handle with the internal plant.
 * Replaces: WalkingController::setFeedback (:612), WalkingZMPController::setFeedback (:665), the joint part of
 * WalkingQPIK::setRobotState (:373) of WM/src/WalkingModule.cpp.
 * Non-finite inputs: a robot with a NaN or an Inf in its dcm_meas, com_meas, zmp_meas or q_meas entries is REJECTED by rule 5 of the sensor
 * form below: it keeps the measured state of tick t - 1 (tick 0: the uploaded one, with the desired joints), wcqp_tick_outputs.feedback_fail
 * counts it, and it is stopped like a robot whose IK failed - dq = 0 from tick t on, ik_fail counting the rejection (when it was not stopped
 * yet) and every tick it runs stopped, tick t included.  Nothing non-finite enters its state; the other robots are unaffected.  (A second
 * call before the tick runs replaces the first; a robot the second call rejects keeps what the first gave it, and feedback_fail counts
 * rejected calls.) */
int wcqp_tick_set_feedback_device(wcqp_tick_t h, const double* dcm_meas, const double* com_meas, const double* zmp_meas,
                                  const double* q_meas, void* stream);
/* the same from HOST pointers: staged through device memory of the handle and IN PLACE when the call returns (it synchronises: the host
 * arrays may be released at once, and the tick may then be run on any stream, a non-blocking one included).  With the device form the
 * caller orders the copy kernel's stream before the stream of the run call (the same stream does).  On a handle with per-tick
 * kinematics it first waits, on the host, for the event behind the handle's last wcqp_tick_run - and behind a wcqp_tick_reset_robots call
 * since -, as wcqp_tick_set_sensor_feedback_host and wcqp_tick_set_desired_host do: new with wcqp_tick_reset_robots, and a host wait a
 * caller whose ticks run on a non-blocking stream did not have before (the feedback of tick t is then never written under tick t - 1). */
int wcqp_tick_set_feedback_host(wcqp_tick_t h, const double* dcm_meas, const double* com_meas, const double* zmp_meas, const double* q_meas);
/* Sensor feedback (EXTERNAL plant with per-tick kinematics): the counterpart of wcqp_tick_set_feedback_* that takes what a robot
 * reports - WalkingModule::getFeedbacks (WM/src/WalkingModule.cpp:547) - and evaluates the measured state on the device, for tick
 * t = the ticks run since the last upload.  DEVICE pointers: q_meas, dq_meas [B][dof] (rad, rad/s); wrench_left, wrench_right [B][6]
 * fx fy fz tx ty tz in that foot's sole frame (iDynTree's Wrench order, as wholeBodyDynamics reports it).  Per robot:
 *   1. updateFKSolver (:1147-1165): forward kinematics at q_meas with the floating base anchored so that tick t's stance sole sits on its
 *      desired pose, world_T_base = world_T_sole,desired * (base_T_sole(q_meas))^-1 - the stance side and desired pose tick t's own
 *      kinematics take: side ((t + phase0) % (2 step_ticks)) / step_ticks, pose from state0.
 *   2. evaluateCoM / evaluateDCM (:1167-1217; WM/src/WalkingForwardKinematics.cpp:258-337): com = the total CoM, v_com = the joint
 *      columns of the MIXED CoM Jacobian times dq_meas (the base twist is zero, WalkingFK::setInternalRobotState),
 *      dcm = com_xy + v_com_xy / omega, omega = sqrt(mpc.gravity / mpc.com_height).
 *   3. evaluateZMP (:826-878): a foot is defined when fz >= 0.001; its ZMP (-ty / fz, tx / fz, 0) in the sole frame is mapped to world by
 *      that sole's pose of step 1; totalZ = fz_left + fz_right; zmp = xy of sum_f (fz_f defined_f / totalZ) zmp_f.
 *   4. com, dcm, zmp xy and q_meas go where wcqp_tick_set_feedback_device puts them: tick t then runs as a plain EXTERNAL tick fed them.
 *   5. A robot with totalZ < 0.1 (updateModule returns false there) or with any input that is not finite is REJECTED: it keeps the
 *      measured state of tick t - 1 (tick 0: the uploaded one, with the desired joints), wcqp_tick_outputs.feedback_fail counts it, and it
 *      is stopped like a robot whose IK failed: dq = 0 from tick t on.  Its ik_fail then counts the rejection (when it was not stopped
 *      yet) and every tick it runs stopped, tick t included.  The other robots are unaffected.
 * Low-pass filters (wcqp_tick_params.joint_velocity_cut_frequency, wrench_cut_frequency, com_cut_frequency; each on when > 0): the
 * reference's three first-order filters, RobotHelper::getFeedbacks (WM/src/RobotHelper.cpp:408-440) and WalkingFK::evaluateCoM /
 * evaluateDCM / getCoMPosition (WM/src/WalkingForwardKinematics.cpp:138-162, 278-340, 354-394).  The filter is 1 / (1 + s tau),
 * tau = 1 / (2 pi f_c), discretised with the bilinear transform at Ts = mpc.sampling_time:
 *   y_k = (Ts (u_k + u_{k-1}) - (Ts - 2 tau) y_{k-1}) / (2 tau + Ts)        (unit DC gain; init(y0): u_{-1} = y_{-1} = y0)
 * (the build's definition: iCub::ctrl::FirstOrderLowPassFilter is upstream).  Per robot, in this order:
 *   a. Finiteness (rule 5) is judged on the RAW readings: nothing non-finite ever enters a filter's state.
 *   b. dq_f = LP(dq_meas) per joint (positions are not filtered: the reference's position filter is commented out); LP of fz, tx, ty of
 *      each wrench - what step 3 reads; the other components have no consumer and no state.
 *   c. Step 1 at q_meas as above; step 2 with v_com formed from dq_f.  CoM filter: com = LP(com_xy), v = LP(v_com_xy),
 *      dcm = com + v / omega; the filtered com is also the CoM the ZMP-CoM controller reads (getCoMPosition).
 *   d. Step 3 on the filtered wrenches: the fz >= 0.001 test and the totalZ >= 0.1 test of rule 5 see filtered forces only.
 *   wcqp_tick_outputs.measured reports what the tick used, so the filtered values.
 * State, per robot, kept in the handle across ticks: wcqp_tick_upload resets it.  The joint-velocity and wrench filters start AT the
 * first sensor reading the handle receives after an upload (RobotHelper::resetFilters), which is its own filtered value.  The CoM
 * position filter starts at the uploaded com0 and the CoM velocity filter at 0 - DEVIATION: the reference starts them at
 * (0, 0, com_height) and 0, once, at configure (WalkingForwardKinematics.cpp:153-160); the robots of a batch stand anywhere, and with
 * com0 = 0 this is the reference's value.  A rejected robot's filters hold their state (it is stopped until the next upload anyway).
 * "A second call before the tick runs replaces the first" holds for the filters too: every call starts from the state the last RUN
 * tick left, and wcqp_tick_run commits the state of the call it consumes - two calls for one tick advance each filter once.  A tick
 * fed by wcqp_tick_set_feedback_* supplies no sample: the filters hold (also when that call replaces a sensor call before the run).
 * Marks the feedback of tick t as set, as wcqp_tick_set_feedback_device does; either form may feed any tick of a handle.  The device form enqueues
 * one kernel on `stream` and retains nothing.  WCQP_E_INVALID for a NULL pointer or a handle that has not been uploaded;
 * WCQP_E_UNSUPPORTED with the internal plant or without per-tick kinematics (use_kinematics = 0). */
int wcqp_tick_set_sensor_feedback_device(wcqp_tick_t h, const double* q_meas, const double* dq_meas, const double* wrench_left,
                                         const double* wrench_right, void* stream);
/* the same from HOST pointers: staged in device memory the handle allocated at create, and IN PLACE when the call returns - it first
 * waits for the handle's last wcqp_tick_run, whatever stream that named (a non-blocking one included); the host arrays may be released
 * at once and the tick may run on any stream. */
int wcqp_tick_set_sensor_feedback_host(wcqp_tick_t h, const double* q_meas, const double* dq_meas, const double* wrench_left,
                                       const double* wrench_right);
/* Streamed trajectories (wcqp_tick_params.streamed_trajectories): the desired stage of tick t = the ticks run since the last upload, per
 * robot - what the reference pops from the front of m_leftTrajectory, m_rightTrajectory, m_leftTwistTrajectory, m_rightTwistTrajectory,
 * m_leftInContact / m_rightInContact, m_isLeftFixedFrame, m_comHeightTrajectory and m_comHeightVelocity on that tick
 * (WM/src/WalkingModule.cpp:509-511, 689-707, 1085-1165). */
typedef struct wcqp_tick_desired {
    const double* left_pose;  const double* right_pose;    /* [B][12] sole: p 3 | R 9 row-major      */
    const double* left_twist; const double* right_twist;   /* [B][6]                                 */
    const uint8_t* contact;                                /* [B] bits as wcqp_tick_inputs.contact   */
    const double* com_height; const double* com_height_vel;/* [B] or NULL: state0[68], 0             */
} wcqp_tick_desired;
/* DEVICE pointers; one kernel on `stream`, nothing retained (the arrays may be reused once it has run).  Order per tick:
 * wcqp_tick_set_desired_* -> wcqp_tick_set_sensor_feedback_* (it anchors at this stage: WCQP_E_INVALID on a streamed handle whose stage of
 * tick t has not been set) or wcqp_tick_set_feedback_* (before or after the stage) -> wcqp_tick_run(h, 1, ...), which returns
 * WCQP_E_INVALID without a stage AND a feedback set since the last tick.  A second call before the run replaces the stage.
 * WCQP_E_UNSUPPORTED on a handle without the mode; WCQP_E_INVALID before an upload or with a NULL required pointer.
 * A robot whose stage is invalid - neither foot in contact, a fixed-frame foot that is not in contact, a non-finite value: the rules of
 * the planned upload - is rejected by the kernel as a bad sensor reading is: it keeps its previous stage, is stopped like a robot whose
 * IK failed (dq = 0 from tick t on), and wcqp_tick_outputs.feedback_fail counts it; the other robots are unaffected. */
int wcqp_tick_set_desired_device(wcqp_tick_t h, const wcqp_tick_desired* desired, void* stream);
/* the same from HOST pointers: checked on the host first (an invalid stage of any robot: WCQP_E_INVALID, the handle unchanged), staged in
 * device memory the handle allocated at create, and IN PLACE when the call returns - it first waits for the handle's last wcqp_tick_run,
 * whatever stream that named; the host arrays may be released at once and the tick may run on any stream. */
int wcqp_tick_set_desired_host(wcqp_tick_t h, const wcqp_tick_desired* desired);
/* A resident plan (wcqp_tick_params_ext.resident_plan, which states the order and the replan rule): ONE kernel on `stream` that stages, for
 * every robot, stage t of the plan the handle holds as the desired stage of the next tick - its record into the robot's live record, the
 * row set the record names into the robot's own.  t = the ticks run since the last upload, read by the kernel from the handle's tick
 * index in device memory: enqueue-only, in stream order behind the ticks already enqueued on `stream`.  Nothing is validated (the upload
 * validated the plan) and no hull is built.  WCQP_E_UNSUPPORTED on a handle without resident_plan; WCQP_E_INVALID before a plan has
 * been uploaded or when t has reached max_ticks. */
int wcqp_tick_set_desired_from_plan(wcqp_tick_t h, void* stream);
int wcqp_tick_download(wcqp_tick_t h, const wcqp_tick_outputs* out);             /* synchronises     */

/* The form a tick handle actually took at wcqp_tick_create (the route follows the IK algorithm, the kinematics hand-off and the
 * controller: the fused kinematics hand-off of an MPC handle falls back to COMPACT at horizons of 55 and more, for example). */
typedef struct wcqp_tick_info {
    int32_t kin_handoff;        /* WCQP_KIN_HANDOFF_* taken; -1 without per-tick kinematics (constant Jacobians)            */
    int32_t ticks_per_launch;   /* effective ticks one launch walks through (1 << 20: all the ticks of a wcqp_tick_run call) */
    int32_t dcm_controller;     /* WCQP_TICK_DCM_*                                                                          */
    int32_t launches_per_tick;  /* kernel launches of a tick that runs alone (the skewed fused kernel: 1)                   */
    int32_t zmp_gain_scheduling;   /* wcqp_tick_params.zmp_gain_scheduling as taken (0 / 1)                                 */
    int32_t planned_trajectories;  /* wcqp_tick_params.planned_trajectories as taken (0 / 1)                                */
    int32_t streamed_trajectories; /* wcqp_tick_params.streamed_trajectories as taken (0 / 1)                               */
    int32_t sensor_filters;        /* low-pass filters of the sensor form taken: bit 0 joint velocity, bit 1 wrench, bit 2 CoM      */
    int32_t plan_generated;        /* 1: the plan in place was generated by wcqp_tick_upload_footsteps; 0: uploaded, or none yet    */
    double  plan_record_ms;        /* plan_generated: device time of that upload's record pass (events around it) [ms]; else 0      */
    int32_t ik_mode;               /* wcqp_tick_params.ik_mode as taken (WCQP_TICK_IK_*)                                            */
} wcqp_tick_info;
int wcqp_tick_get_info(wcqp_tick_t h, wcqp_tick_info* out);
/* ... and what it took of wcqp_tick_params_ext - a struct of its own for the same reason: it only grows at its end */
typedef struct wcqp_tick_info_ext {
    int32_t resident_plan;         /* wcqp_tick_params_ext.resident_plan as taken (0 / 1)                                           */
} wcqp_tick_info_ext;
int wcqp_tick_get_info_ext(wcqp_tick_t h, wcqp_tick_info_ext* out);

/* =====================================================================================
 * Footsteps from per-robot goals: the unicycle planner.  "Robot i, go there" - the reference's setGoal(x, y):
 * WalkingModule::setPlannerInput (WM/src/WalkingModule.cpp:1263-1308) stores the goal, TrajectoryGenerator::updateTrajectories
 * (WM/src/TrajectoryGenerator.cpp:442-484) turns it into the unicycle's desired point, and the unicycle planner, configured at
 * TrajectoryGenerator.cpp:114-132 from plannerParams.ini, turns that into footsteps.  The planner library is upstream of the reference:
 * like the plan of wcqp_tick_upload_footsteps, THE PLANNER IS THIS BUILD'S OWN DEFINITION, stated here (tests/helpers/unicycle_plan.py
 * restates it in numpy).  Its outputs have exactly the shapes wcqp_tick_footsteps / wcqp_tick_replan take.
 *
 * Inputs per robot: left0, right0 [12] the soles' poses in the layout of the desired-foot entries of state0 (position 3 | rotation 9
 * row-major; only x, y and yaw = atan2(R10, R00) are read), goal [2] the argument of setGoal, in the unicycle's frame, and first_side,
 * the foot that swings first (0 left, 1 right).  R(a) is the plane rotation by a, w = nominal_width, d = reference_position,
 * wrap(a) = a - 2 pi rint(a / (2 pi)).
 *   Start     (TrajectoryGenerator.cpp:445-466) the stance foot is the foot that does not swing first, at (p_s, th_s).  The unicycle
 *             starts at p_s + R(th_s) (0, -w/2) for a left stance foot, (0, +w/2) for a right one, with heading th_s.  The desired point
 *             y* = p_u + R(th) (d + goal) is fixed for the whole call, without a feed-forward velocity (the reference adds a single
 *             trajectory point, :231-234).
 *   Unicycle  reference point y = p + R(th) d; control (v, om) = -k B(th)^-1 (y - y*), B = [[cos th, -d_x sin th - d_y cos th],
 *             [sin th, d_x cos th - d_y sin th]] (det B = d_x); then v and om are clamped to +-max_linear_velocity and
 *             +-max_angular_velocity, then v <- v / (1 + g |om|).  Dynamics (x', y', th') = (v cos th, v sin th, om), integrated with
 *             the classical RK4 at step dT, the control evaluated anew at every stage.  Sample n is the state after n steps; th is
 *             never wrapped along the path.  (The heading loop's gain is k L / |d_x| with the desired point L away, and the explicit
 *             RK4 integrates it stably only while k L dT / |d_x| < 2.785 - L < 2.78 m at the reference's values and dT = 0.01.  A
 *             farther goal still yields feasible footsteps, but om chatters between its saturations on the way and the plan then
 *             depends on the last bit of its inputs: send such a robot there through nearer goals.)
 *   Steps     sides alternate from first_side.  Step k knows the swing foot's current footprint, the stance foot (p_st, th_st) and the
 *             path index n_k, n_0 = 0.  Candidate m of 1..D is the unicycle at sample n_k + m: position c = p_u + R(th_u) (0, +-w/2)
 *             (left +), yaw th_u.  With r = R(th_st)^T (c - p_st) it is feasible iff |r| <= max_step_length, the lateral component
 *             of r towards the swing side (r_y for a left swing foot, -r_y for a right one) is >= min_width, and
 *             |wrap(th_u - th_st)| <= max_angle_variation.  m* is the LARGEST feasible m; without one the robot's planning ends
 *             WCQP_UNICYCLE_STUCK and keeps the steps so far.  If candidate m* lies less than min_step_length from the swing foot's
 *             current footprint AND |wrap(th_u - th_swing)| < min_angle_variation the robot has arrived: no step, WCQP_UNICYCLE_DONE.
 *             Otherwise step k is taken: side[k] = the swing foot, target[k] = (c_x, c_y, wrap(th_u - th_swing)) - the yaw INCREMENT
 *             of wcqp_tick_footsteps.target -, the foot's footprint becomes (c, th_u), n_{k+1} = n_k + m*, and the feet swap roles.
 *             K steps taken without arriving: WCQP_UNICYCLE_TRUNCATED.
 *   Outputs   n_steps [B], side [B][K], target [B][K][3], status [B], desired_point [B][2] (y*), unicycle_end [B][3] (x, y, th at
 *             sample n of the last step taken: the start pose without a step).  Entries of steps not taken are zero.
 *   Non-finite inputs ("never report SOLVED for NaN / Inf inputs"): the device form gives a robot with a NaN or an Inf in an entry it
 *             reads, a desired point that overflows or a first_side above 1 WCQP_UNICYCLE_INVALID_INPUT with n_steps = 0 and every output row zero; the other robots
 *             do not notice.  The host form refuses the whole call with WCQP_E_INVALID before anything is copied.
 * DEVIATIONS.  In THIS form step timings are common to a batch, as wcqp_tick_footsteps demands: minStepDuration, maxStepDuration,
 * nominalDuration, timeWeight, positionWeight and switchOverSwingRatio are not read, and a step advances the PATH by at most D samples
 * instead of choosing its duration (wcqp_unicycle_plan_timed_*, below, reads them and chooses).  plannerHorizon is
 * not read: the tick handle's T cuts the plan.  addTerminalStep and startAlwaysSameFoot are not offered: the feet of a DONE
 * robot are aligned to within the two arrival thresholds, not exactly (pitchDelta shapes the swing, not the footsteps:
 * wcqp_tick_swing_profile).  The two saturations are this build's own addition.
 * ===================================================================================== */
#define WCQP_UNICYCLE_DONE          0   /* arrived: the next candidate is no step                      */
#define WCQP_UNICYCLE_TRUNCATED     1   /* max_steps steps taken without arriving                      */
#define WCQP_UNICYCLE_STUCK         2   /* no feasible candidate within step_ticks samples             */
#define WCQP_UNICYCLE_INVALID_INPUT 3   /* device form: a non-finite input, or first_side above 1      */
typedef struct wcqp_unicycle_params {   /* every value is taken as given (capi.UnicyclePlanner holds the defaults) */
    double  dT;                          /* sampling time of the unicycle's path [s]; > 0                                            */
    double  reference_position[2];       /* d: referencePosition (plannerParams.ini), reference (0.1 0.0); d_x != 0 (det B = d_x)     */
    double  unicycle_gain;               /* k: unicycleGain, reference 10; > 0                                                       */
    double  slow_when_turning_gain;      /* g: slowWhenTurningGain, reference 5; >= 0                                                */
    double  max_linear_velocity;         /* saturation of v [m/s], this build's own; > 0                                             */
    double  max_angular_velocity;        /* saturation of om [rad/s], this build's own; > 0                                          */
    double  max_step_length;             /* maxStepLength, reference 0.20; > min_step_length                                         */
    double  min_step_length;             /* minStepLength, reference 0.05; > 0                                                       */
    double  min_width;                   /* minWidth, reference 0.14; > 0, <= nominal_width                                          */
    double  nominal_width;               /* w: nominalWidth, reference 0.16; > 0                                                     */
    double  max_angle_variation;         /* maxAngleVariation, RADIANS here (reference 10 degrees); > 0                              */
    double  min_angle_variation;         /* minAngleVariation, RADIANS here (reference 8 degrees); > 0                               */
    int32_t step_ticks;                  /* D: unicycle samples per step, >= 1; callers pass ss_ticks + ds_ticks                      */
    int32_t max_steps;                   /* K: row length of side / target, >= 0                                                     */
} wcqp_unicycle_params;

typedef struct wcqp_unicycle_inputs {    /* all required */
    const double*  left0;                /* [B][12] */
    const double*  right0;               /* [B][12] */
    const double*  goal;                 /* [B][2]  */
    const uint8_t* first_side;           /* [B]     */
} wcqp_unicycle_inputs;

typedef struct wcqp_unicycle_outputs {   /* n_steps, status and - for K > 0 - side and target are required */
    int32_t* n_steps;                    /* [B]       */
    uint8_t* side;                       /* [B][K]    */
    double*  target;                     /* [B][K][3] */
    int32_t* status;                     /* [B] WCQP_UNICYCLE_* */
    double*  desired_point;              /* [B][2] or NULL */
    double*  unicycle_end;               /* [B][3] or NULL */
} wcqp_unicycle_outputs;

/* (wcqp_unicycle_t: declared above, ahead of wcqp_tick_replan_goals, which takes one) */

/* Refusals need no device: WCQP_E_INVALID for a NULL pointer, a non-finite scalar or one outside the ranges above (d_x = 0,
 * min_width > nominal_width and min_step_length >= max_step_length among them), step_ticks < 1 or max_steps < 0. */
int wcqp_unicycle_create(const wcqp_unicycle_params* params, wcqp_unicycle_t* out);
int wcqp_unicycle_destroy(wcqp_unicycle_t h);
/* DEVICE pointers; one launch on `stream`, enqueue only (no allocation, no synchronisation), nothing retained.  WCQP_E_INVALID for a
 * NULL handle, struct or required pointer or batch < 0; WCQP_E_UNSUPPORTED for a batch whose widest array (target, batch x 24 K bytes,
 * or the soles, batch x 96) passes 2^32 bytes; WCQP_E_HIP without a device. */
int wcqp_unicycle_plan_device(wcqp_unicycle_t h, int32_t batch, const wcqp_unicycle_inputs* in, const wcqp_unicycle_outputs* out, void* stream);
/* the same with HOST pointers: validated on the host first (a non-finite entry that is read, or a first_side above 1, of any robot:
 * WCQP_E_INVALID, nothing copied or written), staged through the handle's own device buffer, and in place on return (it synchronises). */
int wcqp_unicycle_plan_host(wcqp_unicycle_t h, int32_t batch, const wcqp_unicycle_inputs* in, const wcqp_unicycle_outputs* out);

/* =====================================================================================
 * The planner chooses each step's duration.  The reference reads minStepDuration, maxStepDuration, nominalDuration, timeWeight,
 * positionWeight and switchOverSwingRatio (TrajectoryGenerator.cpp:82-103) and hands them to its planner (setCostWeights,
 * setStepTimings, setSwitchOverSwingRatio, :123-136).  The planner library is upstream of the reference, so - as above - THIS IS THIS
 * BUILD'S OWN DEFINITION (tests/helpers/unicycle_plan_timed.py restates it).  Start, unicycle law, RK4, candidate geometry, the three
 * feasibility constraints, the arrival test, the statuses and the treatment of non-finite inputs are those of wcqp_unicycle_plan_*;
 * the handle's step_ticks is not read.  What differs:
 *   Steps     Candidate m of min_step_ticks .. max_step_ticks is the unicycle at sample n_k + m (samples n_k + 1 .. n_k + min_step_ticks
 *             - 1 are integrated and are no candidates).  A feasible candidate is scored
 *                 c(m) = time_weight (1 / (m dT) - 1 / (nominal_step_ticks dT))^2 + position_weight |r_m - r_nom|^2,
 *             r_m = R(th_st)^T (c - p_st) the candidate seen from the stance foot, as in the feasibility test, and r_nom = (0, +w) for
 *             a left swing foot, (0, -w) for a right one.  m* is the feasible m with the SMALLEST c, the smallest such m on a tie;
 *             without a feasible one the robot ends WCQP_UNICYCLE_STUCK.  The arrival test is applied to candidate m*; a step taken
 *             continues the path from sample n_k + m*.
 *   Durations With rho = r / (1 + r), r = switch_over_swing_ratio (double support over single support), computed once on the host:
 *                 ds_k = min(max((int32) floor(m* rho + 0.5), 1), m* - 1),   ss_k = m* - ds_k,
 *             so ss_k, ds_k >= 1 and ss_k + ds_k = m*.  ss_ticks / ds_ticks [B][K] are outputs, zero for steps not taken (and for
 *             every step of a WCQP_UNICYCLE_INVALID_INPUT robot): a step's single-support stages and the double-support stages
 *             behind it.
 * DEVIATIONS that remain: plannerHorizon is not read, addTerminalStep and startAlwaysSameFoot are not offered, and
 * mergePointRatio is not read (a replan's merge stage is the caller's).  The two saturations stay this build's own addition.
 * ===================================================================================== */
typedef struct wcqp_unicycle_timing {
    int32_t min_step_ticks, max_step_ticks, nominal_step_ticks;  /* minStepDuration, maxStepDuration, nominalDuration / dT; 2 <= min <= nominal <= max */
    double  time_weight, position_weight;                        /* timeWeight, positionWeight; >= 0, finite */
    double  switch_over_swing_ratio;                             /* switchOverSwingRatio (double support / single support); > 0, finite */
} wcqp_unicycle_timing;
/* As wcqp_unicycle_plan_device, with DEVICE ss_ticks / ds_ticks [B][K] (required for K > 0); `tm` is read at the call.  Refusals need no
 * device and come before anything is launched: WCQP_E_INVALID for a NULL tm, a tick count or weight or ratio outside the ranges above,
 * a NULL duration row with K > 0, and everything wcqp_unicycle_plan_device refuses. */
int wcqp_unicycle_plan_timed_device(wcqp_unicycle_t h, const wcqp_unicycle_timing* tm, int32_t batch, const wcqp_unicycle_inputs* in,
                                    const wcqp_unicycle_outputs* out, int32_t* ss_ticks, int32_t* ds_ticks, void* stream);
/* the same with HOST pointers, validated, staged and synchronised as wcqp_unicycle_plan_host */
int wcqp_unicycle_plan_timed_host(wcqp_unicycle_t h, const wcqp_unicycle_timing* tm, int32_t batch, const wcqp_unicycle_inputs* in,
                                  const wcqp_unicycle_outputs* out, int32_t* ss_ticks, int32_t* ds_ticks);

#ifdef __cplusplus
}
#endif
#endif /* WCQP_H */
