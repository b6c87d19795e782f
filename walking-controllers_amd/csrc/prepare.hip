// Batched non-linear inverse kinematics (include/wcqp.h: wcqp_prepare_*, which states the problem and the iteration): the posture a walk
// starts from - the reference's WalkingModule::prepareRobot through WalkingIK::computeIK (citations relative to
// /root/reference/modules/Walking_module):
//   src/WalkingModule.cpp:880-1005               prepareRobot: the targets (left sole = the fixed base, right sole, CoM), the neck rule :944-984
//   src/WalkingInverseKinematics.cpp:239-305     setFullModelFeetConstraint / prepareIK: constraints, costs, limits
//   src/WalkingInverseKinematics.cpp:346-424     computeIK
// One launch runs ALL Gauss-Newton iterations: 16 lanes per robot, four robots per wave, one wave per workgroup, as sensors.hip - the
// kinematics are the walk of kin_device.h (walk_*) on this kernel's LDS map with three attached frames.  New here: the Jacobian columns
// of the right sole, the neck and the CoM reduced to the joints by the anchored left sole (its base block [I -S; 0 I] is inverted in
// closed form, as ik4 eliminates the base: the column of a left-leg joint c becomes -[a_c x (p_f - p_c); a_c] in every other frame and
// -a_c x (com - p_c) joins its CoM column), the log map, and the 23-variable QP with nine equality rows and a box, solved in range
// space: H = w_q I + w_n N'N is inverted by the 3 x 3 Woodbury identity, the rows of the equalities and of the active bounds meet in a
// Schur complement of at most 23 rows that is Cholesky-factored in LDS, and an active-set walk adds the most violated bound or drops the
// bound whose multiplier has the wrong sign until neither exists (the QP is strictly convex: the optimum does not depend on the walk).
// A wave loops until its four robots have stopped; a stopped robot takes one more pass of the kinematics - at its final joints, or at
// the clipped guess - to write its outputs, and stores nothing afterwards.  Plain vector loads and stores only.
// The three blocks of a pass - linearisation, QP, step - are the device functions of prepare_device.h, which the tick of the POSITION mode
// (position_tick.hip) runs too; the output pass of a stopped robot is this kernel's own.
#include <cmath>
#include <cstring>
#include <new>
#include <vector>
#include "wcqp_internal.h"
#include "kin_device.h"
#include "prepare_device.h"
#include "position_tick.h"
#include "prepare_rows.h"

namespace {

using namespace wcqp_prep;
constexpr int kStateLen = WCQP_IK_STATE_LEN;

struct PrepDev {
    const double* kin_tab; int kin_rounds; unsigned pm[3];
    int batch;
    const double *left_d, *right_d, *com_d, *Rd_neck, *q_guess;
    double *q, *base, *state, *residual;
    int *status, *iters;
    const double* par;                         // q_reg [23] | q_min [23] | q_max [23]
    double w_q, w_n, step_cap, tol_step, tol_c;
    int max_iter, use_limits;
    const int* n_rows;                         // NULL (the public entry points), or the rows to solve, at most `batch`, counted on the device
};

__global__ __launch_bounds__(64) void prepare_kernel(PrepDev a) {
    // (prepare_rows.h: the launch covers `batch` rows, a wave past the device's count leaves before it reads one)
    if (a.n_rows) { a.batch = min(a.batch, *a.n_rows); if ((long)blockIdx.x * 4 >= a.batch) return; }
    __shared__ __attribute__((aligned(16))) double kmodel[kKinTabSize];
    __shared__ __attribute__((aligned(16))) double smem[4][P_PER];
    const int lane = threadIdx.x, grp = lane >> 4, j = lane & 15;
    for (int k = lane; k < kKinTabSize; k += 64) kmodel[k] = a.kin_tab[k];
    const long inst_raw = (long)blockIdx.x * 4 + grp;
    const bool live = inst_raw < a.batch;
    const size_t i = (size_t)(live ? inst_raw : (long)a.batch - 1);
    double* S = smem[grp];
    const bool var1 = j < kDof - 16;                 // slot 1 is joint 16 + j
    const int cs[2] = {j, var1 ? 16 + j : 0};
    const bool use_neck = a.Rd_neck != nullptr && a.w_n > 0.0;
    const double wq = a.w_q, wn = use_neck ? a.w_n : 0.0, iwq = 1.0 / wq;
    // ---- inputs, and whether all of this robot's are finite
    double tl = 0.0, tr = 0.0, tc = 0.0, tn = 0.0;
    if (j < 12) { tl = a.left_d[i * 12 + j]; tr = a.right_d[i * 12 + j]; }
    if (j < 3) tc = a.com_d[i * 3 + j];
    if (j < 9 && a.Rd_neck) tn = a.Rd_neck[i * 9 + j];
    double qg[2] = {a.q_guess[i * kDof + cs[0]], var1 ? a.q_guess[i * kDof + cs[1]] : 0.0};
    const bool lane_bad = !(isfinite(tl) && isfinite(tr) && isfinite(tc) && isfinite(tn) && isfinite(qg[0]) && isfinite(qg[1]));
    const bool bad = ((__ballot(lane_bad) >> (grp * 16)) & 0xffffull) != 0ull;
    if (bad) {
        // nothing non-finite reaches an output: the robot is evaluated at the sanitised guess with both soles at the origin
        const double id = (j == 3 || j == 7 || j == 11) ? 1.0 : 0.0;
        tl = id; tr = id; tc = 0.0; tn = (j == 0 || j == 4 || j == 8) ? 1.0 : 0.0;
    }
    if (j < 12) { S[P_TG + j] = tl; S[P_TG + TG_RIGHT + j] = tr; }
    if (j < 3) S[P_TG + TG_COM + j] = tc;
    if (j < 9) S[P_TG + TG_NECK + j] = tn;
    double qreg[2], qlo[2], qhi[2];
#pragma unroll
    for (int s_ = 0; s_ < 2; ++s_) {
        qreg[s_] = a.par[cs[s_]];
        qlo[s_] = a.use_limits ? a.par[kDof + cs[s_]] : -HUGE_VAL;
        qhi[s_] = a.use_limits ? a.par[2 * kDof + cs[s_]] : HUGE_VAL;
        if (!isfinite(qg[s_])) qg[s_] = 0.0;
        qg[s_] = fmin(fmax(qg[s_], qlo[s_]), qhi[s_]);          // the guess, clipped into the limits
    }
    int kup[2][3], ksub[2];
    __syncthreads();                                 // the model table is in LDS
    const int kfj = walk_links<3>(kmodel, j, cs, kup, ksub);
    unsigned onL[2], onR[2], onN[2];
#pragma unroll
    for (int s_ = 0; s_ < 2; ++s_) {
        onL[s_] = (a.pm[0] >> cs[s_]) & 1u; onR[s_] = (a.pm[1] >> cs[s_]) & 1u; onN[s_] = use_neck ? (a.pm[2] >> cs[s_]) & 1u : 0u;
    }
    int status = bad ? WCQP_STATUS_NUMERIC : -1;     // -1: iterating
    bool stored = !live;
    int iters = 0, nw = 0;                           // nw: active bounds of the last QP (their list is in LDS)
    unsigned wmask = 0u;
    double qc[2] = {qg[0], qg[1]};
    for (;;) {
        // ================= the kinematics at qc and what the QP reads (prepare_device.h)
        double pb[3], Rb[9], e4[2][4], cmax;
        prep_linearise(kmodel, S, j, cs, var1, kup, ksub, kfj, a.kin_rounds, onL, onR, onN, use_neck, wq, wn, qc, qreg, qlo, qhi, pb, Rb, e4, cmax);
        // ================= a stopped robot writes its outputs from this pass, once
        if (status >= 0 && !stored) {
            // the CoM as the stand-alone kinematics kernel sums it (kin.hip: joint j on lane 6 + j of 32, a scan per 16-lane row), so that
            // the pose block equals wcqp_kin_jacobians_* at (base, q) bit for bit
#pragma unroll
            for (int s_ = 0; s_ < 2; ++s_)
                if (s_ == 0 || var1) { st2(S + P_E4 + cs[s_] * 4, e4[s_][0], e4[s_][1]); st2(S + P_E4 + cs[s_] * 4 + 2, e4[s_][2], e4[s_][3]); }
            if (j == 0) {
#pragma unroll
                for (int k = 0; k < 3; ++k) S[P_BASE + k] = pb[k];
#pragma unroll
                for (int k = 0; k < 9; ++k) S[P_BASE + 3 + k] = Rb[k];
            }
            wcqp::wave_lds_fence();
            double t0[4], t1[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                t0[k] = row_scan(j >= 6 ? S[P_E4 + (j - 6) * 4 + k] : 0.0);
                t1[k] = row_scan(j < 13 ? S[P_E4 + (10 + j) * 4 + k] : 0.0);
            }
            wcqp::wave_lds_fence();
            if (j == 15) {
                const double* rt = kmodel + kKinTabRoot;
                const double rootc[3] = {rt[0], rt[1], rt[2]};
                const double root_mass = rt[3];
                double cr[3], tt[4];
                mat3_vec(Rb, rootc, cr);
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    double r4 = root_mass * (pb[k] + cr[k]);
                    __asm__ volatile("" : "+v"(r4));     // a product and a sum there, not one fused operation
                    tt[k] = (t1[k] + t0[k]) + r4;
                }
                tt[3] = (t1[3] + t0[3]) + root_mass;
                const double im = 1.0 / tt[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) S[P_E4 + k] = tt[k] * im;
            }
            // stationarity at the returned joints: g + A' lambda on the joints off their bounds (on a bound the multiplier takes the rest)
            double sres = 0.0;
            if (status == WCQP_STATUS_SOLVED) {
#pragma unroll
                for (int s_ = 0; s_ < 2; ++s_) {
                    if ((s_ == 0 || var1) && !((wmask >> cs[s_]) & 1u)) {
                        double r = S[P_GR + cs[s_]];
                        for (int k = 0; k < 9; ++k) r += S[P_A + k * 24 + cs[s_]] * S[P_LAM + k];
                        sres = fmax(sres, fabs(r));
                        if (!isfinite(r)) sres = HUGE_VAL;
                    }
                }
            }
            S[P_DQ + j] = sres;
            wcqp::wave_lds_fence();
            for (int k = 0; k < 16; ++k) sres = fmax(sres, S[P_DQ + k]);
            a.q[i * kDof + cs[0]] = qc[0];
            if (var1) a.q[i * kDof + cs[1]] = qc[1];
            if (a.base && j < 12) a.base[i * 12 + j] = S[P_BASE + j];
            if (a.state) {
                double* st = a.state + i * kStateLen;
                for (int e = j; e < kStateLen; e += 16) {
                    double v = 0.0;
                    if (e < 24) { const int f = e / 12, r = e % 12; v = r < 3 ? S[P_FR + f * 12 + 9 + r] : S[P_FR + f * 12 + r - 3]; }
                    else if (e < 48) v = S[P_TG + e - 24];
                    else if (e < 57) v = S[P_FR + 24 + e - 48];
                    else if (e < 66) v = a.Rd_neck ? S[P_TG + TG_NECK + e - 57] : S[P_FR + 24 + e - 57];
                    else if (e < 69) v = S[P_E4 + e - 66];
                    else if (e < 72) v = S[P_TG + TG_COM + e - 69];
                    st[e] = v;
                }
            }
            if (j == 0) {
                a.status[i] = status;
                if (a.iters) a.iters[i] = iters;
                if (a.residual) {
                    const bool ok = status == WCQP_STATUS_SOLVED;
                    a.residual[i * 2] = ok ? cmax : HUGE_VAL;
                    a.residual[i * 2 + 1] = ok ? sres : HUGE_VAL;
                }
            }
            stored = true;
        }
        if (__ballot(!stored) == 0ull) break;
        // ================= one Gauss-Newton iteration of a robot that is still iterating: the QP, then the step
        if (status < 0) {
            const int fail = prep_qp(S, j, cs, var1, wq, wn, iwq, nw, wmask);
            prep_step(S, cs, fail, cmax, a.step_cap, a.tol_step, a.tol_c, a.max_iter, qg, qlo, qhi, qc, iters, status);
            wcqp::wave_lds_fence();
        }
    }
}

}  // namespace

struct wcqp_prepare_s {
    PrepDev dev{};
    std::vector<double> tab, par;
    double* d_tab = nullptr;                   // the model table, then the parameter rows
    wcqp::DeviceScratch scratch;
};

namespace {
int ensure_device(wcqp_prepare_s* h) {
    if (h->d_tab) return WCQP_OK;
    if (const int rc = wcqp::require_device("prepare kernel"); rc != WCQP_OK) return rc;
    const size_t nt = h->tab.size(), np = h->par.size();
    WCQP_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&h->d_tab), (nt + np) * sizeof(double)));
    WCQP_HIP_TRY(hipMemcpy(h->d_tab, h->tab.data(), nt * sizeof(double), hipMemcpyHostToDevice));
    WCQP_HIP_TRY(hipMemcpy(h->d_tab + nt, h->par.data(), np * sizeof(double), hipMemcpyHostToDevice));
    h->dev.kin_tab = h->d_tab;
    h->dev.par = h->d_tab + nt;
    return WCQP_OK;
}

// what both forms of wcqp_prepare_solve_* refuse before they look for a device
int check_call(wcqp_prepare_t h, int32_t batch, const double* left_d, const double* right_d, const double* com_d, const double* q_guess,
               const double* q, const int32_t* status) {
    if (!h || batch < 0) return WCQP_E_INVALID;
    if (!left_d || !right_d || !com_d || !q_guess || !q || !status) return WCQP_E_INVALID;
    if (!wcqp::fits32(batch, kStateLen * 8)) return WCQP_E_UNSUPPORTED;
    return WCQP_OK;
}
}  // namespace

namespace wcqp {

const std::vector<double>& prepare_model_table(wcqp_prepare_t h) { return h->tab; }

int prepare_enqueue_rows(wcqp_prepare_t h, const PrepareRows& r, hipStream_t stream) {
    if (!h || r.max_rows < 1 || !r.n_rows || !r.left_d || !r.right_d || !r.com_d || !r.q_guess || !r.q || !r.state || !r.status || !r.iters || !r.residual)
        return WCQP_E_INVALID;
    if (!fits32(r.max_rows, kStateLen * 8)) return WCQP_E_UNSUPPORTED;
    if (const int rc = ensure_device(h); rc != WCQP_OK) return rc;
    PrepDev a = h->dev;
    a.batch = r.max_rows; a.n_rows = r.n_rows;
    a.left_d = r.left_d; a.right_d = r.right_d; a.com_d = r.com_d; a.Rd_neck = r.Rd_neck; a.q_guess = r.q_guess;
    a.q = r.q; a.base = nullptr; a.state = r.state; a.status = r.status; a.iters = r.iters; a.residual = r.residual;
    hipLaunchKernelGGL(prepare_kernel, dim3((unsigned)((r.max_rows + 3) / 4)), dim3(64), 0, stream, a);
    WCQP_HIP_TRY(hipGetLastError());
    return WCQP_OK;
}

int prepare_check_scalars(const wcqp_prepare_params* p) {
    if (!std::isfinite(p->w_q) || !(p->w_q > 0.0) || !std::isfinite(p->w_n) || !(p->w_n >= 0.0)) return WCQP_E_INVALID;
    if (!std::isfinite(p->step_cap) || !(p->step_cap > 0.0)) return WCQP_E_INVALID;
    if (!std::isfinite(p->tol_step) || !(p->tol_step >= 0.0) || !std::isfinite(p->tol_constraint) || !(p->tol_constraint >= 0.0)) return WCQP_E_INVALID;
    if (p->max_iter < 1) return WCQP_E_INVALID;
    if ((p->q_min == nullptr) != (p->q_max == nullptr)) return WCQP_E_INVALID;
    return WCQP_OK;
}

int prepare_check_arrays(const wcqp_prepare_params* p) {
    if (!p->q_reg || (p->q_min == nullptr) != (p->q_max == nullptr)) return WCQP_E_INVALID;
    for (int k = 0; k < kDof; ++k) {
        if (!std::isfinite(p->q_reg[k])) return WCQP_E_INVALID;
        if (p->q_min && !(p->q_min[k] <= p->q_max[k])) return WCQP_E_INVALID;       // (a NaN limit fails too)
    }
    return WCQP_OK;
}

int prepare_host_tables(wcqp_kin_t kin, const wcqp_prepare_params* p, PrepareHost* t) {
    int stride = 0, off_d = 0;
    // the tree must be one the 16-lane walk runs (the condition of the tick's FUSED hand-off)
    if (!kin_fused_tables(kin, t->tab, &t->kin_rounds) || !kin_compact_layout(kin, t->pm, &stride, &off_d)) return WCQP_E_UNSUPPORTED;
    const int rc = prepare_check_arrays(p);
    if (rc != WCQP_OK) return rc;
    t->par.assign(3 * kDof, 0.0);
    for (int k = 0; k < kDof; ++k) {
        t->par[k] = p->q_reg[k];
        if (p->q_min) { t->par[kDof + k] = p->q_min[k]; t->par[2 * kDof + k] = p->q_max[k]; }
    }
    t->w_q = p->w_q; t->w_n = p->w_n; t->step_cap = p->step_cap; t->tol_step = p->tol_step; t->tol_c = p->tol_constraint;
    t->max_iter = p->max_iter; t->use_limits = p->q_min ? 1 : 0;
    return WCQP_OK;
}

}  // namespace wcqp

extern "C" {

int wcqp_prepare_create(wcqp_kin_t kin, const wcqp_prepare_params* p, wcqp_prepare_t* out) {
    if (!kin || !p || !out || !p->q_reg) return WCQP_E_INVALID;
    int rc = wcqp::prepare_check_scalars(p);
    if (rc != WCQP_OK) return rc;
    wcqp_prepare_s* h = new (std::nothrow) wcqp_prepare_s();
    if (!h) return WCQP_E_NOMEM;
    wcqp::PrepareHost t;
    rc = wcqp::prepare_host_tables(kin, p, &t);
    if (rc != WCQP_OK) { delete h; return rc; }
    h->tab = std::move(t.tab); h->par = std::move(t.par);
    PrepDev& d = h->dev;
    d.kin_rounds = t.kin_rounds;
    for (int k = 0; k < 3; ++k) d.pm[k] = t.pm[k];
    d.w_q = t.w_q; d.w_n = t.w_n; d.step_cap = t.step_cap; d.tol_step = t.tol_step; d.tol_c = t.tol_c;
    d.max_iter = t.max_iter; d.use_limits = t.use_limits;
    *out = h;
    return WCQP_OK;
}

int wcqp_prepare_destroy(wcqp_prepare_t h) {
    if (!h) return WCQP_E_INVALID;
    if (h->d_tab) (void)hipFree(h->d_tab);
    h->scratch.release();
    delete h;
    return WCQP_OK;
}

int wcqp_prepare_solve_device(wcqp_prepare_t h, int32_t batch, const double* left_d, const double* right_d, const double* com_d,
                              const double* Rd_neck, const double* q_guess,
                              double* q, double* base, double* state, int32_t* status, int32_t* iters, double* residual, void* stream) {
    int rc = check_call(h, batch, left_d, right_d, com_d, q_guess, q, status);
    if (rc != WCQP_OK || batch == 0) return rc;
    rc = ensure_device(h);
    if (rc != WCQP_OK) return rc;
    PrepDev a = h->dev;
    a.batch = batch; a.n_rows = nullptr;
    a.left_d = left_d; a.right_d = right_d; a.com_d = com_d; a.Rd_neck = Rd_neck; a.q_guess = q_guess;
    a.q = q; a.base = base; a.state = state; a.status = status; a.iters = iters; a.residual = residual;
    hipLaunchKernelGGL(prepare_kernel, dim3((unsigned)((batch + 3) / 4)), dim3(64), 0, (hipStream_t)stream, a);
    WCQP_HIP_TRY(hipGetLastError());
    return WCQP_OK;
}

int wcqp_prepare_solve_host(wcqp_prepare_t h, int32_t batch, const double* left_d, const double* right_d, const double* com_d,
                            const double* Rd_neck, const double* q_guess,
                            double* q, double* base, double* state, int32_t* status, int32_t* iters, double* residual) {
    int rc = check_call(h, batch, left_d, right_d, com_d, q_guess, q, status);
    if (rc != WCQP_OK || batch == 0) return rc;
    rc = ensure_device(h);
    if (rc != WCQP_OK) return rc;
    const size_t B = (size_t)batch;
    wcqp::HostStage st;
    const auto d_l = st.in(left_d, B * 12), d_r = st.in(right_d, B * 12), d_c = st.in(com_d, B * 3);
    const auto d_n = st.in(Rd_neck, B * 9, /*no neck task without it*/ true), d_g = st.in(q_guess, B * kDof);
    const auto d_q = st.out(q, B * kDof), d_b = st.out(base, B * 12), d_s = st.out(state, B * kStateLen), d_res = st.out(residual, B * 2);
    const auto d_st = st.out(status, B), d_it = st.out(iters, B);
    rc = st.upload(h->scratch);
    if (rc != WCQP_OK) return rc;
    rc = wcqp_prepare_solve_device(h, batch, st[d_l], st[d_r], st[d_c], st[d_n], st[d_g],
                                   st[d_q], st[d_b], st[d_s], st[d_st], st[d_it], st[d_res], nullptr);
    return rc != WCQP_OK ? rc : st.download();
}

}  // extern "C"
