// Periodic orbits by standard shooting on the spectral flow of flow.hip, matrix-free, for BK_PDE_CGL2D on one rank: the functional
// Shooting of src/periodicorbit/StandardShooting.jl (po_residual :138-165, po_jvp :190-257, updatesection! :116-122) with ds = 1 / M
// and the section SectionSS of src/periodicorbit/Sections.jl:6-58, as examples/cGL2d-shooting.jl uses them (:123-150), and the
// matrix-free monodromy MonodromyQaD_matrix_free(::Shooting, ...) of src/periodicorbit/Floquet.jl:89-108.
//
// Orbit vector: M states of N = 2 n doubles on the device, state i = [u1; u2] at x + i N, and ONE host tail scalar T.  With Phi the
// discrete flow, next(i) = i + 1, next(M - 1) = 0 and F the cGL vector field:
//
//     G_i  = Phi(x_i, T / M) - x_next(i)
//     G_T  = (<x_0, normal> - <center, normal>) T                                              (Sections.jl:13)
//     dG_i = dPhi(x_i, T / M) dx_i + F(Phi_i) (dT / M) - dx_next(i)                            (StandardShooting.jl:217)
//     dG_T = (<x_0, normal> - <center, normal>) dT + <dx_0, normal> T                          (Sections.jl:43-45)
//
// The period column is the reference's vector_field(flow, Phi_i) ds dT, NOT the tau-derivative of the discrete map: the two differ by
// the time-discretisation error of the flow, which costs Newton no more than its inexact linear solves already do.
//
// Kernels.  The M segments advance in lock-step through ONE flow of batch M (the reference's parallel = true).  After the march
// shoot_close_kernel<JVP> forms the rows -- the closure, the period column -- and the section dot in one pass with a fixed grid and
// the two-stage sum of stream.h: deterministic.  The operator dG(x, T) marches the base trajectory once, on creation, records u_n and
// the stage value a_n of every step, and then marches the tangent alone (option "shooting_store", default 1); without the record it
// marches state and tangent together in every application.  Both routes give the same bits.
#include <cmath>
#include <vector>

#include "cgl_pw.h"
#include "common.h"
#include "flow.h"
#include "ops.h"
#include "potrap_pw.h"
#include "stream.h"

struct bk_shooting {
    bk_ctx* ctx = nullptr;
    bk_problem* prob = nullptr;
    int M = 0, nsteps = 0;
    size_t n = 0;                  // grid points per field
    bk_flow* flow = nullptr;       // M trajectories: the segments
    bk_flow* flow1 = nullptr;      // one trajectory: the monodromy's sequential segment tangents (created with the first monodromy)
    double* normal = nullptr;      // [N]
    double* center = nullptr;      // [N]
    double c0 = 0.0;               // <center, normal>
    bool has_section = false;
    double* phi = nullptr;         // [3][M N]: Phi_i | dPhi_i dx_i | F(Phi_i)
    std::vector<double*> rec_free; // records of destroyed operators (ShootStore: one size per handle), reused by the next operator
    size_t rec_len() const { return (2 * (size_t)nsteps + 1) * len() + 3 * N(); }
    size_t N() const { return 2 * n; }
    size_t len() const { return 2 * n * (size_t)M; }
    double* dphi() const { return phi + len(); }
    double* fphi() const { return phi + 2 * len(); }
};

namespace bk {
namespace {

// out_i = phi_i [+ c fphi_i] - xs_next(i) over all M N entries, and the partial sums of <xs_0, normal>.  phi: Phi_i (residual) or
// dPhi_i dx_i (JVP); xs: x or dx.
template <bool JVP>
__global__ void __launch_bounds__(kThreads) shoot_close_kernel(size_t N, size_t total, double c, const double* __restrict__ phi,
                                                                const double* __restrict__ fphi, const double* __restrict__ xs,
                                                                const double* __restrict__ normal, double* __restrict__ out,
                                                                double* __restrict__ partials) {
    double s[1] = {0.0};
    for (size_t g = (size_t)blockIdx.x * kThreads + threadIdx.x; g < total; g += (size_t)gridDim.x * kThreads) {
        const size_t gn = g + N < total ? g + N : g + N - total;
        double v = phi[g];
        if (JVP) v = v + fphi[g] * c;
        out[g] = v - xs[gn];
        if (g < N) s[0] = fma(normal[g], xs[g], s[0]);
    }
    block_sum_store<1>(s, partials);
}

int shoot_close(bk_shooting* h, bool jvp, double c, const double* phi, const double* fphi, const double* xs, const double* normal,
                double* out, double* dot) {
    bk_ctx* ctx = h->ctx;
    const size_t total = h->len();
    const int grid = grid_for(total, 1, kRedBlocks);
    {
        ProfScope ps(ctx, jvp ? "shooting_close_jvp" : "shooting_close", 8.0 * (total * (jvp ? 4 : 3) + 2 * h->N()));
        if (jvp) hipLaunchKernelGGL(shoot_close_kernel<true>, dim3(grid), dim3(kThreads), 0, ctx->stream, h->N(), total, c, phi, fphi, xs,
                                    normal, out, ctx->d_partials);
        else hipLaunchKernelGGL(shoot_close_kernel<false>, dim3(grid), dim3(kThreads), 0, ctx->stream, h->N(), total, c, phi, fphi, xs,
                                normal, out, ctx->d_partials);
        BK_HIP(ctx, hipGetLastError());
    }
    BK_TRY(reduce_finish(ctx, grid, 1, 0));
    *dot = ctx->h_red[0];
    return 0;
}

int shoot_check(bk_shooting* h, const char* who) {
    if (!h->has_section)
        return set_error(h->ctx, "%s: no section set (bk_shooting_set_section or bk_shooting_update_section first)", who);
    return 0;
}

double shoot_tau(const bk_shooting* h, double T) { return (1.0 / h->M) * T; }          // sh.ds[i] * T

// fphi_i = F(phi_i), i < M, through the stencil kernel
int shoot_field(bk_shooting* h, const double* params, const double* phi, double* fphi) {
    for (int i = 0; i < h->M; ++i)
        BK_TRY(h->prob->apply(1, phi + i * h->N(), phi + i * h->N(), params, 0.0, 1.0, fphi + i * h->N()));
    return 0;
}

// The record of an operator, ONE block of the handle's size rec_len(): u_n and a_n of every step of a base march ([nsteps][M N]
// each), F(Phi_i) [M N], two work states [2 N] and the normal of the section in force at creation [N].  Blocks go back to the handle
// when the operator is destroyed and the next operator takes them from there: Newton and PALC create one operator per step, and only
// the first allocates.  The handle must outlive its operators (they march on its flow anyway).
struct ShootStore {
    bk_shooting* h = nullptr;
    double* buf = nullptr;
    double *u = nullptr, *a = nullptr, *fphi = nullptr, *tmp = nullptr, *normal = nullptr;
    bool full = false;
    ~ShootStore() {
        if (buf && full) h->rec_free.push_back(buf);
        else if (buf) (void)hipFree(buf);
    }
    // full = false (an operator that recomputes its base): the normal alone, N doubles of its own
    int alloc(bk_shooting* sh, const char* who, bool whole) {
        h = sh;
        full = whole;
        if (!full) {
            if (hipMalloc(&buf, sizeof(double) * h->N()) != hipSuccess) {
                buf = nullptr;
                return set_error(h->ctx, "%s: allocation failed", who);
            }
            normal = buf;
            return v_copy(h->ctx, h->N(), h->normal, normal);
        }
        if (!h->rec_free.empty()) {
            buf = h->rec_free.back();
            h->rec_free.pop_back();
        } else if (hipMalloc(&buf, sizeof(double) * h->rec_len()) != hipSuccess) {
            buf = nullptr;
            return set_error(h->ctx, "%s: allocation of the operator's record (%zu doubles) failed", who, h->rec_len());
        }
        const size_t len = (size_t)h->nsteps * h->len();
        u = buf; a = u + len; fphi = a + len; tmp = fphi + h->len(); normal = tmp + 2 * h->N();
        return v_copy(h->ctx, h->N(), h->normal, normal);
    }
};
// 2 nsteps M N doubles against option "shooting_store_max" (doubles; default 2^28 = 2 GiB)
bool shoot_store_fits(const bk_shooting* h) {
    return 2.0 * h->nsteps * (double)h->len() <= h->ctx->opt("shooting_store_max", 268435456.0);
}

// dG(x, T) on (device vector of M N doubles, host tail dT); references x
struct ShootOp : bk_op {
    bk_shooting* h = nullptr;
    const double* x = nullptr;
    double T = 0.0;
    CglPar par{};
    double params[BK_MAX_PARAMS] = {0};
    bool stored = false;
    ShootStore st;                     // the recomputed route uses its normal alone
    double s0 = 0.0;                   // <x_0, normal> - <center, normal>
    long long base_marches = 0, applications = 0;
    int apply(const double* dx, const double* dxt, double a0, double a1, double* out, double* outt) override {
        if (out == dx) return set_error(ctx, "shooting operator: out must not alias x");
        const double tau = shoot_tau(h, T), c = (1.0 / h->M) * dxt[0];
        double dot = 0.0;
        const double* fp = st.fphi;
        if (stored) {
            BK_TRY(flow_march(h->flow, kFlowTangent, par, nullptr, dx, tau, h->nsteps, nullptr, h->dphi(), nullptr, nullptr, st.u, st.a));
        } else {
            BK_TRY(flow_march(h->flow, kFlowBoth, par, x, dx, tau, h->nsteps, h->phi, h->dphi(), nullptr, nullptr, nullptr, nullptr));
            BK_TRY(shoot_field(h, params, h->phi, h->fphi()));
            fp = h->fphi();
            base_marches += 1;
        }
        BK_TRY(shoot_close(h, true, c, h->dphi(), fp, dx, st.normal, out, &dot));
        if (!(a0 == 0.0 && a1 == 1.0)) BK_TRY(v_axpby(ctx, n, a0, dx, a1, out));
        outt[0] = a0 * dxt[0] + a1 * (s0 * dxt[0] + dot * T);
        applications += 1;
        return 0;
    }
};

// dx -> dPhi(x_{M-1}) .. dPhi(x_0) dx on the recorded base trajectory, length N, no tail; references nothing after creation
struct ShootMonodromyOp : bk_op {
    bk_shooting* h = nullptr;
    double T = 0.0;
    CglPar par{};
    ShootStore st;
    long long base_marches = 0, applications = 0;
    int apply(const double* x, const double*, double a0, double a1, double* out, double*) override {
        if (out == x) return set_error(ctx, "shooting monodromy: out must not alias x");
        const size_t N = h->N();
        const double tau = shoot_tau(h, T);
        const double* v = x;
        for (int i = 0; i < h->M; ++i) {
            double* w = st.tmp + (i & 1) * N;
            BK_TRY(flow_march(h->flow1, kFlowTangent, par, nullptr, v, tau, h->nsteps, nullptr, w, nullptr, nullptr, st.u + i * N, st.a + i * N,
                              h->len()));
            v = w;
        }
        applications += 1;
        return v_axpbyz(ctx, N, a0, x, a1, v, out);
    }
};

}  // namespace
}  // namespace bk

using namespace bk;

extern "C" {

int bk_shooting_create(bk_problem* prob, int M, int nsteps, bk_shooting** out) {
    if (!prob || !out) return -1;
    bk_ctx* ctx = prob->ctx;
    // the rank count first: a BK_PDE_CGL2D problem does not exist on more than one rank, so the problem kind would hide this answer
    if (ctx->nranks > 1) return set_error(ctx, "bk_shooting_create: the shooting functional runs on a single rank");
    const double zero[6] = {0, 0, 0, 0, 0, 0};
    CglPar par;
    BK_TRY(flow_params(prob, zero, 6, &par));
    if (M < 1) return set_error(ctx, "bk_shooting_create: M >= 1 segments (got %d)", M);
    if (nsteps < 1) return set_error(ctx, "bk_shooting_create: nsteps >= 1 time steps per segment (got %d)", nsteps);
    bk_shooting* h = new bk_shooting();
    h->ctx = ctx; h->prob = prob; h->M = M; h->nsteps = nsteps; h->n = prob->nloc / 2;
    int s = flow_create(prob, M, "bk_shooting_create", &h->flow);
    if (s != 0) { delete h; return s; }
    if (hipMalloc(&h->normal, sizeof(double) * h->N()) != hipSuccess || hipMalloc(&h->center, sizeof(double) * h->N()) != hipSuccess ||
        hipMalloc(&h->phi, sizeof(double) * 3 * h->len()) != hipSuccess) {
        bk_shooting_destroy(h);
        return set_error(ctx, "bk_shooting_create: allocation failed");
    }
    *out = h;
    return 0;
}

int bk_shooting_destroy(bk_shooting* h) {
    if (!h) return 0;
    flow_destroy(h->flow);
    flow_destroy(h->flow1);
    if (h->normal) (void)hipFree(h->normal);
    if (h->center) (void)hipFree(h->center);
    if (h->phi) (void)hipFree(h->phi);
    for (double* r : h->rec_free) (void)hipFree(r);
    delete h;
    return 0;
}

int bk_shooting_set_section(bk_shooting* h, const double* normal, const double* center) {
    if (!h || !normal || !center) return -1;
    BK_TRY(v_copy(h->ctx, h->N(), normal, h->normal));
    BK_TRY(v_copy(h->ctx, h->N(), center, h->center));
    BK_TRY(v_dot(h->ctx, h->N(), h->center, h->normal, &h->c0));
    h->has_section = true;
    return 0;
}

int bk_shooting_get_section(bk_shooting* h, double* normal, double* center) {
    if (!h || !normal || !center) return -1;
    BK_TRY(shoot_check(h, "bk_shooting_get_section"));
    if (normal == center) return set_error(h->ctx, "bk_shooting_get_section: normal and center must be distinct");
    BK_TRY(v_copy(h->ctx, h->N(), h->normal, normal));
    return v_copy(h->ctx, h->N(), h->center, center);
}

int bk_shooting_update_section(bk_shooting* h, const double* x, double T, const double* params, int nparams) {
    if (!h || !x || !params) return -1;
    (void)T;
    CglPar par;
    BK_TRY(flow_params(h->prob, params, nparams, &par));
    bk_ctx* ctx = h->ctx;
    if (x == h->normal || x == h->center) return set_error(ctx, "bk_shooting_update_section: x must not alias the section");
    BK_TRY(h->prob->apply(1, x, x, params, 0.0, 1.0, h->normal));
    double nrm = 0.0;
    BK_TRY(v_nrm2(ctx, h->N(), h->normal, &nrm));
    if (!(nrm > 0.0) || !std::isfinite(nrm))
        return set_error(ctx, "bk_shooting_update_section: |F(x_0)| = %g: the first state is an equilibrium or not finite", nrm);
    BK_TRY(v_scale(ctx, h->N(), 1.0 / nrm, h->normal));
    BK_TRY(v_copy(ctx, h->N(), x, h->center));
    BK_TRY(v_dot(ctx, h->N(), h->center, h->normal, &h->c0));
    h->has_section = true;
    return 0;
}

int bk_shooting_residual(bk_shooting* h, const double* x, double T, const double* params, int nparams, double* out, double* out_tail) {
    if (!h || !x || !params || !out || !out_tail) return -1;
    CglPar par;
    BK_TRY(flow_params(h->prob, params, nparams, &par));
    BK_TRY(shoot_check(h, "bk_shooting_residual"));
    if (!std::isfinite(T)) return set_error(h->ctx, "bk_shooting_residual: T must be finite");
    if (out == x) return set_error(h->ctx, "bk_shooting_residual: out must not alias x");
    BK_TRY(flow_march(h->flow, kFlowBase, par, x, nullptr, shoot_tau(h, T), h->nsteps, h->phi, nullptr, nullptr, nullptr, nullptr, nullptr));
    double dot = 0.0;
    BK_TRY(shoot_close(h, false, 0.0, h->phi, h->phi, x, h->normal, out, &dot));
    *out_tail = (dot - h->c0) * T;
    return 0;
}

int bk_shooting_jvp(bk_shooting* h, const double* x, double T, const double* params, int nparams, const double* dx, double dT,
                    double* out, double* out_tail) {
    if (!h || !x || !params || !dx || !out || !out_tail) return -1;
    CglPar par;
    BK_TRY(flow_params(h->prob, params, nparams, &par));
    BK_TRY(shoot_check(h, "bk_shooting_jvp"));
    if (!std::isfinite(T)) return set_error(h->ctx, "bk_shooting_jvp: T must be finite");
    if (out == x || out == dx) return set_error(h->ctx, "bk_shooting_jvp: out must not alias x or dx");
    double sx = 0.0, dot = 0.0;
    BK_TRY(v_dot(h->ctx, h->N(), x, h->normal, &sx));
    BK_TRY(flow_march(h->flow, kFlowBoth, par, x, dx, shoot_tau(h, T), h->nsteps, h->phi, h->dphi(), nullptr, nullptr, nullptr, nullptr));
    BK_TRY(shoot_field(h, params, h->phi, h->fphi()));
    BK_TRY(shoot_close(h, true, (1.0 / h->M) * dT, h->dphi(), h->fphi(), dx, h->normal, out, &dot));
    *out_tail = (sx - h->c0) * dT + dot * T;
    return 0;
}

int bk_shooting_op_create(bk_shooting* h, const double* x, double T, const double* params, int nparams, bk_op** out) {
    if (!h || !x || !params || !out) return -1;
    bk_ctx* ctx = h->ctx;
    CglPar par;
    BK_TRY(flow_params(h->prob, params, nparams, &par));
    BK_TRY(shoot_check(h, "bk_shooting_op_create"));
    if (!std::isfinite(T)) return set_error(ctx, "bk_shooting_op_create: T must be finite");
    ShootOp* op = new ShootOp();
    op->ctx = ctx; op->n = h->len(); op->ntail = 1;
    op->h = h; op->x = x; op->T = T; op->par = par;
    for (int i = 0; i < nparams; ++i) op->params[i] = params[i];
    op->stored = ctx->opt("shooting_store", 1.0) != 0.0 && shoot_store_fits(h);
    int s = v_dot(ctx, h->N(), x, h->normal, &op->s0);
    op->s0 -= h->c0;
    if (s == 0) s = op->st.alloc(h, "bk_shooting_op_create", op->stored);
    if (s == 0 && op->stored) {
        if (s == 0) s = flow_march(h->flow, kFlowBase, par, x, nullptr, shoot_tau(h, T), h->nsteps, h->phi, nullptr, op->st.u, op->st.a, nullptr, nullptr);
        if (s == 0) s = shoot_field(h, op->params, h->phi, op->st.fphi);
        op->base_marches = 1;
    }
    if (s != 0) { delete op; return s; }
    *out = op;
    return 0;
}

int bk_shooting_monodromy_create(bk_shooting* h, const double* x, double T, const double* params, int nparams, bk_op** out) {
    if (!h || !x || !params || !out) return -1;
    bk_ctx* ctx = h->ctx;
    CglPar par;
    BK_TRY(flow_params(h->prob, params, nparams, &par));
    if (!std::isfinite(T)) return set_error(ctx, "bk_shooting_monodromy_create: T must be finite");
    if (!shoot_store_fits(h))
        return set_error(ctx, "bk_shooting_monodromy_create: the base trajectory (2 x %d x %zu doubles) exceeds option shooting_store_max",
                         h->nsteps, h->len());
    if (!h->flow1) BK_TRY(flow_create(h->prob, 1, "bk_shooting_monodromy_create", &h->flow1));
    ShootMonodromyOp* op = new ShootMonodromyOp();
    op->ctx = ctx; op->n = h->N(); op->ntail = 0;
    op->h = h; op->T = T; op->par = par;
    int s = op->st.alloc(h, "bk_shooting_monodromy_create", true);
    if (s == 0) s = flow_march(h->flow, kFlowBase, par, x, nullptr, shoot_tau(h, T), h->nsteps, h->phi, nullptr, op->st.u, op->st.a, nullptr, nullptr);
    op->base_marches = 1;
    if (s != 0) { delete op; return s; }
    *out = op;
    return 0;
}

int bk_shooting_op_stats(bk_op* o, int* stored, long long* base_marches, long long* applications) {
    if (!o) return -1;
    if (ShootOp* op = dynamic_cast<ShootOp*>(o)) {
        if (stored) *stored = op->stored ? 1 : 0;
        if (base_marches) *base_marches = op->base_marches;
        if (applications) *applications = op->applications;
        return 0;
    }
    if (ShootMonodromyOp* op = dynamic_cast<ShootMonodromyOp*>(o)) {
        if (stored) *stored = 1;
        if (base_marches) *base_marches = op->base_marches;
        if (applications) *applications = op->applications;
        return 0;
    }
    return set_error(o->ctx, "bk_shooting_op_stats: op is not an operator of bk_shooting_op_create or bk_shooting_monodromy_create");
}

int bk_shooting_op_apply(bk_op* o, const double* dx, double dT, double* out, double* out_tail) {
    if (!o || !dx || !out || !out_tail) return -1;
    ShootOp* op = dynamic_cast<ShootOp*>(o);
    if (!op) return set_error(o->ctx, "bk_shooting_op_apply: op is not an operator of bk_shooting_op_create");
    if (out == op->x) return set_error(o->ctx, "bk_shooting_op_apply: out must not alias the state of the operator");
    return op->apply(dx, &dT, 0.0, 1.0, out, out_tail);
}

int bk_shooting_transform_paths(bk_shooting* h, int paths[2]) {
    if (!h || !paths) return -1;
    return bk_flow_transform_paths(h->flow, paths);
}

int bk_shooting_solve(bk_ctx* ctx, bk_op* op, const double* rhs, double rhs_tail, double* x, double* x_tail, const bk_gmres_opts* opts,
                      bk_solve_result* result) {
    if (!ctx || !op || !rhs || !x || !x_tail || !opts || !result) return -1;
    if (!dynamic_cast<ShootOp*>(op)) return set_error(ctx, "bk_shooting_solve: op is not an operator of bk_shooting_op_create");
    if (opts->flavor >= BK_KRYLOV_MINRES) return set_error(ctx, "bk_shooting_solve: the shooting Jacobian is not symmetric (use a GMRES flavor)");
    if (opts->pr) return set_error(ctx, "bk_shooting_solve: the solve runs unpreconditioned");
    if (x == rhs) return set_error(ctx, "bk_shooting_solve: x must not alias rhs");
    GmresResult r;
    BK_TRY(gmres_core(ctx, op, rhs, &rhs_tail, x, x_tail, 0.0, 1.0, *opts, &r));
    solve_result_set(result, r);
    return 0;
}

}  // extern "C"
