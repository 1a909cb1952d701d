// Floquet multipliers of the trapezoid periodic orbits of cGL by ONE space-time solve per application of the monodromy, in the
// place of the K = M - 1 sequential slice solves of MonodromyQaD_matrix_free(::Trapeze, ...) (src/periodicorbit/Floquet.jl:285-315):
//
//     x <- (I - hh J_i)^-1 (I + hh J_prev(i)) x,   i = 0 .. K - 1,   prev(0) = K - 1,   hh = T (1 / M) / 2
//
// The same vector is the last slice of the solution of the block lower-bidiagonal initial-value system over all K slices
//
//     A_i y_i - B_{i-1} y_{i-1} = 0 (i >= 1),    A_0 y_0 = B_{K-1} x,    A_i = I - hh J_i,  B_i = I + hh J_i,    M x = y_{K-1},
//
// the rows i < K of dG (potrap.hip) with the cyclic link of row 0 cut.  All K slices y_0 .. y_{K-1} are the space-time
// eigenfunction when x is a Floquet eigenvector (the Val(:ExtractEigenVector) method, :319-355): they come out of the same solve.
//
// Kernels.  The pass IvpMarch applies the initial-value operator to K slices in one launch on the marching skeleton of
// potrap_pw.h (B_{i-1} y_{i-1}'s two parts carried in registers): three streams of 8 K N bytes, u read, y read, out written; no
// F, no period column, no phase dot, no reduction.  The preconditioner is the initial-value kind of potrap.hip's PoPrecond.
#include <cmath>

#include "cgl_pw.h"
#include "common.h"
#include "hopf_pw.h"
#include "ops.h"
#include "potrap_pw.h"
#include "stream.h"

namespace bk {
namespace {

// Rows [r0, r1) of the K rows
//     out_i = (y_i - hh J_i y_i) - (y_{i-1} + hh J_{i-1} y_{i-1}),   out_0 = y_0 - hh J_0 y_0.
// A chunk with r0 > 0 evaluates slice r0 - 1 first (t = -1) by the same code as every other slice, without a store; chunk 0 starts
// from exact zeros (OPEN), and x - 0 is x: a row's bits do not depend on the chunking.  The vectors hold K slices: no closure row.
struct IvpMarch {
    static constexpr int NV = 0;
    static constexpr bool OPEN = true;
    CglPar par;
    double hh;                     // h / 2 = T (1 / M) / 2
    const double* u;               // the orbit: slice i at u + i N
    const double* y;
    double* out;
    struct Carry { double b1, b2; };   // y_{i-1} + hh J_{i-1} y_{i-1}
    __device__ __forceinline__ void step(const PoAt& a, int row, bool store, Carry& c, double*) const {
        const size_t n = a.n, idx = a.idx, sl = (size_t)row * a.N;
        const double c1 = u[sl + idx], c2 = u[sl + idx + n];
        const PoPoint v = po_load(a, y + sl);
        double f1u, f1v, f2u, f2v;
        cgl_jac(par, c1, c2, f1u, f1v, f2u, f2v);
        const double J1 = hh * (v.d1 + f1u * v.c1 + f1v * v.c2);
        const double J2 = hh * (v.d2 + f2u * v.c1 + f2v * v.c2);
        if (store) {
            out[sl + idx] = (v.c1 - J1) - c.b1;
            out[sl + idx + n] = (v.c2 - J2) - c.b2;
        }
        c.b1 = v.c1 + J1;
        c.b2 = v.c2 + J2;
    }
    __device__ __forceinline__ void closure(const PoAt&, double*) const {}
};

// the marching pass on K slices; algorithmic bytes: u read, y read, out written
int ivp_march(bk_potrap* h, const CglPar& par, const double* u, double T, const double* y, double* out) {
    return po_march(h, "monodromy", "monodromy_march", 8.0 * 2 * h->n * (h->M - 1) * 3, IvpMarch{par, T * (1.0 / h->M) / 2.0, u, y, out},
                    nullptr);
}

// the initial-value operator on K slices as a bk_op without a tail; references u
struct IvpOp : bk_op {
    bk_potrap* h = nullptr;
    const double* u = nullptr;
    double T = 0.0;
    CglPar par{};
    int apply(const double* x, const double*, double a0, double a1, double* out, double*) override {
        if (out == x) return set_error(ctx, "monodromy operator: out must not alias x");
        BK_TRY(ivp_march(h, par, u, T, x, out));
        if (!(a0 == 0.0 && a1 == 1.0)) BK_TRY(v_axpby(ctx, n, a0, x, a1, out));
        return 0;
    }
};

// x -> y_{K-1}: one left-preconditioned GMRES on the K N unknowns per application; references u
struct MonodromyOp : bk_op {
    IvpOp A;
    PoPrecOp W;                    // A0^-1 (initial-value operator): what the solve iterates on
    PoPrecond* P = nullptr;
    bk_gmres_opts ls{};
    double params[BK_MAX_PARAMS] = {0};
    double* work = nullptr;        // [3 K N]: tmp | the preconditioned right-hand side | y
    int solves = 0, failed = 0, inner_its = 0;
    size_t KN() const { return W.n; }
    double* y() const { return work + 2 * KN(); }
    ~MonodromyOp() override {
        delete P;
        if (work) (void)hipFree(work);
    }
    // y_0 .. y_{K-1} of M x into y()
    int solve(const double* x, GmresResult* r) {
        const int K = A.h->M - 1;
        double *tmp = work, *prhs = work + KN();
        // f_0 = x + hh J_{K-1} x through the stencil kernel, the other rows zero
        BK_TRY(v_zero(ctx, KN(), tmp));
        BK_TRY(A.h->prob->apply(0, x, A.u + (size_t)(K - 1) * n, params, 1.0, P->hh, tmp));
        BK_TRY(P->apply(tmp, prhs));
        BK_TRY(gmres_core(ctx, &W, prhs, nullptr, y(), nullptr, 0.0, 1.0, ls, r));
        solves += 1;
        inner_its += r->niter;
        if (!r->converged) failed += 1;                      // counted, not fatal
        return 0;
    }
    int apply(const double* x, const double*, double a0, double a1, double* out, double*) override {
        if (out == x) return set_error(ctx, "monodromy operator: out must not alias x");
        GmresResult r;
        BK_TRY(solve(x, &r));
        return v_axpbyz(ctx, n, a0, x, a1, y() + KN() - n, out);
    }
};

}  // namespace
}  // namespace bk

using namespace bk;

extern "C" {

int bk_potrap_ivp_march(bk_potrap* h, const double* u, double T, const double* params, int nparams, const double* y, double* out) {
    if (!h || !u || !params || !y || !out) return -1;
    CglPar par;
    BK_TRY(potrap_params(h, params, nparams, &par));
    if (out == y || out == u) return set_error(h->ctx, "bk_potrap_ivp_march: out must not alias y or u");
    return ivp_march(h, par, u, T, y, out);
}

int bk_precond_potrap_ivp_create(bk_potrap* h, double a, double b, double T, bk_precond** out) {
    if (!h || !out) return -1;
    PoPrecond* P = nullptr;
    BK_TRY(po_precond_create(h, kTsIvp, a, b, T, "bk_precond_potrap_ivp_create", &P));
    *out = P;
    return 0;
}

int bk_precond_potrap_ivp_transform_paths(bk_precond* pl, int paths[2]) {
    if (!pl || !paths) return -1;
    PoPrecond* P = po_precond_cast(pl, true);
    if (!P) return set_error(pl->ctx, "bk_precond_potrap_ivp_transform_paths: not a preconditioner of bk_precond_potrap_ivp_create");
    dst_plan_paths(P->plan, paths);
    return 0;
}

int bk_potrap_monodromy_create(bk_potrap* h, const double* u, double T, const double* params, int nparams, double a, double b,
                               const bk_gmres_opts* opts, bk_op** out) {
    if (!h || !u || !params || !opts || !out) return -1;
    bk_ctx* ctx = h->ctx;
    CglPar par;
    BK_TRY(potrap_params(h, params, nparams, &par));
    BK_TRY(potrap_opts_check(ctx, "bk_potrap_monodromy_create", opts, "the initial-value system"));
    PoPrecond* P = nullptr;
    BK_TRY(po_precond_create(h, kTsIvp, a, b, T, "bk_potrap_monodromy_create", &P));
    MonodromyOp* op = new MonodromyOp();
    const size_t N = 2 * h->n;
    op->ctx = ctx; op->n = N; op->ntail = 0;
    op->ls = *opts;
    op->P = P;
    for (int i = 0; i < nparams && i < BK_MAX_PARAMS; ++i) op->params[i] = params[i];
    op->A.ctx = op->W.ctx = ctx; op->A.n = op->W.n = N * (size_t)(h->M - 1); op->A.ntail = op->W.ntail = 0;
    op->A.h = h; op->A.u = u; op->A.T = T; op->A.par = par;
    op->W.A = &op->A; op->W.P = P;
    if (hipMalloc(&op->work, sizeof(double) * 3 * op->W.n) != hipSuccess) {
        op->work = nullptr;
        delete op;
        return set_error(ctx, "bk_potrap_monodromy_create: allocation failed");
    }
    op->W.tmp = op->work;
    *out = op;
    return 0;
}

int bk_potrap_monodromy_solve(bk_op* o, const double* x, double* y_all, int* converged, int* niter) {
    if (!o || !x || !y_all) return -1;
    MonodromyOp* op = dynamic_cast<MonodromyOp*>(o);
    if (!op) return set_error(o->ctx, "bk_potrap_monodromy_solve: op is not an operator of bk_potrap_monodromy_create");
    GmresResult r;
    BK_TRY(op->solve(x, &r));
    BK_TRY(v_copy(op->ctx, op->KN(), op->y(), y_all));
    if (converged) *converged = r.converged;
    if (niter) *niter = r.niter;
    return 0;
}

int bk_potrap_monodromy_stats(bk_op* o, int* solves, int* failed, int* inner_its, int paths[2]) {
    if (!o) return -1;
    MonodromyOp* op = dynamic_cast<MonodromyOp*>(o);
    if (!op) return set_error(o->ctx, "bk_potrap_monodromy_stats: op is not an operator of bk_potrap_monodromy_create");
    if (solves) *solves = op->solves;
    if (failed) *failed = op->failed;
    if (inner_its) *inner_its = op->inner_its;
    if (paths) dst_plan_paths(op->P->plan, paths);
    return 0;
}

}  // extern "C"
