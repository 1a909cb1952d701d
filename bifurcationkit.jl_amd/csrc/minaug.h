// What the minimally augmented fold (fold.hip) and Hopf (hopf.hip) formulations share: the J \ rhs_k, J \ dpF solves of their
// linear solvers, the checks of the bk_*_linsolve entries and the Newton loop of bk_newton_fold / bk_newton_hopf.  What differs
// between them -- the pointwise tensors, the contractions, the bordered solves, the norms and the 1 x 1 or 2 x 2 scalar system --
// stays in the two files.  JPair and minaug_check also serve the normal forms (hopf_nf.hip, nf1d.hip).
// Internal header.
#pragma once
#include <cmath>

#include "common.h"
#include "ops.h"

namespace bk {
namespace {

// ------------------------------------------------------------------ the formulation
int minaug_check(bk_ctx* ctx, bk_problem* prob, const char* what) {
    if (prob->ctx != ctx) return set_error(ctx, "%s: the problem belongs to another context", what);
    return 0;
}

// J(x, par), and its adjoint when asked for; destroyed by the guard
struct JPair {
    bk_op* J = nullptr;
    bk_op* Jt = nullptr;
    ~JPair() { if (J) bk_op_destroy(J); if (Jt) bk_op_destroy(Jt); }
    int make(bk_problem* prob, const double* x, const double* par, int np, bool adjoint = false) {
        BK_TRY(bk_jacobian(prob, x, par, np, &J));
        return adjoint ? bk_jacobian_adjoint(prob, x, par, np, &Jt) : 0;
    }
};

// The solves of a minimally augmented linear solver: x1_k = J \ rhsu_k into dX[k] (k < nrhs <= 2), x2 = J \ dpF with the analytic
// dpF, the first two concurrently (linsolve2).  X = the vectors of the contraction pass, (x1_0, x1_1 | x2, x2): nrhs + 1 are read.
struct MinAugSolves {
    const double* X[3];
    double* x2;
    int converged, niter;
};
int minaug_solves(bk_ctx* ctx, bk_problem* prob, bk_op* J, const double* x, int ipar, int nrhs, const double* const* rhsu,
                  const bk_gmres_opts& lo, bk_precond* pl, double* const* dX, WsGuard& ws, MinAugSolves* S) {
    const size_t n = prob->nloc;
    double* dpF = nullptr;
    BK_TRY(ws.get(n, &dpF));
    BK_TRY(ws.get(n, &S->x2));
    const size_t npts = prob->desc.pde == BK_PDE_CGL2D ? n / 2 : n;              // grid points per field
    BK_TRY(pde_dparam(ctx, prob->desc.pde, ipar, npts, 1.0, x, dpF));
    GmresResult r0, r1, r2;
    BK_TRY(linsolve2(ctx, J, rhsu[0], dX[0], dpF, S->x2, 0.0, 1.0, lo, pl, &r0, &r2));
    S->converged = r0.converged & r2.converged;
    S->niter = r0.niter + r2.niter;
    if (nrhs == 2) {
        BK_TRY(linsolve(ctx, J, rhsu[1], dX[1], 0.0, 1.0, lo, pl, &r1));
        S->converged &= r1.converged;
        S->niter += r1.niter;
    }
    S->X[0] = dX[0];
    S->X[1] = nrhs == 2 ? dX[1] : S->x2;
    S->X[2] = S->x2;
    return 0;
}

// dX_k = x1_k - dp_k x2 with dp_k = dp[k * stride], the parameter component of the k-th solution
int minaug_update(bk_ctx* ctx, size_t n, const MinAugSolves& S, int nrhs, const double* dp, int stride, double* const* dX) {
    for (int k = 0; k < nrhs; ++k) BK_TRY(v_axpby(ctx, n, -dp[k * stride], S.x2, 1.0, dX[k]));
    return 0;
}

// Context option fold_bordered (default 0 = the solves above): the formulation runs on bordered systems that stay regular where J is
// singular, each ONE GMRES on [J a; b' c] left-preconditioned by diag(Pl, 1) (bordered.hip: bls_matrixfree_pl).
bool minaug_bordered(bk_ctx* ctx) { return ctx->opt("fold_bordered", 0.0) != 0.0; }

// [J a; b' c][u1; u2] = [rhst; rhsb] with an m-column border (fold: m = 1; the shape is what a Hopf system on (re, im) pairs with a
// two-scalar border would hand over, m = 2 and c 2 x 2 row-major).  atil (optional): Pl^-1 a_j shared between solves.
int minaug_bordered_solve(bk_ctx* ctx, bk_op* J, int m, const double* const* a, const double* const* b, const double* c,
                          const double* rhst, const double* rhsb, const bk_gmres_opts& lo, bk_precond* pl, double* u1, double* u2,
                          GmresResult* res, const double* const* atil = nullptr) {
    return bls_matrixfree_pl(ctx, J, m, a, b, 1.0, c, rhst, rhsb, false, 0.0, lo, pl, u1, u2, res, atil);
}

// Context option hopf_bordered (default 0 = BorderingBLS, two shifted solves per bordered vector): a bordered system
// [shift + J, a; b^H, 0][X; l] = [R; n] on (re, im) pairs as ONE GMRES left-preconditioned by diag(Pl, 1) (bordered.hip:
// bls_matrixfree_pl_cshift), regular where shift + J is singular -- the bordered vectors of hopf.hip and the H21 solve of bautin.hip.
bool minaug_hopf_bordered(bk_ctx* ctx) { return ctx->opt("hopf_bordered", 0.0) != 0.0; }
int minaug_hopf_bordered_solve(bk_ctx* ctx, bk_op* J, const double* ar, const double* ai, const double* br, const double* bi,
                               const double* Rr, const double* Ri, double nr, double shift_im, const bk_gmres_opts& lo,
                               bk_precond* pl, double* Xr, double* Xi, double l[2], GmresResult* res) {
    if (!pl) return set_error(ctx, "hopf: hopf_bordered = 1 needs the left preconditioner");
    const double* const a[2] = {ar, ai};
    const double* const b[2] = {br, bi};
    const double* const R[2] = {Rr, Ri};
    const double c[2] = {0.0, 0.0}, nn[2] = {nr, 0.0}, shift[2] = {0.0, shift_im};
    return bls_matrixfree_pl_cshift(ctx, J, a, b, 1.0, c, R, nn, shift, lo, pl, Xr, Xi, l, res);
}

// the right-hand sides and outputs of bk_fold_linsolve / bk_hopf_linsolve (`what`)
int minaug_check_rhs(bk_ctx* ctx, const char* what, int nrhs, const double* const* rhsu, double* const* dX) {
    if (nrhs < 1 || nrhs > 2) return set_error(ctx, "%s: 1 or 2 right-hand sides (got %d)", what, nrhs);
    for (int k = 0; k < nrhs; ++k) {
        if (!rhsu[k] || !dX[k]) return -1;
        for (int j = 0; j < nrhs; ++j)
            if (dX[k] == rhsu[j]) return set_error(ctx, "%s: dX must not alias a right-hand side", what);
    }
    if (nrhs == 2 && dX[0] == dX[1]) return set_error(ctx, "%s: dX[0] and dX[1] must be distinct", what);
    return 0;
}

// Newton on G(x, p[, omega]) = (F, sigma) (src/Newton.jl:66-114).  point(&r, &it): the residual of G at the current unknowns into
// fx and sigma, its norm r, with the bordered vectors of that point, which step(&it) -- one Newton update of x and the scalar
// unknowns -- reuses; both report their GMRES iterations.  x, fx and *p (the current parameter) are what the callback sees.
template <class Point, class Step>
int minaug_newton(const bk_newton_opts* no, bk_newton_result* res, const double* x, const double* fx, const double* p,
                  Point&& point, Step&& step) {
    double r;
    int itlin = 0, nstep = 0;
    BK_TRY(point(&r, &itlin));
    res->residuals[0] = r;
    int compute = newton_cb(no, x, fx, r, 0, 0, *p, nullptr, NAN, 1);
    while (nstep < no->max_iterations && r > no->tol && compute) {
        int its = 0, itp = 0;
        BK_TRY(step(&its));
        BK_TRY(point(&r, &itp));
        itlin += its + itp;
        nstep += 1;
        res->residuals[nstep] = r;
        compute = newton_cb(no, x, fx, r, nstep, its + itp, *p, nullptr, NAN, 1);
    }
    res->converged = (res->residuals[nstep] < no->tol) & newton_cb(no, x, fx, r, nstep, 0, *p, nullptr, NAN, 1);
    res->itnewton = nstep;
    res->itlinear = itlin;
    return 0;
}

}  // namespace
}  // namespace bk
