// The fold of limit cycles of the trapezoid periodic-orbit functional, matrix-free, for BK_PDE_CGL2D on one rank
// (src/codim2/MinAugFold.jl on the Trapeze functional; examples/cGL2d.jl:347-392): the border row of the fold system from the
// second derivative, doubly bordered solves that stay regular where dG is singular, the bordered vectors, the fold linear solver
// and the Newton loop.  The functional, its adjoint and the preconditioners of both are potrap.hip, whose notation this file keeps:
// K = M - 1, next(j) = j + 1 and next(K - 1) = 0, hh = T (1 / M) / 2, s_j = w_j + w_next(j), q_j = J_j^T s_j,
// dG = [A c; phi^T 0] with c_i = -(1 / (2 M)) (F_i + F_prev(i)), c_K = 0.
#include <cmath>

#include "cgl_pw.h"
#include "common.h"
#include "hopf_pw.h"
#include "minaug.h"
#include "ops.h"
#include "potrap_pw.h"
#include "stream.h"

namespace bk {

namespace {

// The border row of the fold system and its two scalars in one pass over u, v, w (3 streams read, 1 written) on the skeleton of
// potrap_pw.h, walked as the adjoint march (step `row` loads slice next(row) of w, the loaded slice is carried):
//     out_j = hh (B_j[v_j, .])^T s_j + dv q_j (j < K), out_K = 0;   s[0] = sum_j <q_j, v_j>;   s[1] = sum_j <s_j, hh D_p(u_j) v_j + dv d_pF(u_j)>
// with B the pointwise Hessian (cgl_hess), D_p = dJ/dp (cgl_djdp), d_pF pointwise (cgl_dpar), dv = v_T / M / 2.
struct PoFoldBorder {
    static constexpr int NV = 2;
    static constexpr bool OPEN = false;
    CglPar par;
    CglCoef coef;
    double hh, dv;
    const double* u;
    const double* v;
    const double* w;
    double* out;
    using Carry = PoPoint;
    __device__ __forceinline__ void step(const PoAt& a, int row, bool store, PoPoint& wc, double* s) const {
        const size_t n = a.n, idx = a.idx;
        const size_t sn = (size_t)(row + 1 == a.g.K ? 0 : row + 1) * a.N;
        const PoPoint wn = po_load(a, w + sn);
        if (store) {
            const size_t sl = (size_t)row * a.N;
            const double u1 = u[sl + idx], u2 = u[sl + idx + n];
            const double v1 = v[sl + idx], v2 = v[sl + idx + n];
            double f1u, f1v, f2u, f2v, h[6], d[4], p1, p2;
            cgl_jac(par, u1, u2, f1u, f1v, f2u, f2v);
            cgl_hess(coef, u1, u2, h);
            cgl_djdp(coef.ipar, u1, u2, d);
            cgl_dpar(coef.ipar, u1, u2, p1, p2);
            const double s1 = wc.c1 + wn.c1, s2 = wc.c2 + wn.c2;
            const double q1 = (wc.d1 + wn.d1) + f1u * s1 + f2u * s2;
            const double q2 = (wc.d2 + wn.d2) + f1v * s1 + f2v * s2;
            const double t1 = s1 * (h[0] * v1 + h[1] * v2) + s2 * (h[3] * v1 + h[4] * v2);
            const double t2 = s1 * (h[1] * v1 + h[2] * v2) + s2 * (h[4] * v1 + h[5] * v2);
            out[sl + idx] = hh * t1 + dv * q1;
            out[sl + idx + n] = hh * t2 + dv * q2;
            s[0] = fma(q1, v1, s[0]);
            s[0] = fma(q2, v2, s[0]);
            const double e1 = hh * (d[0] * v1 + d[1] * v2) + dv * p1;
            const double e2 = hh * (d[2] * v1 + d[3] * v2) + dv * p2;
            s[1] = fma(s1, e1, s[1]);
            s[1] = fma(s2, e2, s[1]);
        }
        wc = wn;
    }
    __device__ __forceinline__ void closure(const PoAt& a, double*) const {
        out[(size_t)a.g.K * a.N + a.idx] = 0.0;
        out[(size_t)a.g.K * a.N + a.idx + a.n] = 0.0;
    }
};

// sigx = the first M N entries of the border row, *sigxT its T entry, *sigp = sigma_p for params[ipar]
int pofold_border(bk_potrap* h, const CglPar& par, const CglCoef& coef, const double* u, double T, const double* v, double vT,
                  const double* w, double* sigx, double* sigxT, double* sigp) {
    double s[2] = {0.0, 0.0};
    BK_TRY(po_march(h, "pofold", "pofold_border", 8.0 * h->len() * 4,
                    PoFoldBorder{par, coef, T * (1.0 / h->M) / 2.0, vT / h->M / 2.0, u, v, w, sigx}, s));
    *sigxT = s[0] / h->M / 2.0;
    *sigp = s[1];
    return 0;
}

// [A a; b' c][x; (t, sigma)] = [rhs; (rhsT, rhsB)] for an orbit operator A with its T tail (dG or dG^T) by ONE GMRES on the
// bordered PoPrecOp.  a, b: device vectors with host T entries; rhs (device, T entry, border scalar); x device, xt[2] = (T entry,
// border scalar)
int potrap_bordered_solve(bk_ctx* ctx, bk_op* op, bk_precond* pl, const double* a, double aT, const double* b, double bT, double c,
                          const double* rhs, double rhsT, double rhsB, double* x, double xt[2], const bk_gmres_opts& opts,
                          GmresResult* r) {
    WsGuard ws(ctx);
    double *tmp = nullptr, *prhs = nullptr, *atil = nullptr;
    BK_TRY(ws.get(op->n, &tmp));
    BK_TRY(ws.get(op->n, &prhs));
    BK_TRY(ws.get(op->n, &atil));
    BK_TRY(pl->apply(a, atil));
    BK_TRY(pl->apply(rhs, prhs));
    PoPrecOp W;
    W.ctx = ctx; W.n = op->n; W.ntail = 2;
    W.A = op; W.P = pl; W.tmp = tmp; W.atil = atil; W.bu = b; W.aT = aT; W.bT = bT; W.c = c;
    const double bt[2] = {rhsT, rhsB};
    return gmres_core(ctx, &W, prhs, bt, x, xt, 0.0, 1.0, opts, r);
}

struct OpPair {
    bk_op* J = nullptr;
    bk_op* Jt = nullptr;
    ~OpPair() { if (J) bk_op_destroy(J); if (Jt) bk_op_destroy(Jt); }
};

// [dG a; b' 0][v; sigma] = [0; 1] and [dG^T b; a' 0][w; sigma2] = [0; 1] (MinAugFold.jl:15-69), one bordered solve each
int pofold_terms(bk_potrap* h, const double* u, double T, const double* par, const double* a, double aT, const double* b, double bT,
                 bk_precond* pl, bk_precond* plT, const bk_gmres_opts& opts, const double* zero, double* v, double* vT, double* w,
                 double* wT, double* sigma, int* converged, int it[2]) {
    OpPair jp;
    BK_TRY(bk_potrap_op_create(h, u, T, par, 6, &jp.J));
    BK_TRY(bk_potrap_op_adjoint_create(h, u, T, par, 6, &jp.Jt));
    BK_TRY(potrap_pair_check(h->ctx, "bk_potrap_fold_terms", jp.J, pl));
    BK_TRY(potrap_pair_check(h->ctx, "bk_potrap_fold_terms", jp.Jt, plT));
    GmresResult r0, r1;
    double xt[2];
    BK_TRY(potrap_bordered_solve(h->ctx, jp.J, pl, a, aT, b, bT, 0.0, zero, 0.0, 1.0, v, xt, opts, &r0));
    *vT = xt[0];
    *sigma = xt[1];
    BK_TRY(potrap_bordered_solve(h->ctx, jp.Jt, plT, b, bT, a, aT, 0.0, zero, 0.0, 1.0, w, xt, opts, &r1));
    *wT = xt[0];
    *converged = r0.converged & r1.converged;
    it[0] = r0.niter;
    it[1] = r1.niter;
    return 0;
}

}  // namespace
}  // namespace bk

using namespace bk;

extern "C" {

int bk_potrap_bordered_solve(bk_ctx* ctx, bk_op* op, bk_precond* pl, const double* a, double a_tail, const double* b, double b_tail,
                             double c, const double* rhs, double rhs_tail, double rhs_border, double* x, double* x_tail,
                             double* x_border, const bk_gmres_opts* opts, bk_solve_result* result) {
    if (!ctx || !op || !pl || !a || !b || !rhs || !x || !x_tail || !x_border || !opts || !result) return -1;
    BK_TRY(potrap_pair_check(ctx, "bk_potrap_bordered_solve", op, pl));
    BK_TRY(potrap_opts_check(ctx, "bk_potrap_bordered_solve", opts));
    if (x == rhs || x == a || x == b) return set_error(ctx, "bk_potrap_bordered_solve: x must not alias rhs, a or b");
    GmresResult r;
    double xt[2] = {0.0, 0.0};
    BK_TRY(potrap_bordered_solve(ctx, op, pl, a, a_tail, b, b_tail, c, rhs, rhs_tail, rhs_border, x, xt, *opts, &r));
    *x_tail = xt[0];
    *x_border = xt[1];
    solve_result_set(result, r);
    return 0;
}

int bk_potrap_fold_border(bk_potrap* h, const double* u, double T, const double* params, int nparams, int ipar, const double* v,
                          double v_T, const double* w, double* sigx, double* sigx_T, double* sigma_p) {
    if (!h || !u || !params || !v || !w || !sigx || !sigx_T || !sigma_p) return -1;
    CglPar par;
    CglCoef coef;
    BK_TRY(potrap_params(h, params, nparams, &par));
    BK_TRY(hopf_coef(h->prob, params, nparams, ipar, &coef));
    if (sigx == u || sigx == v || sigx == w) return set_error(h->ctx, "bk_potrap_fold_border: sigx must not alias u, v or w");
    return pofold_border(h, par, coef, u, T, v, v_T, w, sigx, sigx_T, sigma_p);
}

int bk_potrap_fold_terms(bk_potrap* h, const double* u, double T, const double* params, int nparams, const double* a, double a_T,
                         const double* b, double b_T, bk_precond* pl, bk_precond* pl_adjoint, const bk_gmres_opts* opts, double* v,
                         double* v_T, double* w, double* w_T, double* sigma, int* converged, int itlinear[2]) {
    if (!h || !u || !params || !a || !b || !pl || !pl_adjoint || !opts || !v || !v_T || !w || !w_T || !sigma || !converged || !itlinear)
        return -1;
    CglPar par;
    BK_TRY(potrap_params(h, params, nparams, &par));
    BK_TRY(potrap_check(h, "bk_potrap_fold_terms"));
    BK_TRY(potrap_opts_check(h->ctx, "bk_potrap_fold_terms", opts));
    if (v == w || v == a || v == b || w == a || w == b || v == u || w == u)
        return set_error(h->ctx, "bk_potrap_fold_terms: v and w must be distinct from each other and from u, a and b");
    WsGuard ws(h->ctx);
    double* zero = nullptr;
    BK_TRY(ws.get(h->len(), &zero));
    BK_TRY(v_zero(h->ctx, h->len(), zero));
    return pofold_terms(h, u, T, params, a, a_T, b, b_T, pl, pl_adjoint, *opts, zero, v, v_T, w, w_T, sigma, converged, itlinear);
}

int bk_potrap_fold_linsolve(bk_potrap* h, const double* u, double T, const double* params, int nparams, int ipar, const double* v,
                            double v_T, const double* w, bk_precond* pl, int nrhs, const double* const* rhsu, const double* rhsT,
                            const double* rhsp, const bk_gmres_opts* opts, double* const* dX, double* dXT, double* dsigma,
                            int* converged, int* itlinear) {
    if (!h || !u || !params || !v || !w || !pl || !rhsu || !rhsT || !rhsp || !opts || !dX || !dXT || !dsigma) return -1;
    bk_ctx* ctx = h->ctx;
    CglPar par;
    CglCoef coef;
    BK_TRY(potrap_params(h, params, nparams, &par));
    BK_TRY(hopf_coef(h->prob, params, nparams, ipar, &coef));
    BK_TRY(potrap_check(h, "bk_potrap_fold_linsolve"));
    BK_TRY(potrap_opts_check(ctx, "bk_potrap_fold_linsolve", opts));
    BK_TRY(minaug_check_rhs(ctx, "bk_potrap_fold_linsolve", nrhs, rhsu, dX));
    for (int k = 0; k < nrhs; ++k)
        if (dX[k] == u || dX[k] == v || dX[k] == w) return set_error(ctx, "bk_potrap_fold_linsolve: dX must not alias u, v or w");
    const size_t n = h->len();
    WsGuard ws(ctx);
    double *sigx = nullptr, *dpG = nullptr;
    BK_TRY(ws.get(n, &sigx));
    BK_TRY(ws.get(n, &dpG));
    double sxT = 0.0, sp = 0.0;
    BK_TRY(pofold_border(h, par, coef, u, T, v, v_T, w, sigx, &sxT, &sp));
    BK_TRY(bk_potrap_dparam(h, u, T, params, nparams, ipar, dpG));
    OpPair jp;
    BK_TRY(bk_potrap_op_create(h, u, T, params, nparams, &jp.J));
    BK_TRY(potrap_pair_check(ctx, "bk_potrap_fold_linsolve", jp.J, pl));
    int cv = 1, it = 0;
    for (int k = 0; k < nrhs; ++k) {
        GmresResult r;
        double xt[2] = {0.0, 0.0};
        BK_TRY(potrap_bordered_solve(ctx, jp.J, pl, dpG, 0.0, sigx, sxT, sp, rhsu[k], rhsT[k], rhsp[k], dX[k], xt, *opts, &r));
        dXT[k] = xt[0];
        dsigma[k] = xt[1];
        cv &= r.converged;
        it += r.niter;
    }
    if (converged) *converged = cv;
    if (itlinear) *itlinear = it;
    return 0;
}

int bk_potrap_newton_fold(bk_potrap* h, double* u, double* T, double* p, const double* params, int nparams, int ipar, const double* a,
                          double a_T, const double* b, double b_T, bk_precond* pl, bk_precond* pl_adjoint, const bk_newton_opts* no,
                          const bk_gmres_opts* opts, double* v, double* v_T, double* w, double* w_T, double* sigma,
                          bk_newton_result* res, int* itlinear_steps) {
    if (!h || !u || !T || !p || !params || !a || !b || !pl || !pl_adjoint || !no || !opts || !v || !v_T || !w || !w_T || !sigma || !res)
        return -1;
    bk_ctx* ctx = h->ctx;
    CglPar cp;
    CglCoef cc;
    BK_TRY(potrap_params(h, params, nparams, &cp));                 // the problem kind, the parameter count and index
    BK_TRY(hopf_coef(h->prob, params, nparams, ipar, &cc));
    BK_TRY(potrap_check(h, "bk_potrap_newton_fold"));
    BK_TRY(potrap_opts_check(ctx, "bk_potrap_newton_fold", opts));
    if (no->max_iterations > BK_MAX_NEWTON_ITER) return set_error(ctx, "max_iterations > %d", BK_MAX_NEWTON_ITER);
    if (v == w || v == a || v == b || w == a || w == b || v == u || w == u || u == a || u == b)
        return set_error(ctx, "bk_potrap_newton_fold: u, v and w must be distinct from a and b and from each other");
    const size_t n = h->len();
    const bool inf = no->norm_inf != 0;
    WsGuard ws(ctx);
    double *fx = nullptr, *dX = nullptr, *zero = nullptr, *sigx = nullptr, *dpG = nullptr;
    BK_TRY(ws.get(n, &fx));
    BK_TRY(ws.get(n, &dX));
    BK_TRY(ws.get(n, &zero));
    BK_TRY(ws.get(n, &sigx));
    BK_TRY(ws.get(n, &dpG));
    BK_TRY(v_zero(ctx, n, zero));
    double par[6];
    for (int i = 0; i < 6; ++i) par[i] = params[i];
    double pc = *p, Tc = *T, gT = 0.0;
    int nstep = 0;
    // the fold residual (G, sigma) at (u, Tc, pc) with the bordered vectors of this point, which the step from it reuses
    auto point = [&](double* r, int* itl) -> int {
        par[ipar] = pc;
        int cv = 0, it[2] = {0, 0};
        BK_TRY(pofold_terms(h, u, Tc, par, a, a_T, b, b_T, pl, pl_adjoint, *opts, zero, v, v_T, w, w_T, sigma, &cv, it));
        *itl = it[0] + it[1];
        if (itlinear_steps) { itlinear_steps[3 * nstep] = it[0]; itlinear_steps[3 * nstep + 1] = it[1]; }
        BK_TRY(bk_potrap_residual(h, u, Tc, par, 6, fx, &gT));
        double g = 0.0;
        if (inf) {
            BK_TRY(v_nrminf(ctx, n, fx, &g));
            *r = fmax(fmax(g, fabs(gT)), fabs(*sigma));
            if (g != g || gT != gT || *sigma != *sigma) *r = NAN;
        } else {
            BK_TRY(v_nrm2(ctx, n, fx, &g));
            *r = sqrt(g * g + gT * gT + *sigma * *sigma);
        }
        return 0;
    };
    // [dG d_pG; sigma_x' sigma_p][dX; dp] = [G; sigma] as one bordered solve (MinAugFold.jl:136-145); (u, T, p) -= (dX, dp)
    auto step = [&](int* itl) -> int {
        par[ipar] = pc;
        BK_TRY(potrap_params(h, par, 6, &cp));
        BK_TRY(hopf_coef(h->prob, par, 6, ipar, &cc));
        double sxT = 0.0, sp = 0.0, xt[2] = {0.0, 0.0};
        BK_TRY(pofold_border(h, cp, cc, u, Tc, v, *v_T, w, sigx, &sxT, &sp));
        BK_TRY(bk_potrap_dparam(h, u, Tc, par, 6, ipar, dpG));
        OpPair jp;
        BK_TRY(bk_potrap_op_create(h, u, Tc, par, 6, &jp.J));
        GmresResult r;
        BK_TRY(potrap_bordered_solve(ctx, jp.J, pl, dpG, 0.0, sigx, sxT, sp, fx, gT, *sigma, dX, xt, *opts, &r));
        *itl = r.niter;
        if (itlinear_steps) itlinear_steps[3 * nstep + 2] = r.niter;
        nstep += 1;
        BK_TRY(v_axpby(ctx, n, -1.0, dX, 1.0, u));
        Tc -= xt[0];
        pc -= xt[1];
        return 0;
    };
    BK_TRY(minaug_newton(no, res, u, fx, &pc, point, step));
    *p = pc;
    *T = Tc;
    return 0;
}

}  // extern "C"
