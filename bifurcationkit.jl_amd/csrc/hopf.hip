// Minimally augmented Hopf formulation, matrix-free: src/codim2/MinAugHopf.jl on the preconditioned GMRES path.
//
//   unknowns (x, p, omega), G(x, p, omega) = (F(x, p), Re sigma, Im sigma),
//   [J - i omega, a; b^H, 0][v; sigma] = [0; 1],   [J' + i omega, b; a^H, 0][w; sigma2] = [0; 1]   (:17, :72-76)
//
// With w^H a = 1 the derivatives of sigma are  sigma_x . dx = -w^H d2F(x)[v, dx],  sigma_p = -w^H dJ/dp v,  sigma_omega = i w^H v.
// Defined for BK_PDE_CGL2D, the one problem here whose Jacobian is not symmetric.  Its nonlinearity (examples/cGL2d.jl:24-40)
//   NL(z) = (r + i nu) z - (c3 + i mu) |z|^2 z - c5 |z|^4 z + gamma,   z = u1 + i u2,
// is pointwise and the Laplacian is linear, so d2F = d2NL: per grid point one symmetric 2 x 2 matrix H_f(u) for each field f,
// d2F_f[a, b] = a^T H_f b.  H_f are the u-derivatives of the closed-form Jacobian of stencil.hip:cgl_kernel (f1u, f1v, f2u, f2v);
// dJ/dp is the u-derivative of dparam_kernel's phi_p, a 2 x 2 matrix D_p(u) per point (zero for gamma); both in hopf_pw.h.
// Complex vectors are (re, im) pairs of real device vectors; d2F and dJ/dp act on them by linearity.
#include <cmath>

#include "common.h"
#include "hopf_pw.h"
#include "minaug.h"
#include "ops.h"
#include "stream.h"

namespace bk {

namespace {

// ------------------------------------------------------------------ kernels
// out = d2F(u)[x1, x2] (x2 != NULL) or dJ/dp(u) x1 (x2 == NULL) on the two stacked fields of N points each (bk_hopf_d2f,
// bk_hopf_djdp)
__global__ void __launch_bounds__(kThreads) hopf_pw_kernel(size_t N, const double* __restrict__ u, CglCoef c,
                                                           const double* __restrict__ x1, const double* __restrict__ x2,
                                                           double* __restrict__ out) {
    const size_t stride = (size_t)gridDim.x * kThreads;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < N; i += stride) {
        const double u1 = u[i], u2 = u[i + N], a1 = x1[i], a2 = x1[i + N];
        double o1, o2;
        if (x2) {
            double h[6];
            cgl_hess(c, u1, u2, h);
            const double b1 = x2[i], b2 = x2[i + N];
            o1 = a1 * (h[0] * b1 + h[1] * b2) + a2 * (h[1] * b1 + h[2] * b2);
            o2 = a1 * (h[3] * b1 + h[4] * b2) + a2 * (h[4] * b1 + h[5] * b2);
        } else {
            double d[4];
            cgl_djdp(c.ipar, u1, u2, d);
            o1 = d[0] * a1 + d[1] * a2;
            o2 = d[2] * a1 + d[3] * a2;
        }
        out[i] = o1;
        out[i + N] = o2;
    }
}

// One pass over u, v = (vr, vi), w = (wr, wi) and M real vectors X_k:
//   S_k = w^H d2F(u)[v, X_k] (k < M),   P = w^H dJ/dp(u) v,   Q = w^H v,
// 2 (M + 2) partial sums per workgroup in the order (Re S_0, Im S_0, ..., Re P, Im P, Re Q, Im Q).  Per point the complex
// 2-vector g = sum_f conj(w_f) H_f v does not depend on k, so S_k costs 4 FMAs per point.  The second stage (reduce_finish)
// keeps the fixed order: the sums are bitwise the same run to run and, all-reduced, on every rank.
template <int M>
struct HopfContract {
    static constexpr int NIN = 2 * (5 + M), NV = 2 * (M + 2), U = 1, FIELDS = 2;
    const double* in[NIN / FIELDS];  // u, vr, vi, wr, wi, X_0 .. X_{M-1}
    CglCoef c;
    // one grid point: u = (u1, u2), v = (vr1 + i vi1, vr2 + i vi2), w likewise, X_k = (x1[k], x2[k])
    __device__ __forceinline__ void operator()(const double (&x)[NIN], double (&s)[NV]) const {
        const double u1 = x[0], u2 = x[1], vr1 = x[2], vr2 = x[3], vi1 = x[4], vi2 = x[5], wr1 = x[6], wr2 = x[7], wi1 = x[8],
                     wi2 = x[9];
        if (M > 0) {
            double x1[M > 0 ? M : 1], x2[M > 0 ? M : 1];
#pragma unroll
            for (int k = 0; k < M; ++k) { x1[k] = x[10 + 2 * k]; x2[k] = x[11 + 2 * k]; }
            double h[6];
            cgl_hess(c, u1, u2, h);
            // A_f = H_f vr, B_f = H_f vi
            const double A10 = h[0] * vr1 + h[1] * vr2, A11 = h[1] * vr1 + h[2] * vr2;
            const double B10 = h[0] * vi1 + h[1] * vi2, B11 = h[1] * vi1 + h[2] * vi2;
            const double A20 = h[3] * vr1 + h[4] * vr2, A21 = h[4] * vr1 + h[5] * vr2;
            const double B20 = h[3] * vi1 + h[4] * vi2, B21 = h[4] * vi1 + h[5] * vi2;
            // g = sum_f (wr_f - i wi_f) (A_f + i B_f)
            const double gr0 = (wr1 * A10 + wi1 * B10) + (wr2 * A20 + wi2 * B20);
            const double gr1 = (wr1 * A11 + wi1 * B11) + (wr2 * A21 + wi2 * B21);
            const double gi0 = (wr1 * B10 - wi1 * A10) + (wr2 * B20 - wi2 * A20);
            const double gi1 = (wr1 * B11 - wi1 * A11) + (wr2 * B21 - wi2 * A21);
#pragma unroll
            for (int k = 0; k < M; ++k) {
                s[2 * k] = fma(gr0, x1[k], fma(gr1, x2[k], s[2 * k]));
                s[2 * k + 1] = fma(gi0, x1[k], fma(gi1, x2[k], s[2 * k + 1]));
            }
        }
        double d[4];
        cgl_djdp(c.ipar, u1, u2, d);
        const double Ar1 = d[0] * vr1 + d[1] * vr2, Ar2 = d[2] * vr1 + d[3] * vr2;
        const double Br1 = d[0] * vi1 + d[1] * vi2, Br2 = d[2] * vi1 + d[3] * vi2;
        s[2 * M] += (wr1 * Ar1 + wi1 * Br1) + (wr2 * Ar2 + wi2 * Br2);
        s[2 * M + 1] += (wr1 * Br1 - wi1 * Ar1) + (wr2 * Br2 - wi2 * Ar2);
        s[2 * M + 2] += (wr1 * vr1 + wi1 * vi1) + (wr2 * vr2 + wi2 * vi2);
        s[2 * M + 3] += (wr1 * vi1 - wi1 * vr1) + (wr2 * vi2 - wi2 * vr2);
    }
};

static int v_hopf_pw(bk_ctx* ctx, size_t n, const double* u, const CglCoef& c, const double* x1, const double* x2, double* out) {
    const size_t N = n / 2;
    if (N == 0) return 0;
    ProfScope ps(ctx, "blas1", 8.0 * n * (x2 ? 4 : 3));
    hipLaunchKernelGGL(hopf_pw_kernel, dim3(grid_for(N, 1, 4096)), dim3(kThreads), 0, ctx->stream, N, u, c, x1, x2, out);
    BK_HIP(ctx, hipGetLastError());
    return 0;
}

// out[2 (m + 2)]: (S_0, ..., S_{m-1}, P, Q) as (re, im) pairs; n = 2 N, the local length of both fields
static int v_hopf_contract(bk_ctx* ctx, size_t n, const double* u, const double* vr, const double* vi, const double* wr,
                           const double* wi, int m, const double* const* X, const CglCoef& c, double* out) {
    if (m < 0 || m > 3) return set_error(ctx, "v_hopf_contract: 0 <= m <= 3 (got %d)", m);
    return count_dispatch<0, 3>(m, [&](auto M) {
        HopfContract<decltype(M)::value> pass{{u, vr, vi, wr, wi}, c};
        for (int k = 0; k < m; ++k) pass.in[5 + k] = X[k];
        return stream_reduce(ctx, "hopf_contract", n / 2, pass, out);
    });
}

// ------------------------------------------------------------------ the formulation
// normN of BorderedArray(F, [Re sigma, Im sigma]); the max norm propagates a NaN from any component (as v_nrminf does)
int norm_hopf(bk_ctx* ctx, size_t n, const double* f, const double sigma[2], bool inf, double* out) {
    double r;
    if (inf) {
        BK_TRY(v_nrminf(ctx, n, f, &r));
        double s = std::fabs(sigma[0]);
        const double t = std::fabs(sigma[1]);
        if (t != t || t > s) s = t;
        *out = (r != r || r > s) ? r : s;
    } else {
        BK_TRY(v_nrm2(ctx, n, f, &r));
        *out = std::sqrt(r * r + sigma[0] * sigma[0] + sigma[1] * sigma[1]);
    }
    return 0;
}

// _compute_bordered_vectors (:49-64): v, sigma from bls(J, a, b, 0, 0, 1; shift = -i omega), w from the adjoint handle,
// bls(J', b, a, 0, 0, 1; shift = +i omega).  One BorderingBLS BEC pass each (bk_bls_bordering_cshift); with `bordered` (context
// option hopf_bordered) ONE preconditioned solve of each bordered system, which stays regular at the Hopf point (minaug.h).
int hopf_terms(bk_ctx* ctx, bk_op* J, bk_op* Jt, size_t n, double omega, const double* ar, const double* ai, const double* br,
               const double* bi, const bk_gmres_opts& lo, bk_precond* pl, double* zero, double* vr, double* vi, double* wr,
               double* wi, double sigma[2], int* cv, int it[2], bool bordered) {
    BK_TRY(v_zero(ctx, n, zero));
    if (bordered) {
        GmresResult r1, r2;
        double s2[2];
        BK_TRY(minaug_hopf_bordered_solve(ctx, J, ar, ai, br, bi, zero, nullptr, 1.0, -omega, lo, pl, vr, vi, sigma, &r1));
        BK_TRY(minaug_hopf_bordered_solve(ctx, Jt, br, bi, ar, ai, zero, nullptr, 1.0, omega, lo, pl, wr, wi, s2, &r2));
        *cv = r1.converged & r2.converged;
        it[0] = r1.niter;
        it[1] = r2.niter;
        return 0;
    }
    int c1 = 0, c2 = 0, i1[2] = {0, 0}, i2[2] = {0, 0};
    double s2[2];
    BK_TRY(bk_bls_bordering_cshift(ctx, J, ar, ai, br, bi, 0.0, 0.0, zero, nullptr, 1.0, 0.0, 1.0, 1.0, 0.0, -omega, 1.0, &lo, pl,
                                   vr, vi, sigma, &c1, i1));
    BK_TRY(bk_bls_bordering_cshift(ctx, Jt, br, bi, ar, ai, 0.0, 0.0, zero, nullptr, 1.0, 0.0, 1.0, 1.0, 0.0, omega, 1.0, &lo, pl,
                                   wr, wi, s2, &c2, i2));
    *cv = c1 & c2;
    it[0] = i1[0] + i1[1];
    it[1] = i2[0] + i2[1];
    return 0;
}

// _hopf_MA_linear_solver, usehessian branch (:142-198), for nrhs right-hand sides sharing the J \ dpF solve:
//   x1_k = J \ rhsu_k, x2 = J \ dpF;  S(y) = w^H d2F[v, y], sigma_p = -w^H dJ/dp v, sigma_omega = i w^H v;
//   (sigma_p + S(x2)) dp_k + sigma_omega domega_k = (rhsp_k + i rhsw_k) + S(x1_k)   -- a 2 x 2 real system --
//   dX_k = x1_k - dp_k x2.
// Every sum comes from ONE fused pass (v_hopf_contract).  rhspw / dpw: host (p, omega) pairs per right-hand side.  The Hessian
// and dJ/dp coefficients are taken from `params`, the parameters of the point J belongs to (mu, c3 and c5 enter d2F).
int hopf_linsolve(bk_ctx* ctx, bk_problem* prob, bk_op* J, const double* x, const double* params, int nparams, int ipar,
                  const double* vr, const double* vi, const double* wr, const double* wi, int nrhs, const double* const* rhsu,
                  const double* rhspw, const bk_gmres_opts& lo, bk_precond* pl, double* const* dX, double* dpw, int* cv,
                  int* itlinear) {
    const size_t n = prob->nloc;
    CglCoef c;
    BK_TRY(hopf_coef(prob, params, nparams, ipar, &c));
    WsGuard ws(ctx);
    MinAugSolves S;
    BK_TRY(minaug_solves(ctx, prob, J, x, c.ipar, nrhs, rhsu, lo, pl, dX, ws, &S));           // analytic dpF
    double s[10];
    BK_TRY(v_hopf_contract(ctx, n, x, vr, vi, wr, wi, nrhs + 1, S.X, c, s));
    const int m = nrhs + 1;
    const double s2r = s[2 * nrhs], s2i = s[2 * nrhs + 1];
    const double spr = -s[2 * m], spi = -s[2 * m + 1];                  // sigma_p = -P
    const double swr = -s[2 * m + 3], swi = s[2 * m + 2];               // sigma_omega = i Q
    const double a11 = spr + s2r, a12 = swr, a21 = spi + s2i, a22 = swi;
    const double det = a11 * a22 - a12 * a21;
    if (!(det != 0.0) || !std::isfinite(det)) return set_error(ctx, "hopf: singular 2 x 2 system of the Hopf linear solver");
    for (int k = 0; k < nrhs; ++k) {
        const double b1 = rhspw[2 * k] + s[2 * k], b2 = rhspw[2 * k + 1] + s[2 * k + 1];
        const double dp = (b1 * a22 - a12 * b2) / det, dw = (a11 * b2 - a21 * b1) / det;
        dpw[2 * k] = dp;
        dpw[2 * k + 1] = dw;
    }
    *cv = S.converged;
    *itlinear = S.niter;
    return minaug_update(ctx, n, S, nrhs, dpw, 2, dX);
}

}  // namespace
}  // namespace bk

using namespace bk;

extern "C" {

int bk_hopf_d2f(bk_problem* prob, const double* u, const double* params, int nparams, const double* dx1, const double* dx2,
                double* out) {
    if (!prob || !u || !params || !dx1 || !dx2 || !out) return -1;
    CglCoef c;
    BK_TRY(hopf_coef(prob, params, nparams, 0, &c));
    return v_hopf_pw(prob->ctx, prob->nloc, u, c, dx1, dx2, out);
}

int bk_hopf_djdp(bk_problem* prob, const double* u, const double* params, int nparams, int ipar, const double* dx, double* out) {
    if (!prob || !u || !params || !dx || !out) return -1;
    CglCoef c;
    BK_TRY(hopf_coef(prob, params, nparams, ipar, &c));
    return v_hopf_pw(prob->ctx, prob->nloc, u, c, dx, nullptr, out);
}

int bk_hopf_contract(bk_problem* prob, const double* u, const double* params, int nparams, int ipar, const double* v_re,
                     const double* v_im, const double* w_re, const double* w_im, int m, const double* const* X, double* out) {
    if (!prob || !u || !params || !v_re || !v_im || !w_re || !w_im || !out || (m > 0 && !X)) return -1;
    CglCoef c;
    BK_TRY(hopf_coef(prob, params, nparams, ipar, &c));
    if (m < 0 || m > 3) return set_error(prob->ctx, "bk_hopf_contract: 0 <= m <= 3 (got %d)", m);
    for (int k = 0; k < m; ++k)
        if (!X[k]) return -1;
    return v_hopf_contract(prob->ctx, prob->nloc, u, v_re, v_im, w_re, w_im, m, X, c, out);
}

int bk_hopf_terms(bk_ctx* ctx, bk_problem* prob, const double* x, const double* params, int nparams, int ipar, double omega,
                  const double* a_re, const double* a_im, const double* b_re, const double* b_im, const bk_gmres_opts* lsopts,
                  bk_precond* pl, double* v_re, double* v_im, double* w_re, double* w_im, double sigma[2], double sigma_p[2],
                  double sigma_omega[2], int* converged, int itlinear[2]) {
    if (!ctx || !prob || !x || !params || !a_re || !b_re || !lsopts || !v_re || !v_im || !w_re || !w_im || !sigma) return -1;
    BK_TRY(minaug_check(ctx, prob, "hopf"));
    CglCoef c;
    BK_TRY(hopf_coef(prob, params, nparams, ipar, &c));
    const double* outs[4] = {v_re, v_im, w_re, w_im};
    const double* ins[5] = {a_re, a_im, b_re, b_im, x};
    for (int k = 0; k < 4; ++k) {
        for (const double* i : ins)
            if (outs[k] == i) return set_error(ctx, "bk_hopf_terms: v and w must not alias a, b or x");
        for (int j = 0; j < k; ++j)
            if (outs[k] == outs[j]) return set_error(ctx, "bk_hopf_terms: v_re, v_im, w_re and w_im must be distinct");
    }
    const size_t n = prob->nloc;
    WsGuard ws(ctx);
    double* zero = nullptr;
    BK_TRY(ws.get(n, &zero));
    int cv = 0, it[2] = {0, 0};
    {
        JPair jp;
        BK_TRY(jp.make(prob, x, params, nparams, true));
        BK_TRY(hopf_terms(ctx, jp.J, jp.Jt, n, omega, a_re, a_im, b_re, b_im, *lsopts, pl, zero, v_re, v_im, w_re, w_im, sigma,
                          &cv, it, minaug_hopf_bordered(ctx)));
    }
    if (sigma_p || sigma_omega) {
        double s[4];
        BK_TRY(v_hopf_contract(ctx, n, x, v_re, v_im, w_re, w_im, 0, nullptr, c, s));
        if (sigma_p) { sigma_p[0] = -s[0]; sigma_p[1] = -s[1]; }
        if (sigma_omega) { sigma_omega[0] = -s[3]; sigma_omega[1] = s[2]; }
    }
    if (converged) *converged = cv;
    if (itlinear) { itlinear[0] = it[0]; itlinear[1] = it[1]; }
    return 0;
}

int bk_hopf_linsolve(bk_ctx* ctx, bk_problem* prob, const double* x, const double* params, int nparams, int ipar,
                     const double* v_re, const double* v_im, const double* w_re, const double* w_im, int nrhs,
                     const double* const* rhsu, const double* rhspw, const bk_gmres_opts* lsopts, bk_precond* pl,
                     double* const* dX, double* dpw, int* converged, int* itlinear) {
    if (!ctx || !prob || !x || !params || !v_re || !v_im || !w_re || !w_im || !rhsu || !rhspw || !lsopts || !dX || !dpw) return -1;
    BK_TRY(minaug_check(ctx, prob, "hopf"));
    CglCoef c;
    BK_TRY(hopf_coef(prob, params, nparams, ipar, &c));                // validates the problem kind and parameters up front
    BK_TRY(minaug_check_rhs(ctx, "bk_hopf_linsolve", nrhs, rhsu, dX));
    JPair jp;
    BK_TRY(jp.make(prob, x, params, nparams));
    int cv = 0, it = 0;
    BK_TRY(hopf_linsolve(ctx, prob, jp.J, x, params, nparams, ipar, v_re, v_im, w_re, w_im, nrhs, rhsu, rhspw, *lsopts, pl, dX,
                         dpw, &cv, &it));
    if (converged) *converged = cv;
    if (itlinear) *itlinear = it;
    return 0;
}

int bk_newton_hopf(bk_ctx* ctx, bk_problem* prob, double* x, double* p, double* omega, const double* params, int nparams,
                   int ipar, const double* a_re, const double* a_im, const double* b_re, const double* b_im,
                   const bk_newton_opts* no, const bk_gmres_opts* lsopts, bk_precond* pl, double* v_re, double* v_im,
                   double* w_re, double* w_im, double sigma[2], bk_newton_result* res) {
    if (!ctx || !prob || !x || !p || !omega || !params || !a_re || !b_re || !no || !lsopts || !v_re || !v_im || !w_re || !w_im ||
        !sigma || !res)
        return -1;
    BK_TRY(minaug_check(ctx, prob, "hopf"));
    if (no->max_iterations > BK_MAX_NEWTON_ITER) return set_error(ctx, "max_iterations > %d", BK_MAX_NEWTON_ITER);
    CglCoef c;
    BK_TRY(hopf_coef(prob, params, nparams, ipar, &c));                // validates the problem kind and parameters up front
    const double* outs[5] = {v_re, v_im, w_re, w_im, x};
    const double* ins[4] = {a_re, a_im, b_re, b_im};
    for (int i = 0; i < 5; ++i) {
        for (const double* q : ins)
            if (outs[i] == q) return set_error(ctx, "bk_newton_hopf: x, v and w must be distinct from a and b and from each other");
        for (int j = 0; j < i; ++j)
            if (outs[i] == outs[j]) return set_error(ctx, "bk_newton_hopf: x, v and w must be distinct from a and b and from each other");
    }
    const size_t n = prob->nloc;
    const bool inf = no->norm_inf != 0;
    WsGuard ws(ctx);
    double *fx = nullptr, *dX = nullptr, *zero = nullptr;
    BK_TRY(ws.get(n, &fx));
    BK_TRY(ws.get(n, &dX));
    BK_TRY(ws.get(n, &zero));
    double par[BK_MAX_PARAMS];
    for (int i = 0; i < nparams; ++i) par[i] = params[i];
    double pc = *p, wc = *omega;
    const bool bordered = minaug_hopf_bordered(ctx);         // option hopf_bordered, read once per call
    // one evaluation of the Hopf residual (:22-45) at (x, pc, wc), with the bordered vectors v, w of this point, which the
    // Newton step at the same point reuses (the reference solves them again in _get_bordered_terms)
    auto point = [&](double* r, int* itl) -> int {
        par[ipar] = pc;
        int cv = 0, it[2] = {0, 0};
        {
            JPair jp;
            BK_TRY(jp.make(prob, x, par, nparams, true));
            BK_TRY(hopf_terms(ctx, jp.J, jp.Jt, n, wc, a_re, a_im, b_re, b_im, *lsopts, pl, zero, v_re, v_im, w_re, w_im, sigma,
                              &cv, it, bordered));
        }
        *itl = it[0] + it[1];
        if (!cv) ctx->diag.hopf_unconverged += 1.0;
        BK_TRY(bk_residual(prob, x, par, nparams, fx));
        return norm_hopf(ctx, n, fx, sigma, inf, r);
    };
    // Newton step: J_hopf [dX; dp; domega] = [F; Re sigma; Im sigma] (HopfLinearSolverMinAug), x -= dX, (p, omega) -= (dp, domega)
    auto step = [&](int* itl) -> int {
        par[ipar] = pc;
        const double* rhsu[1] = {fx};
        double* dXs[1] = {dX};
        double dpw[2] = {0.0, 0.0};
        int cv = 0;
        {
            // the coefficients of d2F and dJ/dp follow the current parameter value (par), not the caller's params
            JPair jp;
            BK_TRY(jp.make(prob, x, par, nparams));
            BK_TRY(hopf_linsolve(ctx, prob, jp.J, x, par, nparams, ipar, v_re, v_im, w_re, w_im, 1, rhsu, sigma, *lsopts, pl, dXs,
                                 dpw, &cv, itl));
        }
        if (!cv) ctx->diag.hopf_unconverged += 1.0;
        BK_TRY(v_axpby(ctx, n, -1.0, dX, 1.0, x));
        pc -= dpw[0];
        wc -= dpw[1];
        return 0;
    };
    BK_TRY(minaug_newton(no, res, x, fx, &pc, point, step));
    *p = pc;
    *omega = wc;
    return 0;
}

}  // extern "C"
