// Minimally augmented fold formulation, matrix-free: src/codim2/MinAugFold.jl on the preconditioned GMRES path.
//
//   unknowns (x, p), G(x, p) = (F(x, p), sigma(x, p)),  [J a; b' 0][v; sigma] = [0; 1],  [J' b; a' 0][w; sigma2] = [0; 1]
//
// The Swift-Hohenberg problems are symmetric (J' = J, :79-84), so the adjoint system is the same bordered solve with a and b
// exchanged, and no solve at all when a and b are the same vector.  Their second derivative d2F(x, p)[dx1, dx2] =
// h(u) dx1 dx2 and the parameter derivative of J, dJ/dp = diag(g_p(u)), are pointwise polynomials (fold_pw.h; fold_pw_kernel,
// FoldContract below):
//   BK_PDE_SH   h = 2 nu - 6 u                (examples/SH2d-fronts.jl:40)   g_l = 1,  g_nu = 2 u
//   BK_PDE_SH1D h = 6 nu u - 20 u^3           (examples/SHpde_snaking.jl:26) g_lam = 1, g_nu = 3 u^2
// so sigma_p = -<w, dJ/dp v> (:90-95), dpF (:88-89) and sigma_x . X (:153-157) are evaluated analytically: the reference's
// central differences equal them up to rounding.
#include <cmath>

#include "common.h"
#include "fold_pw.h"
#include "minaug.h"
#include "ops.h"
#include "stream.h"

namespace bk {

namespace {

// ------------------------------------------------------------------ kernels
// out = (f(u) x1) x2, or f(u) x1 when x2 is NULL: d2F(u)[x1, x2] and dJ/dp(u) x1 (bk_d2f, bk_djdp)
__global__ void __launch_bounds__(kThreads) fold_pw_kernel(size_t n, const double* __restrict__ u, FoldPoly P,
                                                           const double* __restrict__ x1, const double* __restrict__ x2,
                                                           double* __restrict__ out) {
    const size_t stride = (size_t)gridDim.x * kThreads;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) {
        const double f = fold_poly(P.h, u[i]) * x1[i];
        out[i] = x2 ? f * x2[i] : f;
    }
}

// One pass over u, v, w and M vectors X_k:  s_k = sum w h(u) v X_k (k < M),  s_M = sum w g(u) v  -- the sigma_x terms of
// foldMALinearSolver (src/codim2/MinAugFold.jl:153-157) and sigma_p (:94-95) without materialising d2F(x, p)[X_k, v].
// M + 1 partial sums per workgroup; the second stage (reduce_finish) keeps the fixed order, so the sums are bitwise the same
// run to run and, all-reduced, on every rank.
template <int M>
struct FoldContract {
    static constexpr int NIN = 3 + M, NV = M + 1, U = 2, FIELDS = 1;
    const double* in[NIN];          // u, v, w, X_0 .. X_{M-1}
    FoldPoly P;
    __device__ __forceinline__ void operator()(const double (&x)[NIN], double (&s)[NV]) const {
        const double uu = x[0], vv = x[1], ww = x[2];
        const double* xs = x + 3;
        const double t = ww * vv;
        const double th = t * fold_poly(P.h, uu);
#pragma unroll
        for (int k = 0; k < M; ++k) s[k] = fma(th, xs[k], s[k]);
        s[M] = fma(t, fold_poly(P.g, uu), s[M]);
    }
};

// sigma_x as a vector: sigx[i] = -((w[i] h(u[i])) v[i]), the border row of the full fold Jacobian (MinAugFold.jl:136-145), so that
// <sigx, X> = -<w, d2F(u)[v, X]>.  Three read streams and one write.
struct FoldBorder {
    static constexpr int NIN = 3, NOUT = 1, U = 2, FIELDS = 1;
    static constexpr bool JOINT = false;
    const double* in[NIN];          // u, v, w
    double* out[NOUT];              // sigx
    FoldPoly P;
    __device__ __forceinline__ void operator()(const double (&x)[NIN], double (&o)[NOUT]) const {
        o[0] = -((x[2] * fold_poly(P.h, x[0])) * x[1]);
    }
};

static int v_fold_border(bk_ctx* ctx, size_t n, const double* u, const double* v, const double* w, const double h[4], double* sigx) {
    FoldBorder pass{{u, v, w}, {sigx}, {}};
    for (int i = 0; i < 4; ++i) { pass.P.h[i] = h[i]; pass.P.g[i] = 0.0; }
    return stream_write(ctx, "fold_border", n, pass);
}

static int v_fold_pw(bk_ctx* ctx, size_t n, const double* u, const double c[4], const double* x1, const double* x2, double* out) {
    if (n == 0) return 0;
    FoldPoly P{};
    for (int i = 0; i < 4; ++i) P.h[i] = c[i];
    ProfScope ps(ctx, "blas1", 8.0 * n * (x2 ? 4 : 3));
    hipLaunchKernelGGL(fold_pw_kernel, dim3(grid_for(n, 1, 4096)), dim3(kThreads), 0, ctx->stream, n, u, P, x1, x2, out);
    BK_HIP(ctx, hipGetLastError());
    return 0;
}

static int v_fold_contract(bk_ctx* ctx, size_t n, const double* u, const double* v, const double* w, int m, const double* const* X,
                    const double h[4], const double g[4], double* out) {
    if (m < 0 || m > 3) return set_error(ctx, "v_fold_contract: 0 <= m <= 3 (got %d)", m);
    return count_dispatch<0, 3>(m, [&](auto M) {
        FoldContract<decltype(M)::value> pass{{u, v, w}, {}};
        for (int i = 0; i < 4; ++i) { pass.P.h[i] = h[i]; pass.P.g[i] = g[i]; }
        for (int k = 0; k < m; ++k) pass.in[3 + k] = X[k];
        return stream_reduce(ctx, "fold_contract", n, pass, out);
    });
}

// ------------------------------------------------------------------ the formulation
int norm_fold(bk_ctx* ctx, size_t n, const double* f, double sigma, bool inf, double* out) {
    double r;
    if (inf) {
        BK_TRY(v_nrminf(ctx, n, f, &r));
        *out = (r != r || r > std::fabs(sigma)) ? r : std::fabs(sigma);          // norminf of BorderedArray(F, sigma)
    } else {
        BK_TRY(v_nrm2(ctx, n, f, &r));
        *out = std::sqrt(r * r + sigma * sigma);
    }
    return 0;
}

// _compute_bordered_vectors (:54-69): v from [J a; b' 0][v; sigma] = [0; 1] with the BorderingBLS path; w from the adjoint
// system [J b; a' 0][w; sigma2] = [0; 1] (J' = J), or w = v when a and b are the same vector.  sigma = the border of the first.
int fold_terms(bk_ctx* ctx, bk_op* J, size_t n, const double* a, const double* b, const bk_bordering_opts& bo,
               const bk_gmres_opts& lo, bk_precond* pl, double* zero, double* v, double* w, double* sigma, int* cv, int it[2]) {
    BK_TRY(v_zero(ctx, n, zero));
    int c1 = 0, c2 = 1, i1[2] = {0, 0}, i2[2] = {0, 0};
    BK_TRY(bls_bordering(ctx, J, a, b, 0.0, zero, 1.0, 1.0, 1.0, false, 0.0, 1.0, bo, lo, pl, v, sigma, &c1, i1));
    if (a == b) {
        if (w != v) BK_TRY(v_copy(ctx, n, v, w));
    } else {
        double s2 = 0.0;
        BK_TRY(bls_bordering(ctx, J, b, a, 0.0, zero, 1.0, 1.0, 1.0, false, 0.0, 1.0, bo, lo, pl, w, &s2, &c2, i2));
    }
    *cv = c1 & c2;
    it[0] = i1[0] + i1[1];
    it[1] = i2[0] + i2[1];
    return 0;
}

// foldMALinearSolver, usehessian branch (:146-164), for nrhs right-hand sides sharing the J \ dpF solve:
//   x1_k = J \ rhsu_k, x2 = J \ dpF, sx_k = -<w, d2F[x1_k, v]>, sx2 = -<w, d2F[x2, v]>, sp = -<w, dJ/dp v>,
//   dsig_k = (rhsp_k - sx_k) / (sp - sx2), dX_k = x1_k - dsig_k x2.
// The sums come from ONE fused pass (v_fold_contract) instead of d2F into a temporary plus an inner product per vector.
int fold_linsolve(bk_ctx* ctx, bk_problem* prob, bk_op* J, const double* x, const double* params, int nparams, int ipar,
                  const double* v, const double* w, int nrhs, const double* const* rhsu, const double* rhsp,
                  const bk_gmres_opts& lo, bk_precond* pl, double* const* dX, double* dsig, int* cv, int* itlinear) {
    const size_t n = prob->nloc;
    double h[4], g[4];
    BK_TRY(fold_polys(prob, params, nparams, ipar, h, g));
    WsGuard ws(ctx);
    MinAugSolves S;
    BK_TRY(minaug_solves(ctx, prob, J, x, ipar, nrhs, rhsu, lo, pl, dX, ws, &S));           // analytic dpF (:88-89)
    double s[4];
    BK_TRY(v_fold_contract(ctx, n, x, v, w, nrhs + 1, S.X, h, g, s));
    const double sx2 = -s[nrhs], sp = -s[nrhs + 1];
    for (int k = 0; k < nrhs; ++k) dsig[k] = (rhsp[k] - (-s[k])) / (sp - sx2);
    *cv = S.converged;
    *itlinear = S.niter;
    return minaug_update(ctx, n, S, nrhs, dsig, 1, dX);
}

// Context option fold_bordered = 1: the same two functions on the system that is regular at the fold (MinAugFold.jl:54-69 and
// :136-145 handed to MatrixFreeBLS with the left preconditioner diag(Pl, 1): minaug_bordered_solve -> bls_matrixfree_pl).
// (v, sigma) from ONE solve of [J a; b' 0][v; sigma] = [0; 1]; w from the adjoint system, or w = v when a and b are the same vector.
int fold_terms_bordered(bk_ctx* ctx, bk_op* J, size_t n, const double* a, const double* b, const bk_gmres_opts& lo, bk_precond* pl,
                        double* zero, double* v, double* w, double* sigma, int* cv, int it[2]) {
    BK_TRY(v_zero(ctx, n, zero));
    const double c0 = 0.0, one = 1.0;
    GmresResult r1, r2;
    r2.converged = 1;
    BK_TRY(minaug_bordered_solve(ctx, J, 1, &a, &b, &c0, zero, &one, lo, pl, v, sigma, &r1));
    if (a == b) {
        if (w != v) BK_TRY(v_copy(ctx, n, v, w));
    } else {
        double s2 = 0.0;
        BK_TRY(minaug_bordered_solve(ctx, J, 1, &b, &a, &c0, zero, &one, lo, pl, w, &s2, &r2));
    }
    *cv = r1.converged & r2.converged;
    it[0] = r1.niter;
    it[1] = r2.niter;
    return 0;
}

// [J dpF; sigx' sigma_p][dX_k; dsig_k] = [rhsu_k; rhsp_k]: sigx from the FoldBorder pass, sigma_p from FoldContract<0>, one bordered
// solve per right-hand side, all sharing atil = Pl^-1 dpF
int fold_linsolve_bordered(bk_ctx* ctx, bk_problem* prob, bk_op* J, const double* x, const double* params, int nparams, int ipar,
                           const double* v, const double* w, int nrhs, const double* const* rhsu, const double* rhsp,
                           const bk_gmres_opts& lo, bk_precond* pl, double* const* dX, double* dsig, int* cv, int* itlinear) {
    const size_t n = prob->nloc;
    if (!pl) return set_error(ctx, "fold: fold_bordered = 1 needs the left preconditioner");
    double h[4], g[4];
    BK_TRY(fold_polys(prob, params, nparams, ipar, h, g));
    WsGuard ws(ctx);
    double *dpF = nullptr, *atil = nullptr, *sigx = nullptr;
    BK_TRY(ws.get(n, &dpF));
    BK_TRY(ws.get(n, &atil));
    BK_TRY(ws.get(n, &sigx));
    BK_TRY(pde_dparam(ctx, prob->desc.pde, ipar, n, 1.0, x, dpF));                // analytic dpF (:88-89)
    BK_TRY(pl->apply(dpF, atil));
    BK_TRY(v_fold_border(ctx, n, x, v, w, h, sigx));
    double t[1];
    BK_TRY(v_fold_contract(ctx, n, x, v, w, 0, nullptr, h, g, t));
    const double sp = -t[0];
    const double* acol[1] = {dpF};
    const double* atl[1] = {atil};
    const double* brow[1] = {sigx};
    *cv = 1;
    *itlinear = 0;
    for (int k = 0; k < nrhs; ++k) {
        GmresResult r;
        BK_TRY(minaug_bordered_solve(ctx, J, 1, acol, brow, &sp, rhsu[k], &rhsp[k], lo, pl, dX[k], &dsig[k], &r, atl));
        *cv &= r.converged;
        *itlinear += r.niter;
    }
    return 0;
}

}  // namespace
}  // namespace bk

using namespace bk;

extern "C" {

int bk_d2f(bk_problem* prob, const double* u, const double* params, int nparams, const double* dx1, const double* dx2,
           double* out) {
    if (!prob || !u || !params || !dx1 || !dx2 || !out) return -1;
    double h[4], g[4];
    BK_TRY(fold_polys(prob, params, nparams, 0, h, g));
    return v_fold_pw(prob->ctx, prob->nloc, u, h, dx1, dx2, out);
}

int bk_djdp(bk_problem* prob, const double* u, const double* params, int nparams, int ipar, const double* dx, double* out) {
    if (!prob || !u || !params || !dx || !out) return -1;
    double h[4], g[4];
    BK_TRY(fold_polys(prob, params, nparams, ipar, h, g));
    return v_fold_pw(prob->ctx, prob->nloc, u, g, dx, nullptr, out);
}

int bk_fold_contract(bk_problem* prob, const double* u, const double* params, int nparams, int ipar, const double* v,
                     const double* w, int m, const double* const* X, double* out) {
    if (!prob || !u || !params || !v || !w || !out || (m > 0 && !X)) return -1;
    double h[4], g[4];
    BK_TRY(fold_polys(prob, params, nparams, ipar, h, g));
    if (m < 0 || m > 3) return set_error(prob->ctx, "bk_fold_contract: 0 <= m <= 3 (got %d)", m);
    for (int k = 0; k < m; ++k)
        if (!X[k]) return -1;
    double s[4];
    BK_TRY(v_fold_contract(prob->ctx, prob->nloc, u, v, w, m, X, h, g, s));
    for (int k = 0; k < m; ++k) out[k] = s[k];
    out[m] = -s[m];
    return 0;
}

int bk_fold_border(bk_problem* prob, const double* u, const double* params, int nparams, int ipar, const double* v, const double* w,
                   double* sigx, double* sigma_p) {
    if (!prob || !u || !params || !v || !w || !sigx) return -1;
    double h[4], g[4];
    BK_TRY(fold_polys(prob, params, nparams, ipar, h, g));
    if (sigx == u || sigx == v || sigx == w) return set_error(prob->ctx, "bk_fold_border: sigx must not alias u, v or w");
    BK_TRY(v_fold_border(prob->ctx, prob->nloc, u, v, w, h, sigx));
    if (sigma_p) {
        double t[1];
        BK_TRY(v_fold_contract(prob->ctx, prob->nloc, u, v, w, 0, nullptr, h, g, t));
        *sigma_p = -t[0];
    }
    return 0;
}

int bk_fold_terms(bk_ctx* ctx, bk_problem* prob, const double* x, const double* params, int nparams, int ipar,
                  const double* a, const double* b, const bk_bordering_opts* bopts, const bk_gmres_opts* lsopts,
                  bk_precond* pl, double* v, double* w, double* sigma, double* sigma_p, int* converged, int itlinear[2]) {
    if (!ctx || !prob || !x || !params || !a || !b || !bopts || !lsopts || !v || !w || !sigma) return -1;
    BK_TRY(minaug_check(ctx, prob, "fold"));
    double h[4], g[4];
    BK_TRY(fold_polys(prob, params, nparams, ipar, h, g));
    if (v == a || v == b || w == a || w == b) return set_error(ctx, "bk_fold_terms: v and w must not alias a or b");
    if (v == w && a != b) return set_error(ctx, "bk_fold_terms: v == w needs a == b");
    const size_t n = prob->nloc;
    WsGuard ws(ctx);
    double* zero = nullptr;
    BK_TRY(ws.get(n, &zero));
    int cv = 0, it[2] = {0, 0};
    {
        JPair jp;
        BK_TRY(jp.make(prob, x, params, nparams));
        if (minaug_bordered(ctx)) BK_TRY(fold_terms_bordered(ctx, jp.J, n, a, b, *lsopts, pl, zero, v, w, sigma, &cv, it));
        else BK_TRY(fold_terms(ctx, jp.J, n, a, b, *bopts, *lsopts, pl, zero, v, w, sigma, &cv, it));
    }
    if (sigma_p) {
        double t[1];
        BK_TRY(v_fold_contract(ctx, n, x, v, w, 0, nullptr, h, g, t));
        *sigma_p = -t[0];
    }
    if (converged) *converged = cv;
    if (itlinear) { itlinear[0] = it[0]; itlinear[1] = it[1]; }
    return 0;
}

int bk_fold_linsolve(bk_ctx* ctx, bk_problem* prob, const double* x, const double* params, int nparams, int ipar,
                     const double* v, const double* w, int nrhs, const double* const* rhsu, const double* rhsp,
                     const bk_gmres_opts* lsopts, bk_precond* pl, double* const* dX, double* dsigma, int* converged,
                     int* itlinear) {
    if (!ctx || !prob || !x || !params || !v || !w || !rhsu || !rhsp || !lsopts || !dX || !dsigma) return -1;
    BK_TRY(minaug_check(ctx, prob, "fold"));
    BK_TRY(minaug_check_rhs(ctx, "bk_fold_linsolve", nrhs, rhsu, dX));
    JPair jp;
    BK_TRY(jp.make(prob, x, params, nparams));
    int cv = 0, it = 0;
    if (minaug_bordered(ctx))
        BK_TRY(fold_linsolve_bordered(ctx, prob, jp.J, x, params, nparams, ipar, v, w, nrhs, rhsu, rhsp, *lsopts, pl, dX, dsigma, &cv, &it));
    else
        BK_TRY(fold_linsolve(ctx, prob, jp.J, x, params, nparams, ipar, v, w, nrhs, rhsu, rhsp, *lsopts, pl, dX, dsigma, &cv, &it));
    if (converged) *converged = cv;
    if (itlinear) *itlinear = it;
    return 0;
}

int bk_newton_fold(bk_ctx* ctx, bk_problem* prob, double* x, double* p, const double* params, int nparams, int ipar,
                   const double* a, const double* b, const bk_newton_opts* no, const bk_bordering_opts* bopts,
                   const bk_gmres_opts* lsopts, bk_precond* pl, double* v, double* w, double* sigma, bk_newton_result* res) {
    if (!ctx || !prob || !x || !p || !params || !a || !b || !no || !bopts || !lsopts || !v || !w || !sigma || !res) return -1;
    BK_TRY(minaug_check(ctx, prob, "fold"));
    if (no->max_iterations > BK_MAX_NEWTON_ITER) return set_error(ctx, "max_iterations > %d", BK_MAX_NEWTON_ITER);
    double h[4], g[4];
    BK_TRY(fold_polys(prob, params, nparams, ipar, h, g));
    if (x == a || x == b || v == a || v == b || w == a || w == b || v == x || w == x)
        return set_error(ctx, "bk_newton_fold: x, v and w must be distinct from a and b and from each other");
    if (v == w && a != b) return set_error(ctx, "bk_newton_fold: v == w needs a == b");
    const size_t n = prob->nloc;
    const bool inf = no->norm_inf != 0;
    WsGuard ws(ctx);
    double *fx = nullptr, *dX = nullptr, *zero = nullptr;
    BK_TRY(ws.get(n, &fx));
    BK_TRY(ws.get(n, &dX));
    BK_TRY(ws.get(n, &zero));
    double par[BK_MAX_PARAMS];
    for (int i = 0; i < nparams; ++i) par[i] = params[i];
    double pc = *p;
    const bool bordered = minaug_bordered(ctx);          // option fold_bordered, read once per call
    // one evaluation of the fold residual (:16-38) at (x, pc): F, and sigma with the bordered vectors v, w of this point, which
    // the Newton step at the same point reuses (the reference solves them again in _get_bordered_terms, :71-99)
    auto point = [&](double* r, int* itl) -> int {
        par[ipar] = pc;
        int cv = 0, it[2] = {0, 0};
        {
            JPair jp;
            BK_TRY(jp.make(prob, x, par, nparams));
            if (bordered) BK_TRY(fold_terms_bordered(ctx, jp.J, n, a, b, *lsopts, pl, zero, v, w, sigma, &cv, it));
            else BK_TRY(fold_terms(ctx, jp.J, n, a, b, *bopts, *lsopts, pl, zero, v, w, sigma, &cv, it));
        }
        *itl = it[0] + it[1];
        if (!cv) ctx->diag.fold_unconverged += 1.0;
        BK_TRY(bk_residual(prob, x, par, nparams, fx));
        return norm_fold(ctx, n, fx, *sigma, inf, r);
    };
    // Newton step: J_fold [dX; dsig] = [F; sigma] with foldMALinearSolver (:119-166), x -= dX, p -= dsig (src/Newton.jl:97)
    auto step = [&](int* itl) -> int {
        par[ipar] = pc;
        const double* rhsu[1] = {fx};
        double* dXs[1] = {dX};
        double rhsp[1] = {*sigma}, dsig[1] = {0.0};
        int cv = 0;
        {
            JPair jp;
            BK_TRY(jp.make(prob, x, par, nparams));
            if (bordered)
                BK_TRY(fold_linsolve_bordered(ctx, prob, jp.J, x, par, nparams, ipar, v, w, 1, rhsu, rhsp, *lsopts, pl, dXs, dsig, &cv, itl));
            else
                BK_TRY(fold_linsolve(ctx, prob, jp.J, x, par, nparams, ipar, v, w, 1, rhsu, rhsp, *lsopts, pl, dXs, dsig, &cv, itl));
        }
        if (!cv) ctx->diag.fold_unconverged += 1.0;
        BK_TRY(v_axpby(ctx, n, -1.0, dX, 1.0, x));
        pc -= dsig[0];
        return 0;
    };
    BK_TRY(minaug_newton(no, res, x, fx, &pc, point, step));
    *p = pc;
    return 0;
}

}  // extern "C"
