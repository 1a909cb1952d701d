// Cusp points on fold curves, matrix-free: the test value b2 along continuation_fold and cusp_normal_form
// (src/codim2/NormalForms.jl:15-123; Kuznetsov 1999) for BK_PDE_SH (2-D / 3-D) and BK_PDE_SH1D.  At a fold (x, p) with q = zeta
// spanning ker J, p = zeta* spanning ker J' (J' = J for these problems, so p may be q itself), |q| = 1 and <q, p> = 1:
//
//   b2 = <p, B(q, q)>                       the quadratic coefficient of the fold: zero at the cusp
//   [J q; p' 0][H2; s] = [b2 q - B(q, q); 0]                                                                  (:107-109)
//   c  = (<p, C(q, q, q)> + 3 <p, B(q, H2)>) / 6                                                              (:112-113)
//
// B = d2F and C = d3F are the pointwise polynomials h(u), t(u) of fold_pw.h, so the scalars and the right-hand side take three
// streaming passes: (<w, h v v>, <v, v>, <w, w>, <v, w>) from one pass over (u, v, w) that writes nothing -- with the bordered
// vectors v, w of a fold-curve point the host forms b2 = <w, h v v> / (|v| <v, w>) without normalising a vector, and with
// normalised q, p the first and last sum are b2 and <q, p> themselves -- the right-hand side from one pass over (u, q), and
// both inner products of c from one pass over (u, q, p, H2).  ONE bordered solve, where bk_normal_form_1d (whose b30 / 6 is c)
// also solves Psi01 and J \ zeta*.  The bordered system is regular at the fold; J alone is not, so with BorderingBLS an
// unconverged solve is a flag.
#include <cmath>

#include "common.h"
#include "fold_pw.h"
#include "minaug.h"
#include "ops.h"
#include "stream.h"

namespace bk {

namespace {

// ------------------------------------------------------------------ passes
// One pass over u, v, w that writes nothing: four partial sums per workgroup,
//   s0 = sum ((h(u) v) v) w,   s1 = sum v v,   s2 = sum w w,   s3 = sum v w.
// w may be the same vector as v (both are only read).  The second stage (reduce_finish) keeps the fixed order: the sums are
// bitwise the same run to run and, all-reduced, on every rank.
struct CuspDots {
    static constexpr int NIN = 3, NV = 4, U = 2, FIELDS = 1;
    const double* in[NIN];          // u, v, w
    FoldPoly P;
    __device__ __forceinline__ void operator()(const double (&x)[NIN], double (&s)[NV]) const {
        const double u = x[0], v = x[1], w = x[2];
        s[0] += ((fold_poly(P.h, u) * v) * v) * w;
        s[1] += v * v;
        s[2] += w * w;
        s[3] += v * w;
    }
};

// One pass over u and q that writes the right-hand side of the H2 solve, r = b2 q - (h(u) q) q.  2 read streams, 1 write.
struct CuspRhs {
    static constexpr int NIN = 2, NOUT = 1, U = 2, FIELDS = 1;
    static constexpr bool JOINT = false;
    const double* in[NIN];          // u, q
    double* out[NOUT];              // r
    FoldPoly P;
    double b2;
    __device__ __forceinline__ void operator()(const double (&x)[NIN], double (&o)[NOUT]) const {
        const double u = x[0], q = x[1];
        o[0] = b2 * q - (fold_poly(P.h, u) * q) * q;
    }
};

// One pass over u, q, p, H2 = g: two partial sums per workgroup,
//   s0 = sum (((t(u) q) q) q) p = <p, C(q, q, q)>,   s1 = sum ((h(u) q) g) p = <p, B(q, H2)>
// without materialising C(q, q, q) and B(q, H2).  4 read streams: 32 N bytes.
struct CuspContract {
    static constexpr int NIN = 4, NV = 2, U = 2, FIELDS = 1;
    const double* in[NIN];          // u, q, p, H2
    FoldPoly P, Q;                  // P.h = h (d2F), Q.h = t (d3F)
    __device__ __forceinline__ void operator()(const double (&x)[NIN], double (&s)[NV]) const {
        const double u = x[0], q = x[1], p = x[2], g = x[3];
        s[0] += (((fold_poly(Q.h, u) * q) * q) * q) * p;
        s[1] += ((fold_poly(P.h, u) * q) * g) * p;
    }
};

// ------------------------------------------------------------------ launchers
// h of d2F and t of d3F (the parameter-derivative factors are not read: index 0); the fold entries' error for any other problem
struct CuspPolys { FoldPoly P, Q; };
int cusp_polys(bk_problem* prob, const double* params, int nparams, CuspPolys* out) {
    BK_TRY(fold_polys(prob, params, nparams, 0, out->P.h, out->P.g));
    fold_polys_d3(prob, params, 0, out->Q.h, out->Q.g);
    return 0;
}

// out[4] = (<w, h v v>, <v, v>, <w, w>, <v, w>)
int v_cusp_dots(bk_ctx* ctx, size_t n, const double* u, const double* v, const double* w, const CuspPolys& C, double* out) {
    return stream_reduce(ctx, "cusp_dots", n, CuspDots{{u, v, w}, C.P}, out);
}

int v_cusp_rhs(bk_ctx* ctx, size_t n, const double* u, const double* q, const CuspPolys& C, double b2, double* r) {
    return stream_write(ctx, "cusp_rhs", n, CuspRhs{{u, q}, {r}, C.P, b2});
}

// out[2] = (<p, C(q, q, q)>, <p, B(q, H2)>)
int v_cusp_contract(bk_ctx* ctx, size_t n, const double* u, const double* q, const double* p, const double* H2, const CuspPolys& C,
                    double* out) {
    return stream_reduce(ctx, "cusp_contract", n, CuspContract{{u, q, p, H2}, C.P, C.Q}, out);
}

}  // namespace
}  // namespace bk

using namespace bk;

extern "C" {

int bk_cusp_dots(bk_problem* prob, const double* u, const double* params, int nparams, const double* v, const double* w,
                 double out[4]) {
    if (!prob || !u || !params || !v || !w || !out) return -1;
    CuspPolys C;
    BK_TRY(cusp_polys(prob, params, nparams, &C));
    return v_cusp_dots(prob->ctx, prob->nloc, u, v, w, C, out);
}

int bk_cusp_rhs(bk_problem* prob, const double* u, const double* params, int nparams, const double* q, double b2, double* out) {
    if (!prob || !u || !params || !q || !out) return -1;
    CuspPolys C;
    BK_TRY(cusp_polys(prob, params, nparams, &C));
    if (out == u || out == q) return set_error(prob->ctx, "bk_cusp_rhs: the output aliases an input");
    return v_cusp_rhs(prob->ctx, prob->nloc, u, q, C, b2, out);
}

int bk_cusp_contract(bk_problem* prob, const double* u, const double* params, int nparams, const double* q, const double* p,
                     const double* H2, double out[2]) {
    if (!prob || !u || !params || !q || !p || !H2 || !out) return -1;
    CuspPolys C;
    BK_TRY(cusp_polys(prob, params, nparams, &C));
    return v_cusp_contract(prob->ctx, prob->nloc, u, q, p, H2, C, out);
}

int bk_cusp_normal_form(bk_ctx* ctx, bk_problem* prob, const double* x, const double* params, int nparams, const double* q,
                        const double* p, const bk_bordering_opts* bopts, const bk_gmres_opts* lsopts, bk_precond* pl, double* H2,
                        double coef[2], int* converged, int itlinear[2]) {
    if (!ctx || !prob || !x || !params || !q || !p || !bopts || !lsopts || !H2 || !coef) return -1;
    BK_TRY(minaug_check(ctx, prob, "cusp normal form"));
    CuspPolys C;
    BK_TRY(cusp_polys(prob, params, nparams, &C));
    if (H2 == x || H2 == q || H2 == p) return set_error(ctx, "bk_cusp_normal_form: H2 must not alias x, q or p");
    const bool bordered = minaug_bordered(ctx);          // option fold_bordered, read once per call
    if (bordered && !pl) return set_error(ctx, "bk_cusp_normal_form: fold_bordered = 1 needs the left preconditioner");
    if (!bordered && bopts->kind == 0 && bopts->k < 1) return set_error(ctx, "BorderingBLS: number of recursions must be positive");
    const size_t n = prob->nloc;
    double d[4];
    BK_TRY(v_cusp_dots(ctx, n, x, q, p, C, d));
    const double b2 = d[0];
    if (!(std::fabs(d[3] - 1.0) <= 1e-8))
        return set_error(ctx, "bk_cusp_normal_form: Error of precision in normalization: <q, p> = %.17g, expected 1", d[3]);
    WsGuard ws(ctx);
    double* r = nullptr;
    BK_TRY(ws.get(n, &r));
    BK_TRY(v_cusp_rhs(ctx, n, x, q, C, b2, r));
    int cv = 0, it[2] = {0, 0};
    double s = 0.0;
    {
        // bls(L, q, p, 0, h2, 0) (:109): [J q; p' 0][H2; s] = [r; 0]
        JPair jp;
        BK_TRY(jp.make(prob, x, params, nparams));
        if (bordered) {
            const double* a[1] = {q};
            const double* b[1] = {p};
            const double c0 = 0.0, n0 = 0.0;
            GmresResult res;
            BK_TRY(minaug_bordered_solve(ctx, jp.J, 1, a, b, &c0, r, &n0, *lsopts, pl, H2, &s, &res));
            cv = res.converged;
            it[0] = res.niter;
        } else if (bopts->kind == 1) {
            BK_TRY(bk_bls_matrixfree(ctx, jp.J, q, p, 0.0, r, 0.0, 1.0, 1.0, 0, 0.0, 1.0, lsopts, H2, &s, &cv, &it[0]));
        } else {
            BK_TRY(bls_bordering(ctx, jp.J, q, p, 0.0, r, 0.0, 1.0, 1.0, false, 0.0, 1.0, *bopts, *lsopts, pl, H2, &s, &cv, it));
        }
    }
    if (!cv) ctx->diag.cusp_unconverged += 1.0;
    double c2[2];
    BK_TRY(v_cusp_contract(ctx, n, x, q, p, H2, C, c2));
    coef[0] = b2;
    coef[1] = (c2[0] + 3.0 * c2[1]) / 6.0;
    if (converged) *converged = cv ? 1 : 0;
    if (itlinear) { itlinear[0] = it[0]; itlinear[1] = it[1]; }
    return 0;
}

}  // extern "C"
