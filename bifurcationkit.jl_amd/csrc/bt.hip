// Minimally augmented Bogdanov-Takens formulation, matrix-free: src/codim2/MinAugBT.jl on preconditioned bordered GMRES solves.
//
//   unknowns (x, p1, p2), G(x, p1, p2) = (F(x, p1, p2), sigma1, sigma2),
//   [J a; b' 0][v1; sigma1] = [0; 1],    [J a; b' 0][v2; sigma2] = [v1; 0]      (:70-102)
//   [J' b; a' 0][w1; .]     = [0; 1],    [J' b; a' 0][w2; .]     = [w1; 0]      (:160-172)
//
// J has a double zero eigenvalue at the point sought, so none of these goes through J^-1: each is ONE GMRES on its bordered system,
// left-preconditioned by diag(Pl, 1) (bordered.hip: bls_matrixfree_pl), the adjoint ones with the preconditioner of the adjoint
// operator.  The derivatives of sigma are analytic where the reference differences (:176-220):
//   sigma1_x = -B(x)[v1, .]' w1,                        sigma1_pk = -<w1, D_k v1>,
//   sigma2_x = -(B(x)[v1, .]' w2 + B(x)[v2, .]' w1),    sigma2_pk = -(<w2, D_k v1> + <w1, D_k v2>),      D_k = dJ/dp_k,
// all of them from ONE streaming pass (BtBorder).  The Newton step is one block-bordered solve with m = 2 (:223).
// Defined for BK_PDE_CGL2D (pointwise tensors in hopf_pw.h), one rank.
#include <cmath>

#include "common.h"
#include "hopf_pw.h"
#include "minaug.h"
#include "ops.h"
#include "stream.h"

namespace bk {

namespace {

// ------------------------------------------------------------------ kernels
// One pass over u and four real vectors v1, v2, w1, w2 for the two rows the BT system adds to [J dpF]:
//   row1 = s B(u)[v1, .]' w1,   row2 = s (B(u)[v1, .]' w2 + B(u)[v2, .]' w1),
//   sums = s <w1, D_k v1>, s (<w2, D_k v1> + <w1, D_k v2>) for the two lenses k, row-major (row, lens): the 2 x 2 block sigma_p.
// B(u)[v, .]' w = sum_f w_f H_f v per grid point (H_f symmetric).  Five vectors read, two written, four sums, on the
// writing-and-reducing pass of stream.h; formed as the reference forms them (differences of the adjoint Jacobian, dJ/dp products
// and dots) on the entry points that existed, the same quantities take 23 vector passes (scripts/bt_probe.py).  s = -1 with the bordered vectors
// gives sigma_x and sigma_p; s = +1 with the Jordan chains (q0, q1, p1, p0) gives A12_1, A12_2 and A22 of the normal form
// (src/NormalForms.jl:252-254; its pBq is 2 B(q, .)' p and it halves it again).
struct BtBorder {
    static constexpr int NIN = 10, NOUT = 4, NV = 4, U = 1, FIELDS = 2;
    const double* in[NIN / FIELDS];   // u, v1, v2, w1, w2
    double* out[NOUT / FIELDS];       // row1, row2
    CglCoef c;
    int ipar2;
    double s;
    __device__ __forceinline__ void operator()(const double (&x)[NIN], double (&o)[NOUT], double (&sum)[NV]) const {
        const double u1 = x[0], u2 = x[1], v1a = x[2], v1b = x[3], v2a = x[4], v2b = x[5], w1a = x[6], w1b = x[7], w2a = x[8],
                     w2b = x[9];
        double h[6];
        cgl_hess(c, u1, u2, h);
        // A_f = H_f v1, C_f = H_f v2
        const double A10 = h[0] * v1a + h[1] * v1b, A11 = h[1] * v1a + h[2] * v1b;
        const double A20 = h[3] * v1a + h[4] * v1b, A21 = h[4] * v1a + h[5] * v1b;
        const double C10 = h[0] * v2a + h[1] * v2b, C11 = h[1] * v2a + h[2] * v2b;
        const double C20 = h[3] * v2a + h[4] * v2b, C21 = h[4] * v2a + h[5] * v2b;
        o[0] = s * (w1a * A10 + w1b * A20);
        o[1] = s * (w1a * A11 + w1b * A21);
        o[2] = s * ((w2a * A10 + w2b * A20) + (w1a * C10 + w1b * C20));
        o[3] = s * ((w2a * A11 + w2b * A21) + (w1a * C11 + w1b * C21));
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            double d[4];
            cgl_djdp(k == 0 ? c.ipar : ipar2, u1, u2, d);
            const double E1 = d[0] * v1a + d[1] * v1b, E2 = d[2] * v1a + d[3] * v1b;      // D_k v1
            const double G1 = d[0] * v2a + d[1] * v2b, G2 = d[2] * v2a + d[3] * v2b;      // D_k v2
            sum[k] += s * (w1a * E1 + w1b * E2);
            sum[2 + k] += s * ((w2a * E1 + w2b * E2) + (w1a * G1 + w1b * G2));
        }
    }
};

static int v_bt_border(bk_ctx* ctx, size_t n, const double* u, const CglCoef& c, int ipar2, double s, const double* v1,
                       const double* v2, const double* w1, const double* w2, double* row1, double* row2, double sums[4]) {
    if (n / 2 == 0) {
        for (int k = 0; k < 4; ++k) sums[k] = 0.0;
        return 0;
    }
    BtBorder pass{{u, v1, v2, w1, w2}, {row1, row2}, c, ipar2, s};
    return stream_write_reduce(ctx, "bt_border", n / 2, pass, sums);
}

// One reducing pass over u and the Jordan chains q0, q1, p0, p1 for the six contractions of the quadratic level of the normal form
// (src/codim2/NormalForms.jl:184-186, 209, 257), B = d2F:
//   <p1, B(q0, q0)>, <p0, B(q0, q0)>, <p1, B(q0, q1)>, <p0, B(q0, q1)>, <p1, B(q1, q1)>, <p0, B(q1, q1)>
// in place of three d2F products and six dots.
struct BtNfDots {
    static constexpr int NIN = 10, NV = 6, U = 1, FIELDS = 2;
    const double* in[NIN / FIELDS];   // u, q0, q1, p0, p1
    CglCoef c;
    __device__ __forceinline__ void operator()(const double (&x)[NIN], double (&s)[NV]) const {
        const double q0a = x[2], q0b = x[3], q1a = x[4], q1b = x[5], p0a = x[6], p0b = x[7], p1a = x[8], p1b = x[9];
        double h[6];
        cgl_hess(c, x[0], x[1], h);
        // A_f = H_f q0, C_f = H_f q1
        const double A10 = h[0] * q0a + h[1] * q0b, A11 = h[1] * q0a + h[2] * q0b;
        const double A20 = h[3] * q0a + h[4] * q0b, A21 = h[4] * q0a + h[5] * q0b;
        const double C10 = h[0] * q1a + h[1] * q1b, C11 = h[1] * q1a + h[2] * q1b;
        const double C20 = h[3] * q1a + h[4] * q1b, C21 = h[4] * q1a + h[5] * q1b;
        const double B00a = q0a * A10 + q0b * A11, B00b = q0a * A20 + q0b * A21;
        const double B01a = q1a * A10 + q1b * A11, B01b = q1a * A20 + q1b * A21;
        const double B11a = q1a * C10 + q1b * C11, B11b = q1a * C20 + q1b * C21;
        s[0] += p1a * B00a + p1b * B00b;
        s[1] += p0a * B00a + p0b * B00b;
        s[2] += p1a * B01a + p1b * B01b;
        s[3] += p0a * B01a + p0b * B01b;
        s[4] += p1a * B11a + p1b * B11b;
        s[5] += p0a * B11a + p0b * B11b;
    }
};

// One writing pass for a right-hand side of the quadratic level: MODE 0: k q1 - B(q0, q0) (k = 2 a, :207), MODE 1:
// k q1 + H - B(q0, q1) (k = b, H = H2000, :212).  B(q0, q1) is never written out on its own.
template <int MODE>
struct BtNfRhs {
    static constexpr int NIN = MODE ? 8 : 6, NOUT = 2, U = 2, FIELDS = 2;
    static constexpr bool JOINT = true;
    const double* in[NIN / FIELDS];   // u, q0, q1[, H]
    double* out[NOUT / FIELDS];
    CglCoef c;
    double k;
    __device__ __forceinline__ void operator()(const double (&x)[NIN], double (&o)[NOUT]) const {
        const double q0a = x[2], q0b = x[3], q1a = x[4], q1b = x[5];
        double h[6];
        cgl_hess(c, x[0], x[1], h);
        const double A10 = h[0] * q0a + h[1] * q0b, A11 = h[1] * q0a + h[2] * q0b;
        const double A20 = h[3] * q0a + h[4] * q0b, A21 = h[4] * q0a + h[5] * q0b;
        if (MODE == 0) {
            o[0] = k * q1a - (q0a * A10 + q0b * A11);
            o[1] = k * q1b - (q0a * A20 + q0b * A21);
        } else {
            o[0] = (k * q1a + x[NIN - 2]) - (q1a * A10 + q1b * A11);
            o[1] = (k * q1b + x[NIN - 1]) - (q1a * A20 + q1b * A21);
        }
    }
};

// One reducing pass over u, p1 and H = H0001 for K2 (:267-272): <p1, B(H, H)> and <p1, D_k H> for the two lenses.
struct BtNfK2 {
    static constexpr int NIN = 6, NV = 3, U = 1, FIELDS = 2;
    const double* in[NIN / FIELDS];   // u, p1, H
    CglCoef c;
    int ipar2;
    __device__ __forceinline__ void operator()(const double (&x)[NIN], double (&s)[NV]) const {
        const double u1 = x[0], u2 = x[1], pa = x[2], pb = x[3], ha = x[4], hb = x[5];
        double h[6];
        cgl_hess(c, u1, u2, h);
        const double Ba = ha * (h[0] * ha + h[1] * hb) + hb * (h[1] * ha + h[2] * hb);
        const double Bb = ha * (h[3] * ha + h[4] * hb) + hb * (h[4] * ha + h[5] * hb);
        s[0] += pa * Ba + pb * Bb;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            double d[4];
            cgl_djdp(k == 0 ? c.ipar : ipar2, u1, u2, d);
            s[1 + k] += pa * (d[0] * ha + d[1] * hb) + pb * (d[2] * ha + d[3] * hb);
        }
    }
};

static int v_bt_nf_dots(bk_ctx* ctx, size_t n, const double* u, const CglCoef& c, const double* q0, const double* q1,
                        const double* p0, const double* p1, double out[6]) {
    BtNfDots pass{{u, q0, q1, p0, p1}, c};
    return stream_reduce(ctx, "bt_nf_dots", n / 2, pass, out);
}

static int v_bt_nf_rhs(bk_ctx* ctx, size_t n, const double* u, const CglCoef& c, int mode, double k, const double* q0,
                       const double* q1, const double* H, double* out) {
    if (mode == 0) {
        BtNfRhs<0> pass{{u, q0, q1}, {out}, c, k};
        return stream_write(ctx, "bt_nf_rhs", n / 2, pass);
    }
    BtNfRhs<1> pass{{u, q0, q1, H}, {out}, c, k};
    return stream_write(ctx, "bt_nf_rhs", n / 2, pass);
}

static int v_bt_nf_k2(bk_ctx* ctx, size_t n, const double* u, const CglCoef& c, int ipar2, const double* p1, const double* H,
                      double out[3]) {
    BtNfK2 pass{{u, p1, H}, c, ipar2};
    return stream_reduce(ctx, "bt_nf_k2", n / 2, pass, out);
}

// ------------------------------------------------------------------ the formulation
int bt_coef(bk_problem* prob, const double* params, int nparams, int ipar1, int ipar2, CglCoef* c) {
    BK_TRY(hopf_coef(prob, params, nparams, ipar1, c));
    if (ipar2 < 0 || ipar2 > 5) return set_error(prob->ctx, "bt: bad parameter index %d", ipar2);
    if (ipar1 == ipar2) return set_error(prob->ctx, "bt: the two lenses must differ (both are parameter %d)", ipar1);
    if (prob->ctx->nranks > 1) return set_error(prob->ctx, "bt: the Bogdanov-Takens formulation runs on a single rank");
    return 0;
}

// normN of BorderedArray(F, [sigma1, sigma2]); the max norm propagates a NaN from any component (as v_nrminf does)
int norm_bt(bk_ctx* ctx, size_t n, const double* f, const double sigma[2], bool inf, double* out) {
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

// The chain of two solves with one bordered matrix [A col; row' 0]: (y1, s1) for the right-hand side (0, 1), (y2, s2) for (y1, 0).
// Pl^-1 col is formed once for both.  cv, it: per solve.
int bt_chain(bk_ctx* ctx, bk_op* A, size_t n, const double* col, const double* row, const bk_gmres_opts& lo, bk_precond* pl,
             const double* zero, double* atil, double* y1, double* y2, double s[2], int cv[2], int it[2]) {
    const double* a[1] = {col};
    const double* b[1] = {row};
    const double* at[1] = {atil};
    const double c[1] = {0.0}, one = 1.0, nul = 0.0;
    BK_TRY(pl->apply(col, atil));
    GmresResult r1, r2;
    BK_TRY(bls_matrixfree_pl(ctx, A, 1, a, b, 1.0, c, zero, &one, false, 0.0, lo, pl, y1, &s[0], &r1, at));
    BK_TRY(bls_matrixfree_pl(ctx, A, 1, a, b, 1.0, c, y1, &nul, false, 0.0, lo, pl, y2, &s[1], &r2, at));
    cv[0] = r1.converged; cv[1] = r2.converged;
    it[0] = r1.niter; it[1] = r2.niter;
    return 0;
}

// (v1, v2, sigma) when v1 is given and (w1, w2) when w1 is given, at (x, par); cv, it: the four solves in the order v1, v2, w1, w2
// (left as they are for the pair that is not solved)
int bt_terms(bk_ctx* ctx, bk_problem* prob, const double* x, const double* par, int np, const double* a, const double* b,
             const bk_gmres_opts& lo, bk_precond* pl, bk_precond* pl_adj, double* v1, double* v2, double* w1, double* w2,
             double sigma[2], int cv[4], int it[4]) {
    const size_t n = prob->nloc;
    if (v1 && !pl) return set_error(ctx, "bt: the bordered solves need the left preconditioner");
    if (w1 && !pl_adj)
        return set_error(ctx, "bt: the adjoint bordered solves need the left preconditioner of the adjoint operator "
                              "(the cGL block with the sign of its rotation part flipped)");
    WsGuard ws(ctx);
    double *zero = nullptr, *atil = nullptr;
    BK_TRY(ws.get(n, &zero));
    BK_TRY(ws.get(n, &atil));
    BK_TRY(v_zero(ctx, n, zero));
    JPair jp;
    BK_TRY(jp.make(prob, x, par, np, w1 != nullptr));
    if (v1) BK_TRY(bt_chain(ctx, jp.J, n, a, b, lo, pl, zero, atil, v1, v2, sigma, cv, it));
    if (w1) {
        double s2[2];
        BK_TRY(bt_chain(ctx, jp.Jt, n, b, a, lo, pl_adj, zero, atil, w1, w2, s2, cv + 2, it + 2));
    }
    return 0;
}

// btMALinearSolver (:118-228) with the bordered vectors of (x, par) given: J_BT [dX; dp] = [rhsu; rhsp] as ONE block-bordered solve,
// columns dF/dp1, dF/dp2 (analytic), rows sigma1_x, sigma2_x and block sigma_p from the BtBorder pass.
int bt_linsolve(bk_ctx* ctx, bk_problem* prob, bk_op* J, const double* x, const CglCoef& c, int ipar2, const double* v1,
                const double* v2, const double* w1, const double* w2, const double* rhsu, const double rhsp[2],
                const bk_gmres_opts& lo, bk_precond* pl, double* dX, double dp[2], int* cv, int* itlinear) {
    const size_t n = prob->nloc;
    if (!pl) return set_error(ctx, "bt: the block-bordered solve needs the left preconditioner");
    WsGuard ws(ctx);
    double *d1 = nullptr, *d2 = nullptr, *r1 = nullptr, *r2 = nullptr;
    BK_TRY(ws.get(n, &d1));
    BK_TRY(ws.get(n, &d2));
    BK_TRY(ws.get(n, &r1));
    BK_TRY(ws.get(n, &r2));
    BK_TRY(pde_dparam(ctx, prob->desc.pde, c.ipar, n / 2, 1.0, x, d1));
    BK_TRY(pde_dparam(ctx, prob->desc.pde, ipar2, n / 2, 1.0, x, d2));
    double sp[4];
    BK_TRY(v_bt_border(ctx, n, x, c, ipar2, -1.0, v1, v2, w1, w2, r1, r2, sp));
    const double* col[2] = {d1, d2};
    const double* row[2] = {r1, r2};
    GmresResult r;
    BK_TRY(bls_matrixfree_pl(ctx, J, 2, col, row, 1.0, sp, rhsu, rhsp, false, 0.0, lo, pl, dX, dp, &r));
    *cv = r.converged;
    *itlinear = r.niter;
    return 0;
}

bool bt_distinct(const double* const* p, int n) {
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < i; ++j)
            if (p[i] && p[i] == p[j]) return false;
    return true;
}

}  // namespace
}  // namespace bk

using namespace bk;

extern "C" {

int bk_bt_border(bk_problem* prob, const double* u, const double* params, int nparams, int ipar1, int ipar2, double s,
                 const double* v1, const double* v2, const double* w1, const double* w2, double* row1, double* row2,
                 double sums[4]) {
    if (!prob || !u || !params || !v1 || !v2 || !w1 || !w2 || !row1 || !row2 || !sums) return -1;
    CglCoef c;
    BK_TRY(bt_coef(prob, params, nparams, ipar1, ipar2, &c));
    const double* ins[5] = {u, v1, v2, w1, w2};
    for (const double* i : ins)
        if (row1 == i || row2 == i) return set_error(prob->ctx, "bk_bt_border: row1 and row2 must not alias u, v1, v2, w1 or w2");
    if (row1 == row2) return set_error(prob->ctx, "bk_bt_border: row1 and row2 must be distinct");
    return v_bt_border(prob->ctx, prob->nloc, u, c, ipar2, s, v1, v2, w1, w2, row1, row2, sums);
}

int bk_bt_terms(bk_ctx* ctx, bk_problem* prob, const double* x, const double* params, int nparams, const double* a,
                const double* b, const bk_gmres_opts* lsopts, bk_precond* pl, bk_precond* pl_adj, double* v1, double* v2,
                double* w1, double* w2, double sigma[2], int converged[4], int itlinear[4]) {
    if (!ctx || !prob || !x || !params || !a || !b || !lsopts) return -1;
    if ((v1 == nullptr) != (v2 == nullptr) || (w1 == nullptr) != (w2 == nullptr) || (!v1 && !w1) || (v1 && !sigma)) return -1;
    BK_TRY(minaug_check(ctx, prob, "bt"));
    CglCoef c;
    BK_TRY(bt_coef(prob, params, nparams, 0, 1, &c));                  // validates the problem kind and parameters up front
    const double* all[7] = {v1, v2, w1, w2, a, b, x};
    if (!bt_distinct(all, 7)) return set_error(ctx, "bk_bt_terms: v1, v2, w1 and w2 must be distinct and must not alias a, b or x");
    int cv[4] = {1, 1, 1, 1}, it[4] = {0, 0, 0, 0};
    BK_TRY(bt_terms(ctx, prob, x, params, nparams, a, b, *lsopts, pl, pl_adj, v1, v2, w1, w2, sigma, cv, it));
    for (int k = 0; k < 4; ++k) {
        if (converged) converged[k] = cv[k];
        if (itlinear) itlinear[k] = it[k];
    }
    return 0;
}

int bk_bt_linsolve(bk_ctx* ctx, bk_problem* prob, const double* x, const double* params, int nparams, int ipar1, int ipar2,
                   const double* v1, const double* v2, const double* w1, const double* w2, const double* rhsu,
                   const double rhsp[2], const bk_gmres_opts* lsopts, bk_precond* pl, double* dX, double dp[2], int* converged,
                   int* itlinear) {
    if (!ctx || !prob || !x || !params || !v1 || !v2 || !w1 || !w2 || !rhsu || !rhsp || !lsopts || !dX || !dp) return -1;
    BK_TRY(minaug_check(ctx, prob, "bt"));
    CglCoef c;
    BK_TRY(bt_coef(prob, params, nparams, ipar1, ipar2, &c));
    const double* ins[6] = {x, v1, v2, w1, w2, rhsu};
    for (const double* i : ins)
        if (dX == i) return set_error(ctx, "bk_bt_linsolve: dX must be a fresh buffer");
    JPair jp;
    BK_TRY(jp.make(prob, x, params, nparams));
    int cv = 0, it = 0;
    BK_TRY(bt_linsolve(ctx, prob, jp.J, x, c, ipar2, v1, v2, w1, w2, rhsu, rhsp, *lsopts, pl, dX, dp, &cv, &it));
    if (converged) *converged = cv;
    if (itlinear) *itlinear = it;
    return 0;
}

int bk_newton_bt(bk_ctx* ctx, bk_problem* prob, double* x, double p[2], const double* params, int nparams, int ipar1, int ipar2,
                 const double* a, const double* b, const bk_newton_opts* no, const bk_gmres_opts* lsopts, bk_precond* pl,
                 bk_precond* pl_adj, double* v1, double* v2, double* w1, double* w2, double sigma[2], bk_newton_result* res,
                 int itsolves[5], int* unconverged) {
    if (!ctx || !prob || !x || !p || !params || !a || !b || !no || !lsopts || !v1 || !v2 || !w1 || !w2 || !sigma || !res) return -1;
    BK_TRY(minaug_check(ctx, prob, "bt"));
    if (no->max_iterations > BK_MAX_NEWTON_ITER) return set_error(ctx, "max_iterations > %d", BK_MAX_NEWTON_ITER);
    CglCoef c;
    BK_TRY(bt_coef(prob, params, nparams, ipar1, ipar2, &c));
    if (!pl) return set_error(ctx, "bt: the bordered solves need the left preconditioner");
    if (!pl_adj)
        return set_error(ctx, "bt: the adjoint bordered solves need the left preconditioner of the adjoint operator "
                              "(the cGL block with the sign of its rotation part flipped)");
    const double* all[7] = {v1, v2, w1, w2, x, a, b};
    if (!bt_distinct(all, 7)) return set_error(ctx, "bk_newton_bt: x, v1, v2, w1 and w2 must be distinct from a and b and from each other");
    const size_t n = prob->nloc;
    const bool inf = no->norm_inf != 0;
    WsGuard ws(ctx);
    double *fx = nullptr, *dX = nullptr;
    BK_TRY(ws.get(n, &fx));
    BK_TRY(ws.get(n, &dX));
    double par[BK_MAX_PARAMS];
    for (int i = 0; i < nparams; ++i) par[i] = params[i];
    double pc[2] = {p[0], p[1]};
    int its[5] = {0, 0, 0, 0, 0}, bad = 0;
    // the residual (:70-102) at (x, pc): v1, v2 and sigma, which the Newton step at the same point reuses
    auto point = [&](double* r, int* itl) -> int {
        par[ipar1] = pc[0]; par[ipar2] = pc[1];
        int cv[4] = {1, 1, 1, 1}, it[4] = {0, 0, 0, 0};
        BK_TRY(bt_terms(ctx, prob, x, par, nparams, a, b, *lsopts, pl, pl_adj, v1, v2, nullptr, nullptr, sigma, cv, it));
        its[0] += it[0]; its[1] += it[1];
        bad += !cv[0] + !cv[1];
        *itl = it[0] + it[1];
        BK_TRY(bk_residual(prob, x, par, nparams, fx));
        return norm_bt(ctx, n, fx, sigma, inf, r);
    };
    // Newton step: w1, w2 of the point, then J_BT [dX; dp] = [F; sigma1; sigma2], x -= dX, p -= dp
    auto step = [&](int* itl) -> int {
        par[ipar1] = pc[0]; par[ipar2] = pc[1];
        int cv[4] = {1, 1, 1, 1}, it[4] = {0, 0, 0, 0}, cvb = 0, itb = 0;
        double s2[2], dp[2] = {0.0, 0.0};
        BK_TRY(bt_terms(ctx, prob, x, par, nparams, a, b, *lsopts, pl, pl_adj, nullptr, nullptr, w1, w2, s2, cv, it));
        CglCoef cc = c;
        cc.mu = par[1]; cc.c3 = par[3]; cc.c5 = par[4];                // the coefficients follow the current parameters
        {
            JPair jp;
            BK_TRY(jp.make(prob, x, par, nparams));
            BK_TRY(bt_linsolve(ctx, prob, jp.J, x, cc, ipar2, v1, v2, w1, w2, fx, sigma, *lsopts, pl, dX, dp, &cvb, &itb));
        }
        its[2] += it[2]; its[3] += it[3]; its[4] += itb;
        bad += !cv[2] + !cv[3] + !cvb;
        *itl = it[2] + it[3] + itb;
        BK_TRY(v_axpby(ctx, n, -1.0, dX, 1.0, x));
        pc[0] -= dp[0];
        pc[1] -= dp[1];
        return 0;
    };
    BK_TRY(minaug_newton(no, res, x, fx, &pc[0], point, step));
    p[0] = pc[0];
    p[1] = pc[1];
    if (itsolves)
        for (int k = 0; k < 5; ++k) itsolves[k] = its[k];
    if (unconverged) *unconverged = bad;
    return 0;
}

int bk_bt_nf_dots(bk_problem* prob, const double* u, const double* params, int nparams, const double* q0, const double* q1,
                  const double* p0, const double* p1, double out[6]) {
    if (!prob || !u || !params || !q0 || !q1 || !p0 || !p1 || !out) return -1;
    CglCoef c;
    BK_TRY(bt_coef(prob, params, nparams, 0, 1, &c));
    return v_bt_nf_dots(prob->ctx, prob->nloc, u, c, q0, q1, p0, p1, out);
}

int bk_bt_nf_rhs(bk_problem* prob, const double* u, const double* params, int nparams, int mode, double k, const double* q0,
                 const double* q1, const double* H, double* out) {
    if (!prob || !u || !params || !q0 || !q1 || !out || (mode != 0 && !H)) return -1;
    CglCoef c;
    BK_TRY(bt_coef(prob, params, nparams, 0, 1, &c));
    if (mode != 0 && mode != 1) return set_error(prob->ctx, "bk_bt_nf_rhs: mode 0 or 1 (got %d)", mode);
    if (out == u || out == q0 || out == q1 || (mode && out == H)) return set_error(prob->ctx, "bk_bt_nf_rhs: out must not alias an input");
    return v_bt_nf_rhs(prob->ctx, prob->nloc, u, c, mode, k, q0, q1, H, out);
}

int bk_bt_nf_k2(bk_problem* prob, const double* u, const double* params, int nparams, int ipar1, int ipar2, const double* p1,
                const double* H0001, double out[3]) {
    if (!prob || !u || !params || !p1 || !H0001 || !out) return -1;
    CglCoef c;
    BK_TRY(bt_coef(prob, params, nparams, ipar1, ipar2, &c));
    return v_bt_nf_k2(prob->ctx, prob->nloc, u, c, ipar2, p1, H0001, out);
}

int bk_bt_normal_form(bk_ctx* ctx, bk_problem* prob, const double* x, const double* params, int nparams, int ipar1, int ipar2,
                      const double* q0, const double* q1, const double* p0, const double* p1, int detailed,
                      const bk_gmres_opts* lsopts, bk_precond* pl, double* H2000, double* H1100, double* H0010, double* H0001,
                      double nf[10], int converged[4], int itlinear[4]) {
    if (!ctx || !prob || !x || !params || !q0 || !q1 || !p0 || !p1 || !nf) return -1;
    if (detailed && (!lsopts || !H2000 || !H1100 || !H0010 || !H0001)) return -1;
    BK_TRY(minaug_check(ctx, prob, "bt"));
    CglCoef c;
    BK_TRY(bt_coef(prob, params, nparams, ipar1, ipar2, &c));
    const size_t n = prob->nloc;
    double d[6];
    BK_TRY(v_bt_nf_dots(ctx, n, x, c, q0, q1, p0, p1, d));
    const double a = 0.5 * d[0], b = d[1] + d[2];
    for (int k = 0; k < 10; ++k) nf[k] = NAN;
    nf[0] = a;
    nf[1] = b;
    if (!detailed) return 0;
    if (!pl) return set_error(ctx, "bt: the bordered solves of the normal form need the left preconditioner");
    const double* all[9] = {H2000, H1100, H0010, H0001, x, q0, q1, p0, p1};
    if (!bt_distinct(all, 9)) return set_error(ctx, "bk_bt_normal_form: H2000, H1100, H0010 and H0001 must be distinct and must not alias an input");
    WsGuard ws(ctx);
    double *rhs = nullptr, *atil = nullptr, *d1 = nullptr, *d2 = nullptr, *r1 = nullptr, *r2 = nullptr, *at1 = nullptr, *at2 = nullptr;
    for (double** w : {&rhs, &atil, &d1, &d2, &r1, &r2, &at1, &at2}) BK_TRY(ws.get(n, w));
    JPair jp;
    BK_TRY(jp.make(prob, x, params, nparams));
    GmresResult r[4];
    // Ainv (:205): [J p1; q0' 0][H; .] = [rhs; 0]
    const double* col[1] = {p1};
    const double* row[1] = {q0};
    const double* at[1] = {atil};
    const double zero1[1] = {0.0}, nul = 0.0;
    double dl;
    BK_TRY(pl->apply(p1, atil));
    BK_TRY(v_bt_nf_rhs(ctx, n, x, c, 0, 2.0 * a, q0, q1, nullptr, rhs));
    BK_TRY(bls_matrixfree_pl(ctx, jp.J, 1, col, row, 1.0, zero1, rhs, &nul, false, 0.0, *lsopts, pl, H2000, &dl, &r[0], at));
    double p0H;
    BK_TRY(v_dot(ctx, n, p0, H2000, &p0H));
    const double gamma = (-2.0 * p0H + 2.0 * d[3] + d[4]) / 2.0;
    BK_TRY(v_axpby(ctx, n, gamma, q0, 1.0, H2000));
    BK_TRY(v_bt_nf_rhs(ctx, n, x, c, 1, b, q0, q1, H2000, rhs));
    BK_TRY(bls_matrixfree_pl(ctx, jp.J, 1, col, row, 1.0, zero1, rhs, &nul, false, 0.0, *lsopts, pl, H1100, &dl, &r[1], at));
    BK_TRY(v_dot(ctx, n, p0, H1100, &p0H));
    const double cc = 3.0 * p0H - d[5];
    // the (n + 2) system [J J1s; A12 A22] (:248-262): A12, A22 from the BtBorder pass with s = +1 on (q0, q1, p1, p0)
    double A22[4];
    BK_TRY(v_bt_border(ctx, n, x, c, ipar2, 1.0, q0, q1, p1, p0, r1, r2, A22));
    BK_TRY(pde_dparam(ctx, prob->desc.pde, c.ipar, n / 2, 1.0, x, d1));
    BK_TRY(pde_dparam(ctx, prob->desc.pde, ipar2, n / 2, 1.0, x, d2));
    BK_TRY(pl->apply(d1, at1));
    BK_TRY(pl->apply(d2, at2));
    const double* cols[2] = {d1, d2};
    const double* rows[2] = {r1, r2};
    const double* ats[2] = {at1, at2};
    const double rb1[2] = {d[4] / 2.0, cc}, rb2[2] = {0.0, 1.0};
    double K10[2], K11[2];
    BK_TRY(bls_matrixfree_pl(ctx, jp.J, 2, cols, rows, 1.0, A22, q1, rb1, false, 0.0, *lsopts, pl, H0010, K10, &r[2], ats));
    BK_TRY(v_zero(ctx, n, rhs));
    BK_TRY(bls_matrixfree_pl(ctx, jp.J, 2, cols, rows, 1.0, A22, rhs, rb2, false, 0.0, *lsopts, pl, H0001, K11, &r[3], ats));
    // K2 (:267-272).  All six cGL parameters enter F linearly, so J2_11 = J2_12 = J2_22 = 0 exactly and kappa3 = 0: the term is dropped.
    double k[3];
    BK_TRY(v_bt_nf_k2(ctx, n, x, c, ipar2, p1, H0001, k));
    const double kappa2 = k[1] * K11[0] + k[2] * K11[1];
    const double f = -(k[0] + 2.0 * kappa2);
    nf[2] = gamma; nf[3] = cc;
    nf[4] = K10[0]; nf[5] = K10[1];
    nf[6] = K11[0]; nf[7] = K11[1];
    nf[8] = f * K10[0]; nf[9] = f * K10[1];
    for (int i = 0; i < 4; ++i) {
        if (converged) converged[i] = r[i].converged;
        if (itlinear) itlinear[i] = r[i].niter;
    }
    return 0;
}

}  // extern "C"
