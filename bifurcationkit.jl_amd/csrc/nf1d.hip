// Normal form at a simple branch point or fold, matrix-free: get_normal_form1d (src/NormalForms.jl:189-353) and the vectors of
// its predictors (:389-531) for BK_PDE_SH (2-D / 3-D) and BK_PDE_SH1D.  At (x, p) with the kernel vector zeta of J and zeta* of
// J' (J' = J for these problems, so zeta* = zeta / <zeta, zeta> in the is_symmetric branch, :261-263), |zeta| = 1,
// <zeta, zeta*> = 1 and E(r) = r - <r, zeta*> zeta:
//
//   a01 = <dpF, zeta*>                                    Psi01 from [J zeta*; zeta' 0][Psi01; s] = [E(-dpF); 0]          (:299-303)
//   b11 = <dJ/dp zeta + d2F[zeta, Psi01], zeta*>                                                                           (:313)
//   a02 = <d2F/dp2 + 2 dJ/dp Psi01 + d2F[Psi01, Psi01], zeta*>                                                             (:322-323)
//   b20 = <d2F[zeta, zeta], zeta*>                        Psi20 from the same matrix with E(-d2F[zeta, zeta])              (:328-333)
//   b30 = <d3F[zeta, zeta, zeta] + 3 d2F[zeta, Psi20], zeta*>                                                              (:335-336)
//
// Every tensor is a pointwise polynomial in u (fold_pw.h) and d2F/dp2 = 0, where the reference uses ForwardDiff or central
// differences of step delta (:289-321).  So the scalars and right-hand sides take three streaming passes: a01, b20 and
// <zeta, zeta*> from one pass over (u, zeta, zeta*) that writes nothing, both projected right-hand sides from one pass over
// (u, zeta), and b11, a02, b30 from one pass over (u, zeta, zeta*, Psi01, Psi20).  The two bordered systems share their matrix:
// with BorderingBLS, J \ r1 and J \ r2 are ONE linsolve2 pair and J \ zeta* is solved once, three GMRES solves where the
// reference's two bls calls run four.  J is singular by construction at these points: an unconverged solve is a flag.
#include <cmath>

#include "common.h"
#include "fold_pw.h"
#include "minaug.h"
#include "ops.h"
#include "stream.h"

namespace bk {

namespace {

// ------------------------------------------------------------------ kernels
// out = ((t(u) x1) x2) x3 = d3F(u)[x1, x2, x3] (bk_d3f)
__global__ void __launch_bounds__(kThreads) nf1d_d3_kernel(size_t n, const double* __restrict__ u, FoldPoly Q,
                                                           const double* __restrict__ x1, const double* __restrict__ x2,
                                                           const double* __restrict__ x3, double* __restrict__ out) {
    const size_t stride = (size_t)gridDim.x * kThreads;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride)
        out[i] = ((fold_poly(Q.h, u[i]) * x1[i]) * x2[i]) * x3[i];
}

// One pass over u, zeta = z, zeta* = zs that writes nothing: three partial sums per workgroup,
//   s0 = sum f(u) zs = a01,   s1 = sum ((h(u) z) z) zs = b20,   s2 = sum z zs = <zeta, zeta*>.
// P = (h, g) of d2F and dJ/dp, Q = (t, f) of d3F and dF/dp.  zs may be the same vector as z (both are only read).  The second
// stage (reduce_finish) keeps the fixed order: the sums are bitwise the same run to run and, all-reduced, on every rank.
struct Nf1dDots {
    static constexpr int NIN = 3, NV = 3, U = 2, FIELDS = 1;
    const double* in[NIN];          // u, z, zs
    FoldPoly P, Q;
    __device__ __forceinline__ void operator()(const double (&x)[NIN], double (&s)[NV]) const {
        const double u = x[0], z = x[1], zs = x[2];
        s[0] += fold_poly(Q.g, u) * zs;
        s[1] += ((fold_poly(P.h, u) * z) * z) * zs;
        s[2] += z * zs;
    }
};

// One pass over u and zeta = z that writes the two projected right-hand sides of the bordered solves,
//   r1 = E(-dpF) = a01 z - f(u),   r2 = E(-d2F[zeta, zeta]) = b20 z - (h(u) z) z.      2 read and 2 write streams.
struct Nf1dRhs {
    static constexpr int NIN = 2, NOUT = 2, U = 1, FIELDS = 1;
    static constexpr bool JOINT = false;
    const double* in[NIN];          // u, z
    double* out[NOUT];              // r1, r2
    FoldPoly P, Q;
    double a01, b20;
    __device__ __forceinline__ void operator()(const double (&x)[NIN], double (&o)[NOUT]) const {
        const double u = x[0], z = x[1];
        o[0] = a01 * z - fold_poly(Q.g, u);
        o[1] = b20 * z - (fold_poly(P.h, u) * z) * z;
    }
};

// One pass over u, zeta = z, zeta* = zs, Psi01 = p, Psi20 = q: three partial sums per workgroup,
//   s0 = sum (g z + (h z) p) zs                  = b11
//   s1 = sum (2 (g p) + (h p) p) zs              = a02      (d2F/dp2 = 0)
//   s2 = sum (((t z) z) z + 3 ((h z) q)) zs      = b30
// without materialising dJ/dp zeta, dJ/dp Psi01, the three d2F and d3F[zeta, zeta, zeta].
struct Nf1dContract {
    static constexpr int NIN = 5, NV = 3, U = 2, FIELDS = 1;
    const double* in[NIN];          // u, z, zs, p, q
    FoldPoly P, Q;
    __device__ __forceinline__ void operator()(const double (&x)[NIN], double (&s)[NV]) const {
        const double u = x[0], z = x[1], zs = x[2], p = x[3], q = x[4];
        const double h = fold_poly(P.h, u), g = fold_poly(P.g, u), t = fold_poly(Q.h, u);
        const double hz = h * z;
        s[0] += (g * z + hz * p) * zs;
        s[1] += (2.0 * (g * p) + (h * p) * p) * zs;
        s[2] += (((t * z) * z) * z + 3.0 * (hz * q)) * zs;
    }
};

// M <= kPredict predictor vectors per launch: out_k = ((x0 + a_k zeta) + b_k Psi01) + c_k tau in one pass over the inputs
// (src/NormalForms.jl:410-419, :480, :524).  Psi01 and tau may be NULL: the stream is then not read and its term is dropped.
// Hand-written on stream_loop, not a pass struct: the optional streams are run-time flags here (as template flags of a struct they
// make 48 instantiations), and each output is stored as it is formed -- the generic writer, which forms all M outputs of an item
// before it stores them, measured 1.5 % slower at M = 4 and 2^27 elements.
constexpr int kPredict = 4;
struct PredictArgs { double a[kPredict], b[kPredict], c[kPredict]; double* out[kPredict]; };

template <int M, int VEC, bool NTH>
__global__ void __launch_bounds__(kThreads) nf1d_predict_kernel(size_t n, const double* __restrict__ x0, const double* __restrict__ pz,
                                                                const double* __restrict__ pp, const double* __restrict__ pt,
                                                                PredictArgs A) {
    const bool hp = pp != nullptr, ht = pt != nullptr;
    auto elem = [&](int k, double x, double z, double p, double t) {
        double r = x + A.a[k] * z;
        if (hp) r = r + A.b[k] * p;
        if (ht) r = r + A.c[k] * t;
        return r;
    };
    if (VEC == 2) {
        const double2 zero = make_double2(0.0, 0.0);
        stream_loop<1>(n >> 1, [&](auto, size_t i, size_t) {
            const double2 x = ld2<NTH>(x0, i), z = ld2<NTH>(pz, i), p = hp ? ld2<NTH>(pp, i) : zero, t = ht ? ld2<NTH>(pt, i) : zero;
#pragma unroll
            for (int k = 0; k < M; ++k) st2(A.out[k], i, elem(k, x.x, z.x, p.x, t.x), elem(k, x.y, z.y, p.y, t.y));
        });
        if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
            const size_t i = n - 1;
#pragma unroll
            for (int k = 0; k < M; ++k) A.out[k][i] = elem(k, x0[i], pz[i], hp ? pp[i] : 0.0, ht ? pt[i] : 0.0);
        }
    } else {
        for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kThreads) {
            const double x = x0[i], z = pz[i], p = hp ? pp[i] : 0.0, t = ht ? pt[i] : 0.0;
#pragma unroll
            for (int k = 0; k < M; ++k) A.out[k][i] = elem(k, x, z, p, t);
        }
    }
}

// ------------------------------------------------------------------ launchers
// (h, g) of d2F, dJ/dp and (t, f) of d3F, dF/dp for params[ipar]; the fold entries' error for any other problem
struct Nf1dPolys { FoldPoly P, Q; };
int nf1d_polys(bk_problem* prob, const double* params, int nparams, int ipar, Nf1dPolys* out) {
    BK_TRY(fold_polys(prob, params, nparams, ipar, out->P.h, out->P.g));
    fold_polys_d3(prob, params, ipar, out->Q.h, out->Q.g);
    return 0;
}

int v_nf1d_d3(bk_ctx* ctx, size_t n, const double* u, const FoldPoly& Q, const double* x1, const double* x2, const double* x3,
              double* out) {
    if (n == 0) return 0;
    ProfScope ps(ctx, "blas1", 8.0 * n * 5);
    hipLaunchKernelGGL(nf1d_d3_kernel, dim3(grid_for(n, 1, 4096)), dim3(kThreads), 0, ctx->stream, n, u, Q, x1, x2, x3, out);
    BK_HIP(ctx, hipGetLastError());
    return 0;
}

// out[3] = (a01, b20, <zeta, zeta*>)
int v_nf1d_dots(bk_ctx* ctx, size_t n, const double* u, const double* z, const double* zs, const Nf1dPolys& C, double* out) {
    return stream_reduce(ctx, "nf1d_dots", n, Nf1dDots{{u, z, zs}, C.P, C.Q}, out);
}

int v_nf1d_rhs(bk_ctx* ctx, size_t n, const double* u, const double* z, const Nf1dPolys& C, double a01, double b20, double* r1,
               double* r2) {
    return stream_write(ctx, "nf1d_rhs", n, Nf1dRhs{{u, z}, {r1, r2}, C.P, C.Q, a01, b20});
}

// out[3] = (b11, a02, b30)
int v_nf1d_contract(bk_ctx* ctx, size_t n, const double* u, const double* z, const double* zs, const double* p, const double* q,
                    const Nf1dPolys& C, double* out) {
    return stream_reduce(ctx, "nf1d_contract", n, Nf1dContract{{u, z, zs, p, q}, C.P, C.Q}, out);
}

int v_nf1d_predict(bk_ctx* ctx, size_t n, const double* x0, const double* z, const double* p, const double* t, int m,
                   const double* a, const double* b, const double* c, double* const* out) {
    PredictArgs A{};
    bool vec = aligned16(x0) && aligned16(z) && (!p || aligned16(p)) && (!t || aligned16(t));
    for (int k = 0; k < m; ++k) {
        A.a[k] = a[k]; A.b[k] = b[k]; A.c[k] = c[k]; A.out[k] = out[k];
        vec = vec && aligned16(out[k]);
    }
    const bool nth = vec && nt_hint(ctx, n);
    const int grid = grid_for(n, vec ? 2 : 1, 4096);
    ProfScope ps(ctx, "nf1d_predict", 8.0 * n * (2 + (p ? 1 : 0) + (t ? 1 : 0) + m));
    count_dispatch<1, kPredict>(m, [&](auto M) {
        load_path_dispatch(vec, nth, [&](auto V, auto NT) {
            hipLaunchKernelGGL((nf1d_predict_kernel<decltype(M)::value, decltype(V)::value, decltype(NT)::value>), dim3(grid),
                               dim3(kThreads), 0, ctx->stream, n, x0, z, p, t, A);
        });
        return 0;
    });
    BK_HIP(ctx, hipGetLastError());
    return 0;
}

// One GMRES solve's flags into the call's: the AND of the convergence flags, the context counter of unconverged solves
void nf1d_note(bk_ctx* ctx, int converged, int* cv) {
    *cv &= converged ? 1 : 0;
    if (!converged) ctx->diag.nf1d_unconverged += 1.0;
}

}  // namespace
}  // namespace bk

using namespace bk;

extern "C" {

int bk_d3f(bk_problem* prob, const double* u, const double* params, int nparams, const double* dx1, const double* dx2,
           const double* dx3, double* out) {
    if (!prob || !u || !params || !dx1 || !dx2 || !dx3 || !out) return -1;
    Nf1dPolys C;
    BK_TRY(nf1d_polys(prob, params, nparams, 0, &C));
    return v_nf1d_d3(prob->ctx, prob->nloc, u, C.Q, dx1, dx2, dx3, out);
}

int bk_nf1d_dots(bk_problem* prob, const double* u, const double* params, int nparams, int ipar, const double* zeta,
                 const double* zeta_star, double out[3]) {
    if (!prob || !u || !params || !zeta || !zeta_star || !out) return -1;
    Nf1dPolys C;
    BK_TRY(nf1d_polys(prob, params, nparams, ipar, &C));
    return v_nf1d_dots(prob->ctx, prob->nloc, u, zeta, zeta_star, C, out);
}

int bk_nf1d_rhs(bk_problem* prob, const double* u, const double* params, int nparams, int ipar, const double* zeta, double a01,
                double b20, double* r01, double* r20) {
    if (!prob || !u || !params || !zeta || !r01 || !r20) return -1;
    Nf1dPolys C;
    BK_TRY(nf1d_polys(prob, params, nparams, ipar, &C));
    if (r01 == r20) return set_error(prob->ctx, "bk_nf1d_rhs: r01 and r20 must be distinct");
    if (r01 == u || r01 == zeta || r20 == u || r20 == zeta) return set_error(prob->ctx, "bk_nf1d_rhs: an output aliases an input");
    return v_nf1d_rhs(prob->ctx, prob->nloc, u, zeta, C, a01, b20, r01, r20);
}

int bk_nf1d_contract(bk_problem* prob, const double* u, const double* params, int nparams, int ipar, const double* zeta,
                     const double* zeta_star, const double* psi01, const double* psi20, double out[3]) {
    if (!prob || !u || !params || !zeta || !zeta_star || !psi01 || !psi20 || !out) return -1;
    Nf1dPolys C;
    BK_TRY(nf1d_polys(prob, params, nparams, ipar, &C));
    return v_nf1d_contract(prob->ctx, prob->nloc, u, zeta, zeta_star, psi01, psi20, C, out);
}

int bk_nf1d_predict(bk_ctx* ctx, size_t n, const double* x0, const double* zeta, const double* psi01, const double* tau, int M,
                    const double* alpha, const double* beta, const double* gamma, double* const* out) {
    if (!ctx || !x0 || !zeta || !alpha || !beta || !gamma || !out) return -1;
    if (M < 1 || M > kPredict) return set_error(ctx, "bk_nf1d_predict: 1 <= M <= %d outputs (got %d)", kPredict, M);
    const double* ins[4] = {x0, zeta, psi01, tau};
    for (int k = 0; k < M; ++k) {
        if (!out[k]) return -1;
        if ((!psi01 && beta[k] != 0.0) || (!tau && gamma[k] != 0.0))
            return set_error(ctx, "bk_nf1d_predict: a non-zero coefficient on a NULL vector (output %d)", k);
        for (const double* i : ins)
            if (out[k] == i) return set_error(ctx, "bk_nf1d_predict: an output aliases an input");
        for (int j = 0; j < k; ++j)
            if (out[k] == out[j]) return set_error(ctx, "bk_nf1d_predict: the output vectors must be distinct");
    }
    if (n == 0) return 0;
    return v_nf1d_predict(ctx, n, x0, zeta, psi01, tau, M, alpha, beta, gamma, out);
}

int bk_normal_form_1d(bk_ctx* ctx, bk_problem* prob, const double* x, const double* params, int nparams, int ipar,
                      const double* zeta, const double* zeta_star, const bk_bordering_opts* bopts, const bk_gmres_opts* lsopts,
                      bk_precond* pl, double* psi01, double* psi20, double coef[5], int* converged, int itlinear[3]) {
    if (!ctx || !prob || !x || !params || !zeta || !zeta_star || !bopts || !lsopts || !psi01 || !psi20 || !coef) return -1;
    BK_TRY(minaug_check(ctx, prob, "normal form"));
    Nf1dPolys C;
    BK_TRY(nf1d_polys(prob, params, nparams, ipar, &C));
    if (psi01 == psi20) return set_error(ctx, "bk_normal_form_1d: Psi01 and Psi20 must be distinct");
    for (const double* o : {(const double*)psi01, (const double*)psi20})
        if (o == x || o == zeta || o == zeta_star)
            return set_error(ctx, "bk_normal_form_1d: the Psi vectors must not alias x, zeta or zeta*");
    if (bopts->kind == 0 && bopts->k < 1) return set_error(ctx, "BorderingBLS: number of recursions must be positive");
    const size_t n = prob->nloc;
    double d[3];
    BK_TRY(v_nf1d_dots(ctx, n, x, zeta, zeta_star, C, d));
    const double a01 = d[0], b20 = d[1];
    if (!(std::fabs(d[2] - 1.0) <= 1e-8))
        return set_error(ctx, "bk_normal_form_1d: Error of precision in normalization: <zeta, zeta*> = %.17g, expected 1", d[2]);
    WsGuard ws(ctx);
    double* R[2] = {nullptr, nullptr};
    BK_TRY(ws.get(n, &R[0]));
    BK_TRY(ws.get(n, &R[1]));
    BK_TRY(v_nf1d_rhs(ctx, n, x, zeta, C, a01, b20, R[0], R[1]));
    double* Psi[2] = {psi01, psi20};
    int cv = 1, it[3] = {0, 0, 0};
    {
        JPair jp;
        BK_TRY(jp.make(prob, x, params, nparams));
        if (bopts->kind == 1) {
            // MatrixFreeBLS: one GMRES on the (N + 1) operator per system, bls(L, zeta*, zeta, 0, R, 0) (:303, :333)
            for (int k = 0; k < 2; ++k) {
                double s = 0.0;
                int c1 = 0;
                BK_TRY(bk_bls_matrixfree(ctx, jp.J, zeta_star, zeta, 0.0, R[k], 0.0, 1.0, 1.0, 0, 0.0, 1.0, lsopts, Psi[k], &s, &c1,
                                         &it[k]));
                nf1d_note(ctx, c1, &cv);
            }
        } else {
            // BorderingBLS (src/LinearBorderSolver.jl:125-144) on both systems at once: x1_k = J \ R_k as one pair, ONE
            // x2 = J \ zeta*, s_k = (0 - <zeta, x1_k>) / (0 - <zeta, x2>), Psi_k = x1_k - s_k x2
            double* x2 = nullptr;
            BK_TRY(ws.get(n, &x2));
            GmresResult r0, r1, r2;
            BK_TRY(linsolve2(ctx, jp.J, R[0], Psi[0], R[1], Psi[1], 0.0, 1.0, *lsopts, pl, &r0, &r1));
            BK_TRY(linsolve(ctx, jp.J, zeta_star, x2, 0.0, 1.0, *lsopts, pl, &r2));
            nf1d_note(ctx, r0.converged, &cv);
            nf1d_note(ctx, r1.converged, &cv);
            nf1d_note(ctx, r2.converged, &cv);
            it[0] = r0.niter; it[1] = r1.niter; it[2] = r2.niter;
            double dx2, dk[2];
            BK_TRY(v_dot(ctx, n, zeta, x2, &dx2));
            BK_TRY(v_dot2(ctx, n, zeta, Psi[0], Psi[1], dk));
            double *dXr = nullptr, *dX1 = nullptr;
            for (int k = 0; k < 2; ++k) {
                double s = dk[k] / dx2;
                BK_TRY(v_axpby(ctx, n, -s, x2, 1.0, Psi[k]));
                // residualBEC (:146-166) and the corrections of check_precision, with the x2 of above
                int pass = 0;
                bool fail = true;
                while (bopts->check_precision && pass < bopts->k && fail) {
                    if (!dXr) { BK_TRY(ws.get(n, &dXr)); BK_TRY(ws.get(n, &dX1)); }
                    BK_TRY(jp.J->apply(Psi[k], nullptr, 0.0, 1.0, dXr, nullptr));
                    BK_TRY(v_axpby(ctx, n, s, zeta_star, 1.0, dXr));
                    BK_TRY(v_axpby(ctx, n, 1.0, R[k], -1.0, dXr));
                    double dd, nr;
                    BK_TRY(v_dot(ctx, n, zeta, Psi[k], &dd));
                    const double sr = 0.0 - dd;
                    BK_TRY(v_nrm2(ctx, n, dXr, &nr));
                    fail = nr > bopts->tol || std::fabs(sr) > bopts->tol;
                    if (fail) {
                        GmresResult rc;
                        BK_TRY(linsolve(ctx, jp.J, dXr, dX1, 0.0, 1.0, *lsopts, pl, &rc));
                        nf1d_note(ctx, rc.converged, &cv);
                        it[k] += rc.niter;
                        double d1;
                        BK_TRY(v_dot(ctx, n, zeta, dX1, &d1));
                        const double s1 = (sr - d1) / (0.0 - dx2);
                        BK_TRY(v_axpby(ctx, n, -s1, x2, 1.0, dX1));
                        BK_TRY(v_axpby(ctx, n, 1.0, dX1, 1.0, Psi[k]));
                        s += s1;
                        pass += 1;
                    }
                }
            }
        }
    }
    double c3[3];
    BK_TRY(v_nf1d_contract(ctx, n, x, zeta, zeta_star, psi01, psi20, C, c3));
    coef[0] = a01; coef[1] = c3[1]; coef[2] = c3[0]; coef[3] = b20; coef[4] = c3[2];
    if (converged) *converged = cv;
    if (itlinear) { itlinear[0] = it[0]; itlinear[1] = it[1]; itlinear[2] = it[2]; }
    return 0;
}

}  // extern "C"
