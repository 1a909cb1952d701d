// Normal form at a branch point whose kernel has dimension N = 2 or 3, matrix-free: get_normal_formNd (src/NormalForms.jl:648-896)
// for BK_PDE_SH (2-D / 3-D) and BK_PDE_SH1D.  J' = J, so this is the is_symmetric branch (:741-743): zeta*_i = zeta_i and
// biorthogonalise (:752) leaves an l2-orthonormal basis zeta_0 .. zeta_{N-1} of the kernel.  With E(r) = r - sum_i <r, zeta_i> zeta_i,
// Z = (zeta_0 ... zeta_{N-1}), the bordered matrix B = [J Z; Z' 0] and the pointwise polynomials of fold_pw.h (h = d2F, t = d3F,
// f = dF/dp, g = dJ/dp, d2F/dp2 = 0):
//
//   a01[i]           = <f(u), zeta_i>                                        Psi01: B [Psi01; s] = [E(-f); 0]                  (:783, :798)
//   b20[i, (j,k)]    = <h zeta_j zeta_k, zeta_i>            (j <= k)          Psijk: B [Psijk; s] = [E(-h zeta_j zeta_k); 0]    (:822-826, :844-857)
//   b11[i, j]        = <g zeta_j + h zeta_j Psi01, zeta_i>                                                                     (:800-803)
//   a02[i]           = <2 g Psi01 + h Psi01 Psi01, zeta_i>                                                                     (:812-813)
//   b30[i, (j,k,l)]  = <t zeta_j zeta_k zeta_l + h (zeta_j Psikl + zeta_k Psijl + zeta_l Psijk), zeta_i>     (j <= k <= l)     (:842-871)
//
// P = N (N + 1) / 2 pairs and T = N (N + 1) (N + 2) / 6 triples, both in lexicographic order.  The reference takes wst = -Psi and
// subtracts; it borders with the first two kernel vectors whatever N is (:759-760), re-solves three systems per triple and
// computes a02 once per column j of b11: here the border has all N columns, every Psijk is solved once and a02 once per i.
// Three streaming passes around 1 + P solves of bls_matrixfree_pl (m = N, a = b = zeta, c = 0), which share Pl^-1 zeta_j:
//   NdDots<N>      reads u and the N zeta, writes nothing: a01, b20 and the Gram matrix <zeta_i, zeta_j>
//   NdRhs<N>       reads u and the N zeta, writes the 1 + P projected right-hand sides
//   NdContract<N>  reads u, the N zeta, Psi01 and the P Psijk (7 | 11 streams): b11, a02, b30 (14 | 42 sums)
// An unconverged solve is a flag (the bordered system is regular at the point itself, so none is expected).
#include <cmath>

#include "common.h"
#include "fold_pw.h"
#include "minaug.h"
#include "ops.h"
#include "stream.h"

namespace bk {

namespace {

constexpr int nd_pairs(int N) { return N * (N + 1) / 2; }
constexpr int nd_triples(int N) { return N * (N + 1) * (N + 2) / 6; }
// position of the pair (j <= k) in the lexicographic list (0,0), (0,1), .., (0,N-1), (1,1), ..
template <int N>
__host__ __device__ constexpr int nd_pair(int j, int k) { return j * N - j * (j - 1) / 2 + (k - j); }

// ------------------------------------------------------------------ passes
// One pass over u and zeta_0 .. zeta_{N-1} that writes nothing: N + N P + N N partial sums per workgroup,
//   s[i] = sum f(u) z_i = a01[i],   s[N + i P + jk] = sum ((h(u) z_j) z_k) z_i = b20[i, jk],   s[N + N P + i N + j] = sum z_i z_j.
template <int N>
struct NdDots {
    static constexpr int P = nd_pairs(N);
    static constexpr int NIN = 1 + N, NV = N + N * P + N * N, U = 2, FIELDS = 1;
    static_assert(NV <= kPartialVals, "partial sums per workgroup");
    const double* in[NIN];          // u, z_0 .. z_{N-1}
    FoldPoly Pq, Q;                 // (h, g) and (t, f)
    __device__ __forceinline__ void operator()(const double (&x)[NIN], double (&s)[NV]) const {
        const double u = x[0];
        const double f = fold_poly(Q.g, u), h = fold_poly(Pq.h, u);
#pragma unroll
        for (int i = 0; i < N; ++i) s[i] += f * x[1 + i];
        int jk = 0;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const double hz = h * x[1 + j];
#pragma unroll
            for (int k = j; k < N; ++k, ++jk) {
                const double w = hz * x[1 + k];
#pragma unroll
                for (int i = 0; i < N; ++i) s[N + i * P + jk] += w * x[1 + i];
            }
        }
#pragma unroll
        for (int i = 0; i < N; ++i)
#pragma unroll
            for (int j = 0; j < N; ++j) s[N + N * P + i * N + j] += x[1 + i] * x[1 + j];
    }
};

// One pass over u and the N zeta that writes the 1 + P projected right-hand sides,
//   r01 = E(-f) = sum_i a01[i] z_i - f(u),   r_jk = E(-h zeta_j zeta_k) = sum_i b20[i, jk] z_i - (h(u) z_j) z_k,
// the sum over i left to right from a01[0] z_0, every product and sum rounded on its own.
template <int N>
struct NdRhs {
    static constexpr int P = nd_pairs(N);
    static constexpr int NIN = 1 + N, NOUT = 1 + P, U = 1, FIELDS = 1;
    static constexpr bool JOINT = false;
    const double* in[NIN];          // u, z_0 .. z_{N-1}
    double* out[NOUT];              // r01, r_jk in pair order
    FoldPoly Pq, Q;
    double a01[N], b20[N * P];
    __device__ __forceinline__ void operator()(const double (&x)[NIN], double (&o)[NOUT]) const {
        const double u = x[0];
        double s = a01[0] * x[1];
#pragma unroll
        for (int i = 1; i < N; ++i) s = s + a01[i] * x[1 + i];
        o[0] = s - fold_poly(Q.g, u);
        const double h = fold_poly(Pq.h, u);
        int jk = 0;
#pragma unroll
        for (int j = 0; j < N; ++j)
#pragma unroll
            for (int k = j; k < N; ++k, ++jk) {
                double r = b20[jk] * x[1];
#pragma unroll
                for (int i = 1; i < N; ++i) r = r + b20[i * P + jk] * x[1 + i];
                o[1 + jk] = r - (h * x[1 + j]) * x[1 + k];
            }
    }
};

// One pass over u, the N zeta, Psi01 = p and the P Psijk = q_jk: N N + N + N T partial sums per workgroup,
//   s[i N + j]           = sum (g z_j + (h z_j) p) z_i                                                  = b11[i, j]
//   s[N N + i]           = sum (2 (g p) + (h p) p) z_i                                                  = a02[i]
//   s[N N + N + i T + jkl] = sum (((t z_j) z_k) z_l + (((h z_j) q_kl + (h z_k) q_jl) + (h z_l) q_jk)) z_i  = b30[i, jkl]
// h, g, t and the products h z_j are formed once per element, every bracket once, then multiplied by the N values z_i.  Written
// through bk_d2f / bk_d3f and dots the same sums read well over a hundred streams at N = 3.
template <int N>
struct NdContract {
    static constexpr int P = nd_pairs(N), T = nd_triples(N);
    static constexpr int NIN = 2 + N + P, NV = N * N + N + N * T, U = N == 2 ? 2 : 1, FIELDS = 1;
    static_assert(NV <= kPartialVals, "partial sums per workgroup");
    const double* in[NIN];          // u, z_0 .. z_{N-1}, p, q_jk in pair order
    FoldPoly Pq, Q;
    __device__ __forceinline__ void operator()(const double (&x)[NIN], double (&s)[NV]) const {
        const double u = x[0], p = x[1 + N];
        const double* z = &x[1];
        const double* q = &x[2 + N];
        const double h = fold_poly(Pq.h, u), g = fold_poly(Pq.g, u), t = fold_poly(Q.h, u);
        double hz[N];
#pragma unroll
        for (int j = 0; j < N; ++j) hz[j] = h * z[j];
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const double b = g * z[j] + hz[j] * p;
#pragma unroll
            for (int i = 0; i < N; ++i) s[i * N + j] += b * z[i];
        }
        const double a = 2.0 * (g * p) + (h * p) * p;
#pragma unroll
        for (int i = 0; i < N; ++i) s[N * N + i] += a * z[i];
        int jkl = 0;
#pragma unroll
        for (int j = 0; j < N; ++j)
#pragma unroll
            for (int k = j; k < N; ++k)
#pragma unroll
                for (int l = k; l < N; ++l, ++jkl) {
                    const double b = ((t * z[j]) * z[k]) * z[l] +
                                     ((hz[j] * q[nd_pair<N>(k, l)] + hz[k] * q[nd_pair<N>(j, l)]) + hz[l] * q[nd_pair<N>(j, k)]);
#pragma unroll
                    for (int i = 0; i < N; ++i) s[N * N + N + i * T + jkl] += b * z[i];
                }
    }
};

// ------------------------------------------------------------------ launchers
struct NdPolys { FoldPoly P, Q; };
int nd_polys(bk_problem* prob, const double* params, int nparams, int ipar, NdPolys* out) {
    BK_TRY(fold_polys(prob, params, nparams, ipar, out->P.h, out->P.g));
    fold_polys_d3(prob, params, ipar, out->Q.h, out->Q.g);
    return 0;
}

int nd_check_n(bk_ctx* ctx, const char* what, int N) {
    if (N != 2 && N != 3) return set_error(ctx, "%s: kernels of dimension 2 and 3 only (got N = %d)", what, N);
    return 0;
}

// out[N + N P + N N] = (a01 | b20 | Gram)
int v_nfnd_dots(bk_ctx* ctx, size_t n, int N, const double* u, const double* const* z, const NdPolys& C, double* out) {
    return count_dispatch<2, 3>(N, [&](auto Nc) {
        constexpr int NN = decltype(Nc)::value;
        NdDots<NN> pass{};
        pass.in[0] = u;
        for (int i = 0; i < NN; ++i) pass.in[1 + i] = z[i];
        pass.Pq = C.P; pass.Q = C.Q;
        return stream_reduce(ctx, "nfnd_dots", n, pass, out);
    });
}

int v_nfnd_rhs(bk_ctx* ctx, size_t n, int N, const double* u, const double* const* z, const NdPolys& C, const double* a01,
               const double* b20, double* const* r) {
    return count_dispatch<2, 3>(N, [&](auto Nc) {
        constexpr int NN = decltype(Nc)::value;
        NdRhs<NN> pass{};
        pass.in[0] = u;
        for (int i = 0; i < NN; ++i) { pass.in[1 + i] = z[i]; pass.a01[i] = a01[i]; }
        for (int i = 0; i < NN * NdRhs<NN>::P; ++i) pass.b20[i] = b20[i];
        for (int i = 0; i < NdRhs<NN>::NOUT; ++i) pass.out[i] = r[i];
        pass.Pq = C.P; pass.Q = C.Q;
        return stream_write(ctx, "nfnd_rhs", n, pass);
    });
}

// out[N N + N + N T] = (b11 | a02 | b30)
int v_nfnd_contract(bk_ctx* ctx, size_t n, int N, const double* u, const double* const* z, const double* psi01,
                    const double* const* psi2, const NdPolys& C, double* out) {
    return count_dispatch<2, 3>(N, [&](auto Nc) {
        constexpr int NN = decltype(Nc)::value;
        NdContract<NN> pass{};
        pass.in[0] = u;
        for (int i = 0; i < NN; ++i) pass.in[1 + i] = z[i];
        pass.in[1 + NN] = psi01;
        for (int i = 0; i < NdContract<NN>::P; ++i) pass.in[2 + NN + i] = psi2[i];
        pass.Pq = C.P; pass.Q = C.Q;
        return stream_reduce(ctx, "nfnd_contract", n, pass, out);
    });
}

// the N zeta (and more read vectors) non-NULL; the `nout` outputs non-NULL, distinct and none of them a read vector
int nd_check_vectors(bk_ctx* ctx, const char* what, int nin, const double* const* in, int nout, double* const* out) {
    for (int i = 0; i < nin; ++i)
        if (!in[i]) return -1;
    for (int k = 0; k < nout; ++k) {
        if (!out[k]) return -1;
        for (int i = 0; i < nin; ++i)
            if (out[k] == in[i]) return set_error(ctx, "%s: an output aliases an input", what);
        for (int j = 0; j < k; ++j)
            if (out[k] == out[j]) return set_error(ctx, "%s: the output vectors must be distinct", what);
    }
    return 0;
}

}  // namespace
}  // namespace bk

using namespace bk;

extern "C" {

int bk_nfnd_dots(bk_problem* prob, const double* u, const double* params, int nparams, int ipar, int N, const double* const* zeta,
                 double* out) {
    if (!prob || !u || !params || !zeta || !out) return -1;
    BK_TRY(nd_check_n(prob->ctx, "bk_nfnd_dots", N));
    NdPolys C;
    BK_TRY(nd_polys(prob, params, nparams, ipar, &C));
    BK_TRY(nd_check_vectors(prob->ctx, "bk_nfnd_dots", N, zeta, 0, nullptr));
    return v_nfnd_dots(prob->ctx, prob->nloc, N, u, zeta, C, out);
}

int bk_nfnd_rhs(bk_problem* prob, const double* u, const double* params, int nparams, int ipar, int N, const double* const* zeta,
                const double* a01, const double* b20, double* const* r) {
    if (!prob || !u || !params || !zeta || !a01 || !b20 || !r) return -1;
    BK_TRY(nd_check_n(prob->ctx, "bk_nfnd_rhs", N));
    NdPolys C;
    BK_TRY(nd_polys(prob, params, nparams, ipar, &C));
    const double* in[4] = {u, nullptr, nullptr, nullptr};
    for (int i = 0; i < N; ++i) in[1 + i] = zeta[i];
    BK_TRY(nd_check_vectors(prob->ctx, "bk_nfnd_rhs", 1 + N, in, 1 + nd_pairs(N), r));
    return v_nfnd_rhs(prob->ctx, prob->nloc, N, u, zeta, C, a01, b20, r);
}

int bk_nfnd_contract(bk_problem* prob, const double* u, const double* params, int nparams, int ipar, int N,
                     const double* const* zeta, const double* psi01, const double* const* psi2, double* out) {
    if (!prob || !u || !params || !zeta || !psi01 || !psi2 || !out) return -1;
    BK_TRY(nd_check_n(prob->ctx, "bk_nfnd_contract", N));
    NdPolys C;
    BK_TRY(nd_polys(prob, params, nparams, ipar, &C));
    BK_TRY(nd_check_vectors(prob->ctx, "bk_nfnd_contract", N, zeta, 0, nullptr));
    BK_TRY(nd_check_vectors(prob->ctx, "bk_nfnd_contract", nd_pairs(N), psi2, 0, nullptr));
    return v_nfnd_contract(prob->ctx, prob->nloc, N, u, zeta, psi01, psi2, C, out);
}

int bk_normal_form_nd(bk_ctx* ctx, bk_problem* prob, const double* x, const double* params, int nparams, int ipar, int N,
                      const double* const* zeta, const bk_gmres_opts* lsopts, bk_precond* pl, double* psi01, double* const* psi2,
                      double* coef, int* converged, int* itlinear) {
    if (!ctx || !prob || !x || !params || !zeta || !lsopts || !psi01 || !psi2 || !coef) return -1;
    BK_TRY(minaug_check(ctx, prob, "normal form"));
    BK_TRY(nd_check_n(ctx, "bk_normal_form_nd", N));
    NdPolys C;
    BK_TRY(nd_polys(prob, params, nparams, ipar, &C));
    if (!pl) return set_error(ctx, "bk_normal_form_nd: the bordered solves need the left preconditioner (pl == NULL)");
    const int P = nd_pairs(N), T = nd_triples(N);
    const double* in[4] = {x, nullptr, nullptr, nullptr};
    for (int i = 0; i < N; ++i) in[1 + i] = zeta[i];
    double* Psi[1 + 6];
    Psi[0] = psi01;
    for (int k = 0; k < P; ++k) Psi[1 + k] = psi2[k];
    BK_TRY(nd_check_vectors(ctx, "bk_normal_form_nd", 1 + N, in, 1 + P, Psi));
    const size_t n = prob->nloc;
    double d[NdDots<3>::NV];
    BK_TRY(v_nfnd_dots(ctx, n, N, x, zeta, C, d));
    const double *a01 = d, *b20 = d + N, *gram = d + N + N * P;
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j)
            if (!(std::fabs(gram[i * N + j] - (i == j ? 1.0 : 0.0)) <= 1e-8))
                return set_error(ctx, "bk_normal_form_nd: the kernel basis is not orthonormal: <zeta_%d, zeta_%d> = %.17g", i, j,
                                 gram[i * N + j]);
    WsGuard ws(ctx);
    double* R[1 + 6];
    for (int k = 0; k < 1 + P; ++k) BK_TRY(ws.get(n, &R[k]));
    BK_TRY(v_nfnd_rhs(ctx, n, N, x, zeta, C, a01, b20, R));
    int cv = 1;
    {
        JPair jp;
        BK_TRY(jp.make(prob, x, params, nparams));
        // bls(L, zeta*, zeta, 0, R, 0) (:763) with all N columns; Pl^-1 zeta_j is formed once for the 1 + P solves
        double* at[3];
        for (int j = 0; j < N; ++j) {
            BK_TRY(ws.get(n, &at[j]));
            BK_TRY(pl->apply(zeta[j], at[j]));
        }
        const double c[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, rb[3] = {0.0, 0.0, 0.0};
        for (int k = 0; k < 1 + P; ++k) {
            double s[3];
            GmresResult r;
            BK_TRY(bls_matrixfree_pl(ctx, jp.J, N, zeta, zeta, 1.0, c, R[k], rb, false, 0.0, *lsopts, pl, Psi[k], s, &r, at));
            cv &= r.converged ? 1 : 0;
            if (!r.converged) ctx->diag.nfnd_unconverged += 1.0;
            if (itlinear) itlinear[k] = r.niter;
        }
    }
    double c3[NdContract<3>::NV];
    BK_TRY(v_nfnd_contract(ctx, n, N, x, zeta, psi01, psi2, C, c3));
    // coef = [a01 | a02 | b11 | b20 | b30]
    double* o = coef;
    for (int i = 0; i < N; ++i) *o++ = a01[i];
    for (int i = 0; i < N; ++i) *o++ = c3[N * N + i];
    for (int i = 0; i < N * N; ++i) *o++ = c3[i];
    for (int i = 0; i < N * P; ++i) *o++ = b20[i];
    for (int i = 0; i < N * T; ++i) *o++ = c3[N * N + N + i];
    if (converged) *converged = cv;
    return 0;
}

}  // extern "C"
