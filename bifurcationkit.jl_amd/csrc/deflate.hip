// Deflation with the exact derivative: DeflationOperator(power, dot, alpha, roots; autodiff = true) (src/DeflationOperator.jl:61-169)
// and Newton on M(u) F(u) (solve(prob, defOp, options, DeflatedProblemCustomLS()), :258-355) for the multicontinuation of
// src/bifdiagram/BranchSwitching.jl:298-352, which deflates 9 to 27 states.  With t_i = u - r_i,
//
//   d_i = <t_i, t_i>,  e_i = <t_i, h>,  m_i = d_i^-power + alpha,
//   M(u) = prod_i m_i,                  dM(u) . h = sum_i (prod_{j != i} m_j) (-2 power d_i^(-power - 1)) e_i      (Val(:Prod))
//   M(u) = (sum_i m_i) / k,             dM(u) . h = (sum_i (-2 power d_i^(-power - 1)) e_i) / k                    (Val(:Mean))
//
// the analytic form of what :159-169 differentiates.  One pass forms every sum:
//   DeflDots<K, D>   reads u, the direction h (D = 1) and K roots (1 + D + K streams), writes nothing: d[K] and, D = 1, e[K]
// more than 8 roots run as ceil(k / 8) launches.  The host forms M and dM . h from the sums in the fixed order above.
//
// The Newton step needs one linear solve: DeflatedProblemCustomLS (:264-312) solves h1 = J^-1 (M F) and h2 = J^-1 F and steps by
// h = (h1 - z h2) / M, z = dM.h1 / (M + dM.h2); h1 = M h2 by linearity, so with e = dM(u) . h2 the step is
//   x <- x - M / (M + e) h2,
// Sherman-Morrison on M J + F grad M'.
#include <cmath>
#include <vector>

#include "common.h"
#include "deflate.h"
#include "ops.h"
#include "stream.h"

namespace bk {

namespace {

// s[i] = sum t_i t_i,  s[K + i] = sum t_i h  (D = 1),  t_i = u - r_i formed once per element.  U depends on K alone: the d of
// the passes with and without h are then the same sums in the same order, bit for bit.
template <int K, int D>
struct DeflDots {
    static constexpr int NIN = 1 + D + K, NV = K * (1 + D), U = defl_unroll(K), FIELDS = 1;
    static_assert(NV <= kPartialVals, "partial sums per workgroup");
    const double* in[NIN];          // u, h (D = 1), r_0 .. r_{K-1}
    __device__ __forceinline__ void operator()(const double (&x)[NIN], double (&s)[NV]) const {
#pragma unroll
        for (int i = 0; i < K; ++i) {
            const double t = x[0] - x[1 + D + i];
            s[i] += t * t;
            if constexpr (D == 1) s[K + i] += t * x[1];
        }
    }
};

// out[k (1 + D)] = (d | e) of the k <= 8 roots
template <int D>
int defl_chunk(bk_ctx* ctx, size_t n, const double* u, const double* h, const double* const* roots, int k, double* out) {
    return count_dispatch<1, kDeflRoots>(k, [&](auto Kc) {
        constexpr int K = decltype(Kc)::value;
        DeflDots<K, D> pass{};
        pass.in[0] = u;
        if constexpr (D == 1) pass.in[1] = h;
        for (int i = 0; i < K; ++i) pass.in[1 + D + i] = roots[i];
        return stream_reduce(ctx, "deflation_dots", n, pass, out);
    });
}

int v_deflation_dots(bk_ctx* ctx, size_t n, const double* u, const double* h, const double* const* roots, int nroots, double* d,
                     double* e) {
    for (int c = 0; c < nroots; c += kDeflRoots) {
        const int k = nroots - c < kDeflRoots ? nroots - c : kDeflRoots;
        double out[2 * kDeflRoots];
        BK_TRY(h ? defl_chunk<1>(ctx, n, u, h, roots + c, k, out) : defl_chunk<0>(ctx, n, u, nullptr, roots + c, k, out));
        for (int i = 0; i < k; ++i) {
            d[c + i] = out[i];
            if (h) e[c + i] = out[k + i];
        }
    }
    return 0;
}

// M from the d_i; with e != NULL also dM . h.  Products left to right; prod_{j != i} = (m_0 .. m_{i-1}) (m_{i+1} .. m_{k-1}).
void defl_M(const double* d, const double* e, int k, double power, double alpha, int mean, double* M, double* dMh) {
    if (k == 0) {
        *M = 1.0;
        if (dMh) *dMh = 0.0;
        return;
    }
    std::vector<double> m(k), suf(k + 1);
    for (int i = 0; i < k; ++i) m[i] = 1.0 / std::pow(d[i], power) + alpha;
    double acc = m[0];
    for (int i = 1; i < k; ++i) acc = mean ? acc + m[i] : acc * m[i];
    *M = mean ? acc / k : acc;
    if (!dMh) return;
    suf[k] = 1.0;
    for (int i = k - 1; i >= 0; --i) suf[i] = m[i] * suf[i + 1];
    double pre = 1.0, s = 0.0;
    for (int i = 0; i < k; ++i) {
        const double g = (-2.0 * power * std::pow(d[i], -power - 1.0)) * e[i];
        s += mean ? g : (pre * suf[i + 1]) * g;
        pre *= m[i];
    }
    *dMh = mean ? s / k : s;
}

}  // namespace

int defl_newton(bk_ctx* ctx, bk_problem* prob, double* x, const double* params, int nparams, const double* const* roots, int nroots,
                double power, double alpha, int accumulator_mean, int stop_plain, int norm_inf, double tol, int max_iterations,
                const bk_gmres_opts* lsopts, bk_precond* pl, double* hist, int cap, DeflNewton* out) {
    const size_t n = prob->nloc;
    WsGuard ws(ctx);
    double *fx = nullptr, *h2 = nullptr;
    BK_TRY(ws.get(n, &fx));
    BK_TRY(ws.get(n, &h2));
    std::vector<double> d(nroots), e(nroots);
    const bool inf = norm_inf != 0;
    double M = 1.0, r = 0.0, rf = 0.0;
    // F(x), the d_i and M(x); r = |M| |F| (the reference's rule: |M F| needs no vector) or |F|
    auto residual = [&]() -> int {
        BK_TRY(bk_residual(prob, x, params, nparams, fx));
        BK_TRY(v_deflation_dots(ctx, n, x, nullptr, roots, nroots, d.data(), nullptr));
        defl_M(d.data(), nullptr, nroots, power, alpha, accumulator_mean, &M, nullptr);
        BK_TRY(inf ? v_nrminf(ctx, n, fx, &rf) : v_nrm2(ctx, n, fx, &rf));
        r = stop_plain ? rf : std::fabs(M) * rf;
        return 0;
    };
    BK_TRY(residual());
    int step = 0, itlin = 0;
    hist[0] = r;
    // a root on x: M is infinite, not converged (with stop_plain the plain residual there is small -- x is a deflated state)
    while (step < max_iterations && std::isfinite(M) && r > tol) {
        bk_op* J = nullptr;
        BK_TRY(bk_jacobian(prob, x, params, nparams, &J));
        GmresResult g;
        const int s = linsolve(ctx, J, fx, h2, 0.0, 1.0, *lsopts, pl, &g);           // h2 = J^-1 F; h1 = M h2
        bk_op_destroy(J);
        if (s != 0) return s;
        itlin += g.niter;
        double dMh = 0.0, Mx;
        if (nroots > 0) {
            // e_i at the same x: its d_i are the sums of the residual evaluation again, bit for bit
            BK_TRY(v_deflation_dots(ctx, n, x, h2, roots, nroots, d.data(), e.data()));
            defl_M(d.data(), e.data(), nroots, power, alpha, accumulator_mean, &Mx, &dMh);
        }
        BK_TRY(v_axpby(ctx, n, -(M / (M + dMh)), h2, 1.0, x));
        BK_TRY(residual());
        step += 1;
        hist[step % cap] = r;
    }
    out->converged = std::isfinite(M) && r < tol;
    out->itnewton = step;
    out->itlinear = itlin;
    out->M = M;
    double dmin = HUGE_VAL;
    for (int i = 0; i < nroots; ++i) dmin = d[i] < dmin ? d[i] : dmin;
    out->min_dist = nroots > 0 ? std::sqrt(dmin) : HUGE_VAL;
    out->plain_residual = rf;
    return 0;
}

}  // namespace bk

using namespace bk;

extern "C" {

int bk_deflation_dots(bk_ctx* ctx, size_t n, const double* u, const double* h, const double* const* roots, int nroots, double* d,
                      double* e) {
    if (!ctx || !u || nroots < 0 || (nroots > 0 && (!roots || !d))) return -1;
    if ((h == nullptr) != (e == nullptr)) return set_error(ctx, "bk_deflation_dots: h and e come together (both or neither NULL)");
    for (int i = 0; i < nroots; ++i)
        if (!roots[i]) return -1;
    return v_deflation_dots(ctx, n, u, h, roots, nroots, d, e);
}

int bk_newton_deflated_exact(bk_ctx* ctx, bk_problem* prob, double* x, const double* params, int nparams,
                             const double* const* roots, int nroots, double power, double alpha, int accumulator_mean,
                             int stop_plain, const bk_newton_opts* no, const bk_gmres_opts* lsopts, bk_precond* pl,
                             bk_deflated_result* res) {
    if (!ctx || !prob || !x || !params || !no || !lsopts || !res || nroots < 0 || (nroots > 0 && !roots)) return -1;
    if (no->max_iterations > BK_MAX_NEWTON_ITER) return set_error(ctx, "max_iterations > %d", BK_MAX_NEWTON_ITER);
    for (int i = 0; i < nroots; ++i) {
        if (!roots[i]) return -1;
        if (roots[i] == x) return set_error(ctx, "bk_newton_deflated_exact: x aliases root %d (the iterate is updated in place)", i);
    }
    DeflNewton o;
    BK_TRY(defl_newton(ctx, prob, x, params, nparams, roots, nroots, power, alpha, accumulator_mean, stop_plain, no->norm_inf, no->tol,
                       no->max_iterations, lsopts, pl, res->residuals, BK_MAX_NEWTON_ITER + 1, &o));
    res->converged = o.converged;
    res->itnewton = o.itnewton;
    res->itlinear = o.itlinear;
    res->M = o.M;
    res->min_dist = o.min_dist;
    return 0;
}

}  // extern "C"
