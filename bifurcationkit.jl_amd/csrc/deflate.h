// What deflate.hip shares with defcont.hip: the launch shape of the deflation passes and the deflated Newton loop.
// Internal header.
#pragma once
#include "common.h"

namespace bk {

constexpr int kDeflRoots = 8;   // roots per launch of a deflation pass
// 16-byte items per lane in flight of a deflation pass over K roots.  It depends on K alone, so every pass that forms
// d_i = sum (u - r_i)^2 -- with h, without it, with the inf-norm next to it -- adds the same terms in the same order.
constexpr int defl_unroll(int K) { return K <= 3 ? 2 : 1; }

struct DeflNewton {             // what defl_newton returns next to x
    int converged, itnewton, itlinear;
    double M;                   // M at the final x
    double min_dist;            // min_i sqrt(d_i) at the final x, +inf without roots
    double plain_residual;      // |F(x)| at the final x in the norm stopped in, from the last evaluation of F
};

// _newton (src/Newton.jl:66-114) on M(u) F(u) with the exact dM and one linear solve per step: the loop of
// bk_newton_deflated_exact and bk_defcont_seek.  Entry k of the residual history goes to hist[k % cap]; there are
// itnewton + 1 of them.
int defl_newton(bk_ctx* ctx, bk_problem* prob, double* x, const double* params, int nparams, const double* const* roots, int nroots,
                double power, double alpha, int accumulator_mean, int stop_plain, int norm_inf, double tol, int max_iterations,
                const bk_gmres_opts* lsopts, bk_precond* pl, double* hist, int cap, DeflNewton* out);

}  // namespace bk
