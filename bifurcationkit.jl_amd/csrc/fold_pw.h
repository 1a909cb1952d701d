// The pointwise polynomial tensors of the Swift-Hohenberg nonlinearities that the minimally augmented fold formulation
// (fold.hip) and the normal form at simple branch points and folds (nf1d.hip) contract.  Every factor is a cubic in u,
// c[0] + u (c[1] + u (c[2] + u c[3])):
//   BK_PDE_SH   d2F: h = 2 nu - 6 u         d3F: t = -6              (examples/SH2d-fronts.jl:40)
//               dF/dp: f_l = u, f_nu = u^2            dJ/dp: g_l = 1, g_nu = 2 u
//   BK_PDE_SH1D d2F: h = 6 nu u - 20 u^3    d3F: t = 6 nu - 60 u^2   (examples/SHpde_snaking.jl:26)
//               dF/dp: f_lam = u, f_nu = u^3          dJ/dp: g_lam = 1, g_nu = 3 u^2
// The linear part is parameter-free, so these are the whole of d2F, d3F, dF/dp and dJ/dp; d2F/dp2 = 0.
// Internal header.
#pragma once
#include "common.h"
#include "ops.h"

namespace bk {
namespace {

// Pointwise polynomial factors c[0] + u (c[1] + u (c[2] + u c[3])) of d2F (h) and dJ/dp (g), evaluated in this one fixed
// Horner order (tests/test_gpu_fold.py restates it).  nf1d.hip carries d3F and dF/dp in a second FoldPoly (h = t, g = f).
struct FoldPoly { double h[4]; double g[4]; };
__device__ __forceinline__ double fold_poly(const double* c, double u) { return c[0] + u * (c[1] + u * (c[2] + u * c[3])); }

// polynomial coefficients (c0 + u (c1 + u (c2 + u c3))) of h(u) and g_ipar(u); an error for problems without the formulation
int fold_polys(bk_problem* prob, const double* params, int nparams, int ipar, double h[4], double g[4]) {
    bk_ctx* ctx = prob->ctx;
    const int pde = prob->desc.pde;
    if (pde != BK_PDE_SH && pde != BK_PDE_SH1D)
        return set_error(ctx, "fold: the minimally augmented fold formulation is available for BK_PDE_SH and BK_PDE_SH1D only "
                              "(symmetric Jacobian with an analytic Hessian), not for problem kind %d", pde);
    if (nparams < 2 || nparams > BK_MAX_PARAMS) return set_error(ctx, "fold: the SH problems take params = {l | lambda, nu}");
    if (ipar < 0 || ipar > 1) return set_error(ctx, "fold: bad parameter index %d", ipar);
    const double nu = params[1];
    for (int i = 0; i < 4; ++i) h[i] = g[i] = 0.0;
    if (pde == BK_PDE_SH) {
        h[0] = 2.0 * nu; h[1] = -6.0;
        if (ipar == 0) g[0] = 1.0; else g[1] = 2.0;
    } else {
        h[1] = 6.0 * nu; h[3] = -20.0;
        if (ipar == 0) g[0] = 1.0; else g[2] = 3.0;
    }
    return 0;
}

// ... and of t(u) = h'(u) (d3F) and f_ipar(u) (dF/dp, g = f'), for a problem fold_polys accepted
void fold_polys_d3(bk_problem* prob, const double* params, int ipar, double t[4], double f[4]) {
    const double nu = params[1];
    for (int i = 0; i < 4; ++i) t[i] = f[i] = 0.0;
    if (prob->desc.pde == BK_PDE_SH) {
        t[0] = -6.0;
        if (ipar == 0) f[1] = 1.0; else f[2] = 1.0;
    } else {
        t[0] = 6.0 * nu; t[2] = -60.0;
        if (ipar == 0) f[1] = 1.0; else f[3] = 1.0;
    }
}

}  // namespace
}  // namespace bk
