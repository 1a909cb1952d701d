// The pointwise tensors of the cGL nonlinearity (examples/cGL2d.jl:24-40) that the Hopf formulation (hopf.hip) and the Hopf
// normal form (hopf_nf.hip) contract:
//   NL(z) = (r + i nu) z - (c3 + i mu) |z|^2 z - c5 |z|^4 z + gamma,   z = u1 + i u2,
// per grid point and field f: the Hessian H_f (symmetric 2 x 2), the third derivative T_f (symmetric 2 x 2 x 2) and
// dJ/dp = D_p (2 x 2), all in closed form.  The Laplacian is linear, so d2F = d2NL and d3F = d3NL.
// Internal header.
#pragma once
#include "common.h"
#include "ops.h"

namespace bk {
namespace {

struct CglCoef { double mu, c3, c5; int ipar; };

// Hessian of NL at (u1, u2): H1 = [[h[0], h[1]], [h[1], h[2]]] (field 1), H2 = [[h[3], h[4]], [h[4], h[5]]] (field 2)
__device__ __forceinline__ void cgl_hess(const CglCoef& c, double u1, double u2, double h[6]) {
    const double ua = u1 * u1 + u2 * u2;
    const double q1 = u1 * (8.0 * u1 * u1 + 12.0 * ua), q2 = u2 * (8.0 * u1 * u1 + 4.0 * ua);
    const double q3 = u1 * (8.0 * u2 * u2 + 4.0 * ua), q4 = u2 * (8.0 * u2 * u2 + 12.0 * ua);
    h[0] = -6.0 * c.c3 * u1 + 2.0 * c.mu * u2 - c.c5 * q1;
    h[1] = -2.0 * c.c3 * u2 + 2.0 * c.mu * u1 - c.c5 * q2;
    h[2] = -2.0 * c.c3 * u1 + 6.0 * c.mu * u2 - c.c5 * q3;
    h[3] = -2.0 * c.c3 * u2 - 6.0 * c.mu * u1 - c.c5 * q2;
    h[4] = -2.0 * c.c3 * u1 - 2.0 * c.mu * u2 - c.c5 * q3;
    h[5] = -6.0 * c.c3 * u2 - 2.0 * c.mu * u1 - c.c5 * q4;
}

// Third derivative of NL at (u1, u2), the u-derivative of cgl_hess: per field the four independent entries of the symmetric
// tensor in the order (111, 112, 122, 222), field 1 in t[0..3], field 2 in t[4..7].  The cubic term gives the constants, the
// quintic term c5 times quadratics in u.
__device__ __forceinline__ void cgl_d3(const CglCoef& c, double u1, double u2, double t[8]) {
    const double a = u1 * u1, b = u2 * u2, m = 24.0 * (u1 * u2), s = 12.0 * (a + b);
    t[0] = -6.0 * c.c3 - c.c5 * (60.0 * a + 12.0 * b);
    t[1] = 2.0 * c.mu - c.c5 * m;
    t[2] = -2.0 * c.c3 - c.c5 * s;
    t[3] = 6.0 * c.mu - c.c5 * m;
    t[4] = -6.0 * c.mu - c.c5 * m;
    t[5] = -2.0 * c.c3 - c.c5 * s;
    t[6] = -2.0 * c.mu - c.c5 * m;
    t[7] = -6.0 * c.c3 - c.c5 * (12.0 * a + 60.0 * b);
}

// dJ/dp at (u1, u2) for params[ipar] = (r, mu, nu, c3, c5, gamma): D = [[d[0], d[1]], [d[2], d[3]]]
__device__ __forceinline__ void cgl_djdp(int ipar, double u1, double u2, double d[4]) {
    const double ua = u1 * u1 + u2 * u2;
    switch (ipar) {
        case 0: d[0] = 1.0; d[1] = 0.0; d[2] = 0.0; d[3] = 1.0; break;
        case 1: d[0] = 2.0 * u1 * u2; d[1] = 2.0 * u2 * u2 + ua; d[2] = -(2.0 * u1 * u1 + ua); d[3] = -2.0 * u1 * u2; break;
        case 2: d[0] = 0.0; d[1] = -1.0; d[2] = 1.0; d[3] = 0.0; break;
        case 3: d[0] = -(2.0 * u1 * u1 + ua); d[1] = -2.0 * u1 * u2; d[2] = d[1]; d[3] = -(2.0 * u2 * u2 + ua); break;
        case 4: d[0] = -(4.0 * ua * u1 * u1 + ua * ua); d[1] = -4.0 * ua * u1 * u2; d[2] = d[1];
                d[3] = -(4.0 * ua * u2 * u2 + ua * ua); break;
        default: d[0] = d[1] = d[2] = d[3] = 0.0; break;
    }
}

// the coefficients of the tensors from the parameters of a BK_PDE_CGL2D problem; any other problem kind is an error
int hopf_coef(bk_problem* prob, const double* params, int nparams, int ipar, CglCoef* c) {
    bk_ctx* ctx = prob->ctx;
    if (prob->desc.pde != BK_PDE_CGL2D)
        return set_error(ctx, "hopf: the minimally augmented Hopf formulation is available for BK_PDE_CGL2D only "
                              "(analytic Hessian of the cGL nonlinearity), not for problem kind %d", prob->desc.pde);
    if (nparams != 6) return set_error(ctx, "hopf: BK_PDE_CGL2D takes params = {r, mu, nu, c3, c5, gamma} (got %d)", nparams);
    if (ipar < 0 || ipar > 5) return set_error(ctx, "hopf: bad parameter index %d", ipar);
    c->mu = params[1]; c->c3 = params[3]; c->c5 = params[4]; c->ipar = ipar;
    return 0;
}

}  // namespace
}  // namespace bk
