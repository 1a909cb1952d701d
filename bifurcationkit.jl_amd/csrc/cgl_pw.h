// The pointwise part of the cGL vector field and its Jacobian block, one copy for every kernel that evaluates them: the stencil
// kernel (stencil.hip: cgl_kernel, dparam_kernel) and the marching kernels of the trapezoid periodic-orbit functional (potrap.hip,
// pofold.hip).
//   NL(z) = (r + i nu) z - (c3 + i mu) |z|^2 z - c5 |z|^4 z + gamma,   z = x1 + i x2      (examples/cGL2d.jl:24-40)
// The expressions are the ones cgl_kernel has always evaluated, term for term: the library is built with -ffp-contract=off, so
// every caller rounds them the same way.
// Internal header.
#pragma once
#include <hip/hip_runtime.h>

namespace bk {

struct CglPar { double r, mu, nu, c3, c5, gamma; };

// (n1, n2) = NL(x1, x2)
__device__ __forceinline__ void cgl_nl(const CglPar& p, double x1, double x2, double& n1, double& n2) {
    const double r = p.r, mu = p.mu, nu = p.nu, c3 = p.c3, c5 = p.c5;
    const double ua = x1 * x1 + x2 * x2;
    n1 = (r * x1 - nu * x2 - ua * (c3 * x1 - mu * x2) - c5 * ua * ua * x1 + p.gamma);
    n2 = (r * x2 + nu * x1 - ua * (c3 * x2 + mu * x1) - c5 * ua * ua * x2);
}

// closed-form Jacobian block of NL at (u1, u2): Jcgl, examples/cGL2d.jl:66-69, [[f1u, f1v], [f2u, f2v]]
__device__ __forceinline__ void cgl_jac(const CglPar& p, double u1, double u2, double& f1u, double& f1v, double& f2u, double& f2v) {
    const double r = p.r, mu = p.mu, nu = p.nu, c3 = p.c3, c5 = p.c5;
    const double ua = u1 * u1 + u2 * u2;
    f1u = r - 2 * u1 * (c3 * u1 - mu * u2) - c3 * ua - 4 * c5 * ua * u1 * u1 - c5 * ua * ua;
    f1v = -nu - 2 * u2 * (c3 * u1 - mu * u2) + mu * ua - 4 * c5 * ua * u1 * u2;
    f2u = nu - 2 * u1 * (c3 * u2 + mu * u1) - mu * ua - 4 * c5 * ua * u1 * u2;
    f2v = r - 2 * u2 * (c3 * u2 + mu * u1) - c3 * ua - 4 * c5 * ua * u2 * u2 - c5 * ua * ua;
}

// (o1, o2) = dNL/dp at (u1, u2) for params[ipar] = (r, mu, nu, c3, c5, gamma): the pointwise parameter derivative of the vector
// field (pde_dparam, stencil.hip) and of the fold border of the orbit functional (pofold.hip)
__device__ __forceinline__ void cgl_dpar(int ipar, double u1, double u2, double& o1, double& o2) {
    const double ua = u1 * u1 + u2 * u2;
    switch (ipar) {
        case 0: o1 = u1; o2 = u2; break;
        case 1: o1 = ua * u2; o2 = -ua * u1; break;
        case 2: o1 = -u2; o2 = u1; break;
        case 3: o1 = -ua * u1; o2 = -ua * u2; break;
        case 4: o1 = -ua * ua * u1; o2 = -ua * ua * u2; break;
        default: o1 = 1.0; o2 = 0.0; break;
    }
}

}  // namespace bk
