// The pointwise tensors of the cGL nonlinearity (examples/cGL2d.jl:24-40) that the Hopf formulation (hopf.hip), the Hopf
// normal form (hopf_nf.hip) and the Bautin normal form (bautin.hip) contract:
//   NL(z) = (r + i nu) z - (c3 + i mu) |z|^2 z - c5 |z|^4 z + gamma,   z = u1 + i u2,
// per grid point and field f: the Hessian H_f (symmetric 2 x 2), the third derivative T_f (symmetric 2 x 2 x 2) and
// dJ/dp = D_p (2 x 2), all in closed form, and for the Bautin normal form the fourth and fifth derivatives with the helpers that
// contract a symmetric tensor with complex 2-vectors.  The Laplacian is linear, so dkF = dkNL for k >= 2.
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

// Fourth derivative of NL at (u1, u2), the u-derivative of cgl_d3: only the quintic term contributes and it is linear in u.  Per
// field the five independent entries of the symmetric tensor in the order (1111, 1112, 1122, 1222, 2222), field 1 in d[0..4],
// field 2 in d[5..9].
__device__ __forceinline__ void cgl_d4(const CglCoef& c, double u1, double u2, double d[10]) {
    const double a = -24.0 * c.c5, p = a * u1, q = a * u2;
    d[0] = 5.0 * p; d[1] = q; d[2] = p; d[3] = q; d[4] = p;
    d[5] = q; d[6] = p; d[7] = q; d[8] = p; d[9] = 5.0 * q;
}

// Fifth derivative of NL, the u-derivative of cgl_d4: constant.  Per field the six entries (11111, 11112, 11122, 11222, 12222,
// 22222), field 1 in e[0..5], field 2 in e[6..11].
__device__ __forceinline__ void cgl_d5(const CglCoef& c, double e[12]) {
    const double a = -24.0 * c.c5;
    e[0] = 5.0 * a; e[1] = 0.0; e[2] = a; e[3] = 0.0; e[4] = a; e[5] = 0.0;
    e[6] = 0.0; e[7] = a; e[8] = 0.0; e[9] = a; e[10] = 0.0; e[11] = 5.0 * a;
}

// ---- complex arguments: a complex number, a complex 2-vector (one per field) and the contraction of a symmetric tensor of the
// two fields with it.  A symmetric tensor of order K is held as its K + 1 entries t[j], j = how many of its indices are 2; one
// argument v lowers the order by one, o[j] = t[j] v.a + t[j + 1] v.b, and K arguments leave the scalar o[0].
struct Cx { double r, i; };
struct Cx2 { Cx a, b; };
struct Re2 { double a, b; };
__device__ __forceinline__ Cx cx(double r, double i = 0.0) { return Cx{r, i}; }
__device__ __forceinline__ Cx operator+(Cx x, Cx y) { return Cx{x.r + y.r, x.i + y.i}; }
__device__ __forceinline__ Cx operator-(Cx x, Cx y) { return Cx{x.r - y.r, x.i - y.i}; }
__device__ __forceinline__ Cx operator*(Cx x, Cx y) { return Cx{x.r * y.r - x.i * y.i, x.r * y.i + x.i * y.r}; }
__device__ __forceinline__ Cx operator*(double s, Cx y) { return Cx{s * y.r, s * y.i}; }
__device__ __forceinline__ Cx conj(Cx x) { return Cx{x.r, -x.i}; }
__device__ __forceinline__ Cx2 conj(Cx2 v) { return Cx2{conj(v.a), conj(v.b)}; }
__device__ __forceinline__ Cx2 operator*(double s, Cx2 v) { return Cx2{s * v.a, s * v.b}; }
__device__ __forceinline__ Cx2 operator+(Cx2 v, Cx2 w) { return Cx2{v.a + w.a, v.b + w.b}; }

template <int K>
__device__ __forceinline__ void sym_lower(const double (&t)[K + 1], Cx2 v, Cx (&o)[K]) {
#pragma unroll
    for (int j = 0; j < K; ++j) o[j] = t[j] * v.a + t[j + 1] * v.b;
}
template <int K>
__device__ __forceinline__ void sym_lower(const Cx (&t)[K + 1], Cx2 v, Cx (&o)[K]) {
#pragma unroll
    for (int j = 0; j < K; ++j) o[j] = t[j] * v.a + t[j + 1] * v.b;
}
template <int K>
__device__ __forceinline__ void sym_lower(const double (&t)[K + 1], Re2 v, double (&o)[K]) {
#pragma unroll
    for (int j = 0; j < K; ++j) o[j] = t[j] * v.a + t[j + 1] * v.b;
}
template <int K>
__device__ __forceinline__ void sym_conj(const Cx (&t)[K], Cx (&o)[K]) {
#pragma unroll
    for (int j = 0; j < K; ++j) o[j] = conj(t[j]);
}
// the last argument: a tensor of order 1 against v
__device__ __forceinline__ Cx sym_dot(const Cx (&t)[2], Cx2 v) { return t[0] * v.a + t[1] * v.b; }
__device__ __forceinline__ Cx sym_dot(const Cx (&t)[2], Re2 v) { return v.a * t[0] + v.b * t[1]; }
__device__ __forceinline__ Cx sym_dot(const double (&t)[2], Cx2 v) { return t[0] * v.a + t[1] * v.b; }
__device__ __forceinline__ double sym_dot(const double (&t)[2], Re2 v) { return t[0] * v.a + t[1] * v.b; }
// a tensor of order 2 against (v, w)
__device__ __forceinline__ Cx sym_dot(const Cx (&t)[3], Cx2 v, Cx2 w) {
    Cx o[2];
    sym_lower<2>(t, v, o);
    return sym_dot(o, w);
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
