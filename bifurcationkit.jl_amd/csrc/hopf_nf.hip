// Hopf normal form, matrix-free: __hopf_normal_form (src/NormalForms.jl:1009-1076) and the orbit of predictor(::Hopf, ds)
// (:1227-1281) for BK_PDE_CGL2D.  At a Hopf point (x, p, omega) with the eigenvectors zeta of J for i omega and zeta* of J' for
// -i omega, |zeta| = 1, <zeta, zeta*> = 1, inner(x, y) = sum conj(x) y (VectorInterface), R2 = d2F / 2, R3 = d3F / 6:
//
//   Psi001 = -J \ dpF                                   real solve            (:1038)
//   Psi110 = -J \ d2F[zeta, conj zeta]                  real solve            (:1056-1058; d2F[zeta, conj zeta] is real)
//   Psi200 = (2 i omega - J) \ (d2F[zeta, zeta] / 2)    bk_gmres_cshift, a0 = 2 i omega, a1 = -1   (:1051-1053)
//   a = < dJ/dp zeta + d2F[zeta, Psi001], zeta* >                                                   (:1041-1049)
//   b = < d2F[zeta, Psi110] + d2F[conj zeta, Psi200] + d3F[zeta, zeta, conj zeta] / 2, zeta* >      (:1061-1063)
//   z' = z (i omega + a dp + b |z|^2):  Re b < 0 supercritical, Re b > 0 subcritical                (:1067-1073)
//
// dpF and dJ/dp are analytic (pde_dparam, cgl_djdp) where the reference differentiates (ForwardDiff or central differences of
// step delta, :1032-1047), as in the minimally augmented solvers.  J is regular at a Hopf point: no solve is bordered.  Both
// real solves are ONE linsolve2 call (two lanes where the context runs them).  d2F, d3F and dJ/dp are pointwise (hopf_pw.h),
// so the right-hand sides of the last two solves come from one pass over (u, zeta) and a, b from one pass over the nine
// vectors.  Complex vectors are (re, im) pairs of real device vectors of the two stacked fields.
#include <cmath>

#include "common.h"
#include "hopf_pw.h"
#include "minaug.h"
#include "ops.h"
#include "stream.h"

namespace bk {

namespace {

// ------------------------------------------------------------------ kernels
// out = d3F(u)[x1, x2, x3] on the two stacked fields of N points each (bk_hopf_d3f): a^T M_f(c) b with the symmetric 2 x 2
// matrix M_f(c) = T_f . c
__global__ void __launch_bounds__(kThreads) hopf_d3_kernel(size_t N, const double* __restrict__ u, CglCoef c,
                                                           const double* __restrict__ x1, const double* __restrict__ x2,
                                                           const double* __restrict__ x3, double* __restrict__ out) {
    const size_t stride = (size_t)gridDim.x * kThreads;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < N; i += stride) {
        double t[8];
        cgl_d3(c, u[i], u[i + N], t);
        const double a1 = x1[i], a2 = x1[i + N], b1 = x2[i], b2 = x2[i + N], c1 = x3[i], c2 = x3[i + N];
        double o[2];
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            const double m11 = t[4 * f] * c1 + t[4 * f + 1] * c2, m12 = t[4 * f + 1] * c1 + t[4 * f + 2] * c2;
            const double m22 = t[4 * f + 2] * c1 + t[4 * f + 3] * c2;
            o[f] = a1 * (m11 * b1 + m12 * b2) + a2 * (m12 * b1 + m22 * b2);
        }
        out[i] = o[0];
        out[i + N] = o[1];
    }
}

// One pass over u and zeta = x + i y that writes the right-hand sides of the Psi200 and Psi110 solves:
//   r20 = d2F[zeta, zeta] / 2 = (x'Hx - y'Hy) / 2 + i x'Hy,     r11 = s11 d2F[zeta, conj zeta] = s11 (x'Hx + y'Hy)
// per field (s11 = -1 inside bk_hopf_normal_form, whose solve wants the negated vector).  3 read and 3 write streams.
struct HopfNfRhs {
    static constexpr int NIN = 6, NOUT = 6, U = 1, FIELDS = 2;
    static constexpr bool JOINT = true;
    const double* in[NIN / FIELDS];     // u, zr, zi
    double* out[NOUT / FIELDS];         // r20r, r20i, r11
    CglCoef c;
    double s11;
    // o = (r20r_1, r20r_2, r20i_1, r20i_2, r11_1, r11_2) of one grid point
    __device__ __forceinline__ void operator()(const double (&x)[NIN], double (&o)[NOUT]) const {
        const double u1 = x[0], u2 = x[1], x1 = x[2], x2 = x[3], y1 = x[4], y2 = x[5];
        double h[6];
        cgl_hess(c, u1, u2, h);
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            const double hA = h[3 * f], hB = h[3 * f + 1], hC = h[3 * f + 2];
            const double hx1 = hA * x1 + hB * x2, hx2 = hB * x1 + hC * x2;
            const double hy1 = hA * y1 + hB * y2, hy2 = hB * y1 + hC * y2;
            const double xx = x1 * hx1 + x2 * hx2, yy = y1 * hy1 + y2 * hy2, xy = x1 * hy1 + x2 * hy2;
            o[f] = 0.5 * (xx - yy);
            o[2 + f] = xy;
            o[4 + f] = s11 * (xx + yy);
        }
    }
};

// One pass over u, zeta = x + i y (zr, zi), zeta* (sr, si), Psi001 = p, Psi110 = q, Psi200 = gr + i gi: four partial sums per
// workgroup, (Re a, Im a, Re b, Im b).  Every term is zeta or conj zeta against a per-point vector of field f,
//   av_f = zeta . e_f,                          e_f = D_p[f, :] + H_f p
//   bv_f = zeta . r_f + conj(zeta) . G_f,       r_f = H_f q + s_f / 2,   G_f = H_f (gr + i gi)
// with s_f = T_f : (x x' + y y'), because d3F[zeta, zeta, conj zeta] = zeta . s_f  (H_f conj(zeta) = conj(H_f zeta)), and
//   a += conj(av_f) zeta*_f,   b += conj(bv_f) zeta*_f.
// The second stage (reduce_finish) keeps the fixed order: the sums are bitwise the same run to run and, all-reduced, on every rank.
struct HopfNfContract {
    static constexpr int NIN = 18, NV = 4, U = 1, FIELDS = 2;
    const double* in[NIN / FIELDS];     // u, zr, zi, sr, si, p, q, gr, gi
    CglCoef c;
    // one grid point; the second index of every name is the field
    __device__ __forceinline__ void operator()(const double (&v)[NIN], double (&s)[NV]) const {
        const double u1 = v[0], u2 = v[1], x1 = v[2], x2 = v[3], y1 = v[4], y2 = v[5], sr1 = v[6], sr2 = v[7], si1 = v[8],
                     si2 = v[9], p1 = v[10], p2 = v[11], q1 = v[12], q2 = v[13], gr1 = v[14], gr2 = v[15], gi1 = v[16],
                     gi2 = v[17];
        double h[6], d[4], t[8];
        cgl_hess(c, u1, u2, h);
        cgl_djdp(c.ipar, u1, u2, d);
        cgl_d3(c, u1, u2, t);
        const double P11 = x1 * x1 + y1 * y1, P12 = x1 * x2 + y1 * y2, P22 = x2 * x2 + y2 * y2;
        const double sr[2] = {sr1, sr2}, si[2] = {si1, si2};
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            const double hA = h[3 * f], hB = h[3 * f + 1], hC = h[3 * f + 2];
            const double e1 = d[2 * f] + (hA * p1 + hB * p2), e2 = d[2 * f + 1] + (hB * p1 + hC * p2);
            const double s1 = (t[4 * f] * P11 + 2.0 * t[4 * f + 1] * P12) + t[4 * f + 2] * P22;
            const double s2 = (t[4 * f + 1] * P11 + 2.0 * t[4 * f + 2] * P12) + t[4 * f + 3] * P22;
            const double r1 = (hA * q1 + hB * q2) + 0.5 * s1, r2 = (hB * q1 + hC * q2) + 0.5 * s2;
            const double Gr1 = hA * gr1 + hB * gr2, Gr2 = hB * gr1 + hC * gr2;
            const double Gi1 = hA * gi1 + hB * gi2, Gi2 = hB * gi1 + hC * gi2;
            const double avr = x1 * e1 + x2 * e2, avi = y1 * e1 + y2 * e2;
            const double bvr = (x1 * r1 + x2 * r2) + ((x1 * Gr1 + x2 * Gr2) + (y1 * Gi1 + y2 * Gi2));
            const double bvi = (y1 * r1 + y2 * r2) + ((x1 * Gi1 + x2 * Gi2) - (y1 * Gr1 + y2 * Gr2));
            s[0] += avr * sr[f] + avi * si[f];
            s[1] += avr * si[f] - avi * sr[f];
            s[2] += bvr * sr[f] + bvi * si[f];
            s[3] += bvr * si[f] - bvi * sr[f];
        }
    }
};

// out_m = x0 + ds Psi001 + 2 Re(zeta A_m) + |A_m|^2 Psi110 + 2 Re(A_m^2 Psi200)  (src/NormalForms.jl:1262-1271) for m < M <= kOrbit
// phases of the predictor's orbit in one pass: the seven inputs are read once, n elements each (the vectors are walked flat, both
// fields alike).  The coefficients of A_m = amp e^{i t_m} are stored as the pass applies them.
constexpr int kOrbit = 8;
template <int M>
struct HopfOrbit {
    static constexpr int NIN = 7, NOUT = M, U = 1, FIELDS = 1;
    static constexpr bool JOINT = false;
    const double* in[NIN];          // x0, zr, zi, Psi001, Psi110, Re Psi200, Im Psi200
    double* out[NOUT];
    double ds;
    double c1r[M], c1i[M];          // 2 Re A_m, -2 Im A_m          (2 Re(zeta A) = 2 Re A zr - 2 Im A zi)
    double cq[M];                   // |A_m|^2
    double c2r[M], c2i[M];          // 2 Re A_m^2, -2 Im A_m^2
    __device__ __forceinline__ void operator()(const double (&v)[NIN], double (&o)[NOUT]) const {
        const double x = v[0], a = v[1], b = v[2], pp = v[3], qq = v[4], g = v[5], k = v[6];
#pragma unroll
        for (int m = 0; m < M; ++m)
            o[m] = ((((x + ds * pp) + c1r[m] * a) + c1i[m] * b) + cq[m] * qq) + (c2r[m] * g + c2i[m] * k);
    }
};

// ------------------------------------------------------------------ launchers
int v_hopf_d3(bk_ctx* ctx, size_t n, const double* u, const CglCoef& c, const double* x1, const double* x2, const double* x3,
              double* out) {
    const size_t N = n / 2;
    if (N == 0) return 0;
    ProfScope ps(ctx, "blas1", 8.0 * n * 5);
    hipLaunchKernelGGL(hopf_d3_kernel, dim3(grid_for(N, 1, 4096)), dim3(kThreads), 0, ctx->stream, N, u, c, x1, x2, x3, out);
    BK_HIP(ctx, hipGetLastError());
    return 0;
}

// r20 = d2F[zeta, zeta] / 2 as (re, im), r11 = s11 d2F[zeta, conj zeta]; n = 2 N, the local length of both fields
int v_hopf_nf_rhs(bk_ctx* ctx, size_t n, const double* u, const CglCoef& c, const double* zr, const double* zi, double s11,
                  double* r20r, double* r20i, double* r11) {
    return stream_write(ctx, "hopf_nf_rhs", n / 2, HopfNfRhs{{u, zr, zi}, {r20r, r20i, r11}, c, s11});
}

// out[4] = (Re a, Im a, Re b, Im b); S = u, zr, zi, sr, si, p, q, gr, gi
int v_hopf_nf_contract(bk_ctx* ctx, size_t n, const double* const (&S)[9], const CglCoef& c, double* out) {
    HopfNfContract pass{{}, c};
    for (int k = 0; k < 9; ++k) pass.in[k] = S[k];
    return stream_reduce(ctx, "hopf_nf_contract", n / 2, pass, out);
}

// m <= kOrbit phases t[0..m) into out[0..m)
int v_hopf_orbit(bk_ctx* ctx, size_t n, const double* x0, const double* zr, const double* zi, const double* p, const double* q,
                 const double* gr, const double* gi, double ds, double amp, int m, const double* t, double* const* out) {
    return count_dispatch<1, kOrbit>(m, [&](auto M) {
        HopfOrbit<decltype(M)::value> pass{{x0, zr, zi, p, q, gr, gi}, {}, ds};
        for (int k = 0; k < m; ++k) {
            const double a2 = amp * amp;
            pass.c1r[k] = 2.0 * (amp * std::cos(t[k]));
            pass.c1i[k] = -2.0 * (amp * std::sin(t[k]));
            pass.cq[k] = a2;
            pass.c2r[k] = 2.0 * (a2 * std::cos(2.0 * t[k]));
            pass.c2i[k] = -2.0 * (a2 * std::sin(2.0 * t[k]));
            pass.out[k] = out[k];
        }
        return stream_write(ctx, "hopf_orbit", n, pass);
    });
}

}  // namespace
}  // namespace bk

using namespace bk;

extern "C" {

int bk_hopf_d3f(bk_problem* prob, const double* u, const double* params, int nparams, const double* dx1, const double* dx2,
                const double* dx3, double* out) {
    if (!prob || !u || !params || !dx1 || !dx2 || !dx3 || !out) return -1;
    CglCoef c;
    BK_TRY(hopf_coef(prob, params, nparams, 0, &c));
    return v_hopf_d3(prob->ctx, prob->nloc, u, c, dx1, dx2, dx3, out);
}

int bk_hopf_nf_rhs(bk_problem* prob, const double* u, const double* params, int nparams, const double* z_re, const double* z_im,
                   double* r20_re, double* r20_im, double* r11) {
    if (!prob || !u || !params || !z_re || !z_im || !r20_re || !r20_im || !r11) return -1;
    CglCoef c;
    BK_TRY(hopf_coef(prob, params, nparams, 0, &c));
    const double* ins[3] = {u, z_re, z_im};
    double* outs[3] = {r20_re, r20_im, r11};
    for (int k = 0; k < 3; ++k) {
        for (const double* i : ins)
            if (outs[k] == i) return set_error(prob->ctx, "bk_hopf_nf_rhs: an output aliases an input");
        for (int j = 0; j < k; ++j)
            if (outs[k] == outs[j]) return set_error(prob->ctx, "bk_hopf_nf_rhs: r20_re, r20_im and r11 must be distinct");
    }
    return v_hopf_nf_rhs(prob->ctx, prob->nloc, u, c, z_re, z_im, 1.0, r20_re, r20_im, r11);
}

int bk_hopf_nf_contract(bk_problem* prob, const double* u, const double* params, int nparams, int ipar, const double* z_re,
                        const double* z_im, const double* zs_re, const double* zs_im, const double* psi001, const double* psi110,
                        const double* psi200_re, const double* psi200_im, double out[4]) {
    if (!prob || !u || !params || !z_re || !z_im || !zs_re || !zs_im || !psi001 || !psi110 || !psi200_re || !psi200_im || !out)
        return -1;
    CglCoef c;
    BK_TRY(hopf_coef(prob, params, nparams, ipar, &c));
    const double* const S[9] = {u, z_re, z_im, zs_re, zs_im, psi001, psi110, psi200_re, psi200_im};
    return v_hopf_nf_contract(prob->ctx, prob->nloc, S, c, out);
}

int bk_hopf_normal_form(bk_ctx* ctx, bk_problem* prob, const double* x, const double* params, int nparams, int ipar, double omega,
                        const double* z_re, const double* z_im, const double* zs_re, const double* zs_im,
                        const bk_gmres_opts* lsopts, bk_precond* pl, double* psi001, double* psi110, double* psi200_re,
                        double* psi200_im, double ab[4], int* converged, int itlinear[3]) {
    if (!ctx || !prob || !x || !params || !z_re || !z_im || !zs_re || !zs_im || !lsopts || !psi001 || !psi110 || !psi200_re ||
        !psi200_im || !ab)
        return -1;
    BK_TRY(minaug_check(ctx, prob, "hopf normal form"));
    CglCoef c;
    BK_TRY(hopf_coef(prob, params, nparams, ipar, &c));
    const double* ins[5] = {x, z_re, z_im, zs_re, zs_im};
    double* outs[4] = {psi001, psi110, psi200_re, psi200_im};
    for (int k = 0; k < 4; ++k) {
        for (const double* i : ins)
            if (outs[k] == i) return set_error(ctx, "bk_hopf_normal_form: the Psi vectors must not alias x, zeta or zeta*");
        for (int j = 0; j < k; ++j)
            if (outs[k] == outs[j]) return set_error(ctx, "bk_hopf_normal_form: the four Psi vectors must be distinct");
    }
    // <zeta, zeta*> = 1 (:1186-1189): Q = zeta*^H zeta of bk_hopf_contract is its conjugate
    double pq[4];
    BK_TRY(bk_hopf_contract(prob, x, params, nparams, ipar, z_re, z_im, zs_re, zs_im, 0, nullptr, pq));
    if (!(std::hypot(pq[2] - 1.0, pq[3]) <= 1e-8))
        return set_error(ctx, "bk_hopf_normal_form: Error of precision in normalization: <zeta, zeta*> = %.17g%+.17gi, expected 1",
                         pq[2], -pq[3]);
    const size_t n = prob->nloc;
    WsGuard ws(ctx);
    double *mdpF = nullptr, *r20r = nullptr, *r20i = nullptr, *mr11 = nullptr;
    BK_TRY(ws.get(n, &mdpF));
    BK_TRY(ws.get(n, &r20r));
    BK_TRY(ws.get(n, &r20i));
    BK_TRY(ws.get(n, &mr11));
    BK_TRY(pde_dparam(ctx, prob->desc.pde, ipar, n / 2, -1.0, x, mdpF));                              // -dpF, analytic
    BK_TRY(v_hopf_nf_rhs(ctx, n, x, c, z_re, z_im, -1.0, r20r, r20i, mr11));
    JPair jp;
    BK_TRY(jp.make(prob, x, params, nparams));
    GmresResult r0, r1;
    BK_TRY(linsolve2(ctx, jp.J, mdpF, psi001, mr11, psi110, 0.0, 1.0, *lsopts, pl, &r0, &r1));
    int cv2 = 0, it2 = 0;
    BK_TRY(bk_gmres_cshift(ctx, jp.J, r20r, r20i, psi200_re, psi200_im, 0.0, 2.0 * omega, -1.0, lsopts, pl, &cv2, &it2, nullptr));
    ctx->diag.hopf_nf_unconverged += (r0.converged ? 0.0 : 1.0) + (r1.converged ? 0.0 : 1.0) + (cv2 ? 0.0 : 1.0);
    const double* const S[9] = {x, z_re, z_im, zs_re, zs_im, psi001, psi110, psi200_re, psi200_im};
    BK_TRY(v_hopf_nf_contract(ctx, n, S, c, ab));
    if (converged) *converged = r0.converged & r1.converged & cv2;
    if (itlinear) { itlinear[0] = r0.niter; itlinear[1] = r1.niter; itlinear[2] = it2; }
    return 0;
}

int bk_hopf_orbit(bk_ctx* ctx, size_t n, const double* x0, const double* z_re, const double* z_im, const double* psi001,
                  const double* psi110, const double* psi200_re, const double* psi200_im, double ds, double amp, int M,
                  const double* t, double* const* out) {
    if (!ctx || !x0 || !z_re || !z_im || !psi001 || !psi110 || !psi200_re || !psi200_im || !t || !out) return -1;
    if (M < 1) return set_error(ctx, "bk_hopf_orbit: M >= 1 phases (got %d)", M);
    const double* ins[7] = {x0, z_re, z_im, psi001, psi110, psi200_re, psi200_im};
    for (int k = 0; k < M; ++k) {
        if (!out[k]) return -1;
        for (const double* i : ins)
            if (out[k] == i) return set_error(ctx, "bk_hopf_orbit: an output aliases an input");
        for (int j = 0; j < k; ++j)
            if (out[k] == out[j]) return set_error(ctx, "bk_hopf_orbit: the output vectors must be distinct");
    }
    if (n == 0) return 0;
    for (int k0 = 0; k0 < M; k0 += kOrbit) {
        const int m = M - k0 < kOrbit ? M - k0 : kOrbit;
        BK_TRY(v_hopf_orbit(ctx, n, x0, z_re, z_im, psi001, psi110, psi200_re, psi200_im, ds, amp, m, t + k0, out + k0));
    }
    return 0;
}

}  // extern "C"
