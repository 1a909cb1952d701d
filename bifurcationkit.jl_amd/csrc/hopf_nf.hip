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

__device__ __forceinline__ void st2(double* p, size_t i, double a, double b) { reinterpret_cast<double2*>(p)[i] = make_double2(a, b); }

// One pass over u and zeta = x + i y that writes the right-hand sides of the Psi200 and Psi110 solves:
//   r20 = d2F[zeta, zeta] / 2 = (x'Hx - y'Hy) / 2 + i x'Hy,     r11 = s11 d2F[zeta, conj zeta] = s11 (x'Hx + y'Hy)
// per field (s11 = -1 inside bk_hopf_normal_form, whose solve wants the negated vector).  3 read and 3 write streams.
template <int VEC, bool NTH>
__global__ void __launch_bounds__(kThreads) hopf_nf_rhs_kernel(size_t N, const double* __restrict__ u, const double* __restrict__ zr,
                                                               const double* __restrict__ zi, CglCoef c, double s11,
                                                               double* __restrict__ r20r, double* __restrict__ r20i,
                                                               double* __restrict__ r11) {
    // o = (r20r_1, r20r_2, r20i_1, r20i_2, r11_1, r11_2) of one grid point
    auto elem = [&](double u1, double u2, double x1, double x2, double y1, double y2, double o[6]) {
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
    };
    if (VEC == 2) {
        // N even and every stream 16-B aligned in both fields (the launcher checks)
        stream_loop<1>(N >> 1, [&](auto, size_t i, size_t) {
            const double2 u1 = ld2<NTH>(u, i), u2 = ld2<NTH>(u + N, i);
            const double2 x1 = ld2<NTH>(zr, i), x2 = ld2<NTH>(zr + N, i);
            const double2 y1 = ld2<NTH>(zi, i), y2 = ld2<NTH>(zi + N, i);
            double a[6], b[6];
            elem(u1.x, u2.x, x1.x, x2.x, y1.x, y2.x, a);
            elem(u1.y, u2.y, x1.y, x2.y, y1.y, y2.y, b);
            st2(r20r, i, a[0], b[0]); st2(r20r + N, i, a[1], b[1]);
            st2(r20i, i, a[2], b[2]); st2(r20i + N, i, a[3], b[3]);
            st2(r11, i, a[4], b[4]); st2(r11 + N, i, a[5], b[5]);
        });
    } else {
        for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < N; i += (size_t)gridDim.x * kThreads) {
            double a[6];
            elem(u[i], u[i + N], zr[i], zr[i + N], zi[i], zi[i + N], a);
            r20r[i] = a[0]; r20r[i + N] = a[1];
            r20i[i] = a[2]; r20i[i + N] = a[3];
            r11[i] = a[4]; r11[i + N] = a[5];
        }
    }
}

// field-1 base pointers of the streams of hopf_nf_contract_kernel; field 2 of each starts N doubles later
struct NfStreams { const double *u, *zr, *zi, *sr, *si, *p, *q, *gr, *gi; };

// One pass over u, zeta = x + i y (zr, zi), zeta* (sr, si), Psi001 = p, Psi110 = q, Psi200 = gr + i gi: four partial sums per
// workgroup, (Re a, Im a, Re b, Im b).  Every term is zeta or conj zeta against a per-point vector of field f,
//   av_f = zeta . e_f,                          e_f = D_p[f, :] + H_f p
//   bv_f = zeta . r_f + conj(zeta) . G_f,       r_f = H_f q + s_f / 2,   G_f = H_f (gr + i gi)
// with s_f = T_f : (x x' + y y'), because d3F[zeta, zeta, conj zeta] = zeta . s_f  (H_f conj(zeta) = conj(H_f zeta)), and
//   a += conj(av_f) zeta*_f,   b += conj(bv_f) zeta*_f.
// The second stage (reduce_finish) keeps the fixed order: the sums are bitwise the same run to run and, all-reduced, on every rank.
template <int VEC, bool NTH>
__global__ void __launch_bounds__(kThreads) hopf_nf_contract_kernel(size_t N, NfStreams S, CglCoef c, double* __restrict__ partials) {
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    // one grid point; the second index of every argument is the field
    auto elem = [&](double u1, double u2, double x1, double x2, double y1, double y2, double sr1, double sr2, double si1,
                    double si2, double p1, double p2, double q1, double q2, double gr1, double gr2, double gi1, double gi2) {
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
    };
    if (VEC == 2) {
        // N even and every stream 16-B aligned in both fields (the launcher checks): N / 2 items, no ragged element
        stream_loop<1>(N >> 1, [&](auto, size_t i, size_t) {
            const double2 u1 = ld2<NTH>(S.u, i), u2 = ld2<NTH>(S.u + N, i);
            const double2 x1 = ld2<NTH>(S.zr, i), x2 = ld2<NTH>(S.zr + N, i);
            const double2 y1 = ld2<NTH>(S.zi, i), y2 = ld2<NTH>(S.zi + N, i);
            const double2 a1 = ld2<NTH>(S.sr, i), a2 = ld2<NTH>(S.sr + N, i);
            const double2 b1 = ld2<NTH>(S.si, i), b2 = ld2<NTH>(S.si + N, i);
            const double2 p1 = ld2<NTH>(S.p, i), p2 = ld2<NTH>(S.p + N, i);
            const double2 q1 = ld2<NTH>(S.q, i), q2 = ld2<NTH>(S.q + N, i);
            const double2 g1 = ld2<NTH>(S.gr, i), g2 = ld2<NTH>(S.gr + N, i);
            const double2 k1 = ld2<NTH>(S.gi, i), k2 = ld2<NTH>(S.gi + N, i);
            elem(u1.x, u2.x, x1.x, x2.x, y1.x, y2.x, a1.x, a2.x, b1.x, b2.x, p1.x, p2.x, q1.x, q2.x, g1.x, g2.x, k1.x, k2.x);
            elem(u1.y, u2.y, x1.y, x2.y, y1.y, y2.y, a1.y, a2.y, b1.y, b2.y, p1.y, p2.y, q1.y, q2.y, g1.y, g2.y, k1.y, k2.y);
        });
    } else {
        for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < N; i += (size_t)gridDim.x * kThreads)
            elem(S.u[i], S.u[i + N], S.zr[i], S.zr[i + N], S.zi[i], S.zi[i + N], S.sr[i], S.sr[i + N], S.si[i], S.si[i + N],
                 S.p[i], S.p[i + N], S.q[i], S.q[i + N], S.gr[i], S.gr[i + N], S.gi[i], S.gi[i + N]);
    }
    block_sum_store<4>(s, partials);
}

// M <= kOrbit phases of the predictor's orbit per launch: the coefficients of A_m = amp e^{i t_m} as the kernel applies them
constexpr int kOrbit = 8;
struct OrbitArgs {
    double c1r[kOrbit], c1i[kOrbit];     // 2 Re A_m, -2 Im A_m          (2 Re(zeta A) = 2 Re A zr - 2 Im A zi)
    double cq[kOrbit];                   // |A_m|^2
    double c2r[kOrbit], c2i[kOrbit];     // 2 Re A_m^2, -2 Im A_m^2
    double* out[kOrbit];
};

// out_m = x0 + ds Psi001 + 2 Re(zeta A_m) + |A_m|^2 Psi110 + 2 Re(A_m^2 Psi200)  (src/NormalForms.jl:1262-1271) for m < M in one
// pass: the seven inputs are read once, n elements each (the vectors are walked flat, both fields alike)
template <int M, int VEC, bool NTH>
__global__ void __launch_bounds__(kThreads) hopf_orbit_kernel(size_t n, const double* __restrict__ x0, const double* __restrict__ zr,
                                                              const double* __restrict__ zi, const double* __restrict__ p,
                                                              const double* __restrict__ q, const double* __restrict__ gr,
                                                              const double* __restrict__ gi, double ds, OrbitArgs A) {
    auto elem = [&](int m, double x, double a, double b, double pp, double qq, double g, double k) {
        return ((((x + ds * pp) + A.c1r[m] * a) + A.c1i[m] * b) + A.cq[m] * qq) + (A.c2r[m] * g + A.c2i[m] * k);
    };
    if (VEC == 2) {
        stream_loop<1>(n >> 1, [&](auto, size_t i, size_t) {
            const double2 x = ld2<NTH>(x0, i), a = ld2<NTH>(zr, i), b = ld2<NTH>(zi, i), pp = ld2<NTH>(p, i), qq = ld2<NTH>(q, i),
                          g = ld2<NTH>(gr, i), k = ld2<NTH>(gi, i);
#pragma unroll
            for (int m = 0; m < M; ++m)
                st2(A.out[m], i, elem(m, x.x, a.x, b.x, pp.x, qq.x, g.x, k.x), elem(m, x.y, a.y, b.y, pp.y, qq.y, g.y, k.y));
        });
    } else {
        for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kThreads) {
            const double x = x0[i], a = zr[i], b = zi[i], pp = p[i], qq = q[i], g = gr[i], k = gi[i];
#pragma unroll
            for (int m = 0; m < M; ++m) A.out[m][i] = elem(m, x, a, b, pp, qq, g, k);
        }
    }
}

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
    const size_t N = n / 2;
    if (N == 0) return 0;
    auto al = [N](const double* p) { return aligned16(p) && aligned16(p + N); };
    const bool vec = (N % 2 == 0) && al(u) && al(zr) && al(zi) && al(r20r) && al(r20i) && al(r11);
    const bool nth = vec && nt_hint(ctx, n);
    const int grid = grid_for(N, vec ? 2 : 1, 4096);
    ProfScope ps(ctx, "hopf_nf_rhs", 8.0 * n * 6);
    load_path_dispatch(vec, nth, [&](auto V, auto NT) {
        hipLaunchKernelGGL((hopf_nf_rhs_kernel<decltype(V)::value, decltype(NT)::value>), dim3(grid), dim3(kThreads), 0,
                           ctx->stream, N, u, zr, zi, c, s11, r20r, r20i, r11);
    });
    BK_HIP(ctx, hipGetLastError());
    return 0;
}

// out[4] = (Re a, Im a, Re b, Im b)
int v_hopf_nf_contract(bk_ctx* ctx, size_t n, const NfStreams& S, const CglCoef& c, double* out) {
    const size_t N = n / 2;
    auto al = [N](const double* p) { return aligned16(p) && aligned16(p + N); };
    const bool vec = (N % 2 == 0) && al(S.u) && al(S.zr) && al(S.zi) && al(S.sr) && al(S.si) && al(S.p) && al(S.q) && al(S.gr) &&
                     al(S.gi);
    const bool nth = vec && nt_hint(ctx, n);
    const int grid = grid_for(N, vec ? 2 : 1, kRedBlocks);
    {
        ProfScope ps(ctx, "hopf_nf_contract", 8.0 * n * 9);
        load_path_dispatch(vec, nth, [&](auto V, auto NT) {
            hipLaunchKernelGGL((hopf_nf_contract_kernel<decltype(V)::value, decltype(NT)::value>), dim3(grid), dim3(kThreads), 0,
                               ctx->stream, N, S, c, ctx->d_partials);
        });
        BK_HIP(ctx, hipGetLastError());
    }
    BK_TRY(reduce_finish(ctx, grid, 4, 0));
    for (int k = 0; k < 4; ++k) out[k] = ctx->h_red[k];
    return 0;
}

// m <= kOrbit phases t[0..m) into A.out[0..m)
int v_hopf_orbit(bk_ctx* ctx, size_t n, const double* x0, const double* zr, const double* zi, const double* p, const double* q,
                 const double* gr, const double* gi, double ds, double amp, int m, const double* t, double* const* out) {
    OrbitArgs A{};
    bool vec = (n % 2 == 0) && aligned16(x0) && aligned16(zr) && aligned16(zi) && aligned16(p) && aligned16(q) && aligned16(gr) &&
               aligned16(gi);
    for (int k = 0; k < m; ++k) {
        const double a2 = amp * amp;
        A.c1r[k] = 2.0 * (amp * std::cos(t[k]));
        A.c1i[k] = -2.0 * (amp * std::sin(t[k]));
        A.cq[k] = a2;
        A.c2r[k] = 2.0 * (a2 * std::cos(2.0 * t[k]));
        A.c2i[k] = -2.0 * (a2 * std::sin(2.0 * t[k]));
        A.out[k] = out[k];
        vec = vec && aligned16(out[k]);
    }
    const bool nth = vec && nt_hint(ctx, n);
    const int grid = grid_for(n, vec ? 2 : 1, 4096);
    ProfScope ps(ctx, "hopf_orbit", 8.0 * n * (7 + m));
    auto variant = [&](auto M) {
        load_path_dispatch(vec, nth, [&](auto V, auto NT) {
            hipLaunchKernelGGL((hopf_orbit_kernel<decltype(M)::value, decltype(V)::value, decltype(NT)::value>), dim3(grid),
                               dim3(kThreads), 0, ctx->stream, n, x0, zr, zi, p, q, gr, gi, ds, A);
        });
    };
    switch (m) {
        case 1: variant(std::integral_constant<int, 1>{}); break;
        case 2: variant(std::integral_constant<int, 2>{}); break;
        case 3: variant(std::integral_constant<int, 3>{}); break;
        case 4: variant(std::integral_constant<int, 4>{}); break;
        case 5: variant(std::integral_constant<int, 5>{}); break;
        case 6: variant(std::integral_constant<int, 6>{}); break;
        case 7: variant(std::integral_constant<int, 7>{}); break;
        default: variant(std::integral_constant<int, 8>{}); break;
    }
    BK_HIP(ctx, hipGetLastError());
    return 0;
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
    const NfStreams S{u, z_re, z_im, zs_re, zs_im, psi001, psi110, psi200_re, psi200_im};
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
    const NfStreams S{x, z_re, z_im, zs_re, zs_im, psi001, psi110, psi200_re, psi200_im};
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
