// Periodic orbits by the trapezoid rule, matrix-free, for BK_PDE_CGL2D on one rank: the functional Trapeze of
// src/periodicorbit/PeriodicOrbitTrapeze.jl (po_residual! :249-269, po_residual_bare! :272-287, po_jvp! :294-330, Jc :362-386,
// updatesection! :665-681) as it is used in the second half of examples/cGL2d.jl (:166-260), its adjoint dG(u, T)^T (the left
// null vector of src/codim2/MinAugFold.jl), and a space-time spectral preconditioner, forward, transposed and for the monodromy's
// initial-value system, in the place of the example's ILU of the assembled Jacobian (:209-213).
//
// Orbit vector (:139-142): M slices of N = 2 n doubles on the device, slice i = [u1; u2] at u + i N, and ONE host tail scalar T.
// With K = M - 1, prev(0) = K - 1, prev(i) = i - 1, next(j) = j + 1, next(K - 1) = 0 and F the cGL vector field:
//
//     G_i = u_i - u_prev(i) - (h / 2) (F(u_i) + F(u_prev(i))),   i < K          h = T (1 / M)
//     G_K = u_K - u_0                                            the closure
//     G_T = <u, phi> - <xpi, phi>                                the phase condition over all M slices
//
//     dG_i = du_i - du_prev(i) - (h / 2) (J_i du_i + J_prev(i) du_prev(i)) - (dT / M / 2) (F(u_i) + F(u_prev(i)))
//     dG_K = du_K - du_0,     dG_T = <du, phi>
//
// The adjoint on (w, tau), with hh = h / 2, s_j = w_j + w_next(j) and q_j = J_j^T s_j (ONE adjoint stencil evaluation per slice:
// the Laplacian is linear and symmetric, so the two slices' Laplacians add):
//
//     out_j = (w_j - w_next(j)) - hh q_j - [j = 0] w_K + tau phi_j        j < K
//     out_K = w_K + tau phi_K
//     tail  = -(1 / (2 M)) sum_{j < K} <F(u_j), s_j>
//
// THE TIME STEP: h = T / M on each of the M - 1 intervals -- get_time_step of an integer TimeMesh is 1 / M (src/TimeMesh.jl:21)
// while the cyclic system has M - 1 intervals.  The quirk is kept: the entry called T is M / (M - 1) times the orbit's period,
// and every guess and result of the reference is in this convention.
//
// Kernels.  The three marching passes (PoMarch<JVP>, PoAdjMarch) run on the skeleton of potrap_pw.h: every slice's stencil is
// evaluated once, the forward ones carry F(u_prev) (JVP: J_prev du_prev too) and the centre values of the previous slice, the adjoint
// one the loaded slice of w, and the phase dot (the tail dot) is formed in the same pass.  Nothing but the result is written.
// The pointwise terms are those of cgl_pw.h, the one copy the stencil kernel uses.  po_timesolve_kernel is the middle of the
// preconditioner: per sine mode the bidiagonal system in time, solved exactly by one recurrence (below, PoPrecond).
#include <cmath>
#include <complex>
#include <vector>

#include "cgl_pw.h"
#include "common.h"
#include "hopf_pw.h"
#include "ops.h"
#include "potrap_pw.h"
#include "stream.h"

namespace bk {

namespace {

// Residual and JVP.  Step `row` evaluates slice row (t = -1: the predecessor of the chunk's first row, prev(0) = K - 1) and
// completes the row from it and the carried F, J du and centre values of the slice before.  s[0]: the phase dot <x, phi>, x = u or du.
template <bool JVP>
struct PoMarch {
    static constexpr int NV = 1;
    static constexpr bool OPEN = false;
    CglPar par;
    double hh;                     // h / 2 = T / M / 2
    double dh;                     // JVP: dT / M / 2
    const double* u;
    const double* du;              // JVP only
    const double* phi;
    double* out;
    struct Carry { double F1, F2, J1, J2, c1, c2; };
    __device__ __forceinline__ void step(const PoAt& a, int row, bool store, Carry& c, double* s) const {
        const size_t n = a.n, idx = a.idx, sl = (size_t)(row < 0 ? a.g.K - 1 : row) * a.N;
        const PoPoint q = po_load(a, u + sl);
        double n1, n2;
        cgl_nl(par, q.c1, q.c2, n1, n2);
        const double F1 = q.d1 + n1, F2 = q.d2 + n2;
        double J1 = 0.0, J2 = 0.0, x1 = q.c1, x2 = q.c2;
        if (JVP) {
            const PoPoint v = po_load(a, du + sl);
            double f1u, f1v, f2u, f2v;
            cgl_jac(par, q.c1, q.c2, f1u, f1v, f2u, f2v);
            J1 = v.d1 + f1u * v.c1 + f1v * v.c2;
            J2 = v.d2 + f2u * v.c1 + f2v * v.c2;
            x1 = v.c1;
            x2 = v.c2;
        }
        if (store) {
            double o1, o2;
            if (JVP) {
                o1 = ((x1 - c.c1) - hh * (J1 + c.J1)) - dh * (F1 + c.F1);
                o2 = ((x2 - c.c2) - hh * (J2 + c.J2)) - dh * (F2 + c.F2);
            } else {
                o1 = (x1 - c.c1) - hh * (F1 + c.F1);
                o2 = (x2 - c.c2) - hh * (F2 + c.F2);
            }
            out[sl + idx] = o1;
            out[sl + idx + n] = o2;
            s[0] = fma(phi[sl + idx], x1, s[0]);
            s[0] = fma(phi[sl + idx + n], x2, s[0]);
        }
        c = Carry{F1, F2, J1, J2, x1, x2};
    }
    // the closure row and the last slice's share of the phase dot
    __device__ __forceinline__ void closure(const PoAt& a, double* s) const {
        const double* x = JVP ? du : u;
        const size_t n = a.n, idx = a.idx, sl = (size_t)a.g.K * a.N;
        const double a1 = x[sl + idx], a2 = x[sl + idx + n];
        out[sl + idx] = a1 - x[idx];
        out[sl + idx + n] = a2 - x[idx + n];
        s[0] = fma(phi[sl + idx], a1, s[0]);
        s[0] = fma(phi[sl + idx + n], a2, s[0]);
    }
};

// The adjoint.  Step `row` loads slice next(row) of w and completes row `row` from it and the carried slice; t = -1 only loads the
// chunk's first slice.  s[0] = sum_j <F(u_j), s_j>.  Streams: u, w, phi read, out written.
struct PoAdjMarch {
    static constexpr int NV = 1;
    static constexpr bool OPEN = false;
    CglPar par;
    double hh;                     // h / 2 = T / M / 2
    double tau;
    const double* u;
    const double* w;
    const double* phi;
    double* out;
    using Carry = PoPoint;
    __device__ __forceinline__ void step(const PoAt& a, int row, bool store, PoPoint& wc, double* s) const {
        const size_t n = a.n, idx = a.idx;
        const size_t sn = (size_t)(row + 1 == a.g.K ? 0 : row + 1) * a.N;
        const PoPoint wn = po_load(a, w + sn);
        if (store) {
            const size_t sl = (size_t)row * a.N, slK = (size_t)a.g.K * a.N;
            const PoPoint q = po_load(a, u + sl);
            double n1, n2, f1u, f1v, f2u, f2v;
            cgl_nl(par, q.c1, q.c2, n1, n2);
            cgl_jac(par, q.c1, q.c2, f1u, f1v, f2u, f2v);
            const double F1 = q.d1 + n1, F2 = q.d2 + n2;
            const double s1 = wc.c1 + wn.c1, s2 = wc.c2 + wn.c2;
            const double q1 = (wc.d1 + wn.d1) + f1u * s1 + f2u * s2;
            const double q2 = (wc.d2 + wn.d2) + f1v * s1 + f2v * s2;
            double o1 = (wc.c1 - wn.c1) - hh * q1;
            double o2 = (wc.c2 - wn.c2) - hh * q2;
            if (row == 0) {
                o1 -= w[slK + idx];
                o2 -= w[slK + idx + n];
            }
            out[sl + idx] = o1 + tau * phi[sl + idx];
            out[sl + idx + n] = o2 + tau * phi[sl + idx + n];
            s[0] = fma(F1, s1, s[0]);
            s[0] = fma(F2, s2, s[0]);
        }
        wc = wn;
    }
    __device__ __forceinline__ void closure(const PoAt& a, double*) const {
        const size_t n = a.n, idx = a.idx, slK = (size_t)a.g.K * a.N;
        out[slK + idx] = w[slK + idx] + tau * phi[slK + idx];
        out[slK + idx + n] = w[slK + idx + n] + tau * phi[slK + idx + n];
    }
};

// out_i = -(h / 2) (dpF(u_i) + dpF(u_prev(i))) from tmp_i = -(h / 2) dpF(u_i), i < K; the closure row is zero
__global__ void __launch_bounds__(kThreads) potrap_dparam_combine_kernel(size_t N, int M, const double* __restrict__ tmp,
                                                                          double* __restrict__ out) {
    const size_t total = N * (size_t)M;
    const int K = M - 1;
    for (size_t g = (size_t)blockIdx.x * kThreads + threadIdx.x; g < total; g += (size_t)gridDim.x * kThreads) {
        const size_t row = g / N, e = g % N;
        out[g] = (int)row == K ? 0.0 : tmp[g] + tmp[(row == 0 ? (size_t)K - 1 : row - 1) * N + e];
    }
}

// The time solve of the preconditioners, one thread per sine mode k and w = u1^ + i u2^, in place, coalesced across modes.  With
// mu = a + lam_k + i b, alpha = 1 - hh mu, beta = 1 + hh mu, rho = beta / alpha (po_mode; the transposed system has conj(mu): the
// DST-I is symmetric and L0^T acts on w^ as the multiplication by conj(mu_k), so it enters with mi = -b) the K rows read
//   kTsCyclic         alpha w_i - beta w_prev(i) = f_i, i.e. w_i = rho w_prev(i) + f_i / alpha, cyclic in i.  First walk: acc <- rho
//                     acc + f_i / alpha over the K slices, rho^K accumulated alongside; w_{K-1} = acc / (1 - rho^K).  Second walk:
//                     the recurrence itself, written out.  Closure: w_K = f_K + w_0.  Two reads and one write of the spectrum.
//   kTsCyclicAdjoint  w_K = f_K, f_0 <- f_0 + f_K and the recurrence backwards in time, w_j = rho w_next(j) + g_j / alpha with
//                     g_0 = f_0 + f_K, g_j = f_j.  First walk, j = K - 1 .. 0, as above; w_0 = acc / (1 - rho^K).  Second walk: the
//                     recurrence from w_next(K - 1) = w_0 (row 0, the last one written, is read before that).  Row K stays.
//   kTsIvp            alpha w_i - beta w_{i-1} = f_i from w_{-1} = 0: one read and one write; no closure row and no division by
//                     1 - rho^K, so the only guard left is |alpha|.
struct PoTs {
    int nx, ny, K;
    double a, b, hh;
    const double* lx;
    const double* ly;
    double* spec;
};
struct PoMode { Cx inva, rho; };
__device__ __forceinline__ PoMode po_mode(const PoTs& P, size_t k, double mi) {
    const double mr = P.a + (P.lx[k % P.nx] + P.ly[k / P.nx]);
    const Cx alpha{1.0 - P.hh * mr, -P.hh * mi}, beta{1.0 + P.hh * mr, P.hh * mi};
    const double ia = 1.0 / (alpha.r * alpha.r + alpha.i * alpha.i);
    const Cx inva{alpha.r * ia, -alpha.i * ia};
    return PoMode{inva, beta * inva};
}
template <int KIND>
__global__ void __launch_bounds__(kThreads) po_timesolve_kernel(PoTs P) {
    const size_t n = (size_t)P.nx * P.ny, N = 2 * n;
    const size_t k = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (k >= n) return;
    const int K = P.K;
    const PoMode m = po_mode(P, k, KIND == kTsCyclicAdjoint ? -P.b : P.b);
    const Cx inva = m.inva, rho = m.rho;
    auto f = [&](int i) { return Cx{P.spec[(size_t)i * N + k], P.spec[(size_t)i * N + n + k]}; };
    auto put = [&](int i, Cx w) {
        P.spec[(size_t)i * N + k] = w.r;
        P.spec[(size_t)i * N + n + k] = w.i;
    };
    if constexpr (KIND == kTsIvp) {
        Cx w{0.0, 0.0};
        for (int i = 0; i < K; ++i) {
            w = rho * w + f(i) * inva;
            put(i, w);
        }
    } else if constexpr (KIND == kTsCyclic) {
        Cx acc{0.0, 0.0}, rk{1.0, 0.0};
        for (int i = 0; i < K; ++i) {
            acc = rho * acc + f(i) * inva;
            rk = rk * rho;
        }
        const Cx den{1.0 - rk.r, -rk.i};
        const double id = 1.0 / (den.r * den.r + den.i * den.i);
        Cx w = acc * Cx{den.r * id, -den.i * id};
        Cx w0{0.0, 0.0};
        for (int i = 0; i < K; ++i) {
            w = rho * w + f(i) * inva;
            put(i, w);
            if (i == 0) w0 = w;
        }
        P.spec[(size_t)K * N + k] += w0.r;
        P.spec[(size_t)K * N + n + k] += w0.i;
    } else {
        const Cx fK = f(K);
        auto g = [&](int j) {
            Cx v = f(j);
            if (j == 0) v = v + fK;
            return v;
        };
        Cx acc{0.0, 0.0}, rk{1.0, 0.0};
        for (int j = K - 1; j >= 0; --j) {
            acc = rho * acc + g(j) * inva;
            rk = rk * rho;
        }
        const Cx den{1.0 - rk.r, -rk.i};
        const double id = 1.0 / (den.r * den.r + den.i * den.i);
        Cx w = acc * Cx{den.r * id, -den.i * id};
        for (int j = K - 1; j >= 0; --j) {
            w = rho * w + g(j) * inva;
            put(j, w);
        }
    }
}

}  // namespace

// The chunk length of the marching kernels.  The spatial tiles alone are 4 workgroups at the example's 41 x 21 grid, so the K
// rows are cut into chunks until about two workgroups per compute unit are in flight: nchunks = ceil(2 CUs / tiles) clamped to
// [1, K], C = ceil(K / nchunks).  Context option "potrap_chunks" > 0 forces the chunk count (clamped the same way).
int potrap_chunking(bk_ctx* ctx, size_t n, int M, unsigned* ntiles, int* C, int* nchunks) {
    const int K = M - 1;
    const size_t tiles = (n + kThreads - 1) / kThreads;
    long want = (long)ctx->opt("potrap_chunks", 0.0);
    if (want <= 0) want = (long)((2 * (size_t)ctx->num_cu + tiles - 1) / tiles);
    if (want < 1) want = 1;
    if (want > K) want = K;
    *C = (K + (int)want - 1) / (int)want;
    *nchunks = (K + *C - 1) / *C;
    if (tiles * (size_t)*nchunks > kPartialDoubles)
        return set_error(ctx, "potrap: %zu tiles x %d chunks exceed the reduction scratch", tiles, *nchunks);
    *ntiles = (unsigned)tiles;
    return 0;
}

int potrap_params(bk_potrap* h, const double* params, int nparams, CglPar* par) {
    CglCoef c;
    BK_TRY(hopf_coef(h->prob, params, nparams, 0, &c));       // the problem kind and parameter count, as the Hopf entries check them
    *par = CglPar{params[0], params[1], params[2], params[3], params[4], params[5]};
    return 0;
}

int potrap_check(bk_potrap* h, const char* who) {
    if (!h->has_section)
        return set_error(h->ctx, "%s: no section set (bk_potrap_set_section or bk_potrap_update_section first)", who);
    return 0;
}

int potrap_opts_check(bk_ctx* ctx, const char* who, const bk_gmres_opts* opts, const char* what) {
    if (opts->flavor >= BK_KRYLOV_MINRES) return set_error(ctx, "%s: %s is not symmetric (use a GMRES flavor)", who, what);
    if (opts->pr) return set_error(ctx, "%s: left preconditioner only", who);
    return 0;
}

namespace {

// out and the phase dot <x, phi> (x = u, or du for the JVP); algorithmic bytes: u (and du) read, out written, phi read
int potrap_march(bk_potrap* h, const CglPar& par, const double* u, double T, const double* du, double dT, double* out, double* dot) {
    const double hh = T * (1.0 / h->M) / 2.0, dh = dT / h->M / 2.0;
    if (du) return po_march(h, "potrap", "potrap_jvp", 8.0 * h->len() * 4, PoMarch<true>{par, hh, dh, u, du, h->phi, out}, dot);
    return po_march(h, "potrap", "potrap_residual", 8.0 * h->len() * 3, PoMarch<false>{par, hh, dh, u, du, h->phi, out}, dot);
}

// out = the first M N entries of dG^T (w, tau), *tail the last; algorithmic bytes: u, w, phi read, out written
int potrap_adjoint_march(bk_potrap* h, const CglPar& par, const double* u, double T, const double* w, double tau, double* out,
                         double* tail) {
    double s = 0.0;
    BK_TRY(po_march(h, "potrap", "potrap_jvp_adjoint", 8.0 * h->len() * 4,
                    PoAdjMarch{par, T * (1.0 / h->M) / 2.0, tau, u, w, h->phi, out}, &s));
    *tail = -(s / h->M / 2.0);
    return 0;
}

// dG(u, T), or its transpose, as an operator on (device vector of M N doubles, host tail dT); references u
struct PoTrapOp : bk_op {
    bk_potrap* h = nullptr;
    const double* u = nullptr;
    double T = 0.0;
    CglPar par{};
    bool adjoint = false;
    int apply(const double* x, const double* xt, double a0, double a1, double* out, double* outt) override {
        if (out == x) return set_error(ctx, "potrap operator: out must not alias x");
        double dot = 0.0;
        if (adjoint) BK_TRY(potrap_adjoint_march(h, par, u, T, x, xt[0], out, &dot));
        else BK_TRY(potrap_march(h, par, u, T, x, xt[0], out, &dot));
        if (!(a0 == 0.0 && a1 == 1.0)) BK_TRY(v_axpby(ctx, n, a0, x, a1, out));
        outt[0] = a0 * xt[0] + a1 * dot;
        return 0;
    }
};

}  // namespace

// P = diag(A0, 1): A0 = the cyclic-plus-closure matrix above with every J_i replaced by L0 = Lap (x) I_2 + [[a, -b], [b, a]], the
// operator bk_precond_cgl_create inverts; kTsCyclicAdjoint: diag(A0^T, 1); kTsIvp: the rows i < K with the cyclic link of row 0
// cut (floquet.hip).  Only the time solve differs between the three.
int PoPrecond::apply(const double* v, double* out) {
    if (!period_set) return set_error(ctx, "potrap preconditioner: no period set (bk_precond_potrap_set_period first)");
    double* spec = dst_plan_scratch(plan);
    BK_TRY(dst_transform(ctx, plan, 0, v, spec));
    {
        static const char* const scope[3] = {"potrap_timesolve", "potrap_adjoint_timesolve", "monodromy_timesolve"};
        ProfScope ps(ctx, scope[kind], 8.0 * n * (kind == kTsIvp ? 2 : 3));
        const PoTs P{nx, ny, M - 1, a, b, hh, dst_plan_lam(plan, 0), dst_plan_lam(plan, 1), spec};
        const dim3 grid((unsigned)(((size_t)nx * ny + kThreads - 1) / kThreads));
        if (kind == kTsCyclic) hipLaunchKernelGGL(po_timesolve_kernel<kTsCyclic>, grid, dim3(kThreads), 0, ctx->stream, P);
        else if (kind == kTsCyclicAdjoint) hipLaunchKernelGGL(po_timesolve_kernel<kTsCyclicAdjoint>, grid, dim3(kThreads), 0, ctx->stream, P);
        else hipLaunchKernelGGL(po_timesolve_kernel<kTsIvp>, grid, dim3(kThreads), 0, ctx->stream, P);
        BK_HIP(ctx, hipGetLastError());
    }
    return dst_transform(ctx, plan, 1, spec, out);
}

// T: the initial-value kind only, whose period is fixed here
int po_precond_create(bk_potrap* h, PoTsKind kind, double a, double b, double T, const char* who, PoPrecond** out) {
    bk_ctx* ctx = h->ctx;
    PoPrecond* P = new PoPrecond();
    P->fields = 2 * (kind == kTsIvp ? h->M - 1 : h->M);
    P->ctx = ctx; P->n = h->n * (size_t)P->fields; P->kind = kind;
    P->nx = h->prob->desc.n[0]; P->ny = h->prob->desc.n[1]; P->M = h->M; P->a = a; P->b = b;
    int s = dst_plan_create(ctx, h->prob->desc.n, h->prob->ainv, 0.0, P->fields, &P->plan);
    if (s != 0) { delete P; return s; }
    P->lx.resize(P->nx);
    P->ly.resize(P->ny);
    if (hipMemcpy(P->lx.data(), dst_plan_lam(P->plan, 0), sizeof(double) * P->nx, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(P->ly.data(), dst_plan_lam(P->plan, 1), sizeof(double) * P->ny, hipMemcpyDeviceToHost) != hipSuccess) {
        delete P;
        return set_error(ctx, "%s: reading the eigenvalue tables failed", who);
    }
    if (kind == kTsIvp && (s = po_precond_set_period(P, T, who)) != 0) { delete P; return s; }
    *out = P;
    return 0;
}

// The guards of a period: min |alpha| over the sine modes and, for the cyclic kinds, min |1 - rho^K| (equal for A0 and A0^T: the
// moduli do not see the conjugation), each with its mode
int po_precond_set_period(PoPrecond* P, double T, const char* who) {
    const double hh = T * (1.0 / P->M) / 2.0;
    const int K = P->M - 1;
    double min_a = INFINITY, min_d = INFINITY;
    int ka[2] = {0, 0}, kd[2] = {0, 0};
    for (int j = 0; j < P->ny; ++j)
        for (int i = 0; i < P->nx; ++i) {
            const std::complex<double> mu(P->a + (P->lx[i] + P->ly[j]), P->b);
            const std::complex<double> alpha = 1.0 - hh * mu, beta = 1.0 + hh * mu;
            const double aa = std::abs(alpha);
            if (!(aa >= min_a)) { min_a = aa; ka[0] = i; ka[1] = j; }
            if (P->kind == kTsIvp || !(aa >= kPoPivot)) continue;
            const std::complex<double> rho = beta / alpha;
            std::complex<double> rk(1.0, 0.0);
            for (int q = 0; q < K; ++q) rk *= rho;
            const double dd = std::abs(1.0 - rk);
            if (!(dd >= min_d)) { min_d = dd; kd[0] = i; kd[1] = j; }
        }
    if (!(min_a >= kPoPivot))
        return set_error(P->ctx, "%s: |alpha| = |1 - (h/2) mu| = %.3g below %.0e at sine mode (%d, %d): move a (or T) away from it", who,
                         min_a, kPoPivot, ka[0] + 1, ka[1] + 1);
    if (P->kind != kTsIvp && !(min_d >= kPoPivot))
        return set_error(P->ctx, "%s: |1 - rho^K| = %.3g below %.0e at sine mode (%d, %d): the mode is Hopf-critical for (a, b) = "
                                 "(%.17g, %.17g) at this period; move a away from it",
                         who, min_d, kPoPivot, kd[0] + 1, kd[1] + 1, P->a, P->b);
    P->hh = hh;
    P->period_set = true;
    return 0;
}

PoPrecond* po_precond_cast(bk_precond* pl, bool ivp) {
    PoPrecond* P = dynamic_cast<PoPrecond*>(pl);
    return P && (P->kind == kTsIvp) == ivp ? P : nullptr;
}

int potrap_pair_check(bk_ctx* ctx, const char* who, bk_op* op, bk_precond* pl) {
    PoTrapOp* pop = dynamic_cast<PoTrapOp*>(op);
    if (!pop) return set_error(ctx, "%s: op is not an operator of bk_potrap_op_create", who);
    PoPrecond* ppl = po_precond_cast(pl, false);
    if (!ppl || pl->n != op->n) return set_error(ctx, "%s: pl is not a preconditioner of bk_precond_potrap_create for this orbit", who);
    const bool padj = ppl->kind == kTsCyclicAdjoint;
    if (pop->adjoint != padj)
        return set_error(ctx, "%s: %s operator with %s preconditioner (pair bk_potrap_op_adjoint_create with "
                              "bk_precond_potrap_adjoint_create)", who, pop->adjoint ? "an adjoint" : "a forward",
                         padj ? "an adjoint" : "a forward");
    return 0;
}

}  // namespace bk

using namespace bk;

extern "C" {

int bk_potrap_create(bk_problem* prob, int M, bk_potrap** out) {
    if (!prob || !out) return -1;
    bk_ctx* ctx = prob->ctx;
    const double zero[6] = {0, 0, 0, 0, 0, 0};
    CglCoef c;
    BK_TRY(hopf_coef(prob, zero, 6, 0, &c));
    if (ctx->nranks > 1) return set_error(ctx, "bk_potrap_create: the trapezoid periodic-orbit functional runs on a single rank");
    if (M < 3) return set_error(ctx, "bk_potrap_create: M >= 3 time slices (got %d): M - 1 >= 2 intervals make a cycle", M);
    bk_potrap* h = new bk_potrap();
    h->ctx = ctx; h->prob = prob; h->M = M; h->n = prob->nloc / 2;
    if (hipMalloc(&h->phi, sizeof(double) * h->len()) != hipSuccess || hipMalloc(&h->xpi, sizeof(double) * h->len()) != hipSuccess) {
        if (h->phi) (void)hipFree(h->phi);
        delete h;
        return set_error(ctx, "bk_potrap_create: allocation failed");
    }
    *out = h;
    return 0;
}

int bk_potrap_destroy(bk_potrap* h) {
    if (!h) return 0;
    if (h->phi) (void)hipFree(h->phi);
    if (h->xpi) (void)hipFree(h->xpi);
    delete h;
    return 0;
}

int bk_potrap_set_section(bk_potrap* h, const double* phi, const double* xpi) {
    if (!h || !phi || !xpi) return -1;
    BK_TRY(v_copy(h->ctx, h->len(), phi, h->phi));
    BK_TRY(v_copy(h->ctx, h->len(), xpi, h->xpi));
    BK_TRY(v_dot(h->ctx, h->len(), h->xpi, h->phi, &h->c0));
    h->has_section = true;
    return 0;
}

int bk_potrap_get_section(bk_potrap* h, double* phi, double* xpi) {
    if (!h || !phi || !xpi) return -1;
    BK_TRY(potrap_check(h, "bk_potrap_get_section"));
    if (phi == xpi) return set_error(h->ctx, "bk_potrap_get_section: phi and xpi must be distinct");
    BK_TRY(v_copy(h->ctx, h->len(), h->phi, phi));
    return v_copy(h->ctx, h->len(), h->xpi, xpi);
}

int bk_potrap_residual(bk_potrap* h, const double* u, double T, const double* params, int nparams, double* out, double* out_tail) {
    if (!h || !u || !params || !out || !out_tail) return -1;
    CglPar par;
    BK_TRY(potrap_params(h, params, nparams, &par));
    BK_TRY(potrap_check(h, "bk_potrap_residual"));
    if (out == u || out == h->phi || out == h->xpi) return set_error(h->ctx, "bk_potrap_residual: out must not alias u or the section");
    double dot = 0.0;
    BK_TRY(potrap_march(h, par, u, T, nullptr, 0.0, out, &dot));
    *out_tail = dot - h->c0;
    return 0;
}

int bk_potrap_jvp(bk_potrap* h, const double* u, double T, const double* params, int nparams, const double* du, double dT,
                  double* out, double* out_tail) {
    if (!h || !u || !params || !du || !out || !out_tail) return -1;
    CglPar par;
    BK_TRY(potrap_params(h, params, nparams, &par));
    BK_TRY(potrap_check(h, "bk_potrap_jvp"));
    if (out == u || out == du || out == h->phi || out == h->xpi)
        return set_error(h->ctx, "bk_potrap_jvp: out must not alias u, du or the section");
    return potrap_march(h, par, u, T, du, dT, out, out_tail);
}

int bk_potrap_jvp_adjoint(bk_potrap* h, const double* u, double T, const double* params, int nparams, const double* w, double tau,
                          double* out, double* out_tail) {
    if (!h || !u || !params || !w || !out || !out_tail) return -1;
    CglPar par;
    BK_TRY(potrap_params(h, params, nparams, &par));
    BK_TRY(potrap_check(h, "bk_potrap_jvp_adjoint"));
    if (out == u || out == w || out == h->phi || out == h->xpi)
        return set_error(h->ctx, "bk_potrap_jvp_adjoint: out must not alias u, w or the section");
    return potrap_adjoint_march(h, par, u, T, w, tau, out, out_tail);
}

static int potrap_op_create(bk_potrap* h, const double* u, double T, const double* params, int nparams, bool adjoint, bk_op** out) {
    if (!h || !u || !params || !out) return -1;
    CglPar par;
    BK_TRY(potrap_params(h, params, nparams, &par));
    BK_TRY(potrap_check(h, adjoint ? "bk_potrap_op_adjoint_create" : "bk_potrap_op_create"));
    PoTrapOp* op = new PoTrapOp();
    op->ctx = h->ctx; op->n = h->len(); op->ntail = 1;
    op->h = h; op->u = u; op->T = T; op->par = par; op->adjoint = adjoint;
    *out = op;
    return 0;
}

int bk_potrap_op_create(bk_potrap* h, const double* u, double T, const double* params, int nparams, bk_op** out) {
    return potrap_op_create(h, u, T, params, nparams, false, out);
}

int bk_potrap_op_adjoint_create(bk_potrap* h, const double* u, double T, const double* params, int nparams, bk_op** out) {
    return potrap_op_create(h, u, T, params, nparams, true, out);
}

int bk_potrap_update_section(bk_potrap* h, const double* u, double T, const double* params, int nparams) {
    if (!h || !u || !params) return -1;
    (void)T;                                       // updatesection! reads the period and does not use it (:669)
    CglPar par;
    BK_TRY(potrap_params(h, params, nparams, &par));
    if (u == h->phi || u == h->xpi) return set_error(h->ctx, "bk_potrap_update_section: u must not alias the section");
    const size_t N = 2 * h->n;
    BK_TRY(v_copy(h->ctx, h->len(), u, h->xpi));
    for (int i = 0; i < h->M; ++i)                 // phi_i = F(u_i) / M, the scale in the stencil kernel's store stage
        BK_TRY(h->prob->apply(1, u + i * N, u + i * N, params, 0.0, 1.0 / h->M, h->phi + i * N));
    BK_TRY(v_dot(h->ctx, h->len(), h->xpi, h->phi, &h->c0));
    h->has_section = true;
    return 0;
}

int bk_potrap_dparam(bk_potrap* h, const double* u, double T, const double* params, int nparams, int ipar, double* out) {
    if (!h || !u || !params || !out) return -1;
    CglPar par;
    BK_TRY(potrap_params(h, params, nparams, &par));
    bk_ctx* ctx = h->ctx;
    if (ipar < 0 || ipar > 5) return set_error(ctx, "bk_potrap_dparam: bad parameter index %d", ipar);
    if (out == u) return set_error(ctx, "bk_potrap_dparam: out must not alias u");
    const size_t N = 2 * h->n;
    const double hh = T * (1.0 / h->M) / 2.0;
    WsGuard ws(ctx);
    double* tmp = nullptr;
    BK_TRY(ws.get(h->len(), &tmp));
    for (int i = 0; i < h->M - 1; ++i) BK_TRY(pde_dparam(ctx, h->prob->desc.pde, ipar, h->n, -hh, u + i * N, tmp + i * N));
    hipLaunchKernelGGL(potrap_dparam_combine_kernel, dim3(grid_for(h->len(), 1, 4096)), dim3(kThreads), 0, ctx->stream, N, h->M, tmp,
                       out);
    BK_HIP(ctx, hipGetLastError());
    return 0;
}

static int potrap_precond_create(bk_potrap* h, PoTsKind kind, double a, double b, bk_precond** out) {
    if (!h || !out) return -1;
    PoPrecond* P = nullptr;
    BK_TRY(po_precond_create(h, kind, a, b, 0.0, "bk_precond_potrap_create", &P));
    *out = P;
    return 0;
}

int bk_precond_potrap_create(bk_potrap* h, double a, double b, bk_precond** out) { return potrap_precond_create(h, kTsCyclic, a, b, out); }

int bk_precond_potrap_adjoint_create(bk_potrap* h, double a, double b, bk_precond** out) {
    return potrap_precond_create(h, kTsCyclicAdjoint, a, b, out);
}

int bk_precond_potrap_set_period(bk_precond* pl, double T) {
    if (!pl) return -1;
    PoPrecond* P = po_precond_cast(pl, false);
    if (!P) return set_error(pl->ctx, "bk_precond_potrap_set_period: not a preconditioner of bk_precond_potrap_create");
    return po_precond_set_period(P, T, "bk_precond_potrap_set_period");
}

int bk_precond_potrap_transform_paths(bk_precond* pl, int paths[2]) {
    if (!pl || !paths) return -1;
    PoPrecond* P = po_precond_cast(pl, false);
    if (!P) return set_error(pl->ctx, "bk_precond_potrap_transform_paths: not a preconditioner of bk_precond_potrap_create");
    dst_plan_paths(P->plan, paths);
    return 0;
}

int bk_potrap_solve(bk_ctx* ctx, bk_op* op, bk_precond* pl, const double* rhs, double rhs_tail, double* x, double* x_tail,
                    const bk_gmres_opts* opts, bk_solve_result* result) {
    if (!ctx || !op || !pl || !rhs || !x || !x_tail || !opts || !result) return -1;
    BK_TRY(potrap_pair_check(ctx, "bk_potrap_solve", op, pl));
    BK_TRY(potrap_opts_check(ctx, "bk_potrap_solve", opts));
    if (x == rhs) return set_error(ctx, "bk_potrap_solve: x must not alias rhs");
    WsGuard ws(ctx);
    double *tmp = nullptr, *prhs = nullptr;
    BK_TRY(ws.get(op->n, &tmp));
    BK_TRY(ws.get(op->n, &prhs));
    PoPrecOp W;
    W.ctx = ctx; W.n = op->n; W.ntail = 1;
    W.A = op; W.P = pl; W.tmp = tmp;
    BK_TRY(pl->apply(rhs, prhs));                 // the top of the right-hand side; the tail is untouched
    GmresResult r;
    BK_TRY(gmres_core(ctx, &W, prhs, &rhs_tail, x, x_tail, 0.0, 1.0, *opts, &r));
    solve_result_set(result, r);
    return 0;
}

}  // extern "C"
