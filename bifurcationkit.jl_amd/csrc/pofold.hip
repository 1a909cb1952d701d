// The fold of limit cycles of the trapezoid periodic-orbit functional, matrix-free, for BK_PDE_CGL2D on one rank
// (src/codim2/MinAugFold.jl on the Trapeze functional; examples/cGL2d.jl:347-392): the adjoint dG(u, T)^T on (w, tau) and the
// transposed space-time preconditioner A0^T (the left null vector), the border row of the fold system from the second derivative,
// doubly bordered solves that stay regular where dG is singular, the bordered vectors, the fold linear solver and the Newton loop.  Notation of potrap.hip: K = M - 1, prev(0) = K - 1,
// next(j) = j + 1 and next(K - 1) = 0, hh = T (1 / M) / 2, dG = [A c; phi^T 0] with c_i = -(1 / (2 M)) (F_i + F_prev(i)), c_K = 0.
//
// With s_j = w_j + w_next(j) and q_j = J_j^T s_j (ONE adjoint stencil evaluation per slice: the Laplacian is linear and symmetric,
// so the two slices' Laplacians add):
//
//     out_j = (w_j - w_next(j)) - hh q_j - [j = 0] w_K + tau phi_j        j < K
//     out_K = w_K + tau phi_K
//     tail  = -(1 / (2 M)) sum_{j < K} <F(u_j), s_j>
//
// Kernels.  potrap_adjoint_march_kernel is tiled as potrap_march_kernel: a workgroup owns 256 grid points and a chunk of consecutive
// rows, loads every slice of w once (centre pair and Laplacian, po_load) and carries it to the next row; a chunk loads the slice
// of its first row once more, through the same code and without a store, so a row's bits do not depend on the chunking.  The tail
// dot rides in the same pass (block_sum_store / reduce_finish).  Streams: u, w, phi read, out written.
// potrap_adjoint_timesolve_kernel is the middle of A0^-T: the DST-I is symmetric and L0^T acts on w^ = u1^ + i u2^ as the
// multiplication by conj(mu_k), so per sine mode w_K = f_K, f_0 <- f_0 + f_K and the cyclic recurrence runs backwards in time,
// w_j = conj(rho) w_next(j) + f_j / conj(alpha), closed with 1 - conj(rho)^K.
#include <cmath>

#include "cgl_pw.h"
#include "common.h"
#include "hopf_pw.h"
#include "minaug.h"
#include "ops.h"
#include "potrap_pw.h"
#include "stream.h"

namespace bk {

namespace {

struct PoAdjK {
    int nx, ny, M;
    int C;                         // rows per chunk
    unsigned ntiles;
    double ax, ay;
    CglPar par;
    double hh;                     // h / 2 = T / M / 2
    double tau;
    const double* u;
    const double* w;
    const double* phi;
    double* out;
};

// Grid: blockIdx.x = chunk * ntiles + tile, rows [r0, r1) of the K cyclic rows.  Step t loads slice next(r0 + t) of w and completes
// row r0 + t from it and the carried slice; t = -1 only loads slice r0.  The last chunk also writes row K.  One partial sum of
// sum_j <F(u_j), s_j> per workgroup.
__global__ void __launch_bounds__(kThreads) potrap_adjoint_march_kernel(PoAdjK P, double* __restrict__ partials) {
    const size_t n = (size_t)P.nx * P.ny, N = 2 * n;
    const unsigned tile = blockIdx.x % P.ntiles, chunk = blockIdx.x / P.ntiles;
    const size_t idx = (size_t)tile * kThreads + threadIdx.x;
    const int K = P.M - 1;
    const int r0 = (int)chunk * P.C, r1 = min(K, r0 + P.C);
    double s[1] = {0.0};
    if (idx < n) {
        const int i = (int)(idx % P.nx), j = (int)(idx / P.nx);
        const size_t slK = (size_t)K * N;
        PoPoint wc{0.0, 0.0, 0.0, 0.0};
        for (int t = -1; t < r1 - r0; ++t) {
            const int row = r0 + t;
            const size_t sn = (size_t)(row + 1 == K ? 0 : row + 1) * N;
            const PoPoint wn = po_load(P, P.w + sn, n, idx, i, j);
            if (t >= 0) {
                const size_t sl = (size_t)row * N;
                const PoPoint q = po_load(P, P.u + sl, n, idx, i, j);
                double n1, n2, f1u, f1v, f2u, f2v;
                cgl_nl(P.par, q.c1, q.c2, n1, n2);
                cgl_jac(P.par, q.c1, q.c2, f1u, f1v, f2u, f2v);
                const double F1 = q.d1 + n1, F2 = q.d2 + n2;
                const double s1 = wc.c1 + wn.c1, s2 = wc.c2 + wn.c2;
                const double q1 = (wc.d1 + wn.d1) + f1u * s1 + f2u * s2;
                const double q2 = (wc.d2 + wn.d2) + f1v * s1 + f2v * s2;
                double o1 = (wc.c1 - wn.c1) - P.hh * q1;
                double o2 = (wc.c2 - wn.c2) - P.hh * q2;
                if (row == 0) {
                    o1 -= P.w[slK + idx];
                    o2 -= P.w[slK + idx + n];
                }
                P.out[sl + idx] = o1 + P.tau * P.phi[sl + idx];
                P.out[sl + idx + n] = o2 + P.tau * P.phi[sl + idx + n];
                s[0] = fma(F1, s1, s[0]);
                s[0] = fma(F2, s2, s[0]);
            }
            wc = wn;
        }
        if (r1 == K) {
            P.out[slK + idx] = P.w[slK + idx] + P.tau * P.phi[slK + idx];
            P.out[slK + idx + n] = P.w[slK + idx + n] + P.tau * P.phi[slK + idx + n];
        }
    }
    block_sum_store<1>(s, partials);
}

// One thread per sine mode k, w = u1^ + i u2^, alpha, rho of potrap_timesolve_kernel conjugated.  First walk, j = K - 1 .. 0:
// acc <- rho acc + g_j / alpha with g_0 = f_0 + f_K, g_j = f_j, rho^K alongside; w_0 = acc / (1 - rho^K).  Second walk: the
// recurrence itself from w_next(K - 1) = w_0, written in place (row 0, the last one written, is read before that).  Row K stays.
struct PoAdjTs {
    int nx, ny, M;
    double a, b, hh;
    const double* lx;
    const double* ly;
    double* spec;
};
__global__ void __launch_bounds__(kThreads) potrap_adjoint_timesolve_kernel(PoAdjTs P) {
    const size_t n = (size_t)P.nx * P.ny, N = 2 * n;
    const size_t k = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (k >= n) return;
    const int K = P.M - 1;
    const double mr = P.a + (P.lx[k % P.nx] + P.ly[k / P.nx]), mi = -P.b;
    const Cx alpha{1.0 - P.hh * mr, -P.hh * mi}, beta{1.0 + P.hh * mr, P.hh * mi};
    const double ia = 1.0 / (alpha.r * alpha.r + alpha.i * alpha.i);
    const Cx inva{alpha.r * ia, -alpha.i * ia};
    const Cx rho = beta * inva;
    const Cx fK{P.spec[(size_t)K * N + k], P.spec[(size_t)K * N + n + k]};
    auto g = [&](int j) {
        Cx f{P.spec[(size_t)j * N + k], P.spec[(size_t)j * N + n + k]};
        if (j == 0) f = f + fK;
        return f;
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
        P.spec[(size_t)j * N + k] = w.r;
        P.spec[(size_t)j * N + n + k] = w.i;
    }
}

// The border row of the fold system and its two scalars in one pass over u, v, w (3 streams read, 1 written), walked as the adjoint
// march (w carried, s_j and q_j as there):
//     out_j = hh (B_j[v_j, .])^T s_j + dv q_j (j < K), out_K = 0;   s[0] = sum_j <q_j, v_j>;   s[1] = sum_j <s_j, hh D_p(u_j) v_j + dv d_pF(u_j)>
// with B the pointwise Hessian (cgl_hess), D_p = dJ/dp (cgl_djdp), d_pF pointwise (cgl_dpar), dv = v_T / M / 2.
struct PoFbK {
    int nx, ny, M;
    int C;
    unsigned ntiles;
    double ax, ay;
    CglPar par;
    CglCoef coef;
    double hh, dv;
    const double* u;
    const double* v;
    const double* w;
    double* out;
};
__global__ void __launch_bounds__(kThreads) pofold_border_kernel(PoFbK P, double* __restrict__ partials) {
    const size_t n = (size_t)P.nx * P.ny, N = 2 * n;
    const unsigned tile = blockIdx.x % P.ntiles, chunk = blockIdx.x / P.ntiles;
    const size_t idx = (size_t)tile * kThreads + threadIdx.x;
    const int K = P.M - 1;
    const int r0 = (int)chunk * P.C, r1 = min(K, r0 + P.C);
    double s[2] = {0.0, 0.0};
    if (idx < n) {
        const int i = (int)(idx % P.nx), j = (int)(idx / P.nx);
        PoPoint wc{0.0, 0.0, 0.0, 0.0};
        for (int t = -1; t < r1 - r0; ++t) {
            const int row = r0 + t;
            const size_t sn = (size_t)(row + 1 == K ? 0 : row + 1) * N;
            const PoPoint wn = po_load(P, P.w + sn, n, idx, i, j);
            if (t >= 0) {
                const size_t sl = (size_t)row * N;
                const double u1 = P.u[sl + idx], u2 = P.u[sl + idx + n];
                const double v1 = P.v[sl + idx], v2 = P.v[sl + idx + n];
                double f1u, f1v, f2u, f2v, h[6], d[4], p1, p2;
                cgl_jac(P.par, u1, u2, f1u, f1v, f2u, f2v);
                cgl_hess(P.coef, u1, u2, h);
                cgl_djdp(P.coef.ipar, u1, u2, d);
                cgl_dpar(P.coef.ipar, u1, u2, p1, p2);
                const double s1 = wc.c1 + wn.c1, s2 = wc.c2 + wn.c2;
                const double q1 = (wc.d1 + wn.d1) + f1u * s1 + f2u * s2;
                const double q2 = (wc.d2 + wn.d2) + f1v * s1 + f2v * s2;
                const double t1 = s1 * (h[0] * v1 + h[1] * v2) + s2 * (h[3] * v1 + h[4] * v2);
                const double t2 = s1 * (h[1] * v1 + h[2] * v2) + s2 * (h[4] * v1 + h[5] * v2);
                P.out[sl + idx] = P.hh * t1 + P.dv * q1;
                P.out[sl + idx + n] = P.hh * t2 + P.dv * q2;
                s[0] = fma(q1, v1, s[0]);
                s[0] = fma(q2, v2, s[0]);
                const double e1 = P.hh * (d[0] * v1 + d[1] * v2) + P.dv * p1;
                const double e2 = P.hh * (d[2] * v1 + d[3] * v2) + P.dv * p2;
                s[1] = fma(s1, e1, s[1]);
                s[1] = fma(s2, e2, s[1]);
            }
            wc = wn;
        }
        if (r1 == K) {
            P.out[(size_t)K * N + idx] = 0.0;
            P.out[(size_t)K * N + idx + n] = 0.0;
        }
    }
    block_sum_store<2>(s, partials);
}

// [A a; b' c] on (x, (t, sigma)) for an orbit operator A with its T tail (dG or dG^T), left-preconditioned by diag(P, 1, 1):
//     out.u = P^-1 (A (x, t)).u + sigma atil,   out.t = (A (x, t)).t + a_T sigma,   out.sigma = <b_u, x> + b_T t + c sigma
// atil = P^-1 a_u is formed once per solve; per application the column update and the row dot are ONE pass (bordered_tail).
struct PoBorderedOp : bk_op {
    bk_op* A = nullptr;
    bk_precond* P = nullptr;
    double* tmp = nullptr;
    const double* atil = nullptr;
    const double* bu = nullptr;
    double aT = 0.0, bT = 0.0, c = 0.0;
    int apply(const double* x, const double* xt, double a0, double a1, double* out, double* outt) override {
        double tt = 0.0, d = 0.0;
        BK_TRY(A->apply(x, xt, 0.0, 1.0, tmp, &tt));
        BK_TRY(P->apply(tmp, out));
        const double* const at[1] = {atil};
        const double* const bb[1] = {bu};
        BK_TRY(bordered_tail(ctx, n, 1, out, x, at, bb, &xt[1], &d));
        if (!(a0 == 0.0 && a1 == 1.0)) BK_TRY(v_axpby(ctx, n, a0, x, a1, out));
        outt[0] = a0 * xt[0] + a1 * (tt + aT * xt[1]);
        outt[1] = a0 * xt[1] + a1 * ((d + bT * xt[0]) + c * xt[1]);
        return 0;
    }
};

// a, b: device vectors with host T entries; rhs (device, T entry, border scalar); x device, xt[2] = (T entry, border scalar)
int potrap_bordered_solve(bk_ctx* ctx, bk_op* op, bk_precond* pl, const double* a, double aT, const double* b, double bT, double c,
                          const double* rhs, double rhsT, double rhsB, double* x, double xt[2], const bk_gmres_opts& opts,
                          GmresResult* r) {
    WsGuard ws(ctx);
    double *tmp = nullptr, *prhs = nullptr, *atil = nullptr;
    BK_TRY(ws.get(op->n, &tmp));
    BK_TRY(ws.get(op->n, &prhs));
    BK_TRY(ws.get(op->n, &atil));
    BK_TRY(pl->apply(a, atil));
    BK_TRY(pl->apply(rhs, prhs));
    PoBorderedOp W;
    W.ctx = ctx; W.n = op->n; W.ntail = 2;
    W.A = op; W.P = pl; W.tmp = tmp; W.atil = atil; W.bu = b; W.aT = aT; W.bT = bT; W.c = c;
    const double bt[2] = {rhsT, rhsB};
    return gmres_core(ctx, &W, prhs, bt, x, xt, 0.0, 1.0, opts, r);
}

int pofold_check(bk_potrap* h, const char* who) {
    if (!h->has_section)
        return set_error(h->ctx, "%s: no section set (bk_potrap_set_section or bk_potrap_update_section first)", who);
    return 0;
}

int pofold_opts_check(bk_ctx* ctx, const char* who, const bk_gmres_opts* opts) {
    if (opts->flavor >= BK_KRYLOV_MINRES) return set_error(ctx, "%s: the orbit Jacobian is not symmetric (use a GMRES flavor)", who);
    if (opts->pr) return set_error(ctx, "%s: left preconditioner only", who);
    return 0;
}

struct OpPair {
    bk_op* J = nullptr;
    bk_op* Jt = nullptr;
    ~OpPair() { if (J) bk_op_destroy(J); if (Jt) bk_op_destroy(Jt); }
};

// [dG a; b' 0][v; sigma] = [0; 1] and [dG^T b; a' 0][w; sigma2] = [0; 1] (MinAugFold.jl:15-69), one bordered solve each
int pofold_terms(bk_potrap* h, const double* u, double T, const double* par, const double* a, double aT, const double* b, double bT,
                 bk_precond* pl, bk_precond* plT, const bk_gmres_opts& opts, const double* zero, double* v, double* vT, double* w,
                 double* wT, double* sigma, int* converged, int it[2]) {
    OpPair jp;
    BK_TRY(bk_potrap_op_create(h, u, T, par, 6, &jp.J));
    BK_TRY(bk_potrap_op_adjoint_create(h, u, T, par, 6, &jp.Jt));
    BK_TRY(potrap_pair_check(h->ctx, "bk_potrap_fold_terms", jp.J, pl));
    BK_TRY(potrap_pair_check(h->ctx, "bk_potrap_fold_terms", jp.Jt, plT));
    GmresResult r0, r1;
    double xt[2];
    BK_TRY(potrap_bordered_solve(h->ctx, jp.J, pl, a, aT, b, bT, 0.0, zero, 0.0, 1.0, v, xt, opts, &r0));
    *vT = xt[0];
    *sigma = xt[1];
    BK_TRY(potrap_bordered_solve(h->ctx, jp.Jt, plT, b, bT, a, aT, 0.0, zero, 0.0, 1.0, w, xt, opts, &r1));
    *wT = xt[0];
    *converged = r0.converged & r1.converged;
    it[0] = r0.niter;
    it[1] = r1.niter;
    return 0;
}

}  // namespace

// sigx = the first M N entries of the border row, *sigxT its T entry, *sigp = sigma_p for params[ipar]
int pofold_border(bk_potrap* h, const CglPar& par, const CglCoef& coef, const double* u, double T, const double* v, double vT,
                  const double* w, double* sigx, double* sigxT, double* sigp) {
    bk_ctx* ctx = h->ctx;
    const bk_problem_desc& d = h->prob->desc;
    PoFbK P{d.n[0], d.n[1], h->M, 1, 1u, h->prob->ainv[0], h->prob->ainv[1], par, coef, T * (1.0 / h->M) / 2.0, vT / h->M / 2.0,
            u, v, w, sigx};
    int nchunks = 1;
    BK_TRY(potrap_chunking(ctx, h->n, h->M, &P.ntiles, &P.C, &nchunks));
    const unsigned grid = P.ntiles * (unsigned)nchunks;
    if ((size_t)grid * 2 > kPartialDoubles)
        return set_error(ctx, "pofold: %u workgroups x 2 sums exceed the reduction scratch", grid);
    {
        ProfScope ps(ctx, "pofold_border", 8.0 * h->len() * 4);
        hipLaunchKernelGGL(pofold_border_kernel, dim3(grid), dim3(kThreads), 0, ctx->stream, P, ctx->d_partials);
        BK_HIP(ctx, hipGetLastError());
    }
    BK_TRY(reduce_finish(ctx, (int)grid, 2, 0));
    *sigxT = ctx->h_red[0] / h->M / 2.0;
    *sigp = ctx->h_red[1];
    return 0;
}

// the adjoint marching pass: out = the first M N entries of dG^T (w, tau), *tail the last; algorithmic bytes: u, w, phi read, out
// written
int potrap_adjoint_march(bk_potrap* h, const CglPar& par, const double* u, double T, const double* w, double tau, double* out,
                         double* tail) {
    bk_ctx* ctx = h->ctx;
    const bk_problem_desc& d = h->prob->desc;
    PoAdjK P{d.n[0], d.n[1], h->M, 1, 1u, h->prob->ainv[0], h->prob->ainv[1], par, T * (1.0 / h->M) / 2.0, tau, u, w, h->phi, out};
    int nchunks = 1;
    BK_TRY(potrap_chunking(ctx, h->n, h->M, &P.ntiles, &P.C, &nchunks));
    const unsigned grid = P.ntiles * (unsigned)nchunks;
    {
        ProfScope ps(ctx, "potrap_jvp_adjoint", 8.0 * h->len() * 4);
        hipLaunchKernelGGL(potrap_adjoint_march_kernel, dim3(grid), dim3(kThreads), 0, ctx->stream, P, ctx->d_partials);
        BK_HIP(ctx, hipGetLastError());
    }
    BK_TRY(reduce_finish(ctx, (int)grid, 1, 0));
    *tail = -(ctx->h_red[0] / h->M / 2.0);
    return 0;
}

// the time solve of A0^-T on the spectrum of all 2 M fields, in place
int potrap_adjoint_timesolve(bk_ctx* ctx, int nx, int ny, int M, double a, double b, double hh, const double* lx, const double* ly,
                             double* spec) {
    const size_t npts = (size_t)nx * ny;
    ProfScope ps(ctx, "potrap_adjoint_timesolve", 8.0 * 2 * npts * M * 3);
    const PoAdjTs P{nx, ny, M, a, b, hh, lx, ly, spec};
    hipLaunchKernelGGL(potrap_adjoint_timesolve_kernel, dim3((unsigned)((npts + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       ctx->stream, P);
    BK_HIP(ctx, hipGetLastError());
    return 0;
}

}  // namespace bk

using namespace bk;

extern "C" {

int bk_potrap_jvp_adjoint(bk_potrap* h, const double* u, double T, const double* params, int nparams, const double* w, double tau,
                          double* out, double* out_tail) {
    if (!h || !u || !params || !w || !out || !out_tail) return -1;
    CglPar par;
    BK_TRY(potrap_params(h, params, nparams, &par));
    if (!h->has_section)
        return set_error(h->ctx, "bk_potrap_jvp_adjoint: no section set (bk_potrap_set_section or bk_potrap_update_section first)");
    if (out == u || out == w || out == h->phi || out == h->xpi)
        return set_error(h->ctx, "bk_potrap_jvp_adjoint: out must not alias u, w or the section");
    return potrap_adjoint_march(h, par, u, T, w, tau, out, out_tail);
}

int bk_potrap_bordered_solve(bk_ctx* ctx, bk_op* op, bk_precond* pl, const double* a, double a_tail, const double* b, double b_tail,
                             double c, const double* rhs, double rhs_tail, double rhs_border, double* x, double* x_tail,
                             double* x_border, const bk_gmres_opts* opts, bk_solve_result* result) {
    if (!ctx || !op || !pl || !a || !b || !rhs || !x || !x_tail || !x_border || !opts || !result) return -1;
    BK_TRY(potrap_pair_check(ctx, "bk_potrap_bordered_solve", op, pl));
    BK_TRY(pofold_opts_check(ctx, "bk_potrap_bordered_solve", opts));
    if (x == rhs || x == a || x == b) return set_error(ctx, "bk_potrap_bordered_solve: x must not alias rhs, a or b");
    GmresResult r;
    double xt[2] = {0.0, 0.0};
    BK_TRY(potrap_bordered_solve(ctx, op, pl, a, a_tail, b, b_tail, c, rhs, rhs_tail, rhs_border, x, xt, *opts, &r));
    *x_tail = xt[0];
    *x_border = xt[1];
    result->converged = r.converged;
    result->niter = r.niter;
    result->resnorm = r.resnorm;
    return 0;
}

int bk_potrap_fold_border(bk_potrap* h, const double* u, double T, const double* params, int nparams, int ipar, const double* v,
                          double v_T, const double* w, double* sigx, double* sigx_T, double* sigma_p) {
    if (!h || !u || !params || !v || !w || !sigx || !sigx_T || !sigma_p) return -1;
    CglPar par;
    CglCoef coef;
    BK_TRY(potrap_params(h, params, nparams, &par));
    BK_TRY(hopf_coef(h->prob, params, nparams, ipar, &coef));
    if (sigx == u || sigx == v || sigx == w) return set_error(h->ctx, "bk_potrap_fold_border: sigx must not alias u, v or w");
    return pofold_border(h, par, coef, u, T, v, v_T, w, sigx, sigx_T, sigma_p);
}

int bk_potrap_fold_terms(bk_potrap* h, const double* u, double T, const double* params, int nparams, const double* a, double a_T,
                         const double* b, double b_T, bk_precond* pl, bk_precond* pl_adjoint, const bk_gmres_opts* opts, double* v,
                         double* v_T, double* w, double* w_T, double* sigma, int* converged, int itlinear[2]) {
    if (!h || !u || !params || !a || !b || !pl || !pl_adjoint || !opts || !v || !v_T || !w || !w_T || !sigma || !converged || !itlinear)
        return -1;
    CglPar par;
    BK_TRY(potrap_params(h, params, nparams, &par));
    BK_TRY(pofold_check(h, "bk_potrap_fold_terms"));
    BK_TRY(pofold_opts_check(h->ctx, "bk_potrap_fold_terms", opts));
    if (v == w || v == a || v == b || w == a || w == b || v == u || w == u)
        return set_error(h->ctx, "bk_potrap_fold_terms: v and w must be distinct from each other and from u, a and b");
    WsGuard ws(h->ctx);
    double* zero = nullptr;
    BK_TRY(ws.get(h->len(), &zero));
    BK_TRY(v_zero(h->ctx, h->len(), zero));
    return pofold_terms(h, u, T, params, a, a_T, b, b_T, pl, pl_adjoint, *opts, zero, v, v_T, w, w_T, sigma, converged, itlinear);
}

int bk_potrap_fold_linsolve(bk_potrap* h, const double* u, double T, const double* params, int nparams, int ipar, const double* v,
                            double v_T, const double* w, bk_precond* pl, int nrhs, const double* const* rhsu, const double* rhsT,
                            const double* rhsp, const bk_gmres_opts* opts, double* const* dX, double* dXT, double* dsigma,
                            int* converged, int* itlinear) {
    if (!h || !u || !params || !v || !w || !pl || !rhsu || !rhsT || !rhsp || !opts || !dX || !dXT || !dsigma) return -1;
    bk_ctx* ctx = h->ctx;
    CglPar par;
    CglCoef coef;
    BK_TRY(potrap_params(h, params, nparams, &par));
    BK_TRY(hopf_coef(h->prob, params, nparams, ipar, &coef));
    BK_TRY(pofold_check(h, "bk_potrap_fold_linsolve"));
    BK_TRY(pofold_opts_check(ctx, "bk_potrap_fold_linsolve", opts));
    BK_TRY(minaug_check_rhs(ctx, "bk_potrap_fold_linsolve", nrhs, rhsu, dX));
    for (int k = 0; k < nrhs; ++k)
        if (dX[k] == u || dX[k] == v || dX[k] == w) return set_error(ctx, "bk_potrap_fold_linsolve: dX must not alias u, v or w");
    const size_t n = h->len();
    WsGuard ws(ctx);
    double *sigx = nullptr, *dpG = nullptr;
    BK_TRY(ws.get(n, &sigx));
    BK_TRY(ws.get(n, &dpG));
    double sxT = 0.0, sp = 0.0;
    BK_TRY(pofold_border(h, par, coef, u, T, v, v_T, w, sigx, &sxT, &sp));
    BK_TRY(bk_potrap_dparam(h, u, T, params, nparams, ipar, dpG));
    OpPair jp;
    BK_TRY(bk_potrap_op_create(h, u, T, params, nparams, &jp.J));
    BK_TRY(potrap_pair_check(ctx, "bk_potrap_fold_linsolve", jp.J, pl));
    int cv = 1, it = 0;
    for (int k = 0; k < nrhs; ++k) {
        GmresResult r;
        double xt[2] = {0.0, 0.0};
        BK_TRY(potrap_bordered_solve(ctx, jp.J, pl, dpG, 0.0, sigx, sxT, sp, rhsu[k], rhsT[k], rhsp[k], dX[k], xt, *opts, &r));
        dXT[k] = xt[0];
        dsigma[k] = xt[1];
        cv &= r.converged;
        it += r.niter;
    }
    if (converged) *converged = cv;
    if (itlinear) *itlinear = it;
    return 0;
}

int bk_potrap_newton_fold(bk_potrap* h, double* u, double* T, double* p, const double* params, int nparams, int ipar, const double* a,
                          double a_T, const double* b, double b_T, bk_precond* pl, bk_precond* pl_adjoint, const bk_newton_opts* no,
                          const bk_gmres_opts* opts, double* v, double* v_T, double* w, double* w_T, double* sigma,
                          bk_newton_result* res, int* itlinear_steps) {
    if (!h || !u || !T || !p || !params || !a || !b || !pl || !pl_adjoint || !no || !opts || !v || !v_T || !w || !w_T || !sigma || !res)
        return -1;
    bk_ctx* ctx = h->ctx;
    CglPar cp;
    CglCoef cc;
    BK_TRY(potrap_params(h, params, nparams, &cp));                 // the problem kind, the parameter count and index
    BK_TRY(hopf_coef(h->prob, params, nparams, ipar, &cc));
    BK_TRY(pofold_check(h, "bk_potrap_newton_fold"));
    BK_TRY(pofold_opts_check(ctx, "bk_potrap_newton_fold", opts));
    if (no->max_iterations > BK_MAX_NEWTON_ITER) return set_error(ctx, "max_iterations > %d", BK_MAX_NEWTON_ITER);
    if (v == w || v == a || v == b || w == a || w == b || v == u || w == u || u == a || u == b)
        return set_error(ctx, "bk_potrap_newton_fold: u, v and w must be distinct from a and b and from each other");
    const size_t n = h->len();
    const bool inf = no->norm_inf != 0;
    WsGuard ws(ctx);
    double *fx = nullptr, *dX = nullptr, *zero = nullptr, *sigx = nullptr, *dpG = nullptr;
    BK_TRY(ws.get(n, &fx));
    BK_TRY(ws.get(n, &dX));
    BK_TRY(ws.get(n, &zero));
    BK_TRY(ws.get(n, &sigx));
    BK_TRY(ws.get(n, &dpG));
    BK_TRY(v_zero(ctx, n, zero));
    double par[6];
    for (int i = 0; i < 6; ++i) par[i] = params[i];
    double pc = *p, Tc = *T, gT = 0.0;
    int nstep = 0;
    // the fold residual (G, sigma) at (u, Tc, pc) with the bordered vectors of this point, which the step from it reuses
    auto point = [&](double* r, int* itl) -> int {
        par[ipar] = pc;
        int cv = 0, it[2] = {0, 0};
        BK_TRY(pofold_terms(h, u, Tc, par, a, a_T, b, b_T, pl, pl_adjoint, *opts, zero, v, v_T, w, w_T, sigma, &cv, it));
        *itl = it[0] + it[1];
        if (itlinear_steps) { itlinear_steps[3 * nstep] = it[0]; itlinear_steps[3 * nstep + 1] = it[1]; }
        BK_TRY(bk_potrap_residual(h, u, Tc, par, 6, fx, &gT));
        double g = 0.0;
        if (inf) {
            BK_TRY(v_nrminf(ctx, n, fx, &g));
            *r = fmax(fmax(g, fabs(gT)), fabs(*sigma));
            if (g != g || gT != gT || *sigma != *sigma) *r = NAN;
        } else {
            BK_TRY(v_nrm2(ctx, n, fx, &g));
            *r = sqrt(g * g + gT * gT + *sigma * *sigma);
        }
        return 0;
    };
    // [dG d_pG; sigma_x' sigma_p][dX; dp] = [G; sigma] as one bordered solve (MinAugFold.jl:136-145); (u, T, p) -= (dX, dp)
    auto step = [&](int* itl) -> int {
        par[ipar] = pc;
        BK_TRY(potrap_params(h, par, 6, &cp));
        BK_TRY(hopf_coef(h->prob, par, 6, ipar, &cc));
        double sxT = 0.0, sp = 0.0, xt[2] = {0.0, 0.0};
        BK_TRY(pofold_border(h, cp, cc, u, Tc, v, *v_T, w, sigx, &sxT, &sp));
        BK_TRY(bk_potrap_dparam(h, u, Tc, par, 6, ipar, dpG));
        OpPair jp;
        BK_TRY(bk_potrap_op_create(h, u, Tc, par, 6, &jp.J));
        GmresResult r;
        BK_TRY(potrap_bordered_solve(ctx, jp.J, pl, dpG, 0.0, sigx, sxT, sp, fx, gT, *sigma, dX, xt, *opts, &r));
        *itl = r.niter;
        if (itlinear_steps) itlinear_steps[3 * nstep + 2] = r.niter;
        nstep += 1;
        BK_TRY(v_axpby(ctx, n, -1.0, dX, 1.0, u));
        Tc -= xt[0];
        pc -= xt[1];
        return 0;
    };
    BK_TRY(minaug_newton(no, res, u, fx, &pc, point, step));
    *p = pc;
    *T = Tc;
    return 0;
}

}  // extern "C"
