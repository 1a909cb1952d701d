// Floquet multipliers of the trapezoid periodic orbits of cGL by ONE space-time solve per application of the monodromy, in the
// place of the K = M - 1 sequential slice solves of MonodromyQaD_matrix_free(::Trapeze, ...) (src/periodicorbit/Floquet.jl:285-315):
//
//     x <- (I - hh J_i)^-1 (I + hh J_prev(i)) x,   i = 0 .. K - 1,   prev(0) = K - 1,   hh = T (1 / M) / 2
//
// The same vector is the last slice of the solution of the block lower-bidiagonal initial-value system over all K slices
//
//     A_i y_i - B_{i-1} y_{i-1} = 0 (i >= 1),    A_0 y_0 = B_{K-1} x,    A_i = I - hh J_i,  B_i = I + hh J_i,    M x = y_{K-1},
//
// the rows i < K of dG (potrap.hip) with the cyclic link of row 0 cut.  All K slices y_0 .. y_{K-1} are the space-time
// eigenfunction when x is a Floquet eigenvector (the Val(:ExtractEigenVector) method, :319-355): they come out of the same solve.
//
// Kernels.  monodromy_march_kernel applies the initial-value operator to K slices in one launch, tiled as potrap_march_kernel
// (256 grid points per workgroup, chunks of consecutive rows from potrap_chunking, B_{i-1} y_{i-1}'s two parts carried in
// registers): three streams of 8 K N bytes, u read, y read, out written; no F, no period column, no phase dot, no reduction.
// monodromy_timesolve_kernel is the middle of the preconditioner: per sine mode w_i = rho w_{i-1} + f_i / alpha from w_{-1} = 0,
// one read and one write of the spectrum; no closure row and no division by 1 - rho^K, so the only guard left is |alpha|.
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

struct IvK {
    int nx, ny, K;
    int C;                         // rows per chunk
    unsigned ntiles;
    double ax, ay;
    CglPar par;
    double hh;                     // h / 2 = T (1 / M) / 2
    const double* u;               // the orbit: slice i at u + i N
    const double* y;
    double* out;
};

// Grid: blockIdx.x = chunk * ntiles + tile.  Rows [r0, r1) of the K rows
//     out_i = (y_i - hh J_i y_i) - (y_{i-1} + hh J_{i-1} y_{i-1}),   out_0 = y_0 - hh J_0 y_0.
// A chunk with r0 > 0 evaluates slice r0 - 1 first (t = -1) by the same code as every other slice, without a store; chunk 0 starts
// from exact zeros, and x - 0 is x: a row's bits do not depend on the chunking.
__global__ void __launch_bounds__(kThreads) monodromy_march_kernel(IvK P) {
    const size_t n = (size_t)P.nx * P.ny, N = 2 * n;
    const unsigned tile = blockIdx.x % P.ntiles, chunk = blockIdx.x / P.ntiles;
    const size_t idx = (size_t)tile * kThreads + threadIdx.x;
    if (idx >= n) return;
    const int r0 = (int)chunk * P.C, r1 = min(P.K, r0 + P.C);
    const int i = (int)(idx % P.nx), j = (int)(idx / P.nx);
    double b1 = 0.0, b2 = 0.0;     // y_{i-1} + hh J_{i-1} y_{i-1}
    for (int t = r0 > 0 ? -1 : 0; t < r1 - r0; ++t) {
        const size_t sl = (size_t)(r0 + t) * N;
        const double c1 = P.u[sl + idx], c2 = P.u[sl + idx + n];
        const PoPoint v = po_load(P, P.y + sl, n, idx, i, j);
        double f1u, f1v, f2u, f2v;
        cgl_jac(P.par, c1, c2, f1u, f1v, f2u, f2v);
        const double J1 = P.hh * (v.d1 + f1u * v.c1 + f1v * v.c2);
        const double J2 = P.hh * (v.d2 + f2u * v.c1 + f2v * v.c2);
        if (t >= 0) {
            P.out[sl + idx] = (v.c1 - J1) - b1;
            P.out[sl + idx + n] = (v.c2 - J2) - b2;
        }
        b1 = v.c1 + J1;
        b2 = v.c2 + J2;
    }
}

// The time solve of the initial-value preconditioner, one thread per sine mode k and w = u1^ + i u2^: alpha, beta, rho exactly
// as in potrap_timesolve_kernel (mu = a + lam_k + i b, alpha = 1 - hh mu, beta = 1 + hh mu, rho = beta / alpha); the rows read
// alpha w_i - beta w_{i-1} = f_i with w_{-1} = 0.  In place, coalesced across modes.
struct IvTs {
    int nx, ny, K;
    double a, b, hh;
    const double* lx;
    const double* ly;
    double* spec;
};
__global__ void __launch_bounds__(kThreads) monodromy_timesolve_kernel(IvTs P) {
    const size_t n = (size_t)P.nx * P.ny, N = 2 * n;
    const size_t k = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (k >= n) return;
    const double mr = P.a + (P.lx[k % P.nx] + P.ly[k / P.nx]), mi = P.b;
    const Cx alpha{1.0 - P.hh * mr, -P.hh * mi}, beta{1.0 + P.hh * mr, P.hh * mi};
    const double ia = 1.0 / (alpha.r * alpha.r + alpha.i * alpha.i);
    const Cx inva{alpha.r * ia, -alpha.i * ia};
    const Cx rho = beta * inva;
    Cx w{0.0, 0.0};
    for (int i = 0; i < P.K; ++i) {
        const Cx f{P.spec[(size_t)i * N + k], P.spec[(size_t)i * N + n + k]};
        w = rho * w + f * inva;
        P.spec[(size_t)i * N + k] = w.r;
        P.spec[(size_t)i * N + n + k] = w.i;
    }
}

// the marching pass on K slices; algorithmic bytes: u read, y read, out written
int ivp_march(bk_potrap* h, const CglPar& par, const double* u, double T, const double* y, double* out) {
    bk_ctx* ctx = h->ctx;
    const bk_problem_desc& d = h->prob->desc;
    const int K = h->M - 1;
    IvK P{d.n[0], d.n[1], K, 1, 1u, h->prob->ainv[0], h->prob->ainv[1], par, T * (1.0 / h->M) / 2.0, u, y, out};
    int nchunks = 1;
    BK_TRY(potrap_chunking(ctx, h->n, h->M, &P.ntiles, &P.C, &nchunks));
    ProfScope ps(ctx, "monodromy_march", 8.0 * 2 * h->n * K * 3);
    hipLaunchKernelGGL(monodromy_march_kernel, dim3(P.ntiles * (unsigned)nchunks), dim3(kThreads), 0, ctx->stream, P);
    BK_HIP(ctx, hipGetLastError());
    return 0;
}

// A0^-1 for the initial-value matrix A0: the rows above with every J_i replaced by L0 = Lap (x) I_2 + [[a, -b], [b, a]].  The DST-I
// of all 2 K fields in one batched plan, the time solve per mode, the DST-I back.
struct IvpPrecond : bk_precond {
    DctPlan* plan = nullptr;
    int nx = 0, ny = 0, K = 0;
    double a = 0.0, b = 0.0, hh = 0.0;
    ~IvpPrecond() override { dct_plan_destroy(plan); }
    int apply(const double* v, double* out) override {
        double* spec = dst_plan_scratch(plan);
        BK_TRY(dst_transform(ctx, plan, 0, v, spec));
        {
            const size_t npts = (size_t)nx * ny;
            ProfScope ps(ctx, "monodromy_timesolve", 8.0 * n * 2);
            const IvTs P{nx, ny, K, a, b, hh, dst_plan_lam(plan, 0), dst_plan_lam(plan, 1), spec};
            hipLaunchKernelGGL(monodromy_timesolve_kernel, dim3((unsigned)((npts + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                               ctx->stream, P);
            BK_HIP(ctx, hipGetLastError());
        }
        return dst_transform(ctx, plan, 1, spec, out);
    }
};

int ivp_precond_create(bk_potrap* h, double a, double b, double T, const char* who, IvpPrecond** out) {
    bk_ctx* ctx = h->ctx;
    IvpPrecond* P = new IvpPrecond();
    const int K = h->M - 1;
    P->ctx = ctx; P->n = 2 * h->n * (size_t)K;
    P->nx = h->prob->desc.n[0]; P->ny = h->prob->desc.n[1]; P->K = K; P->a = a; P->b = b;
    P->hh = T * (1.0 / h->M) / 2.0;
    const int s = dst_plan_create(ctx, h->prob->desc.n, h->prob->ainv, 0.0, 2 * K, &P->plan);
    if (s != 0) { delete P; return s; }
    std::vector<double> lx(P->nx), ly(P->ny);
    if (hipMemcpy(lx.data(), dst_plan_lam(P->plan, 0), sizeof(double) * P->nx, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(ly.data(), dst_plan_lam(P->plan, 1), sizeof(double) * P->ny, hipMemcpyDeviceToHost) != hipSuccess) {
        delete P;
        return set_error(ctx, "%s: reading the eigenvalue tables failed", who);
    }
    double min_a = INFINITY;
    int ka[2] = {0, 0};
    for (int j = 0; j < P->ny; ++j)
        for (int i = 0; i < P->nx; ++i) {
            const std::complex<double> mu(a + (lx[i] + ly[j]), b);
            const double aa = std::abs(1.0 - P->hh * mu);
            if (!(aa >= min_a)) { min_a = aa; ka[0] = i; ka[1] = j; }
        }
    if (!(min_a >= kPoPivot)) {
        delete P;
        return set_error(ctx, "%s: |alpha| = |1 - (h/2) mu| = %.3g below %.0e at sine mode (%d, %d): move a (or T) away from it", who,
                         min_a, kPoPivot, ka[0] + 1, ka[1] + 1);
    }
    *out = P;
    return 0;
}

// A0^-1 (initial-value operator): what the left-preconditioned solve iterates on
struct IvpPrecOp : bk_op {
    bk_potrap* h = nullptr;
    const double* u = nullptr;
    double T = 0.0;
    CglPar par{};
    IvpPrecond* P = nullptr;
    double* tmp = nullptr;
    int apply(const double* x, const double*, double a0, double a1, double* out, double*) override {
        if (out == x) return set_error(ctx, "monodromy operator: out must not alias x");
        BK_TRY(ivp_march(h, par, u, T, x, tmp));
        BK_TRY(P->apply(tmp, out));
        if (!(a0 == 0.0 && a1 == 1.0)) BK_TRY(v_axpby(ctx, n, a0, x, a1, out));
        return 0;
    }
};

// x -> y_{K-1}: one left-preconditioned GMRES on the K N unknowns per application; references u
struct MonodromyOp : bk_op {
    IvpPrecOp W;
    bk_gmres_opts ls{};
    double params[BK_MAX_PARAMS] = {0};
    double* work = nullptr;        // [3 K N]: tmp | the preconditioned right-hand side | y
    int solves = 0, failed = 0, inner_its = 0;
    size_t KN() const { return W.n; }
    double* y() const { return work + 2 * KN(); }
    ~MonodromyOp() override {
        delete W.P;
        if (work) (void)hipFree(work);
    }
    // y_0 .. y_{K-1} of M x into y()
    int solve(const double* x, GmresResult* r) {
        const int K = W.h->M - 1;
        double *tmp = work, *prhs = work + KN();
        // f_0 = x + hh J_{K-1} x through the stencil kernel, the other rows zero
        BK_TRY(v_zero(ctx, KN(), tmp));
        BK_TRY(W.h->prob->apply(0, x, W.u + (size_t)(K - 1) * n, params, 1.0, W.P->hh, tmp));
        BK_TRY(W.P->apply(tmp, prhs));
        BK_TRY(gmres_core(ctx, &W, prhs, nullptr, y(), nullptr, 0.0, 1.0, ls, r));
        solves += 1;
        inner_its += r->niter;
        if (!r->converged) failed += 1;                      // counted, not fatal
        return 0;
    }
    int apply(const double* x, const double*, double a0, double a1, double* out, double*) override {
        if (out == x) return set_error(ctx, "monodromy operator: out must not alias x");
        GmresResult r;
        BK_TRY(solve(x, &r));
        return v_axpbyz(ctx, n, a0, x, a1, y() + KN() - n, out);
    }
};

}  // namespace
}  // namespace bk

using namespace bk;

extern "C" {

int bk_potrap_ivp_march(bk_potrap* h, const double* u, double T, const double* params, int nparams, const double* y, double* out) {
    if (!h || !u || !params || !y || !out) return -1;
    CglPar par;
    BK_TRY(potrap_params(h, params, nparams, &par));
    if (out == y || out == u) return set_error(h->ctx, "bk_potrap_ivp_march: out must not alias y or u");
    return ivp_march(h, par, u, T, y, out);
}

int bk_precond_potrap_ivp_create(bk_potrap* h, double a, double b, double T, bk_precond** out) {
    if (!h || !out) return -1;
    IvpPrecond* P = nullptr;
    BK_TRY(ivp_precond_create(h, a, b, T, "bk_precond_potrap_ivp_create", &P));
    *out = P;
    return 0;
}

int bk_precond_potrap_ivp_transform_paths(bk_precond* pl, int paths[2]) {
    if (!pl || !paths) return -1;
    IvpPrecond* P = dynamic_cast<IvpPrecond*>(pl);
    if (!P) return set_error(pl->ctx, "bk_precond_potrap_ivp_transform_paths: not a preconditioner of bk_precond_potrap_ivp_create");
    paths[0] = dst_plan_last_path(P->plan, 0);
    paths[1] = dst_plan_last_path(P->plan, 1);
    return 0;
}

int bk_potrap_monodromy_create(bk_potrap* h, const double* u, double T, const double* params, int nparams, double a, double b,
                               const bk_gmres_opts* opts, bk_op** out) {
    if (!h || !u || !params || !opts || !out) return -1;
    bk_ctx* ctx = h->ctx;
    CglPar par;
    BK_TRY(potrap_params(h, params, nparams, &par));
    if (opts->flavor >= BK_KRYLOV_MINRES)
        return set_error(ctx, "bk_potrap_monodromy_create: the initial-value system is not symmetric (use a GMRES flavor)");
    if (opts->pr) return set_error(ctx, "bk_potrap_monodromy_create: left preconditioner only");
    IvpPrecond* P = nullptr;
    BK_TRY(ivp_precond_create(h, a, b, T, "bk_potrap_monodromy_create", &P));
    MonodromyOp* op = new MonodromyOp();
    const size_t N = 2 * h->n;
    op->ctx = ctx; op->n = N; op->ntail = 0;
    op->ls = *opts;
    for (int i = 0; i < nparams && i < BK_MAX_PARAMS; ++i) op->params[i] = params[i];
    op->W.ctx = ctx; op->W.n = N * (size_t)(h->M - 1); op->W.ntail = 0;
    op->W.h = h; op->W.u = u; op->W.T = T; op->W.par = par; op->W.P = P;
    if (hipMalloc(&op->work, sizeof(double) * 3 * op->W.n) != hipSuccess) {
        op->work = nullptr;
        delete op;
        return set_error(ctx, "bk_potrap_monodromy_create: allocation failed");
    }
    op->W.tmp = op->work;
    *out = op;
    return 0;
}

int bk_potrap_monodromy_solve(bk_op* o, const double* x, double* y_all, int* converged, int* niter) {
    if (!o || !x || !y_all) return -1;
    MonodromyOp* op = dynamic_cast<MonodromyOp*>(o);
    if (!op) return set_error(o->ctx, "bk_potrap_monodromy_solve: op is not an operator of bk_potrap_monodromy_create");
    GmresResult r;
    BK_TRY(op->solve(x, &r));
    BK_TRY(v_copy(op->ctx, op->KN(), op->y(), y_all));
    if (converged) *converged = r.converged;
    if (niter) *niter = r.niter;
    return 0;
}

int bk_potrap_monodromy_stats(bk_op* o, int* solves, int* failed, int* inner_its, int paths[2]) {
    if (!o) return -1;
    MonodromyOp* op = dynamic_cast<MonodromyOp*>(o);
    if (!op) return set_error(o->ctx, "bk_potrap_monodromy_stats: op is not an operator of bk_potrap_monodromy_create");
    if (solves) *solves = op->solves;
    if (failed) *failed = op->failed;
    if (inner_its) *inner_its = op->inner_its;
    if (paths) {
        paths[0] = dst_plan_last_path(op->W.P->plan, 0);
        paths[1] = dst_plan_last_path(op->W.P->plan, 1);
    }
    return 0;
}

}  // extern "C"
