// Periodic orbits by the trapezoid rule, matrix-free, for BK_PDE_CGL2D on one rank: the functional Trapeze of
// src/periodicorbit/PeriodicOrbitTrapeze.jl (po_residual! :249-269, po_residual_bare! :272-287, po_jvp! :294-330, Jc :362-386,
// updatesection! :665-681) as it is used in the second half of examples/cGL2d.jl (:166-260), and a space-time spectral
// preconditioner in the place of the example's ILU of the assembled Jacobian (:209-213).
//
// Orbit vector (:139-142): M slices of N = 2 n doubles on the device, slice i = [u1; u2] at u + i N, and ONE host tail scalar T.
// With K = M - 1, prev(0) = K - 1, prev(i) = i - 1 and F the cGL vector field:
//
//     G_i = u_i - u_prev(i) - (h / 2) (F(u_i) + F(u_prev(i))),   i < K          h = T (1 / M)
//     G_K = u_K - u_0                                            the closure
//     G_T = <u, phi> - <xpi, phi>                                the phase condition over all M slices
//
//     dG_i = du_i - du_prev(i) - (h / 2) (J_i du_i + J_prev(i) du_prev(i)) - (dT / M / 2) (F(u_i) + F(u_prev(i)))
//     dG_K = du_K - du_0,     dG_T = <du, phi>
//
// THE TIME STEP: h = T / M on each of the M - 1 intervals -- get_time_step of an integer TimeMesh is 1 / M (src/TimeMesh.jl:21)
// while the cyclic system has M - 1 intervals.  The quirk is kept: the entry called T is M / (M - 1) times the orbit's period,
// and every guess and result of the reference is in this convention.
//
// Kernels.  potrap_march_kernel<JVP> marches in time per spatial tile: a workgroup owns 256 grid points and a chunk of
// consecutive rows, evaluates every slice's stencil once, carries F(u_prev) (JVP: J_prev du_prev too) and the centre values of
// the previous slice in registers, and forms the phase dot in the same pass (block_sum_store / reduce_finish: fixed order,
// bitwise run to run).  Nothing but the result is written.  A chunk evaluates the slice before its first row once more
// (cost (C + 1) / C); the chunk length C comes from potrap_chunking.  The pointwise terms are those of cgl_pw.h, the one copy
// the stencil kernel uses.  potrap_timesolve_kernel is the middle of the preconditioner: per sine mode the cyclic bidiagonal
// system in time, solved exactly by one recurrence (below, PoTrapPrecond).
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

struct PoK {
    int nx, ny, M;
    int C;                         // rows per chunk
    unsigned ntiles;
    double ax, ay;
    CglPar par;
    double hh;                     // h / 2 = T / M / 2
    double dh;                     // JVP: dT / M / 2
    const double* u;
    const double* du;              // JVP only
    const double* phi;
    double* out;
};

// Grid: blockIdx.x = chunk * ntiles + tile.  Rows [r0, r1) of the K = M - 1 cyclic rows; the walk starts one slice earlier
// (t = -1: the predecessor of row r0, evaluated by the same code as every other slice and not stored, so a row's bits do not
// depend on the chunking); the last chunk also writes the closure row.  One partial sum of the phase dot per workgroup.
template <bool JVP>
__global__ void __launch_bounds__(kThreads) potrap_march_kernel(PoK P, double* __restrict__ partials) {
    const size_t n = (size_t)P.nx * P.ny, N = 2 * n;
    const unsigned tile = blockIdx.x % P.ntiles, chunk = blockIdx.x / P.ntiles;
    const size_t idx = (size_t)tile * kThreads + threadIdx.x;
    const int K = P.M - 1;
    const int r0 = (int)chunk * P.C, r1 = min(K, r0 + P.C);
    double s[1] = {0.0};
    if (idx < n) {
        const int i = (int)(idx % P.nx), j = (int)(idx / P.nx);
        double Fp1 = 0.0, Fp2 = 0.0, Jp1 = 0.0, Jp2 = 0.0, cp1 = 0.0, cp2 = 0.0;
        for (int t = -1; t < r1 - r0; ++t) {
            const int row = r0 + t;
            const size_t sl = (size_t)(row < 0 ? K - 1 : row) * N;
            const PoPoint q = po_load(P, P.u + sl, n, idx, i, j);
            double n1, n2;
            cgl_nl(P.par, q.c1, q.c2, n1, n2);
            const double F1 = q.d1 + n1, F2 = q.d2 + n2;
            double J1 = 0.0, J2 = 0.0, x1 = q.c1, x2 = q.c2;
            if (JVP) {
                const PoPoint v = po_load(P, P.du + sl, n, idx, i, j);
                double f1u, f1v, f2u, f2v;
                cgl_jac(P.par, q.c1, q.c2, f1u, f1v, f2u, f2v);
                J1 = v.d1 + f1u * v.c1 + f1v * v.c2;
                J2 = v.d2 + f2u * v.c1 + f2v * v.c2;
                x1 = v.c1;
                x2 = v.c2;
            }
            if (t >= 0) {
                double o1, o2;
                if (JVP) {
                    o1 = ((x1 - cp1) - P.hh * (J1 + Jp1)) - P.dh * (F1 + Fp1);
                    o2 = ((x2 - cp2) - P.hh * (J2 + Jp2)) - P.dh * (F2 + Fp2);
                } else {
                    o1 = (x1 - cp1) - P.hh * (F1 + Fp1);
                    o2 = (x2 - cp2) - P.hh * (F2 + Fp2);
                }
                P.out[sl + idx] = o1;
                P.out[sl + idx + n] = o2;
                s[0] = fma(P.phi[sl + idx], x1, s[0]);
                s[0] = fma(P.phi[sl + idx + n], x2, s[0]);
            }
            Fp1 = F1; Fp2 = F2; Jp1 = J1; Jp2 = J2; cp1 = x1; cp2 = x2;
        }
        if (r1 == K) {
            // the closure row and the last slice's share of the phase dot
            const double* x = JVP ? P.du : P.u;
            const size_t sl = (size_t)K * N;
            const double a1 = x[sl + idx], a2 = x[sl + idx + n];
            P.out[sl + idx] = a1 - x[idx];
            P.out[sl + idx + n] = a2 - x[idx + n];
            s[0] = fma(P.phi[sl + idx], a1, s[0]);
            s[0] = fma(P.phi[sl + idx + n], a2, s[0]);
        }
    }
    block_sum_store<1>(s, partials);
}

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

// The time solve of the preconditioner, one thread per sine mode k and w = u1^ + i u2^: with mu = a + lam_k + i b,
// alpha = 1 - (h / 2) mu, beta = 1 + (h / 2) mu, rho = beta / alpha, the rows i < K read alpha w_i - beta w_prev(i) = f_i, i.e.
//     w_i = rho w_prev(i) + f_i / alpha        cyclic in i
// First walk: acc <- rho acc + f_i / alpha over the K slices, rho^K accumulated alongside; w_{K-1} = acc / (1 - rho^K).  Second
// walk: the recurrence itself, written out in place.  Closure: w_K = f_K + w_0.  Two reads and one write of the spectrum,
// coalesced across modes.
struct PoTs {
    int nx, ny, M;
    double a, b, hh;
    const double* lx;
    const double* ly;
    double* spec;
};
__global__ void __launch_bounds__(kThreads) potrap_timesolve_kernel(PoTs P) {
    const size_t n = (size_t)P.nx * P.ny, N = 2 * n;
    const size_t k = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (k >= n) return;
    const int K = P.M - 1;
    const double mr = P.a + (P.lx[k % P.nx] + P.ly[k / P.nx]), mi = P.b;
    const Cx alpha{1.0 - P.hh * mr, -P.hh * mi}, beta{1.0 + P.hh * mr, P.hh * mi};
    const double ia = 1.0 / (alpha.r * alpha.r + alpha.i * alpha.i);
    const Cx inva{alpha.r * ia, -alpha.i * ia};
    const Cx rho = beta * inva;
    Cx acc{0.0, 0.0}, rk{1.0, 0.0};
    for (int i = 0; i < K; ++i) {
        const Cx f{P.spec[(size_t)i * N + k], P.spec[(size_t)i * N + n + k]};
        acc = rho * acc + f * inva;
        rk = rk * rho;
    }
    const Cx den{1.0 - rk.r, -rk.i};
    const double id = 1.0 / (den.r * den.r + den.i * den.i);
    Cx w = acc * Cx{den.r * id, -den.i * id};
    Cx w0{0.0, 0.0};
    for (int i = 0; i < K; ++i) {
        const Cx f{P.spec[(size_t)i * N + k], P.spec[(size_t)i * N + n + k]};
        w = rho * w + f * inva;
        P.spec[(size_t)i * N + k] = w.r;
        P.spec[(size_t)i * N + n + k] = w.i;
        if (i == 0) w0 = w;
    }
    P.spec[(size_t)K * N + k] += w0.r;
    P.spec[(size_t)K * N + n + k] += w0.i;
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

namespace {

// the marching pass: out and the phase dot <x, phi> (x = u, or du for the JVP); algorithmic bytes: u (and du) read, out written,
// phi read
int potrap_march(bk_potrap* h, const CglPar& par, const double* u, double T, const double* du, double dT, double* out, double* dot) {
    bk_ctx* ctx = h->ctx;
    const bk_problem_desc& d = h->prob->desc;
    PoK P{d.n[0], d.n[1], h->M, 1, 1u, h->prob->ainv[0], h->prob->ainv[1], par, T * (1.0 / h->M) / 2.0, dT / h->M / 2.0,
          u, du, h->phi, out};
    int nchunks = 1;
    BK_TRY(potrap_chunking(ctx, h->n, h->M, &P.ntiles, &P.C, &nchunks));
    const unsigned grid = P.ntiles * (unsigned)nchunks;
    {
        ProfScope ps(ctx, du ? "potrap_jvp" : "potrap_residual", 8.0 * h->len() * (du ? 4 : 3));
        if (du) hipLaunchKernelGGL(potrap_march_kernel<true>, dim3(grid), dim3(kThreads), 0, ctx->stream, P, ctx->d_partials);
        else hipLaunchKernelGGL(potrap_march_kernel<false>, dim3(grid), dim3(kThreads), 0, ctx->stream, P, ctx->d_partials);
        BK_HIP(ctx, hipGetLastError());
    }
    BK_TRY(reduce_finish(ctx, (int)grid, 1, 0));
    *dot = ctx->h_red[0];
    return 0;
}

int potrap_check(bk_potrap* h, const char* who, bool need_section) {
    if (need_section && !h->has_section)
        return set_error(h->ctx, "%s: no section set (bk_potrap_set_section or bk_potrap_update_section first)", who);
    return 0;
}

// dG(u, T), or its transpose (adjoint: the pass of pofold.hip), as an operator on (device vector of M N doubles, host tail dT);
// references u
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

// P = diag(A0, 1): A0 = the cyclic-plus-closure matrix above with every J_i replaced by L0 = Lap (x) I_2 + [[a, -b], [b, a]], the
// operator bk_precond_cgl_create inverts.  The DST-I of all 2 M fields in one batched plan diagonalises the Laplacian; per mode
// what is left is the scalar complex system potrap_timesolve_kernel solves.  adjoint: diag(A0^T, 1) -- the DST-I is symmetric, so
// only the time solve differs (pofold.hip).
struct PoTrapPrecond : bk_precond {
    DctPlan* plan = nullptr;
    int nx = 0, ny = 0, M = 0;
    double a = 0.0, b = 0.0, hh = 0.0;
    bool period_set = false;
    bool adjoint = false;
    std::vector<double> lx, ly;    // host copies of the eigenvalue tables (the guards of set_period)
    ~PoTrapPrecond() override { dct_plan_destroy(plan); }
    int apply(const double* v, double* out) override {
        if (!period_set) return set_error(ctx, "potrap preconditioner: no period set (bk_precond_potrap_set_period first)");
        double* spec = dst_plan_scratch(plan);
        BK_TRY(dst_transform(ctx, plan, 0, v, spec));
        if (adjoint) {
            BK_TRY(potrap_adjoint_timesolve(ctx, nx, ny, M, a, b, hh, dst_plan_lam(plan, 0), dst_plan_lam(plan, 1), spec));
        } else {
            const size_t npts = (size_t)nx * ny;
            ProfScope ps(ctx, "potrap_timesolve", 8.0 * n * 3);
            const PoTs P{nx, ny, M, a, b, hh, dst_plan_lam(plan, 0), dst_plan_lam(plan, 1), spec};
            hipLaunchKernelGGL(potrap_timesolve_kernel, dim3((unsigned)((npts + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                               ctx->stream, P);
            BK_HIP(ctx, hipGetLastError());
        }
        return dst_transform(ctx, plan, 1, spec, out);
    }
};

// diag(A0^-1, 1) dG: the operator of the left-preconditioned solve
struct PoTrapPrecOp : bk_op {
    bk_op* A = nullptr;
    bk_precond* P = nullptr;
    double* tmp = nullptr;
    int apply(const double* x, const double* xt, double a0, double a1, double* out, double* outt) override {
        double tt = 0.0;
        BK_TRY(A->apply(x, xt, 0.0, 1.0, tmp, &tt));
        BK_TRY(P->apply(tmp, out));
        if (!(a0 == 0.0 && a1 == 1.0)) BK_TRY(v_axpby(ctx, n, a0, x, a1, out));
        outt[0] = a0 * xt[0] + a1 * tt;
        return 0;
    }
};

}  // namespace

int potrap_pair_check(bk_ctx* ctx, const char* who, bk_op* op, bk_precond* pl) {
    PoTrapOp* pop = dynamic_cast<PoTrapOp*>(op);
    if (!pop) return set_error(ctx, "%s: op is not an operator of bk_potrap_op_create", who);
    PoTrapPrecond* ppl = dynamic_cast<PoTrapPrecond*>(pl);
    if (!ppl || pl->n != op->n) return set_error(ctx, "%s: pl is not a preconditioner of bk_precond_potrap_create for this orbit", who);
    if (pop->adjoint != ppl->adjoint)
        return set_error(ctx, "%s: %s operator with %s preconditioner (pair bk_potrap_op_adjoint_create with "
                              "bk_precond_potrap_adjoint_create)", who, pop->adjoint ? "an adjoint" : "a forward",
                         ppl->adjoint ? "an adjoint" : "a forward");
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
    BK_TRY(potrap_check(h, "bk_potrap_get_section", true));
    if (phi == xpi) return set_error(h->ctx, "bk_potrap_get_section: phi and xpi must be distinct");
    BK_TRY(v_copy(h->ctx, h->len(), h->phi, phi));
    return v_copy(h->ctx, h->len(), h->xpi, xpi);
}

int bk_potrap_residual(bk_potrap* h, const double* u, double T, const double* params, int nparams, double* out, double* out_tail) {
    if (!h || !u || !params || !out || !out_tail) return -1;
    CglPar par;
    BK_TRY(potrap_params(h, params, nparams, &par));
    BK_TRY(potrap_check(h, "bk_potrap_residual", true));
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
    BK_TRY(potrap_check(h, "bk_potrap_jvp", true));
    if (out == u || out == du || out == h->phi || out == h->xpi)
        return set_error(h->ctx, "bk_potrap_jvp: out must not alias u, du or the section");
    return potrap_march(h, par, u, T, du, dT, out, out_tail);
}

static int potrap_op_create(bk_potrap* h, const double* u, double T, const double* params, int nparams, bool adjoint, bk_op** out) {
    if (!h || !u || !params || !out) return -1;
    CglPar par;
    BK_TRY(potrap_params(h, params, nparams, &par));
    BK_TRY(potrap_check(h, adjoint ? "bk_potrap_op_adjoint_create" : "bk_potrap_op_create", true));
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

static int potrap_precond_create(bk_potrap* h, double a, double b, bool adjoint, bk_precond** out) {
    if (!h || !out) return -1;
    bk_ctx* ctx = h->ctx;
    PoTrapPrecond* P = new PoTrapPrecond();
    P->ctx = ctx; P->n = h->len(); P->adjoint = adjoint;
    P->nx = h->prob->desc.n[0]; P->ny = h->prob->desc.n[1]; P->M = h->M; P->a = a; P->b = b;
    const int s = dst_plan_create(ctx, h->prob->desc.n, h->prob->ainv, 0.0, 2 * h->M, &P->plan);
    if (s != 0) { delete P; return s; }
    P->lx.resize(P->nx);
    P->ly.resize(P->ny);
    if (hipMemcpy(P->lx.data(), dst_plan_lam(P->plan, 0), sizeof(double) * P->nx, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(P->ly.data(), dst_plan_lam(P->plan, 1), sizeof(double) * P->ny, hipMemcpyDeviceToHost) != hipSuccess) {
        delete P;
        return set_error(ctx, "bk_precond_potrap_create: reading the eigenvalue tables failed");
    }
    *out = P;
    return 0;
}

int bk_precond_potrap_create(bk_potrap* h, double a, double b, bk_precond** out) { return potrap_precond_create(h, a, b, false, out); }

int bk_precond_potrap_adjoint_create(bk_potrap* h, double a, double b, bk_precond** out) {
    return potrap_precond_create(h, a, b, true, out);
}

int bk_precond_potrap_set_period(bk_precond* pl, double T) {
    if (!pl) return -1;
    PoTrapPrecond* P = dynamic_cast<PoTrapPrecond*>(pl);
    if (!P) return set_error(pl->ctx, "bk_precond_potrap_set_period: not a preconditioner of bk_precond_potrap_create");
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
            if (!(aa >= kPoPivot)) continue;
            const std::complex<double> rho = beta / alpha;
            std::complex<double> rk(1.0, 0.0);
            for (int q = 0; q < K; ++q) rk *= rho;
            const double dd = std::abs(1.0 - rk);
            if (!(dd >= min_d)) { min_d = dd; kd[0] = i; kd[1] = j; }
        }
    if (!(min_a >= kPoPivot))
        return set_error(P->ctx, "bk_precond_potrap_set_period: |alpha| = |1 - (h/2) mu| = %.3g below %.0e at sine mode (%d, %d): "
                                 "move a (or T) away from it", min_a, kPoPivot, ka[0] + 1, ka[1] + 1);
    if (!(min_d >= kPoPivot))
        return set_error(P->ctx, "bk_precond_potrap_set_period: |1 - rho^K| = %.3g below %.0e at sine mode (%d, %d): the mode is "
                                 "Hopf-critical for (a, b) = (%.17g, %.17g) at this period; move a away from it",
                         min_d, kPoPivot, kd[0] + 1, kd[1] + 1, P->a, P->b);
    P->hh = hh;
    P->period_set = true;
    return 0;
}

int bk_precond_potrap_transform_paths(bk_precond* pl, int paths[2]) {
    if (!pl || !paths) return -1;
    PoTrapPrecond* P = dynamic_cast<PoTrapPrecond*>(pl);
    if (!P) return set_error(pl->ctx, "bk_precond_potrap_transform_paths: not a preconditioner of bk_precond_potrap_create");
    paths[0] = dst_plan_last_path(P->plan, 0);
    paths[1] = dst_plan_last_path(P->plan, 1);
    return 0;
}

int bk_potrap_solve(bk_ctx* ctx, bk_op* op, bk_precond* pl, const double* rhs, double rhs_tail, double* x, double* x_tail,
                    const bk_gmres_opts* opts, bk_solve_result* result) {
    if (!ctx || !op || !pl || !rhs || !x || !x_tail || !opts || !result) return -1;
    BK_TRY(potrap_pair_check(ctx, "bk_potrap_solve", op, pl));
    if (opts->flavor >= BK_KRYLOV_MINRES) return set_error(ctx, "bk_potrap_solve: the orbit Jacobian is not symmetric (use a GMRES flavor)");
    if (opts->pr) return set_error(ctx, "bk_potrap_solve: left preconditioner only");
    if (x == rhs) return set_error(ctx, "bk_potrap_solve: x must not alias rhs");
    WsGuard ws(ctx);
    double *tmp = nullptr, *prhs = nullptr;
    BK_TRY(ws.get(op->n, &tmp));
    BK_TRY(ws.get(op->n, &prhs));
    PoTrapPrecOp W;
    W.ctx = ctx; W.n = op->n; W.ntail = 1;
    W.A = op; W.P = pl; W.tmp = tmp;
    BK_TRY(pl->apply(rhs, prhs));                 // the top of the right-hand side; the tail is untouched
    GmresResult r;
    BK_TRY(gmres_core(ctx, &W, prhs, &rhs_tail, x, x_tail, 0.0, 1.0, *opts, &r));
    result->converged = r.converged;
    result->niter = r.niter;
    result->resnorm = r.resnorm;
    return 0;
}

}  // extern "C"
