// The time-T map of cGL and its tangent by a fixed-step spectral ETDRK2, for BK_PDE_CGL2D on one rank: what
// evolve(flow, x, par, tau) and jvp(flow, x, par, dx, tau) of src/periodicorbit/Flow.jl return for the flow that
// examples/cGL2d-shooting.jl builds from SplitODEProblem(Lap, NL) and ETDRK2 (:108-128).
//
// The split of the example: L = Lap (x) I_2 is treated exactly, N = NL is every pointwise term (cgl_pw.h).  The Dirichlet Laplacian is
// diagonal under the DST-I of the batched plan (dct.hip: dst_plan_create / dst_transform), so with z_k = h lam_k, lam_k = lam_x[i] +
// lam_y[j], and ^ the transform, one step of Cox-Matthews ETDRK2 is
//
//     a^       = e^z u_n^ + h phi1(z) N^(u_n)                       phi1(z) = (e^z - 1) / z
//     u_{n+1}^ = a^ + h phi2(z) (N^(a) - N^(u_n))                   phi2(z) = (e^z - 1 - z) / z^2
//
// and the tangent (v_n, b) of (u_n, a) obeys the same two lines with N^(.) replaced by (J_N(.) .)^: the EXACT derivative of the
// discrete map, h = tau / nsteps with nsteps fixed by the caller.  (The example's krylov = true approximates the phi functions and
// its FiniteDifferencesMF the tangent; both are exact per mode here.)
//
// Kernels: flow_coef_kernel fills the three tables E, h phi1, h phi2 for a step h; flow_pw_kernel<MODE> evaluates N(u) and / or
// J_N(u) du in physical space; flow_stage1_kernel<NS> and flow_stage2_kernel<NS> form the two lines above for NS vector sets (state,
// tangent) with one read of the tables per mode, shared by both fields and all sets.  A step is four batched transforms, two
// pointwise passes and two spectral passes.  All B trajectories of a call advance in lock-step; trajectory i is [u1; u2] at i N.
#include <cmath>

#include "cgl_pw.h"
#include "common.h"
#include "flow.h"
#include "hopf_pw.h"
#include "ops.h"
#include "potrap_pw.h"
#include "stream.h"

namespace bk {

namespace {

// phi2(z) = sum_k z^k / (k + 2)! for |z| < 1 (21 terms: 1 / 22! < eps / 2 of the leading 1 / 2), the closed form from expm1 beyond:
// there (e^z - 1) - z loses less than two bits.  phi1 = expm1(z) / z has no cancellation at any z.  z -> -inf: E = 0, phi1 = -1 / z,
// phi2 = (-1 - z) / z^2, all finite.
__device__ __forceinline__ double flow_phi2(double z, double em1) {
    if (fabs(z) < 1.0) {
        // 2! .. 22!, each exact in a double, so every coefficient 1 / (k + 2)! carries one rounding
        constexpr double fact[21] = {2.0, 6.0, 24.0, 120.0, 720.0, 5040.0, 40320.0, 362880.0, 3628800.0, 39916800.0, 479001600.0,
                                     6227020800.0, 87178291200.0, 1307674368000.0, 20922789888000.0, 355687428096000.0,
                                     6402373705728000.0, 121645100408832000.0, 2432902008176640000.0, 51090942171709440000.0,
                                     1124000727777607680000.0};
        double s = 1.0 / fact[20];
#pragma unroll
        for (int k = 19; k >= 0; --k) s = s * z + 1.0 / fact[k];
        return s;
    }
    return (em1 - z) / (z * z);
}

__global__ void __launch_bounds__(kThreads) flow_coef_kernel(int nx, int ny, double h, const double* __restrict__ lx,
                                                              const double* __restrict__ ly, double* __restrict__ tab) {
    const size_t n = (size_t)nx * ny;
    const size_t k = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (k >= n) return;
    const double z = h * (lx[k % nx] + ly[k / nx]);
    const double em1 = expm1(z);
    const double p1 = z == 0.0 ? 1.0 : em1 / z;
    tab[k] = exp(z);
    tab[n + k] = h * p1;
    tab[2 * n + k] = h * flow_phi2(z, em1);
}

// J_N(u) d at one grid point: the one copy every mode evaluates
__device__ __forceinline__ void flow_jn(const CglPar& par, double u1, double u2, double d1, double d2, double& j1, double& j2) {
    double f1u, f1v, f2u, f2v;
    cgl_jac(par, u1, u2, f1u, f1v, f2u, f2v);
    j1 = f1u * d1 + f1v * d2;
    j2 = f2u * d1 + f2v * d2;
}

// Grid (tiles of the n points, B): blockIdx.y is the trajectory, so no lane divides.  u, du, nu, jdu: B trajectories [f1; f2] each.
// kFlowBase: nu = N(u); kFlowTangent: jdu = J_N(u) du; kFlowBoth: both.
template <int MODE>
__global__ void __launch_bounds__(kThreads) flow_pw_kernel(CglPar par, size_t n, const double* __restrict__ u,
                                                            const double* __restrict__ du, double* __restrict__ nu,
                                                            double* __restrict__ jdu) {
    const size_t base = (size_t)blockIdx.y * 2 * n;
    for (size_t k = (size_t)blockIdx.x * kThreads + threadIdx.x; k < n; k += (size_t)gridDim.x * kThreads) {
        const size_t i = base + k;
        const double u1 = u[i], u2 = u[i + n];
        if (MODE != kFlowTangent) {
            double n1, n2;
            cgl_nl(par, u1, u2, n1, n2);
            nu[i] = n1;
            nu[i + n] = n2;
        }
        if (MODE != kFlowBase) {
            double j1, j2;
            flow_jn(par, u1, u2, du[i], du[i + n], j1, j2);
            jdu[i] = j1;
            jdu[i + n] = j2;
        }
    }
}

// a^ = E x^ + (h phi1) n^ on NS sets of B trajectories (set s at s * set): one thread per (trajectory = blockIdx.y, mode), both fields
template <int NS>
__global__ void __launch_bounds__(kThreads) flow_stage1_kernel(size_t n, size_t set, const double* __restrict__ tab,
                                                                const double* __restrict__ xh, const double* __restrict__ nh,
                                                                double* __restrict__ ah) {
    const size_t base = (size_t)blockIdx.y * 2 * n;
    for (size_t k = (size_t)blockIdx.x * kThreads + threadIdx.x; k < n; k += (size_t)gridDim.x * kThreads) {
        const size_t i = base + k;
        const double E = tab[k], P1 = tab[n + k];
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
            for (int f = 0; f < 2; ++f) {
                const size_t j = s * set + i + f * n;
                ah[j] = E * xh[j] + P1 * nh[j];
            }
    }
}

// x^ = a^ + (h phi2) (na^ - n^)
template <int NS>
__global__ void __launch_bounds__(kThreads) flow_stage2_kernel(size_t n, size_t set, const double* __restrict__ tab,
                                                                const double* __restrict__ ah, const double* __restrict__ nah,
                                                                const double* __restrict__ nh, double* __restrict__ xh) {
    const size_t base = (size_t)blockIdx.y * 2 * n;
    for (size_t k = (size_t)blockIdx.x * kThreads + threadIdx.x; k < n; k += (size_t)gridDim.x * kThreads) {
        const size_t i = base + k;
        const double P2 = tab[2 * n + k];
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
            for (int f = 0; f < 2; ++f) {
                const size_t j = s * set + i + f * n;
                xh[j] = ah[j] + P2 * (nah[j] - nh[j]);
            }
    }
}

int flow_tables(bk_flow* f, double h) {
    if (f->tab_set && f->tab_h == h) return 0;
    bk_ctx* ctx = f->ctx;
    ProfScope ps(ctx, "flow_coef", 8.0 * f->n * 3);
    hipLaunchKernelGGL(flow_coef_kernel, dim3((unsigned)((f->n + kThreads - 1) / kThreads)), dim3(kThreads), 0, ctx->stream, f->nx, f->ny,
                       h, dst_plan_lam(f->plan1, 0), dst_plan_lam(f->plan1, 1), f->tab);
    BK_HIP(ctx, hipGetLastError());
    f->tab_h = h;
    f->tab_set = true;
    f->launches += 1;
    return 0;
}

}  // namespace

int flow_params(bk_problem* prob, const double* params, int nparams, CglPar* par) {
    CglCoef c;
    BK_TRY(hopf_coef(prob, params, nparams, 0, &c));          // the problem kind and parameter count, as the Hopf entries check them
    *par = CglPar{params[0], params[1], params[2], params[3], params[4], params[5]};
    return 0;
}

void flow_destroy(bk_flow* f) {
    if (!f) return;
    if (f->plan1) dct_plan_destroy(f->plan1);
    if (f->plan2) dct_plan_destroy(f->plan2);
    if (f->tab) (void)hipFree(f->tab);
    if (f->work) (void)hipFree(f->work);
    delete f;
}

int flow_create(bk_problem* prob, int B, const char* who, bk_flow** out) {
    bk_ctx* ctx = prob->ctx;
    // the rank count first: a BK_PDE_CGL2D problem does not exist on more than one rank, so the problem kind would hide this answer
    if (ctx->nranks > 1) return set_error(ctx, "%s: the spectral flow runs on a single rank", who);
    const double zero[6] = {0, 0, 0, 0, 0, 0};
    CglPar par;
    BK_TRY(flow_params(prob, zero, 6, &par));
    if (B < 1 || B > 65535) return set_error(ctx, "%s: 1 to 65535 trajectories (got %d): the trajectory is the second grid index", who, B);
    bk_flow* f = new bk_flow();
    f->ctx = ctx; f->prob = prob; f->B = B; f->nx = prob->desc.n[0]; f->ny = prob->desc.n[1]; f->n = prob->nloc / 2;
    int s = dst_plan_create(ctx, prob->desc.n, prob->ainv, 0.0, 2 * B, &f->plan1);
    if (s != 0) { f->plan1 = nullptr; flow_destroy(f); return s; }
    if (hipMalloc(&f->tab, sizeof(double) * 3 * f->n) != hipSuccess || hipMalloc(&f->work, sizeof(double) * 12 * f->len()) != hipSuccess) {
        flow_destroy(f);
        return set_error(ctx, "%s: allocation failed", who);
    }
    *out = f;
    return 0;
}

int flow_march(bk_flow* f, FlowMode mode, const CglPar& par, const double* x, const double* dx, double tau, int nsteps, double* out,
               double* dout, double* store_u, double* store_a, const double* base_u, const double* base_a, size_t base_stride) {
    bk_ctx* ctx = f->ctx;
    const size_t n = f->n, BN = f->len(), S = 2 * BN, bs = base_stride ? base_stride : BN;
    const int NS = mode == kFlowBoth ? 2 : 1;
    if (NS == 2 && !f->plan2) BK_TRY(dst_plan_create(ctx, f->prob->desc.n, f->prob->ainv, 0.0, 4 * f->B, &f->plan2));
    DctPlan* plan = NS == 2 ? f->plan2 : f->plan1;
    f->last = plan;
    BK_TRY(flow_tables(f, tau / nsteps));
    double *X = f->work, *Xh = X + S, *Nh = X + 2 * S, *Ah = X + 3 * S, *A = X + 4 * S, *Nah = X + 5 * S;
    const dim3 grid((unsigned)grid_for(n, 1, 4096), (unsigned)f->B), block(kThreads);
    auto pw = [&](const double* u, const double* du, double* dst) -> int {
        ProfScope ps(ctx, mode == kFlowTangent ? "flow_pw_tangent" : "flow_pw", 8.0 * BN * (mode == kFlowBoth ? 4 : (mode == kFlowBase ? 2 : 3)));
        if (mode == kFlowBase) hipLaunchKernelGGL(flow_pw_kernel<kFlowBase>, grid, block, 0, ctx->stream, par, n, u, du, dst, dst);
        else if (mode == kFlowBoth) hipLaunchKernelGGL(flow_pw_kernel<kFlowBoth>, grid, block, 0, ctx->stream, par, n, u, du, dst, dst + BN);
        else hipLaunchKernelGGL(flow_pw_kernel<kFlowTangent>, grid, block, 0, ctx->stream, par, n, u, du, dst, dst);
        BK_HIP(ctx, hipGetLastError());
        return 0;
    };
    auto tr = [&](const double* in, double* o) -> int { return dst_transform(ctx, plan, 0, in, o); };
    const double* cur;                                     // the current vectors in physical space, NS sets
    if (mode == kFlowBoth) {
        BK_TRY(v_copy(ctx, BN, x, X));
        BK_TRY(v_copy(ctx, BN, dx, X + BN));
        cur = X;
    } else if (mode == kFlowBase) {
        if (store_u) BK_TRY(v_copy(ctx, BN, x, store_u));
        cur = store_u ? store_u : x;
    } else {
        cur = dx;
    }
    BK_TRY(tr(cur, Xh));
    for (int s = 0; s < nsteps; ++s) {
        const bool last = s + 1 == nsteps;
        BK_TRY(pw(mode == kFlowTangent ? base_u + (size_t)s * bs : cur, mode == kFlowBoth ? cur + BN : cur, Nh));
        BK_TRY(tr(Nh, Nh));
        {
            ProfScope ps(ctx, "flow_stage1", 8.0 * NS * BN * 3);
            if (NS == 2) hipLaunchKernelGGL(flow_stage1_kernel<2>, grid, block, 0, ctx->stream, n, BN, f->tab, Xh, Nh, Ah);
            else hipLaunchKernelGGL(flow_stage1_kernel<1>, grid, block, 0, ctx->stream, n, BN, f->tab, Xh, Nh, Ah);
            BK_HIP(ctx, hipGetLastError());
        }
        double* Ap = mode == kFlowBase && store_a ? store_a + (size_t)s * BN : A;
        BK_TRY(tr(Ah, Ap));
        BK_TRY(pw(mode == kFlowTangent ? base_a + (size_t)s * bs : Ap, mode == kFlowBoth ? Ap + BN : Ap, Nah));
        BK_TRY(tr(Nah, Nah));
        {
            ProfScope ps(ctx, "flow_stage2", 8.0 * NS * BN * 4);
            if (NS == 2) hipLaunchKernelGGL(flow_stage2_kernel<2>, grid, block, 0, ctx->stream, n, BN, f->tab, Ah, Nah, Nh, Xh);
            else hipLaunchKernelGGL(flow_stage2_kernel<1>, grid, block, 0, ctx->stream, n, BN, f->tab, Ah, Nah, Nh, Xh);
            BK_HIP(ctx, hipGetLastError());
        }
        double* nxt = X;
        if (mode == kFlowBase) nxt = last ? out : (store_u ? store_u + (size_t)(s + 1) * BN : X);
        if (mode == kFlowTangent && last) nxt = dout;
        BK_TRY(tr(Xh, nxt));
        cur = nxt;
    }
    if (mode == kFlowBoth) {
        BK_TRY(v_copy(ctx, BN, X, out));
        BK_TRY(v_copy(ctx, BN, X + BN, dout));
    }
    if (mode != kFlowTangent) f->base_marches += 1;
    f->launches += 12LL * nsteps + 2 + (mode == kFlowBoth ? 4 : (mode == kFlowBase && store_u ? 1 : 0));
    return 0;
}

}  // namespace bk

using namespace bk;

extern "C" {

int bk_flow_create(bk_problem* prob, int B, bk_flow** out) {
    if (!prob || !out) return -1;
    return flow_create(prob, B, "bk_flow_create", out);
}

int bk_flow_destroy(bk_flow* f) {
    flow_destroy(f);
    return 0;
}

static int flow_args_check(bk_flow* f, const char* who, double tau, int nsteps) {
    if (nsteps < 1) return set_error(f->ctx, "%s: nsteps >= 1 (got %d)", who, nsteps);
    if (!std::isfinite(tau)) return set_error(f->ctx, "%s: tau must be finite", who);
    return 0;
}

int bk_flow_evolve(bk_flow* f, const double* x, double tau, int nsteps, const double* params, int nparams, double* out) {
    if (!f || !x || !params || !out) return -1;
    CglPar par;
    BK_TRY(flow_params(f->prob, params, nparams, &par));
    BK_TRY(flow_args_check(f, "bk_flow_evolve", tau, nsteps));
    if (out == x) return set_error(f->ctx, "bk_flow_evolve: out must not alias x");
    return flow_march(f, kFlowBase, par, x, nullptr, tau, nsteps, out, nullptr, nullptr, nullptr, nullptr, nullptr);
}

int bk_flow_jvp(bk_flow* f, const double* x, const double* dx, double tau, int nsteps, const double* params, int nparams, double* out,
                double* dout) {
    if (!f || !x || !dx || !params || !out || !dout) return -1;
    CglPar par;
    BK_TRY(flow_params(f->prob, params, nparams, &par));
    BK_TRY(flow_args_check(f, "bk_flow_jvp", tau, nsteps));
    if (out == x || out == dx) return set_error(f->ctx, "bk_flow_jvp: out must not alias x or dx");
    if (dout == x || dout == dx || dout == out) return set_error(f->ctx, "bk_flow_jvp: dout must not alias x, dx or out");
    return flow_march(f, kFlowBoth, par, x, dx, tau, nsteps, out, dout, nullptr, nullptr, nullptr, nullptr);
}

int bk_flow_coefficients(bk_flow* f, double h, double* E, double* P1, double* P2) {
    if (!f || !E || !P1 || !P2) return -1;
    bk_ctx* ctx = f->ctx;
    if (!std::isfinite(h)) return set_error(ctx, "bk_flow_coefficients: h must be finite");
    BK_TRY(flow_tables(f, h));
    BK_TRY(ctx_sync(ctx));
    double* dst[3] = {E, P1, P2};
    for (int t = 0; t < 3; ++t) BK_HIP(ctx, hipMemcpy(dst[t], f->tab + (size_t)t * f->n, sizeof(double) * f->n, hipMemcpyDeviceToHost));
    return 0;
}

int bk_flow_transform_paths(bk_flow* f, int paths[2]) {
    if (!f || !paths) return -1;
    dst_plan_paths(f->last ? f->last : f->plan1, paths);
    return 0;
}

int bk_flow_stats(bk_flow* f, long long* base_marches, long long* launches) {
    if (!f) return -1;
    if (base_marches) *base_marches = f->base_marches;
    if (launches) *launches = f->launches;
    return 0;
}

}  // extern "C"
