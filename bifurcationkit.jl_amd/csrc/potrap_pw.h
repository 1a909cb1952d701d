// What potrap.hip (the trapezoid periodic-orbit functional in both directions and its preconditioner), pofold.hip (the fold of limit
// cycles) and floquet.hip (the monodromy's initial-value system) share: the handle, one slice's stencil load, the skeleton of the
// marching passes, the preconditioned operator wrapper and the declarations that cross files.  The pointwise Jacobian block
// (cgl_jac) is in cgl_pw.h.
//
// The marching skeleton.  A workgroup owns 256 grid points (a tile) and a chunk of consecutive rows [r0, r1) of the K = M - 1 rows,
// blockIdx.x = chunk * ntiles + tile; the chunk length C comes from potrap_chunking.  It walks t = first .. r1 - r0 - 1 with one
// slice carried in registers; the warm-up step t = -1 runs through the same code as every other step and stores nothing, so a
// row's bits do not depend on the chunking (cost (C + 1) / C).  The last chunk also writes the closure row, and each workgroup
// leaves one record of NV partial sums (block_sum_store / reduce_finish: fixed order, bitwise run to run for one chunk count).
//
// How to add a marching pass: write a plain struct with its pointers and coefficients, `static constexpr int NV` (the number of
// sums, 0 for none), `static constexpr bool OPEN` (true: row 0 has no predecessor, chunk 0 starts at t = 0 from a zero carry),
// `struct Carry` (what one step hands to the next, zero-initialised) and the mathematics
//   step(at, row, store, c, s)   load the slice this step needs (the pass's own choice: row itself, with prev(-1) = K - 1, on the
//                                forward walks; next(row) on the adjoint walks), complete row `row` from it and the carry -- write
//                                it and add its terms to s only if `store` --, and update the carry
//   closure(at, s)               row K, last chunk only
// Fill it on the host and call po_march(h, who, scope, bytes, pass, sums).  Geometry, tile / chunk / row decoding, the idx < n guard,
// the walk, the scratch bound, the profiling scope and the two-stage sum are the skeleton's.
// Internal header.
#pragma once
#include <vector>

#include "cgl_pw.h"
#include "common.h"
#include "ops.h"
#include "stream.h"

struct bk_potrap {
    bk_ctx* ctx = nullptr;
    bk_problem* prob = nullptr;
    int M = 0;
    size_t n = 0;                  // grid points per field; a slice holds N = 2 n doubles
    double* phi = nullptr;         // [M N] the normals of the section
    double* xpi = nullptr;         // [M N] its reference point
    double c0 = 0.0;               // <xpi, phi>
    bool has_section = false;
    size_t len() const { return 2 * n * (size_t)M; }
};

namespace bk {

constexpr double kPoPivot = 1e-8;      // the project's pivot threshold: a guard, not a tolerance

// potrap.hip
int potrap_chunking(bk_ctx* ctx, size_t n, int M, unsigned* ntiles, int* C, int* nchunks);
int potrap_params(bk_potrap* h, const double* params, int nparams, CglPar* par);
// "who: no section set ..." unless the handle has one
int potrap_check(bk_potrap* h, const char* who);
// "who: ..." unless opts ask for a GMRES flavor and no right preconditioner; what: the system named in the first message
int potrap_opts_check(bk_ctx* ctx, const char* who, const bk_gmres_opts* opts, const char* what = "the orbit Jacobian");
// "who: ..." unless op and pl are an orbit operator and an orbit preconditioner of the same length and the same kind (both
// forward or both adjoint)
int potrap_pair_check(bk_ctx* ctx, const char* who, bk_op* op, bk_precond* pl);

// The space-time preconditioner A0^-1: the DST-I of all `fields` fields in one batched plan diagonalises the Laplacian, per sine
// mode one recurrence in time is left (potrap.hip: po_timesolve_kernel), then the DST-I back.  The cyclic kinds take their period
// from bk_precond_potrap_set_period, the initial-value kind at creation.
enum PoTsKind { kTsCyclic = 0, kTsCyclicAdjoint = 1, kTsIvp = 2 };
struct PoPrecond : bk_precond {
    DctPlan* plan = nullptr;
    PoTsKind kind = kTsCyclic;
    int nx = 0, ny = 0, M = 0;
    int fields = 0;                // 2 M (cyclic: the closure row included) or 2 K (initial value)
    double a = 0.0, b = 0.0, hh = 0.0;
    bool period_set = false;
    std::vector<double> lx, ly;    // host copies of the eigenvalue tables (the guards of po_precond_set_period)
    ~PoPrecond() override { dct_plan_destroy(plan); }
    int apply(const double* v, double* out) override;
};
int po_precond_create(bk_potrap* h, PoTsKind kind, double a, double b, double T, const char* who, PoPrecond** out);
// hh = T (1 / M) / 2 after the guards: "who: |alpha| ..." and, cyclic kinds only, "who: |1 - rho^K| ..."
int po_precond_set_period(PoPrecond* P, double T, const char* who);
// pl as a PoPrecond of the initial-value kind (ivp) or of a cyclic kind (!ivp), else null
PoPrecond* po_precond_cast(bk_precond* pl, bool ivp);
// per axis the kernel the plan's last transform passes ran on
inline void dst_plan_paths(DctPlan* plan, int paths[2]) {
    paths[0] = dst_plan_last_path(plan, 0);
    paths[1] = dst_plan_last_path(plan, 1);
}

inline void solve_result_set(bk_solve_result* result, const GmresResult& r) {
    result->converged = r.converged;
    result->niter = r.niter;
    result->resnorm = r.resnorm;
}

namespace {

// P^-1 A on (x, tails) for an operator A with ntail = 0 (the initial-value system) or a T tail (dG or dG^T), the operator of the
// left-preconditioned solves; with ntail = 2 the bordered [A a; b' c] on (x, (t, sigma)), left-preconditioned by diag(P, 1, 1):
//     out.u = P^-1 (A (x, t)).u + sigma atil,   out.t = (A (x, t)).t + a_T sigma,   out.sigma = <b_u, x> + b_T t + c sigma
// atil = P^-1 a_u is formed once per solve; per application the column update and the row dot are ONE pass (bordered_tail).
struct PoPrecOp : bk_op {
    bk_op* A = nullptr;
    bk_precond* P = nullptr;
    double* tmp = nullptr;
    const double* atil = nullptr;  // the border, ntail = 2 only
    const double* bu = nullptr;
    double aT = 0.0, bT = 0.0, c = 0.0;
    int apply(const double* x, const double* xt, double a0, double a1, double* out, double* outt) override {
        double tt = 0.0, d = 0.0;
        BK_TRY(A->apply(x, xt, 0.0, 1.0, tmp, &tt));
        BK_TRY(P->apply(tmp, out));
        if (ntail == 2) {
            const double* const at[1] = {atil};
            const double* const bb[1] = {bu};
            BK_TRY(bordered_tail(ctx, n, 1, out, x, at, bb, &xt[1], &d));
        }
        if (!(a0 == 0.0 && a1 == 1.0)) BK_TRY(v_axpby(ctx, n, a0, x, a1, out));
        if (ntail == 1) outt[0] = a0 * xt[0] + a1 * tt;
        if (ntail == 2) {
            outt[0] = a0 * xt[0] + a1 * (tt + aT * xt[1]);
            outt[1] = a0 * xt[1] + a1 * ((d + bT * xt[0]) + c * xt[1]);
        }
        return 0;
    }
};

// The geometry and chunking of a launch, and what a step sees of its lane: n, the slice stride N = 2 n, its grid point idx = (i, j)
struct PoGeom {
    int nx, ny, K;
    int C;                         // rows per chunk
    unsigned ntiles;
    double ax, ay;
};
struct PoAt {
    const PoGeom& g;
    size_t n, N, idx;
    int i, j;
};

// One slice's values at a grid point: the centre pair and the 5-point Dirichlet Laplacian of both fields (cgl_kernel's lap)
struct PoPoint { double c1, c2, d1, d2; };
__device__ __forceinline__ PoPoint po_load(const PoAt& a, const double* s) {
    const PoGeom& P = a.g;
    const size_t idx = a.idx;
    const int i = a.i, j = a.j;
    auto lap = [&](const double* f, double c) {
        const double w = i > 0 ? f[idx - 1] : 0.0, e = i + 1 < P.nx ? f[idx + 1] : 0.0;
        const double so = j > 0 ? f[idx - P.nx] : 0.0, nn = j + 1 < P.ny ? f[idx + P.nx] : 0.0;
        return P.ax * ((w + e) - 2.0 * c) + P.ay * ((so + nn) - 2.0 * c);
    };
    PoPoint q;
    q.c1 = s[idx];
    q.c2 = s[idx + a.n];
    q.d1 = lap(s, q.c1);
    q.d2 = lap(s + a.n, q.c2);
    return q;
}

template <class Pass>
__global__ void __launch_bounds__(kThreads) po_march_kernel(PoGeom G, Pass pass, double* __restrict__ partials) {
    const size_t n = (size_t)G.nx * G.ny;
    const unsigned tile = blockIdx.x % G.ntiles, chunk = blockIdx.x / G.ntiles;
    const size_t idx = (size_t)tile * kThreads + threadIdx.x;
    const int r0 = (int)chunk * G.C, r1 = min(G.K, r0 + G.C);
    double s[Pass::NV > 0 ? Pass::NV : 1] = {0.0};
    if (idx < n) {
        const PoAt at{G, n, 2 * n, idx, (int)(idx % G.nx), (int)(idx / G.nx)};
        typename Pass::Carry c{};
        for (int t = Pass::OPEN && r0 == 0 ? 0 : -1; t < r1 - r0; ++t) pass.step(at, r0 + t, t >= 0, c, s);
        if (r1 == G.K) pass.closure(at, s);
    }
    // the epilogue holds a barrier: every lane of the workgroup reaches it, or (no sums) it is not there at all
    if constexpr (Pass::NV > 0) block_sum_store<Pass::NV>(s, partials);
}

// One marching pass over the K rows (and the closure row) of the orbit of h under the profiling scope `scope` with its
// algorithmic bytes; sums[0..NV) = the pass's sums; who: the prefix of the scratch-bound message.
template <class Pass>
int po_march(bk_potrap* h, const char* who, const char* scope, double bytes, const Pass& pass, double* sums) {
    bk_ctx* ctx = h->ctx;
    const bk_problem_desc& d = h->prob->desc;
    PoGeom G{d.n[0], d.n[1], h->M - 1, 1, 1u, h->prob->ainv[0], h->prob->ainv[1]};
    int nchunks = 1;
    BK_TRY(potrap_chunking(ctx, h->n, h->M, &G.ntiles, &G.C, &nchunks));
    const unsigned grid = G.ntiles * (unsigned)nchunks;
    if ((size_t)grid * Pass::NV > kPartialDoubles)
        return set_error(ctx, "%s: %u workgroups x %d sums exceed the reduction scratch", who, grid, Pass::NV);
    {
        ProfScope ps(ctx, scope, bytes);
        hipLaunchKernelGGL(po_march_kernel<Pass>, dim3(grid), dim3(kThreads), 0, ctx->stream, G, pass, ctx->d_partials);
        BK_HIP(ctx, hipGetLastError());
    }
    if constexpr (Pass::NV > 0) {
        BK_TRY(reduce_finish(ctx, (int)grid, Pass::NV, 0));
        for (int k = 0; k < Pass::NV; ++k) sums[k] = ctx->h_red[k];
    }
    return 0;
}

}  // namespace
}  // namespace bk
