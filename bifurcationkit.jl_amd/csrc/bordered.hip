// MatrixFreeBLS with a left preconditioner: ONE GMRES on the (N + m) operator of src/LinearBorderSolver.jl:326-352, :424-450 with
// Pl = diag(Pl, 1) in front of it,
//
//     out.u = Pl^-1 ((J + shift I) x.u) + sum_j x.p[j] atil_j,        atil_j = Pl^-1 a_j, formed ONCE per solve
//     out.p = bscale [<b_i, x.u>]_i + c x.p
//
// and the right-hand side (Pl^-1 rhs.u, rhs.p): the KrylovKit arrangement of src/LinearSolver.jl:270-278 applied to the bordered map.
// The bordered system is regular where J is singular (folds, branch points), and with the spectral preconditioner its iteration
// count does not depend on the distance to the singular point.
//
// The unbordered part goes through the operator linsolve itself would set up (solver.hip: ShiftPrecOp behind prec_op_create), in
// whichever mode it chooses: the literal chain, or the stencil-free T with Pl^-1 J = alpha0 I + alpha1 T, (alpha0, alpha1) the
// solve's t_alpha0 / t_alpha1.  In that mode the solve runs on alpha0 I + alpha1 M' with
//
//     M' = [ T              atil / alpha1       ]        alpha0 I + alpha1 M' = [ Pl^-1 J      atil ]
//          [ bscale b' / alpha1   (c - alpha0 I) / alpha1 ]                      [ bscale b'    c    ]
//
// i.e. the border block is handed over as (c - alpha0 I) / alpha1 so that the identity part reaches the tail too (on the literal
// chain (alpha0, alpha1) = (0, 1) and M' is the operator itself).  tests/test_fold_bordered_reference.py restates the identity
// with dense matrices.
//
// Per application, after the unbordered apply has written y: ONE pass (bordered_tail_kernel) forms y += sum_j coef_j atil_j and the
// m dots <b_j, x> -- (3 + 2 m) 8 N bytes instead of the 40 m N bytes of the m v_axpby and m v_dot launches of BorderedMapOp::apply.
#include <cmath>
#include <utility>

#include "common.h"
#include "ops.h"
#include "stream.h"

namespace bk {

namespace {

template <int M>
struct TailCoef { double c[M]; };

// y[i] += sum_j coef_j atil_j[i] (each product and each sum rounded on its own, in j order) and s_j = sum_i b_j[i] x[i].
// `in` = y, x, atil_0 .. atil_{M-1}, b_0 .. b_{M-1}: one pointer per vector, the read-only ones as __restrict__ kernel parameters
// (stream.h: stream_write_kernel); y is read through in[0] and written in place, every element by the lane that read it.
// M partial sums per workgroup (block_sum_store); every lane adds its elements in the order of stream_visit, so the dots have
// the same bits on every run.
template <int M, int VEC, bool NTH, class... In>
__global__ void __launch_bounds__(kThreads) bordered_tail_kernel(size_t n, TailCoef<M> coef, double* y, double* __restrict__ partials,
                                                                 In* __restrict__... in) {
    constexpr int NIN = 2 + 2 * M;
    constexpr int U = M <= 2 ? 2 : 1;
    static_assert(sizeof...(In) == NIN - 1, "x, M x atil, M x b");
    const double* const ins[NIN] = {y, in...};
    double s[M];
#pragma unroll
    for (int j = 0; j < M; ++j) s[j] = 0.0;
    stream_visit<U, VEC, NTH, 1>(n, ins, [&](auto kc, size_t i, const auto& v) {
        constexpr int K = decltype(kc)::value;
        double o[K];
#pragma unroll
        for (int e = 0; e < K; ++e) {
            double t = v[e][0];
#pragma unroll
            for (int j = 0; j < M; ++j) {
                t = __dadd_rn(t, __dmul_rn(coef.c[j], v[e][2 + j]));
                s[j] = fma(v[e][2 + M + j], v[e][1], s[j]);
            }
            o[e] = t;
        }
        if constexpr (K == 2) st2(y, i, o[0], o[1]);
        else y[i] = o[0];
    });
    block_sum_store<M>(s, partials);
}

template <int M, int VEC, bool NTH, size_t... Q>
void bordered_tail_launch(bk_ctx* ctx, int grid, size_t n, const TailCoef<M>& coef, double* y, const double* const* rd,
                          std::index_sequence<Q...>) {
    bordered_tail_kernel<M, VEC, NTH><<<dim3(grid), dim3(kThreads), 0, ctx->stream>>>(n, coef, y, ctx->d_partials, rd[Q]...);
}

}  // namespace

// y += sum_j coef[j] atil[j], dots[j] = <b[j], x> (all-reduced), j < m <= BK_MAX_BORDER; y must not alias any other operand
int bordered_tail(bk_ctx* ctx, size_t n, int m, double* y, const double* x, const double* const* atil, const double* const* b,
                  const double* coef, double* dots) {
    if (m < 1 || m > BK_MAX_BORDER) return set_error(ctx, "bordered_tail: 1 <= m <= %d (got %d)", BK_MAX_BORDER, m);
    if (y == x) return set_error(ctx, "bordered_tail: y must not alias x");
    for (int j = 0; j < m; ++j)
        if (atil[j] == y || b[j] == y) return set_error(ctx, "bordered_tail: y must not alias a border vector");
    if (n == 0) {
        for (int j = 0; j < m; ++j) dots[j] = 0.0;
        return 0;
    }
    const double* rd[1 + 2 * BK_MAX_BORDER];
    rd[0] = x;
    bool vec = aligned16(y) && aligned16(x);
    for (int j = 0; j < m; ++j) {
        rd[1 + j] = atil[j];
        rd[1 + m + j] = b[j];
        vec = vec && aligned16(atil[j]) && aligned16(b[j]);
    }
    const bool nth = vec && nt_hint(ctx, n);
    int grid = 0;
    {
        ProfScope ps(ctx, "bordered_tail", 8.0 * n * (3 + 2 * m));
        count_dispatch<1, BK_MAX_BORDER>(m, [&](auto Mc) {
            constexpr int M = decltype(Mc)::value;
            static_assert(M <= kPartialVals, "partial sums per workgroup");
            grid = grid_for(n, vec ? 2 * (M <= 2 ? 2 : 1) : 1, kRedBlocks);
            TailCoef<M> cf;
            for (int j = 0; j < M; ++j) cf.c[j] = coef[j];
            load_path_dispatch(vec, nth, [&](auto V, auto NT) {
                bordered_tail_launch<M, decltype(V)::value, decltype(NT)::value>(ctx, grid, n, cf, y, rd, std::make_index_sequence<1 + 2 * M>{});
            });
            return 0;
        });
        BK_HIP(ctx, hipGetLastError());
    }
    BK_TRY(reduce_finish(ctx, grid, m, 0));
    for (int j = 0; j < m; ++j) dots[j] = ctx->h_red[j];
    return 0;
}

namespace {

// M' above.  apply: out = b0 x + b1 M' x through the operator's Arnoldi form; apply_check: the same through its original chain
// (stencil kernel, plain preconditioner), so the explicit residual of a solve stays independent of the stencil-free identity.
struct PlBorderedOp : bk_op {
    bk_op* W = nullptr;                  // the unbordered preconditioned operator (T in stencil-free mode)
    const double* atil[BK_MAX_BORDER];   // Pl^-1 a_j
    const double* bvec[BK_MAX_BORDER];
    double ascale = 1.0;                 // 1 / alpha1: the columns are atil_j / alpha1 ...
    double bscale = 1.0;                 // ... the rows bscale b_j / alpha1 (alpha1 folded in by the caller)
    double c[BK_MAX_BORDER * BK_MAX_BORDER];     // (c - alpha0 I) / alpha1, row-major m x m
    int tail(const double* x, const double* xt, double b0, double b1, double* out, double* outt) {
        const int m = ntail;
        double coef[BK_MAX_BORDER], d[BK_MAX_BORDER];
        for (int j = 0; j < m; ++j) coef[j] = b1 * xt[j] * ascale;
        BK_TRY(bordered_tail(ctx, n, m, out, x, atil, bvec, coef, d));
        for (int i = 0; i < m; ++i) {
            double cx = 0.0;
            for (int j = 0; j < m; ++j) cx += c[i * m + j] * xt[j];
            outt[i] = b0 * xt[i] + b1 * (bscale * d[i] + cx);
        }
        return 0;
    }
    int apply(const double* x, const double* xt, double b0, double b1, double* out, double* outt) override {
        BK_TRY(W->apply(x, nullptr, b0, b1, out, nullptr));
        return tail(x, xt, b0, b1, out, outt);
    }
    int apply_check(const double* x, const double* xt, double c0, double c1, double* out, double* outt) override {
        BK_TRY(W->apply_check(x, nullptr, c0, c1, out, nullptr));
        return tail(x, xt, c0, c1, out, outt);
    }
    // (no hessenberg_shift, check_norm, apply_block, arm_v0: bordered operators take Gram-corrected single steps and the spectral
    // check stays declined for bordered tails -- DESIGN 3.  What follows from it: the explicit residuals gmres_core forms -- KrylovKit
    // after every converged cycle, every flavor at a restart -- go through apply_check above, but the IterativeSolvers and Krylov.jl
    // flavors return `converged` on the Arnoldi estimate of a first cycle, also when W ran stencil-free: the extra check of an
    // unbordered stencil-free solve (gmres_core, "rearranged operator") is tied to hessenberg_shift and passes no tails.  DESIGN 9b.)
};

struct OpGuard {
    bk_op* op = nullptr;
    ~OpGuard() { delete op; }
};

}  // namespace

int bls_matrixfree_pl(bk_ctx* ctx, bk_op* J, int m, const double* const* a, const double* const* b, double bscale, const double* c,
                      const double* rhst, const double* rhsb, bool has_shift, double shift, const bk_gmres_opts& ls, bk_precond* pl,
                      double* u1, double* u2, GmresResult* res, const double* const* atil) {
    if (m < 1 || m > BK_MAX_BORDER) return set_error(ctx, "Linear bordered solver, wrong sizes! (1 <= m <= %d)", BK_MAX_BORDER);
    if (J->ntail != 0) return set_error(ctx, "MatrixFreeBLS: J must be unbordered");
    if (!pl) return set_error(ctx, "MatrixFreeBLS with use_pl needs a left preconditioner (without one: bk_bls_matrixfree)");
    if (ls.flavor >= BK_KRYLOV_MINRES) return set_error(ctx, "MatrixFreeBLS: the bordered operator is not symmetric (use a GMRES flavor)");
    if (ls.pr) return set_error(ctx, "MatrixFreeBLS with use_pl: a right preconditioner has no bordered form here (left only)");
    if (ctx->nranks > 1) return set_error(ctx, "MatrixFreeBLS with use_pl runs on a single rank");
    const size_t n = J->n;
    WsGuard ws(ctx);
    double *tmp = nullptr, *prhs = nullptr;
    BK_TRY(ws.get(n, &tmp));
    BK_TRY(ws.get(n, &prhs));
    // Pl^-1 ((shift + J) x): KrylovKit without a shift keeps its own chain (order 0, Pl^-1 (J x)); a shift, and the IterativeSolvers /
    // Krylov.jl flavors always, take their arrangement Pl^-1 (a0 + a1 J) (order 1) -- the shift belongs inside the map, under Pl^-1
    const int order = (ls.flavor == BK_GMRES_KRYLOVKIT && !has_shift) ? 0 : 1;
    PrecOpView V;
    BK_TRY(prec_op_create(ctx, J, pl, has_shift ? shift : 0.0, 1.0, order, tmp, &V));
    OpGuard guard;
    guard.op = V.op;
    PlBorderedOp M;
    M.ctx = ctx; M.n = n; M.ntail = m;
    M.W = V.op;
    M.ascale = 1.0 / V.alpha1;
    M.bscale = bscale / V.alpha1;
    for (int i = 0; i < m; ++i) {
        if (!a[i] || !b[i]) return -1;
        M.bvec[i] = b[i];
        if (atil) {
            M.atil[i] = atil[i];
        } else {
            double* t = nullptr;
            BK_TRY(ws.get(n, &t));
            BK_TRY(pl->apply(a[i], t));
            M.atil[i] = t;
        }
        // alpha0 I + alpha1 M' = diag(Pl^-1, 1) [J + shift, a; bscale b', c]  <=>  the border block of M' is (c - alpha0 I) / alpha1
        for (int j = 0; j < m; ++j) M.c[i * m + j] = (c[i * m + j] - (i == j ? V.alpha0 : 0.0)) / V.alpha1;
    }
    BK_TRY(pl->apply(rhst, prhs));                // the top of the right-hand side; the tail is untouched
    return gmres_core(ctx, &M, prhs, rhsb, u1, u2, V.alpha0, V.alpha1, ls, res);
}

}  // namespace bk

using namespace bk;

extern "C" {

int bk_bordered_tail(bk_ctx* ctx, size_t n, int m, double* y, const double* x, const double* const* atil, const double* const* b,
                     const double* coef, double* dots) {
    if (!ctx || !y || !x || !atil || !b || !coef || !dots) return -1;
    if (m < 1 || m > BK_MAX_BORDER) return set_error(ctx, "bk_bordered_tail: 1 <= m <= %d (got %d)", BK_MAX_BORDER, m);
    for (int j = 0; j < m; ++j)
        if (!atil[j] || !b[j]) return -1;
    return bordered_tail(ctx, n, m, y, x, atil, b, coef, dots);
}

int bk_bls_matrixfree_pl(bk_ctx* ctx, bk_op* J, const double* dR, const double* dzu, double dzp, const double* R, double n, double xiu,
                         double xip, int has_shift, double shift, double dotscale, const bk_gmres_opts* lsopts, bk_precond* pl,
                         double* dX, double* dl, int* converged, int* itlinear) {
    if (!ctx || !J || !dR || !dzu || !R || !lsopts || !dX || !dl) return -1;
    if (dX == R || dX == dR || dX == dzu) return set_error(ctx, "bk_bls_matrixfree_pl: dX must be a fresh buffer");
    const double* a[1] = {dR};
    const double* b[1] = {dzu};
    const double c[1] = {dzp * xip};
    GmresResult r;
    BK_TRY(bls_matrixfree_pl(ctx, J, 1, a, b, xiu * dotscale, c, R, &n, has_shift != 0, shift, *lsopts, pl, dX, dl, &r));
    if (converged) *converged = r.converged;
    if (itlinear) *itlinear = r.niter;
    return 0;
}

int bk_bls_block_matrixfree_pl(bk_ctx* ctx, bk_op* J, int m, const double* const* a, const double* const* b, const double* c,
                               const double* rhst, const double* rhsb, int has_shift, double shift, double dotscale,
                               const bk_gmres_opts* lsopts, bk_precond* pl, double* u1, double* u2, int* converged, int* itlinear) {
    if (!ctx || !J || !a || !b || !c || !rhst || !rhsb || !lsopts || !u1 || !u2) return -1;
    if (u1 == rhst) return set_error(ctx, "bk_bls_block_matrixfree_pl: u1 must be a fresh buffer");
    GmresResult r;
    BK_TRY(bls_matrixfree_pl(ctx, J, m, a, b, dotscale, c, rhst, rhsb, has_shift != 0, shift, *lsopts, pl, u1, u2, &r));
    if (converged) *converged = r.converged;
    if (itlinear) *itlinear = r.niter;
    return 0;
}

}  // extern "C"
