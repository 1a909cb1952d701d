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
//
// The complex counterpart (bls_matrixfree_pl_cshift, bk_bls_matrixfree_pl_cshift): the same construction on (re, im) pairs for the
// bordered systems of src/codim2/MinAugHopf.jl:17, 72-76, [J - i omega, a; b^H, 0], regular where J - i omega is singular.  The
// unbordered part is the real-equivalent operator of cshift.hip (ComplexShiftOp, order 1: the shift under Pl^-1), the tail two host
// scalars (Re sigma, Im sigma), the pass cbordered_tail_kernel: y += sigma atil and b^H x over eight read streams, 80 N bytes.
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

// The complex tail on (re, im) pairs: y += xi atil, every product and sum rounded on its own in the fixed order yr + xr atr - xi ati,
// yi + xr ati + xi atr, and the four sums br.xr, bi.xi, br.xi, bi.xr of d = b^H x = (br.xr + bi.xi) + i (br.xi - bi.xr).  `in` = xr, xi,
// atr, ati, br, bi; yr, yi are read through ins[0], ins[1] and written in place, every element by the lane that read it.  Eight
// read streams and two written: 80 n bytes, where bordered_tail_kernel<2> on stacked vectors of length 2 n reads y, x and two
// rotated copies [-ati; atr], [-bi; br] next to [atr; ati], [br; bi] -- 112 n bytes, and the copies to be written per solve.
// Two 16-byte items per lane in flight, as bordered_tail_kernel<1>: 0.509 ms against 0.579 ms with one at n = 2^25.
struct CTailCoef { double r, i; };
constexpr int kCTailU = 2;
template <int VEC, bool NTH, class... In>
__global__ void __launch_bounds__(kThreads) cbordered_tail_kernel(size_t n, CTailCoef xi, double* yr, double* yi,
                                                                  double* __restrict__ partials, In* __restrict__... in) {
    static_assert(sizeof...(In) == 6, "xr, xi, atr, ati, br, bi");
    const double* const ins[8] = {yr, yi, in...};
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    stream_visit<kCTailU, VEC, NTH, 1>(n, ins, [&](auto kc, size_t i, const auto& v) {
        constexpr int K = decltype(kc)::value;
        double pr[K], pi[K];
#pragma unroll
        for (int e = 0; e < K; ++e) {
            const double xr = v[e][2], xim = v[e][3], atr = v[e][4], ati = v[e][5], br = v[e][6], bi = v[e][7];
            pr[e] = __dadd_rn(__dadd_rn(v[e][0], __dmul_rn(xi.r, atr)), -__dmul_rn(xi.i, ati));
            pi[e] = __dadd_rn(__dadd_rn(v[e][1], __dmul_rn(xi.r, ati)), __dmul_rn(xi.i, atr));
            s[0] = fma(br, xr, s[0]);
            s[1] = fma(bi, xim, s[1]);
            s[2] = fma(br, xim, s[2]);
            s[3] = fma(bi, xr, s[3]);
        }
        if constexpr (K == 2) { st2(yr, i, pr[0], pr[1]); st2(yi, i, pi[0], pi[1]); }
        else { yr[i] = pr[0]; yi[i] = pi[0]; }
    });
    block_sum_store<4>(s, partials);
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

int cbordered_tail(bk_ctx* ctx, size_t n, double* yr, double* yi, const double* xr, const double* xi, const double* atr,
                   const double* ati, const double* br, const double* bi, const double* coef, double* dots) {
    const double* rd[6] = {xr, xi, atr, ati, br, bi};
    if (yr == yi) return set_error(ctx, "cbordered_tail: y_re must not alias y_im");
    bool vec = aligned16(yr) && aligned16(yi);
    for (const double* p : rd) {
        if (p == yr || p == yi) return set_error(ctx, "cbordered_tail: y must not alias x or a border vector");
        vec = vec && aligned16(p);
    }
    if (n == 0) {
        dots[0] = dots[1] = 0.0;
        return 0;
    }
    const bool nth = vec && nt_hint(ctx, n);
    const int grid = grid_for(n, vec ? 2 * kCTailU : 1, kRedBlocks);
    {
        ProfScope ps(ctx, "cbordered_tail", 8.0 * n * 10);
        const CTailCoef cf{coef[0], coef[1]};
        load_path_dispatch(vec, nth, [&](auto V, auto NT) {
            cbordered_tail_kernel<decltype(V)::value, decltype(NT)::value><<<dim3(grid), dim3(kThreads), 0, ctx->stream>>>(
                n, cf, yr, yi, ctx->d_partials, rd[0], rd[1], rd[2], rd[3], rd[4], rd[5]);
        });
        BK_HIP(ctx, hipGetLastError());
    }
    BK_TRY(reduce_finish(ctx, grid, 4, 0));
    dots[0] = ctx->h_red[0] + ctx->h_red[1];
    dots[1] = ctx->h_red[2] - ctx->h_red[3];
    return 0;
}

namespace {

// The unbordered preconditioned operator W and the tail of a border on top of it.  apply: out = b0 x + b1 M x through W's Arnoldi
// form; apply_check: the same through its original chain (stencil kernel, plain preconditioner), so the explicit residual of a
// solve stays independent of the stencil-free identity.
struct PlBordered : bk_op {
    bk_op* W = nullptr;
    virtual int tail(const double* x, const double* xt, double b0, double b1, double* out, double* outt) = 0;
    int apply(const double* x, const double* xt, double b0, double b1, double* out, double* outt) override {
        BK_TRY(W->apply(x, nullptr, b0, b1, out, nullptr));
        return tail(x, xt, b0, b1, out, outt);
    }
    int apply_check(const double* x, const double* xt, double c0, double c1, double* out, double* outt) override {
        BK_TRY(W->apply_check(x, nullptr, c0, c1, out, nullptr));
        return tail(x, xt, c0, c1, out, outt);
    }
};

// M' above.
struct PlBorderedOp : PlBordered {    // W: the unbordered preconditioned operator (T in stencil-free mode)
    const double* atil[BK_MAX_BORDER];   // Pl^-1 a_j
    const double* bvec[BK_MAX_BORDER];
    double ascale = 1.0;                 // 1 / alpha1: the columns are atil_j / alpha1 ...
    double bscale = 1.0;                 // ... the rows bscale b_j / alpha1 (alpha1 folded in by the caller)
    double c[BK_MAX_BORDER * BK_MAX_BORDER];     // (c - alpha0 I) / alpha1, row-major m x m
    int tail(const double* x, const double* xt, double b0, double b1, double* out, double* outt) override {
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
    // (no hessenberg_shift, check_norm, apply_block, arm_v0: bordered operators take Gram-corrected single steps and the spectral
    // check stays declined for bordered tails -- DESIGN 3.  What follows from it: the explicit residuals gmres_core forms -- KrylovKit
    // after every converged cycle, every flavor at a restart -- go through apply_check above, but the IterativeSolvers and Krylov.jl
    // flavors return `converged` on the Arnoldi estimate of a first cycle, also when W ran stencil-free: the extra check of an
    // unbordered stencil-free solve (gmres_core, "rearranged operator") is tied to hessenberg_shift and passes no tails.  DESIGN 9b.)
};

// The same on (re, im) pairs, x = [xr; xi] of length n = 2 N with the tail (Re sigma, Im sigma): W = the real-equivalent operator of
// Pl^-1 (shift + J) (cshift.hip: ComplexShiftOp), one complex border column atil = Pl^-1 a and row bscale b^H, block c.
//     out.u = b0 x.u + b1 (W x.u + sigma atil),     out.p = b0 sigma + b1 (bscale b^H x.u + c sigma)
struct PlCBorderedOp : PlBordered {
    const double *atr = nullptr, *ati = nullptr, *br = nullptr, *bi = nullptr;
    double bscale = 1.0, cr = 0.0, ci = 0.0;
    int tail(const double* x, const double* xt, double b0, double b1, double* out, double* outt) override {
        const size_t N = n / 2;
        const double coef[2] = {b1 * xt[0], b1 * xt[1]};
        double d[2];
        BK_TRY(cbordered_tail(ctx, N, out, out + N, x, x + N, atr, ati, br, bi, coef, d));
        outt[0] = b0 * xt[0] + b1 * (bscale * d[0] + (cr * xt[0] - ci * xt[1]));
        outt[1] = b0 * xt[1] + b1 * (bscale * d[1] + (cr * xt[1] + ci * xt[0]));
        return 0;
    }
};

struct OpGuard {
    bk_op* op = nullptr;
    ~OpGuard() { delete op; }
};

// what both preconditioned bordered solves refuse
int pl_bordered_check(bk_ctx* ctx, bk_op* J, const bk_gmres_opts& ls, bk_precond* pl) {
    if (J->ntail != 0) return set_error(ctx, "MatrixFreeBLS: J must be unbordered");
    if (!pl) return set_error(ctx, "MatrixFreeBLS with use_pl needs a left preconditioner (without one: bk_bls_matrixfree)");
    if (ls.flavor >= BK_KRYLOV_MINRES) return set_error(ctx, "MatrixFreeBLS: the bordered operator is not symmetric (use a GMRES flavor)");
    if (ls.pr) return set_error(ctx, "MatrixFreeBLS with use_pl: a right preconditioner has no bordered form here (left only)");
    if (ctx->nranks > 1) return set_error(ctx, "MatrixFreeBLS with use_pl runs on a single rank");
    return 0;
}

}  // namespace

int bls_matrixfree_pl(bk_ctx* ctx, bk_op* J, int m, const double* const* a, const double* const* b, double bscale, const double* c,
                      const double* rhst, const double* rhsb, bool has_shift, double shift, const bk_gmres_opts& ls, bk_precond* pl,
                      double* u1, double* u2, GmresResult* res, const double* const* atil) {
    if (m < 1 || m > BK_MAX_BORDER) return set_error(ctx, "Linear bordered solver, wrong sizes! (1 <= m <= %d)", BK_MAX_BORDER);
    BK_TRY(pl_bordered_check(ctx, J, ls, pl));
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

// The complex counterpart: the shift always sits under Pl^-1 (ComplexShiftOp order 1 in every flavor, as a shifted solve above), the
// right-hand side is (Pl^-1 rhst, rhsb), Pl^-1 is applied per half and atil = Pl^-1 a is formed once per solve.
int bls_matrixfree_pl_cshift(bk_ctx* ctx, bk_op* J, const double* const a[2], const double* const b[2], double bscale, const double c[2],
                             const double* const rhst[2], const double rhsb[2], const double shift[2], const bk_gmres_opts& ls,
                             bk_precond* pl, double* u1_re, double* u1_im, double u2[2], GmresResult* res) {
    BK_TRY(pl_bordered_check(ctx, J, ls, pl));
    if (J->n % 2 != 0) return set_error(ctx, "bk_bls_matrixfree_pl_cshift: odd local length (the stacked halves must stay 16-B aligned)");
    if (!a[0] || !b[0] || !rhst[0]) return -1;
    const size_t N = J->n;
    WsGuard ws(ctx);
    double *tmp = nullptr, *prhs = nullptr, *at = nullptr, *bz = nullptr, *u = nullptr;
    BK_TRY(ws.get(N, &tmp));
    BK_TRY(ws.get(2 * N, &prhs));
    BK_TRY(ws.get(2 * N, &at));
    BK_TRY(ws.get(2 * N, &u));
    // Pl^-1 of a complex vector, half by half; a missing imaginary part is zero
    auto pinv = [&](const double* const v[2], double* out2) -> int {
        BK_TRY(pl->apply(v[0], out2));
        return v[1] ? pl->apply(v[1], out2 + N) : v_zero(ctx, N, out2 + N);
    };
    OpGuard guard;
    BK_TRY(cshift_op_create(ctx, J, pl, shift[0], shift[1], 1.0, 1, tmp, &guard.op));
    PlCBorderedOp M;
    M.ctx = ctx; M.n = 2 * N; M.ntail = 2;
    M.W = guard.op;
    BK_TRY(pinv(a, at));
    M.atr = at; M.ati = at + N;
    M.br = b[0]; M.bi = b[1];
    if (!b[1]) {
        BK_TRY(ws.get(N, &bz));
        BK_TRY(v_zero(ctx, N, bz));
        M.bi = bz;
    }
    M.bscale = bscale; M.cr = c[0]; M.ci = c[1];
    BK_TRY(pinv(rhst, prhs));
    BK_TRY(gmres_core(ctx, &M, prhs, rhsb, u, u2, 0.0, 1.0, ls, res));
    BK_TRY(v_copy(ctx, N, u, u1_re));
    return v_copy(ctx, N, u + N, u1_im);
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

int bk_cbordered_tail(bk_ctx* ctx, size_t n, double* y_re, double* y_im, const double* x_re, const double* x_im, const double* at_re,
                      const double* at_im, const double* b_re, const double* b_im, const double coef[2], double dots[2]) {
    if (!ctx || !y_re || !y_im || !x_re || !x_im || !at_re || !at_im || !b_re || !b_im || !coef || !dots) return -1;
    return cbordered_tail(ctx, n, y_re, y_im, x_re, x_im, at_re, at_im, b_re, b_im, coef, dots);
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

int bk_bls_matrixfree_pl_cshift(bk_ctx* ctx, bk_op* J, const double* dR_re, const double* dR_im, const double* dzu_re,
                                const double* dzu_im, double dzp_re, double dzp_im, const double* R_re, const double* R_im, double n_re,
                                double n_im, double xiu, double xip, double shift_re, double shift_im, double dotscale,
                                const bk_gmres_opts* lsopts, bk_precond* pl, double* dX_re, double* dX_im, double dl[2], int* converged,
                                int* itlinear) {
    if (!ctx || !J || !dR_re || !dzu_re || !R_re || !lsopts || !dX_re || !dX_im || !dl) return -1;
    if (dX_re == dX_im) return set_error(ctx, "bk_bls_matrixfree_pl_cshift: dX_re and dX_im must be distinct");
    const double* const a[2] = {dR_re, dR_im};
    const double* const b[2] = {dzu_re, dzu_im};
    const double* const R[2] = {R_re, R_im};
    const double c[2] = {dzp_re * xip, dzp_im * xip}, nn[2] = {n_re, n_im}, shift[2] = {shift_re, shift_im};
    GmresResult r;
    BK_TRY(bls_matrixfree_pl_cshift(ctx, J, a, b, xiu * dotscale, c, R, nn, shift, *lsopts, pl, dX_re, dX_im, dl, &r));
    if (converged) *converged = r.converged;
    if (itlinear) *itlinear = r.niter;
    return 0;
}

}  // extern "C"
