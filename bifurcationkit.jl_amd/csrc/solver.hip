// Device-resident Krylov solvers behind the reference's plugin surface:
//   gmres_core / linsolve   GMRESKrylovKit + GMRESIterativeSolvers      src/LinearSolver.jl:149-291
//   bk_bls_bordering        BorderingBLS (BEC + k refinements)           src/LinearBorderSolver.jl:88-166
//   bk_bls_matrixfree       MatrixFreeBLS on BorderedArray(u, p)         src/LinearBorderSolver.jl:326-335,424-437
//                           (with the left preconditioner diag(Pl, 1): bordered.hip, on prec_op_create below)
//   bk_eig_shiftinvert      ShiftInvert + Krylov-Schur outer iteration   src/EigSolver.jl:246-266, examples/SH3d.jl:96-113
//   bk_newton               _newton                                      src/Newton.jl:66-114
//   bk_newton_palc          newton_palc                                  src/continuation/Palc.jl:187-305
//
// MI355X design.  The Krylov basis never leaves HBM; the host only sees (k+2) doubles per Arnoldi step.
// Orthogonalisation is classical Gram-Schmidt with DGKS selective re-orthogonalisation, done as TWO
// streaming passes per step instead of the reference packages' 2k..4k BLAS-1 passes:
//   pass A  multidot : h = V'w and ||w||^2        reads (k+1) vectors
//   pass B  multiaxpy: v_{k+1} = (w - V h)/beta   reads (k+1), writes 1; beta^2 = ||w||^2 - ||h||^2
// (re-orthogonalise with a second A/B pair only when beta < eta ||w||).  The Hessenberg matrix, Givens
// rotations, the (a0, a1) shift and the restart logic stay on the host, as in the packages.
#include <cmath>
#include <cstdio>
#include <thread>
#include <vector>

#include "dense.h"
#include "ops.h"
#include "sstep.h"
#include "stream.h"

namespace bk {

namespace {

// The explicit residual check of a converged solve (option gmres_check_spectral): 1 = its norm from the preconditioner's spectrum where
// ShiftPrecOp::check_norm can have it, 0 = the residual vector through the whole chain.
constexpr double kCheckSpectralDefault = 1.0;

// First block of a solve on a rearranged operator A = W + theta0 I (ShiftPrecOp, stencil-free form): 0 = powers of A itself,
// 1 = powers of the literal operator W (see gmres_core: first block).  Option gmres_monomial_shift.
constexpr double kMonomialShiftDefault = 0.0;

inline size_t round_up(size_t n, size_t m) { return (n + m - 1) / m * m; }

struct Basis {                 // (m+1) device vectors + host tails (nt scalars per vector: the border block)
    double* V = nullptr;
    size_t ld = 0;
    int nt = 0;
    double dlt = 0.0;          // running estimate of the orthogonality defect ||I - V'V|| of the current cycle (arnoldi_step)
    double orth_tol = 1e-8;    // ... which single Gram-Schmidt passes may not push beyond this
    std::vector<double> t;     // tails, t[i * nt + q]
    // Gram-corrected single-pass step (arnoldi_step): G(i, j) = <v_i, v_j> as MEASURED, column by column, by the fused
    // multidot pass of the step that follows the creation of v_j; gram_n = columns known so far (reset per cycle)
    bool use_gram = false;
    int gram_n = 0;
    std::vector<double> G;     // (kMaxBasis + 1)^2, column-major
    double& g(int i, int j) { return G[(size_t)i + (size_t)j * (kMaxBasis + 1)]; }
    double* vec(int i) { return V + (size_t)i * ld; }
    double* tail(int i) { return t.data() + (size_t)i * nt; }
    double tdot(int i, const double* y) { double s = 0.0; for (int q = 0; q < nt; ++q) s += t[(size_t)i * nt + q] * y[q]; return s; }
};

// ---------------------------------------------------------------- bordered-vector helpers
struct VecOps {
    bk_ctx* ctx;
    size_t n;
    int ntail;
    int nrm2(const double* x, const double* xt, double* out) {
        double s;
        BK_TRY(v_dot(ctx, n, x, x, &s));
        for (int q = 0; q < ntail; ++q) s += xt[q] * xt[q];
        *out = std::sqrt(s);
        return 0;
    }
};

// One Arnoldi step: w = A V[j]; orthogonalise against V[0..j]; write V[j+1] = w / beta.
// h[0..j] receives the projections, *beta the norm of the remainder (0 => breakdown, V[j+1] not written).
// eta = DGKS threshold: a second Gram-Schmidt pass runs when the remainder keeps less than eta of ||w|| (eta > 1:
// always, the choice for the eigensolver's outer Arnoldi where ghost Ritz values punish any loss of orthogonality).
// A single classical Gram-Schmidt pass leaves V'v_new = (I - V'V) h / beta: the defect of the basis is amplified by
// rho = ||w|| / beta at EVERY single-pass step, whatever the DGKS test says (measured on Pl^-1 J: x3 per step, 1e-9 after 11
// steps, O(1) after 21 -- GMRES then stagnates; a0 I + J with a large a0: stagnation at 3e-9 after 10 steps).  So the step also
// carries the running estimate dlt <- (dlt + 2 eps) rho (it tracks the measured defect within a factor of 2) and takes
// the second pass whenever the estimate would exceed orth_tol (1e-8; the budget orth_tol / eps = 2e7 allows ~15 single-pass
// steps at rho = 3).  Round 3 tried to buy back the second passes of the 512^3 corrector (14 % of its time: the late
// steps of each solve, rho > 10) by relaxing either knob -- both measured, both rejected:
//  * orth_tol 1e-6 ... 1e-4: fine on the well-conditioned Pl^-1 J (measured defect <= 8 orth_tol, same iteration counts:
//    tests/test_gpu_parity.py::test_single_pass_gram_schmidt_policy_...), worth <= 2 % there, but the shifted operator
//    a0 I + J with a large a0 (rho ~ 10 at EVERY step) then needs 67 iterations instead of the oracle's 14
//    (test_gmres_unpreconditioned_shift_and_restart) -- a basis that is only 1e-6-orthogonal does delay GMRES there;
//  * DGKS eta 0.01 / 0.001 (single passes up to rho = 100 / 1000): the 512^3 corrector goes from 26 to 57-59 operator
//    applications (profiles/r3_gram_schmidt_policy_512.txt).
int arnoldi_step(bk_ctx* ctx, bk_op* A, Basis& B, int j, double* w, double* h, double* beta, double op_a0,
                 double op_a1, double eta) {
    const size_t n = A->n;
    const int nt = A->ntail;
    double wt[BK_MAX_BORDER] = {0.0};
    BK_TRY(A->apply(B.vec(j), nt ? B.tail(j) : nullptr, op_a0, op_a1, w, wt));
    const int k = j + 1;
    double hh[kMaxBasis + 1], c[kMaxBasis];
    // ---- Gram-corrected single pass (option gmres_gram, default on; the eigensolver's outer Arnoldi takes it too: eig_gram).
    // The multidot pass also measures g = V'v_j, the Gram column of the newest vector (no extra traffic: v_j is one of the
    // streams).  With G known, the coefficients of the ORTHOGONAL projection of w onto span(V) are c = G^-1 (V'w) -- for the
    // nearly orthonormal V at hand c = a - E a + E E a, E = G - I -- and w - V c is orthogonal to every v_i up to the
    // rounding of this one pass (eps * rho), whatever defect the earlier vectors carry: nothing accumulates, so the second
    // "twice is enough" pass (14 % of the 512^3 corrector in round 2, all of its late steps) is not needed.
    // The Arnoldi relation A v_j = V c + beta v_{j+1} holds exactly as before (H column = c), beta^2 = w'w - c'a.
    if (B.use_gram && B.gram_n == j && v_multidot_gram_ok(ctx, n, B.V, B.ld, k, w)) {
        double gcol[kMaxBasis];
        BK_TRY(v_multidot_gram(ctx, n, B.V, B.ld, k, w, hh, gcol));
        double ww = hh[k];
        if (nt) {
            for (int i = 0; i < k; ++i) { hh[i] += B.tdot(i, wt); gcol[i] += B.tdot(i, B.tail(j)); }
            for (int q = 0; q < nt; ++q) ww += wt[q] * wt[q];
        }
        for (int i = 0; i < k; ++i) { B.g(i, j) = gcol[i]; B.g(j, i) = gcol[i]; }
        B.gram_n = k;
        if (ww == 0.0) { *beta = 0.0; return 0; }
        double e1[kMaxBasis], e2[kMaxBasis];
        for (int i = 0; i < k; ++i) {
            double s_ = 0.0;
            for (int l = 0; l < k; ++l) s_ += (B.g(i, l) - (i == l ? 1.0 : 0.0)) * hh[l];
            e1[i] = s_;
        }
        double proj = 0.0;
        for (int i = 0; i < k; ++i) {
            double s_ = 0.0;
            for (int l = 0; l < k; ++l) s_ += (B.g(i, l) - (i == l ? 1.0 : 0.0)) * e1[l];
            e2[i] = s_;
            c[i] = hh[i] - e1[i] + e2[i];
            proj += c[i] * hh[i];
        }
        const double b2 = ww - proj;
        if (b2 > kCancelTol * ww) {
            const double be = std::sqrt(b2);
            double cm[kMaxBasis];
            for (int i = 0; i < k; ++i) { h[i] = c[i]; cm[i] = -c[i]; }
            BK_TRY(v_multiaxpy(ctx, n, B.V, B.ld, k, cm, w, 1.0 / be, B.vec(k), nullptr));
            for (int q = 0; q < nt; ++q) {
                double t = wt[q];
                for (int i = 0; i < k; ++i) t -= c[i] * B.tail(i)[q];
                B.tail(k)[q] = t / be;
            }
            *beta = be;
            return 0;
        }
        // severe cancellation (w is in span(V) to 1e-4): the explicit path below, on the raw projections
        B.dlt = B.orth_tol;
    } else {
        if (B.use_gram) B.dlt = B.orth_tol;        // beyond the tracked columns: the two-pass policy, on the safe side
        BK_TRY(v_multidot(ctx, n, B.V, B.ld, k, w, hh));
        if (nt)
            for (int i = 0; i < k; ++i) hh[i] += B.tdot(i, wt);
    }
    double ww = hh[k];
    if (nt)
        for (int q = 0; q < nt; ++q) ww += wt[q] * wt[q];
    if (ww == 0.0) { *beta = 0.0; return 0; }
    double hsq = 0.0;
    for (int i = 0; i < k; ++i) { h[i] = hh[i]; hsq += hh[i] * hh[i]; c[i] = -hh[i]; }
    const double b2 = ww - hsq;                 // Pythagoras: ||w - V h||^2, relative error ~ eps * ww / b2
    if (b2 > kCancelTol * ww) {
        // pass B with the normalisation folded in: v_{k} = (w - V h) / sqrt(b2)
        const double be = std::sqrt(b2);
        BK_TRY(v_multiaxpy(ctx, n, B.V, B.ld, k, c, w, 1.0 / be, B.vec(k), nullptr));
        for (int q = 0; q < nt; ++q) {
            double t = wt[q];
            for (int i = 0; i < k; ++i) t -= h[i] * B.tail(i)[q];
            B.tail(k)[q] = t / be;
        }
        *beta = be;
        if (b2 >= eta * eta * ww) {              // DGKS: no cancellation in THIS step ...
            const double grown = (B.dlt + 4.440892098500626e-16) * std::sqrt(ww / b2);
            if (grown <= B.orth_tol) {           // ... and the accumulated defect stays small: one pass is enough
                if (grown > B.dlt) B.dlt = grown;
                return 0;
            }
        }
    } else {
        // severe cancellation: the Pythagorean estimate is noise; take the norm of the remainder explicitly
        double nn = 0.0;
        BK_TRY(v_multiaxpy(ctx, n, B.V, B.ld, k, c, w, 1.0, w, &nn));
        for (int q = 0; q < nt; ++q) {
            for (int i = 0; i < k; ++i) wt[q] -= h[i] * B.tail(i)[q];
            nn += wt[q] * wt[q];
        }
        if (!(nn > 1e-30 * ww)) { *beta = 0.0; return 0; }       // w is in span(V) to working precision: breakdown
        const double bn = std::sqrt(nn);
        BK_TRY(v_axpbyz(ctx, n, 1.0 / bn, w, 0.0, nullptr, B.vec(k)));
        for (int q = 0; q < nt; ++q) B.tail(k)[q] = wt[q] / bn;
        *beta = bn;
    }
    // second pass ("twice is enough"), with the norm of the result taken explicitly
    double ss[kMaxBasis + 1];
    BK_TRY(v_multidot(ctx, n, B.V, B.ld, k, B.vec(k), ss));
    double vv = ss[k];
    if (nt) {
        for (int i = 0; i < k; ++i) ss[i] += B.tdot(i, B.tail(k));
        vv += B.tdot(k, B.tail(k));
    }
    for (int i = 0; i < k; ++i) c[i] = -ss[i];
    double nn2 = 0.0;
    BK_TRY(v_multiaxpy(ctx, n, B.V, B.ld, k, c, B.vec(k), 1.0, B.vec(k), &nn2));
    for (int q = 0; q < nt; ++q) {
        double t = B.tail(k)[q];
        for (int i = 0; i < k; ++i) t -= ss[i] * B.tail(i)[q];
        B.tail(k)[q] = t;
        nn2 += t * t;
    }
    if (!(nn2 > 1e-30 * vv)) { *beta = 0.0; return 0; }
    const double cn = std::sqrt(nn2);
    BK_TRY(v_scale(ctx, n, 1.0 / cn, B.vec(k)));
    for (int q = 0; q < nt; ++q) B.tail(k)[q] /= cn;
    for (int i = 0; i < k; ++i) h[i] += (*beta) * ss[i];
    *beta = (*beta) * cn;
    return 0;
}

// s Arnoldi steps from V[j] as ONE block (sstep.h): p_{i+1} = A p_i straight into the basis slots j+1 .. j+s, one pass of dots
// over the basis and the block, the coefficient algebra on the host, one update pass in place.  Against the per-step pair of
// passes (2k + 3 vector streams per step) a block moves 2k + 3s - 1 .. 2k + 3s + 8 streams per s steps; at 512^3 the two
// Gram-Schmidt passes were 46 % of the corrector.  theta (optional): Newton shifts, p_{i+1} = (A - theta_i) p_i.  On return *s_eff <= s steps were accepted (sstep.h: the block is truncated
// where its vectors lose independence; the trailing operator applications are then void) and the raw Hessenberg columns
// j .. j + *s_eff - 1 are in Hraw; *s_eff = 0: nothing usable (or out of the kernels' range) -- the caller repeats the step on the
// single-vector path from V[j] (the measured Gram matrix stays valid up to and including column j - 1).
struct PendingBlock {              // a block whose update pass (pass 2) has not run yet: slots k .. k+s-1 still hold the raw P
    bool active = false;
    int k = 0, s = 0;
    double Cm[32 * sstep::kS], Tm[sstep::kS * sstep::kS];
};

int arnoldi_block(bk_ctx* ctx, bk_op* A, Basis& B, int j, int s, double* Hraw, int ldh, double op_a0, double op_a1, int* s_eff,
                  double* last_ratio, const double* theta, PendingBlock* defer = nullptr) {
    const size_t n = A->n;
    const int k = j + 1, u = k - B.gram_n;
    *s_eff = 0;
    if (A->ntail != 0 || !B.use_gram || u < 0 || u > sstep::kS || s < 1 || s > sstep::kS || u + s > sstep::kR || k > 32 ||
        !v_block_ok(ctx, n, B.V, B.ld))
        return 0;
    // p_{i+1} = (op_a0 + op_a1 A) p_i - theta_i p_i: the shift rides in the operator's own a0 term
    double* outs[sstep::kS];
    for (int i = 0; i < s; ++i) outs[i] = B.vec(j + i + 1);
    BK_TRY(A->apply_block(B.vec(j), s, op_a0, op_a1, theta, outs));
    double D[33 * sstep::kR], T[sstep::kTri];
    PendingBlock local;
    PendingBlock* pb = defer ? defer : &local;
    BK_TRY(v_block_dots(ctx, n, B.V, B.ld, k - u, k - u, u + s, D, T));
    const int st = sstep::block_coefficients(k, u, s, D, T, B.G.data(), kMaxBasis + 1, Hraw, ldh, pb->Cm, pb->Tm, s_eff, last_ratio, theta);
    B.gram_n = st == 0 ? k : j;                      // (a refused block: column j is measured again by the single step)
    if (st != 0) { *s_eff = 0; return 0; }
    // deferred: the Hessenberg columns are complete without the update pass; the caller runs it when the new vectors are needed
    // explicitly -- or folds it into the solution update if the solve ends inside this block (gmres_core)
    if (defer) { pb->active = true; pb->k = k; pb->s = *s_eff; return 0; }
    return v_block_axpy(ctx, n, B.V, B.ld, k, *s_eff, pb->Cm, pb->Tm);
}

}  // namespace

// Arnoldi step on a caller-owned basis (eig.hip)
// G / gram_n != NULL: the Gram-corrected single-pass step on the caller's Gram matrix ((kMaxBasis + 1)^2, column-major; the
// caller rotates it with the basis at a thick restart); a step that cannot take it falls back to the two passes.
int arnoldi_step_public(bk_ctx* ctx, bk_op* A, double* V, size_t ld, std::vector<double>& tails, int j, double* w,
                        double* h, double* beta, std::vector<double>* G, int* gram_n) {
    Basis B;
    B.V = V;
    B.ld = ld;
    B.nt = A->ntail;
    B.t.swap(tails);
    if (G && gram_n) { B.use_gram = true; B.G.swap(*G); B.gram_n = *gram_n; }
    const int s = arnoldi_step(ctx, A, B, j, w, h, beta, 0.0, 1.0, 2.0);      // (eta = 2: a step that cannot take the Gram pass takes two passes)
    if (G && gram_n) { B.G.swap(*G); *gram_n = B.gram_n; }
    B.t.swap(tails);
    return s;
}

// ================================================================== GMRES
int gmres_core(bk_ctx* ctx, bk_op* A, const double* b, const double* bt, double* x, double* xt, double alpha0,
               double alpha1, const bk_gmres_opts& o, GmresResult* res) {
    const size_t n = A->n;
    const int nt = A->ntail;
    const int m = o.dim;
    if (m < 1 || m > kMaxBasis - 1) return set_error(ctx, "gmres: Krylov dimension %d outside [1, %d]", m, kMaxBasis - 1);
    const bool kk = (o.flavor == BK_GMRES_KRYLOVKIT);
    // KrylovKit builds the Krylov space on A and applies (alpha0, alpha1) to the Hessenberg matrix;
    // IterativeSolvers iterates on the shifted operator itself.
    // (operators that ask for it -- bk_op::hessenberg_shift -- get KrylovKit's arrangement in every flavor: same space, same
    // iterates, and the shift costs no stream)
    const bool hs = kk || A->hessenberg_shift();
    const double op_a0 = hs ? 0.0 : alpha0, op_a1 = hs ? 1.0 : alpha1;
    const double s0 = hs ? alpha0 : 0.0, s1 = hs ? alpha1 : 1.0;
    VecOps vo{ctx, n, nt};
    // DGKS threshold: re-orthogonalise only when the remainder keeps less than eta of the norm.  One CGS pass leaves
    // |V'v| <= ~eps/eta, so eta = 0.1 still gives orthogonality ~2e-15 while skipping the second pass on operators
    // close to the identity (KrylovKit's IR variants use 1/sqrt(2); measured at 512^3: same residuals, half the time).
    const double eta = ctx->opt("dgks_eta", 0.1);
    WsGuard ws(ctx);
    Basis B;
    B.ld = round_up(n, 32);
    BK_TRY(ws.get(B.ld * (size_t)(m + 1), &B.V));
    B.nt = nt;
    B.orth_tol = ctx->opt("orth_tol", 1e-8);
    B.t.assign((size_t)(m + 1) * (nt > 0 ? nt : 1), 0.0);
    B.use_gram = ctx->opt("gmres_gram", 1.0) != 0.0;
    if (B.use_gram) B.G.assign((size_t)(kMaxBasis + 1) * (kMaxBasis + 1), 0.0);
    double *w = nullptr, *r = nullptr;
    BK_TRY(ws.get(B.ld, &w));
    BK_TRY(ws.get(B.ld, &r));

    // Device-resident Arnoldi chunks (option gmres_chunk; default: 4 steps for vectors that live in the caches, 1 = the
    // host-driven step for HBM-sized vectors): `chunk` steps are enqueued back to back -- operator, V'w, coefficients,
    // V_k = (w - V h)/beta all in the stream, coefficients never leaving the device -- and the host picks the Hessenberg
    // columns up after ONE synchronisation, replaying its Givens / convergence logic on them.  Steps past convergence are
    // discarded (they cost launch-bound microseconds at these sizes); a step whose classical Gram-Schmidt pass needs the
    // DGKS second pass (or broke down) is flagged by the device and repeated on the host path.  Counters (numops / iters)
    // count consumed steps only, so they equal the host-driven run.
    // (round 2 switched the chunks off above 8 MiB: every step speculated past convergence costs a whole operator application
    // there.  With the convergence-predicted cap below the speculation is almost never wasted, and at 512^3 the chunks are worth
    // 2 % -- 6.33 -> 6.19 ms per operator application, profiles/r3_bench_512_variants.txt -- and 8 % on the 128-MiB z-slab of an
    // 8-rank run, where the host round trip per Arnoldi step is a larger share.)
    // The decision must be the same on every rank (a rank on the device path issues in-stream all-reduces its peer on the
    // host path never joins): it does not look at the rank-local length at all -- ragged z-slabs may straddle any size
    // threshold -- only at options and at the communicator kind.
    const bool rccl_ranks = ctx->nranks > 1;        // (both communicator kinds enqueue their collectives in the stream)
    // Block Arnoldi (round 4, option gmres_sstep = largest block, default 4 for vectors that stream from HBM, 0 = off): s
    // operator applications, then ONE pair of Gram-Schmidt passes for the s steps (arnoldi_block, sstep.h).  The steps of a
    // block are speculated like the device-resident chunks -- the convergence-predicted cap below applies -- and the host
    // consumes the Hessenberg columns one at a time with the same Givens / stopping logic, so iterates and counters are those
    // of the step-by-step run.  The decision looks at options and the GLOBAL problem only (every rank takes the same one).
    // On at every size (a negative value = the default, 4): for vectors that stream from HBM it halves the Gram-Schmidt traffic,
    // for cache-resident ones it replaces ~8 dependent launches per step by ~5 and one host synchronisation per block (C2, SH2d
    // 512^2: 51.6 -> 39.2 us per operator application, profiles/r4_c2_block_ab.jsonl).  No rank-local quantity decides.
    const double sstep_opt = ctx->opt("gmres_sstep", -1.0);
    const int sstep_max = std::min(sstep_opt < 0.0 ? 4 : (int)sstep_opt, sstep::kS);
    const bool sstep_on = sstep_max >= 1 && nt == 0 && B.use_gram && m >= 2 && v_block_ok(ctx, n, B.V, B.ld);
    const int ldh = m + 2;
    std::vector<double> Hraw(sstep_on ? (size_t)ldh * m : 0, 0.0);   // raw (unrotated) Hessenberg columns of the cycle
    // Block length.  A solve does NOT depend on the solves before it (results are reproducible whatever the call sequence; the
    // two lanes of linsolve2 reproduce the sequential calls bitwise): its first block is monomial and at most kMonomialMax = 3
    // long -- down a monomial block the pivots fall by ~1e-2 per vector (sstep.h), three stay above the truncation threshold --,
    // the later ones take Newton shifts from the Hessenberg matrix at hand and may be sstep_max long; a truncated block
    // shrinks the next ones, a comfortable last pivot lets them grow again.  The one thing carried over is the ramp of the
    // device-resident chunks: a solve whose predecessor needed <= 2 steps (config 3 with the exact block preconditioner
    // converges in ONE) starts with single steps -- block boundaries move, iterates and counters do not.
    constexpr int kMonomialMax = 3;
    int blk_cur = ctx->gmres_last_steps <= 2 ? 1 : sstep_max;
    // Newton shifts of the blocks (sstep.h: Conditioning): up to kS Ritz values of the operator in Leja order, where a shift is
    // free (bk_op::shift_is_free), from the Hessenberg matrix of THIS solve as soon as one block exists.  (Option
    // gmres_newton_carry = 1 also starts from the previous solve's set -- correctors solve with the same operator family again
    // and again: 2 % at 512^3 -- at the price of solves that depend on the context's history; a carried set that truncates a
    // block is dropped.  Any real numbers give a valid basis: the shifts only steer its conditioning.)
    const bool use_shifts = sstep_on && ctx->opt("gmres_newton", 1.0) != 0.0 && A->shift_is_free();
    const bool carry = use_shifts && ctx->opt("gmres_newton_carry", 0.0) != 0.0;
    std::vector<double> shifts;
    bool shifts_carried = false;
    if (carry && !ctx->newton_shifts.empty()) { shifts = ctx->newton_shifts; shifts_carried = true; }
    // First block (no Ritz values yet).  On the stencil-free operator T = W + theta0 I (ShiftPrecOp) there are two candidates: powers of
    // the literal operator W = Pl^-1 J (bk_op::monomial_shift = theta0; rounds 4-5) and powers of T itself (the default since round 6,
    // kMonomialShiftDefault).  W's spectrum clusters at -1, so W^k p is dominated by (-1)^k p and three vectors leave a last pivot ratio
    // of 6.6e-7 / 6.9e-7 on the 512^3 headline solves -- one and a half orders above the truncation threshold 1e-8 (sstep.h); T's
    // clusters at 0 and three powers of it keep 8.1e-3 / 2.6e-3 (profiles/r6_first_block_ab_512.txt; round 5's experiment:
    // r5_block_log_first_block_T_powers.txt).  Every later block is identical either way (its Newton shifts come from the Hessenberg
    // matrix, Leja-ordered from W's origin: bk_op::rearranged_origin), the step is 2.4 % shorter on identical inputs (no shift stream in
    // the x-inverse pass of three applications per solve), and a first block of FOUR powers of T truncates the second block (4th pivot
    // 1.7e-5, +4 ms per step): kMonomialMax stays 3.
    // (Round 4's "structural first-block shift" on the LITERAL CHAIN -- the same powers of T reached by folding the shift a0 - a1 through
    // the stencil kernel, first blocks 4 long -- is what truncated at 512^3 then: 122.9 vs 116.6 ms per step.)
    const bool leja_origin_on = ctx->opt("gmres_leja_origin", 1.0) != 0.0;
    auto ritz_shifts = [&](int kk) {              // Leja-ordered real parts of the eigenvalues of Hraw[0:kk, 0:kk]
        if (!use_shifts || kk < 2) return;
        dense::Mat Hm(kk, kk);
        for (int c = 0; c < kk; ++c)
            for (int r = 0; r < kk && r <= c + 1; ++r) Hm(r, c) = Hraw[(size_t)r + (size_t)c * ldh];
        std::vector<dense::cplx> ev;
        dense::CMat Y;
        if (dense::eig_general(Hm, ev, Y) != 0) return;
        std::vector<double> pts;
        for (const auto& e : ev) pts.push_back(e.real());
        std::vector<double> lj;
        std::vector<char> used(pts.size(), 0);
        // Leja order: the first point is the one farthest from the origin of the operator the solve is about -- for an operator that
        // iterates on a rearranged form A = W + theta0 I (bk_op::monomial_shift) that origin sits at theta0, so the order (and with it the
        // blocks' conditioning) is the one the literal operator W would get: the later points only depend on mutual distances
        const double origin = leja_origin_on ? A->rearranged_origin() : 0.0;
        for (int t = 0; t < sstep::kS && t < (int)pts.size(); ++t) {
            int best = -1;
            double bv = -1.0;
            for (size_t i = 0; i < pts.size(); ++i) {
                if (used[i]) continue;
                double v = t == 0 ? std::fabs(pts[i] - origin) : 1.0;
                for (double q : lj) v *= std::fabs(pts[i] - q);
                if (v > bv) { bv = v; best = (int)i; }
            }
            used[best] = 1;
            lj.push_back(pts[best]);
        }
        shifts = lj;
        shifts_carried = false;
    };
    int chunk = (int)ctx->opt("gmres_chunk", 4.0);
    // (with blocks on, the chunks only take over where the basis has outgrown the block kernels -- beyond 32 vectors: restart = 63
    // cycles, unpreconditioned solves -- instead of host-synchronised single steps)
    if (nt != 0 || chunk < 2 || !ctx->h_rec_dev) chunk = 1;
    if (chunk > kRecChunks) chunk = kRecChunks;
    // Speculation cap from the residual history (all quantities are all-reduced, i.e. identical on every rank): with the
    // last reduction factor rho = beta_k / beta_{k-1} the estimate reaches the tolerance after `need` further steps; never
    // enqueue more than that.  GMRES converges at least that fast from there on (superlinearly, usually), so a speculated
    // step is rarely wasted, and when the prediction was too optimistic the next chunk simply follows.  For vectors that
    // stream from HBM a wasted step is a whole operator application; the cache-resident sizes keep the plain ramp
    // (option gmres_predict: 1 = always, 0 = never, default: HBM-sized vectors and RCCL ranks).
    const bool predict = ctx->opt("gmres_predict", (rccl_ranks || sstep_on || n > ((size_t)1 << 20)) ? 1.0 : 0.0) != 0.0;
    // (the prediction asks for the estimate to reach pmargin x tolerance: option gmres_predict_margin, default 1.  An optimistic prediction
    // costs a whole extra block -- projection pass, update pass, synchronisation: 4-5 ms at 512^3 -- for the one step it missed, a
    // pessimistic one at most one operator application past convergence (3.6 ms), and the estimate of a nearly converged solve flattens
    // out rather than speeds up.  Rounds 3-4 used 2: measured in round 5 on two sizes x two block orderings, 1 wins every pairing
    // (512^3 headline 98 -> 92 ms; profiles/r5_predict_margin_leja_sweep.txt))
    const double pmargin = ctx->opt("gmres_predict_margin", 1.0);
    // (options read once per solve: nothing inside the block loop looks anything up by name)
    const bool block_log = ctx->opt("gmres_block_log", 0.0) != 0.0;
    const bool defer_update = ctx->opt("gmres_defer_update", 1.0) != 0.0;
    const bool orth_probe = ctx->opt("orth_probe", 0.0) != 0.0;
    // cycle start (option gmres_fuse_v0): V[0] = r / beta written by the first operator application of the cycle instead of a pass of
    // its own -- block cycles of unbordered operators only (the blocks' chained applications are what the fused pass belongs to)
    const bool fuse_v0 = sstep_on && nt == 0 && ctx->opt("gmres_fuse_v0", 1.0) != 0.0;
    if (block_log) ctx->block_log_solves += 1;
    double beta_prev = 0.0, beta_now = 0.0, tol_now = 0.0;
    double* d_coef = nullptr;
    const double* h_rec = ctx->h_rec;          // the records land in pinned, device-mapped host memory: no copy operation
    int q_first = 0, q_count = 0;              // columns q_first .. q_first + q_count - 1 of this cycle wait in h_rec
    // Speculation ramp: a solve whose predecessor on this context needed <= 2 steps (an exact preconditioner: config 3 on the
    // trivial branch converges in ONE) starts with a chunk of 1 and doubles from there, so that it does not pay for 3
    // speculative operator applications per solve (cGL 1024^2 eigensolve: 1.38 -> 0.70 s); everything else starts with full chunks
    int ramp = (ctx->gmres_last_steps <= 2) ? 1 : chunk;
    if (chunk > 1) BK_TRY(ws.get((size_t)kMaxBasis + 4, &d_coef));
    // device Gram matrix of the Gram-corrected step; dev_gram: every column of this cycle was measured on the device so far
    double* d_gram = nullptr;
    bool dev_gram = false, cycle_on_host = false;
    bool blocks_done = false;                  // this cycle's basis is past the block kernels' range: the device chunks continue it
    if (chunk > 1 && B.use_gram && !sstep_on) BK_TRY(ws.get((size_t)(kMaxBasis + 1) * (kMaxBasis + 1), &d_gram));
    // next Hessenberg column (Arnoldi step from V[j]): from the queue of device-computed columns, else computed now
    // The update pass of a block (Q_new = (P - QC) R^-1, k + 2s vector streams) is DEFERRED: the block's Hessenberg columns
    // do not need it.  It runs when the new vectors are needed explicitly -- the next block, a restart's residual -- and is
    // folded into the solution update when the solve ends inside the block: x = Q y_old + Q_new y_new =
    // Q (y_old - C R^-1 y_new) + P (R^-1 y_new), ONE multiaxpy over [Q, P] instead of the update pass plus a multiaxpy over
    // [Q, Q_new] (the last block of every solve: ~13 % of the Gram-Schmidt traffic of a 12-step solve).
    int blk_accepted = 0, blk_consumed = 0;         // diagnostics: block steps accepted by the host algebra / handed to the Givens logic
    PendingBlock pend;
    auto flush_pending = [&]() -> int {
        if (!pend.active) return 0;
        pend.active = false;
        return v_block_axpy(ctx, n, B.V, B.ld, pend.k, pend.s, pend.Cm, pend.Tm);
    };
    auto next_column = [&](int j, double* hcol, double* hnext_out) -> int {
        if (!(q_count > 0 && j >= q_first && j < q_first + q_count)) BK_TRY(flush_pending());   // new work starts from explicit vectors
        if (sstep_on && !cycle_on_host && !blocks_done && chunk > 1 && j + 1 > 32 &&
            !(q_count > 0 && j >= q_first && j < q_first + q_count)) {
            // hand the rest of the cycle to the device-resident chunks (two-pass policy: the device has no Gram matrix of this basis, its
            // defect estimate starts at the tolerance, i.e. on the safe side -- what the host path does in the same situation)
            blocks_done = true;
            ctx->diag.chunk_handover += 1.0;
            dev_gram = false;
            q_count = 0;
            const double ot = B.orth_tol;
            BK_HIP(ctx, hipMemcpyAsync(d_coef + kMaxBasis + 2, &ot, sizeof(double), hipMemcpyHostToDevice, ctx->stream));
            BK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        }
        if (sstep_on && !cycle_on_host && !blocks_done) {
            if (!(q_count > 0 && j >= q_first && j < q_first + q_count)) {
                int steps = std::min(std::min(blk_cur, shifts.empty() ? kMonomialMax : sstep_max), m - j);
                const bool capped = steps < blk_cur;
                bool predicted = false;
                if (predict && steps > 1 && beta_now > 0.0) {
                    const double rho = (beta_prev > 0.0 && beta_now < beta_prev) ? beta_now / beta_prev : 1.0;
                    int need = 1;
                    for (double b_ = beta_now * rho; b_ > pmargin * tol_now && need < steps; b_ *= rho) ++need;
                    predicted = need < steps;
                    steps = need;
                }
                int got = 0;
                double ratio = 0.0;
                double theta[sstep::kS] = {0.0, 0.0, 0.0, 0.0};
                for (int i = 0; i < steps && !shifts.empty(); ++i) theta[i] = shifts[i % shifts.size()];
                const double mono = shifts.empty() ? A->monomial_shift() : 0.0;      // (blocks without Ritz values: bk_op::monomial_shift)
                if (mono != 0.0) for (int i = 0; i < steps; ++i) theta[i] = mono;
                const bool shifted = !(shifts.empty() && mono == 0.0);
                BK_TRY(arnoldi_block(ctx, A, B, j, steps, Hraw.data(), ldh, op_a0, op_a1, &got, &ratio, shifted ? theta : nullptr,
                                     defer_update ? &pend : nullptr));
                if (block_log) {
                    // one record per block (bk_solver_block_log; common.h: kBlockLogRec); theta slots the block did not use are NaN
                    const double rec[bk_ctx::kBlockLogRec] = {(double)ctx->block_log_solves, (double)j, (double)steps, (double)got, ratio,
                                                              shifted && steps > 0 ? theta[0] : NAN, shifted && steps > 1 ? theta[1] : NAN,
                                                              shifted && steps > 2 ? theta[2] : NAN, shifted && steps > 3 ? theta[3] : NAN,
                                                              beta_now, tol_now};
                    ctx->block_log.insert(ctx->block_log.end(), rec, rec + bk_ctx::kBlockLogRec);
                }
                if (got < steps && shifts_carried) { shifts.clear(); shifts_carried = false; }     // a stale set: back to the monomial block
                if (got > 0 && !shifts_carried && ((int)shifts.size() < sstep::kS || j + got <= 12)) ritz_shifts(j + got);
                // diagnostics (bench.py reports them): operator applications issued by blocks / of those void (truncated tails)
                // ("truncated": tails of blocks cut at a small pivot; "unconsumed", counted at the end of the solve: accepted steps the
                // host never needed because the solve converged earlier in the block -- speculation past convergence)
                ctx->diag.block_steps += steps;
                ctx->diag.block_truncated += steps - got;
                blk_accepted += got;
                if (got > 0) {
                    q_first = j; q_count = got;
                    // next block: shorter after a truncation, one step longer when the last pivot left room (sstep.h)
                    if (got < steps) blk_cur = got;
                    else if (!capped && !predicted && blk_cur < sstep_max && ratio >= sstep::kGrowRatio) blk_cur += 1;
                } else {
                    cycle_on_host = true; q_count = 0;           // refused: the rest of the cycle runs step by step
                }
            }
            if (!cycle_on_host) {
                for (int i = 0; i <= j; ++i) hcol[i] = Hraw[(size_t)i + (size_t)j * ldh];
                *hnext_out = Hraw[(size_t)(j + 1) + (size_t)j * ldh];
                blk_consumed += 1;
                return 0;
            }
        }
        if (chunk > 1 && !cycle_on_host && (!sstep_on || blocks_done)) {
            if (!(q_count > 0 && j >= q_first && j < q_first + q_count)) {
                int steps = std::min(std::min(ramp, chunk), m - j);
                if (predict && steps > 1 && beta_now > 0.0) {
                    const double rho = (beta_prev > 0.0 && beta_now < beta_prev) ? beta_now / beta_prev : 1.0;
                    int need = 1;
                    for (double b_ = beta_now * rho; b_ > pmargin * tol_now && need < steps; b_ *= rho) ++need;
                    steps = need;
                }
                ramp = std::min(chunk, 2 * ramp);
                for (int s2 = 0; s2 < steps; ++s2) {
                    BK_TRY(A->apply(B.vec(j + s2), nullptr, op_a0, op_a1, w, nullptr));
                    // beyond the Gram kernels' range (32 vectors) the cycle continues with the two-pass device policy
                    const bool gstep = dev_gram && j + s2 + 1 <= 32;
                    if (dev_gram && !gstep) {
                        dev_gram = false;
                        const double ot = B.orth_tol;
                        BK_HIP(ctx, hipMemcpyAsync(d_coef + kMaxBasis + 2, &ot, sizeof(double), hipMemcpyHostToDevice, ctx->stream));
                        BK_HIP(ctx, hipStreamSynchronize(ctx->stream));
                    }
                    BK_TRY(v_arnoldi_step_dev(ctx, n, B.V, B.ld, j + s2 + 1, w, eta, B.orth_tol,
                                              ctx->h_rec_dev + (size_t)s2 * (kMaxBasis + 2), d_coef, gstep ? d_gram : nullptr));
                }
                BK_TRY(ctx_sync(ctx));
                q_first = j; q_count = steps;
            }
            const double* rec = h_rec + (size_t)(j - q_first) * (kMaxBasis + 2);
            if (rec[kMaxBasis + 1] == 0.0) {
                for (int i = 0; i <= j; ++i) hcol[i] = rec[i];
                *hnext_out = rec[kMaxBasis];
                return 0;
            }
            if (dev_gram) cycle_on_host = true;   // (the device Gram matrix misses this step's column: the cycle stays on the host)
            q_count = j - q_first;             // flagged: this and the later speculative steps are void; redo on the host path
            B.dlt = B.orth_tol;                // (the device kept the defect estimate: stay on the safe side on the host ...
            {                                  //  ... and on the device, whose later chunks would otherwise trust a stale estimate)
                const double ot = B.orth_tol;
                BK_HIP(ctx, hipMemcpyAsync(d_coef + kMaxBasis + 2, &ot, sizeof(double), hipMemcpyHostToDevice, ctx->stream));
                BK_HIP(ctx, hipStreamSynchronize(ctx->stream));
            }
        }
        return arnoldi_step(ctx, A, B, j, w, hcol, hnext_out, op_a0, op_a1, eta);
    };

    bool x_zero = true;                        // x0 = 0 is never materialised: the first update writes x = V y
    double xtail[BK_MAX_BORDER] = {0.0};
    double bnorm = 0.0;
    BK_TRY(vo.nrm2(b, bt, &bnorm));
    double beta = bnorm;                       // x0 = 0  =>  r0 = b
    // stopping rules: KrylovKit max(atol, rtol*||b||); IterativeSolvers max(reltol*||r0||, abstol); Krylov.jl
    // atol + rtol*||r0||  
    const double tol = kk ? std::max(o.atol, o.rtol * bnorm)
                          : (o.flavor == BK_GMRES_KRYLOVJL ? o.atol + o.rtol * bnorm : std::max(o.rtol * bnorm, o.atol));
    int numops = kk ? 1 : 0;                   // KrylovKit applies A once to x0 to fix the scalar type
    int iters = 0;                             // IterativeSolvers counts inner iterations
    res->converged = 0;
    if (kk ? (beta < tol) : (beta <= tol)) {
        BK_TRY(v_zero(ctx, n, x));
        res->converged = 1; res->niter = kk ? numops : 0; res->resnorm = beta;
        if (xt) for (int q = 0; q < nt; ++q) xt[q] = 0.0;
        return 0;
    }
    const double* rsrc = b;                    // first cycle: r0 = b, read in place (no copy)
    double rt[BK_MAX_BORDER] = {0.0};
    for (int q = 0; q < nt; ++q) rt[q] = bt[q];

    std::vector<double> R((size_t)m * m, 0.0), y(m + 1, 0.0), cs(m, 0.0), sn(m, 0.0), h(m + 1, 0.0), col(m + 1, 0.0);
    auto Rat = [&](int i, int j) -> double& { return R[(size_t)i + (size_t)j * m]; };
    int numiter = 0;
    double hnext = 0.0;
    const bool trace = ctx->opt("solver_trace", 0.0) != 0.0;
    if (trace) { ctx->hist_solves += 1; ctx->hist.push_back(-(double)ctx->hist_solves); ctx->hist.push_back(beta); }

    auto start_cycle = [&]() -> int {        // V[0] = r / beta ; first Arnoldi column
        // (fuse_v0: the operator writes V[0] in the first transform pass of the application next_column(0) starts with -- bk_op::arm_v0;
        // the same product per element, one read stream and one launch fewer)
        if (!(fuse_v0 && aligned16(rsrc) && rsrc != B.vec(0) && A->arm_v0(rsrc, 1.0 / beta, B.vec(0))))
            BK_TRY(v_axpbyz(ctx, n, 1.0 / beta, rsrc, 0.0, nullptr, B.vec(0)));
        rsrc = r;
        for (int q = 0; q < nt; ++q) B.tail(0)[q] = rt[q] / beta;
        B.dlt = 0.0;                           // a single vector is orthonormal
        B.gram_n = 0;                          // ... and its Gram column is measured by the first step
        dev_gram = d_gram != nullptr;
        cycle_on_host = false;
        blocks_done = false;
        if (chunk > 1) BK_HIP(ctx, hipMemsetAsync(d_coef + kMaxBasis + 2, 0, sizeof(double), ctx->stream));
        q_count = 0;                           // a new cycle: nothing speculative carries over
        pend.active = false;                   // (a deferred update of the finished cycle is void with its basis)
        beta_prev = 0.0; beta_now = beta; tol_now = tol;
        const int e0 = next_column(0, h.data(), &hnext);
        if (e0 != 0) { A->disarm_v0(); return e0; }      // (an armed V[0] does not outlive a failed cycle start)
        numops += 1;
        return 0;
    };

    const int max_cycles = kk ? o.maxiter : 1 << 30;
    BK_TRY(start_cycle());
    while (numiter < max_cycles) {
        numiter += 1;
        std::fill(y.begin(), y.end(), 0.0);
        y[0] = beta;
        int k = 0;
        bool stop = false;
        while (true) {
            // column k of the (shifted) Hessenberg is in h[0..k], hnext
            k += 1;
            iters += 1;
            for (int i = 0; i < k; ++i) col[i] = s1 * h[i];
            col[k - 1] += s0;
            for (int i = 0; i < k - 1; ++i) {
                const double t = cs[i] * col[i] + sn[i] * col[i + 1];
                col[i + 1] = -sn[i] * col[i] + cs[i] * col[i + 1];
                col[i] = t;
            }
            double rr;
            dense::givens(col[k - 1], s1 * hnext, cs[k - 1], sn[k - 1], rr);
            col[k - 1] = rr;
            for (int i = 0; i < k; ++i) Rat(i, k - 1) = col[i];
            y[k] = -sn[k - 1] * y[k - 1];
            y[k - 1] = cs[k - 1] * y[k - 1];
            beta_prev = beta;
            beta = std::fabs(y[k]);
            beta_now = beta;
            if (trace) ctx->hist.push_back(beta);
            const bool conv = kk ? !(beta > tol) : (beta <= tol);
            if (conv || k >= m || hnext == 0.0) break;
            if (!kk && iters >= o.maxiter) { stop = true; break; }
            BK_TRY(next_column(k, h.data(), &hnext));
            numops += 1;
        }
        if (orth_probe && nt == 0) {
            BK_TRY(flush_pending());
            // diagnostics (tests): the MEASURED orthogonality defect max |V'V - I| of this cycle's basis V[0..k] next to the
            // running estimate the single-pass policy steers by -- options gmres_last_orth_defect / gmres_last_orth_estimate
            double worst = 0.0, row[kMaxBasis + 1];
            const int nb = hnext != 0.0 ? k + 1 : k;
            for (int i = 0; i < nb; ++i) {
                BK_TRY(v_multidot(ctx, n, B.V, B.ld, nb, B.vec(i), row));
                for (int j = 0; j < nb; ++j) worst = std::max(worst, std::fabs(row[j] - (i == j ? 1.0 : 0.0)));
            }
            double est = B.dlt;
            if (chunk > 1) {
                BK_HIP(ctx, hipMemcpyAsync(&est, d_coef + kMaxBasis + 2, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
                BK_HIP(ctx, hipStreamSynchronize(ctx->stream));
                est = std::max(est, B.dlt);
            }
            ctx->diag.last_orth_defect = std::max(worst, numiter > 1 ? ctx->diag.last_orth_defect : 0.0);
            ctx->diag.last_orth_estimate = est;
        }
        // solve R yk = y[0..k) and update x += V[0..k) yk
        std::vector<double> yk(k);
        for (int i = k - 1; i >= 0; --i) {
            double s = y[i];
            for (int j = i + 1; j < k; ++j) s -= Rat(i, j) * yk[j];
            yk[i] = s / Rat(i, i);
        }
        if (pend.active && k > pend.k) {
            // the solve (or the cycle) ends inside the deferred block: c of its vectors carry solution coefficients
            std::vector<double> cf(k, 0.0);
            ctx->diag.block_folded += 1.0;
            sstep::fold_solution_coefficients(pend.k, k - pend.k, pend.Cm, pend.Tm, yk.data(), cf.data());
            BK_TRY(v_multiaxpy(ctx, n, B.V, B.ld, k, cf.data(), x_zero ? nullptr : x, 1.0, x, nullptr));
        } else {
            BK_TRY(v_multiaxpy(ctx, n, B.V, B.ld, k, yk.data(), x_zero ? nullptr : x, 1.0, x, nullptr));
        }
        x_zero = false;
        for (int q = 0; q < nt; ++q) for (int i = 0; i < k; ++i) xtail[q] += yk[i] * B.tail(i)[q];

        if (kk) {
            if (beta > tol && hnext != 0.0) {
                // residual from the Krylov data: r = y[k] * V[0..k] * (G_1' ... G_k' e_{k+1})
                std::vector<double> z(k + 1, 0.0);
                z[k] = 1.0;
                for (int i = k - 1; i >= 0; --i) {
                    const double t = cs[i] * z[i] - sn[i] * z[i + 1];
                    z[i + 1] = sn[i] * z[i] + cs[i] * z[i + 1];
                    z[i] = t;
                }
                for (int i = 0; i <= k; ++i) z[i] *= y[k];
                BK_TRY(flush_pending());           // the residual vector needs V[0..k] explicitly
                BK_TRY(v_multiaxpy(ctx, n, B.V, B.ld, k + 1, z.data(), nullptr, 1.0, r, nullptr));
                for (int q = 0; q < nt; ++q) { rt[q] = 0.0; for (int i = 0; i <= k; ++i) rt[q] += z[i] * B.tail(i)[q]; }
            } else {
                // explicit residual r = b - (a0 + a1 A) x, "to ensure that no numerical errors have accumulated"
                double wt[BK_MAX_BORDER] = {0.0};
                numops += 1;
                // the norm alone first where the operator has it without the residual vector (bk_op::check_norm: from the spectrum
                // of the preconditioner, three passes instead of seven); a value that passes is all the solve takes from the check
                bool spectral_failed = false;
                if (nt == 0) {
                    int have = 0;
                    double bs = 0.0;
                    BK_TRY(A->check_norm(x, alpha0, alpha1, &bs, &have));
                    if (have && bs < tol) { beta = bs; res->converged = 1; break; }
                    spectral_failed = have != 0;
                }
                // (a value that failed: the same check through the chain, continued from the stencil pass check_norm has run)
                if (spectral_failed) BK_TRY(A->apply_check_resume(x, alpha0, alpha1, w));
                else BK_TRY(A->apply_check(x, nt ? xtail : nullptr, alpha0, alpha1, w, wt));
                for (int q = 0; q < nt; ++q) rt[q] = bt[q] - wt[q];
                // the norm first, from b and w as they are (two read streams); the residual VECTOR is only formed when the check fails
                // and another cycle has to start from it
                BK_TRY(v_diff_nrm2(ctx, n, b, w, &beta));
                if (nt) { double s_ = beta * beta; for (int q = 0; q < nt; ++q) s_ += rt[q] * rt[q]; beta = std::sqrt(s_); }
                if (beta < tol) { res->converged = 1; break; }
                BK_TRY(v_axpbyz(ctx, n, 1.0, b, -1.0, w, r));
            }
            if (numiter < max_cycles) {
                BK_TRY(vo.nrm2(r, rt, &beta));
                if (beta == 0.0) { res->converged = 1; break; }
                BK_TRY(start_cycle());
            }
        } else {
            if (beta <= tol) {
                if (!A->hessenberg_shift()) { res->converged = 1; break; }
                // The cycle ran on an algebraically rearranged operator (ShiftPrecOp, stencil-free form): before the solve returns
                // `converged` on the Arnoldi estimate alone, the residual is evaluated once through the ORIGINAL chain (stencil kernel,
                // plain preconditioner), as the KrylovKit flavor does after every converged cycle -- a mismatch between the stencil's L1
                // and the spectral one cannot pass silently in any flavor.  Within 1.5 x the tolerance the estimate stands
                // (and is what the solve reports, as IterativeSolvers / Krylov.jl do); beyond it the solve continues from the true residual.
                double bt_ = 0.0;
                int have = 0;
                BK_TRY(A->check_norm(x, alpha0, alpha1, &bt_, &have));
                if (have && bt_ <= 1.5 * tol) { res->converged = 1; break; }
                if (have) BK_TRY(A->apply_check_resume(x, alpha0, alpha1, w));
                else BK_TRY(A->apply_check(x, nullptr, alpha0, alpha1, w, nullptr));
                BK_TRY(v_diff_nrm2(ctx, n, b, w, &bt_));
                if (bt_ <= 1.5 * tol) { res->converged = 1; break; }
                ctx->diag.check_mismatch += 1.0;
                if (stop || iters >= o.maxiter) { beta = bt_; break; }
                BK_TRY(v_axpbyz(ctx, n, 1.0, b, -1.0, w, r));
                beta = bt_;
                BK_TRY(start_cycle());
                continue;
            }
            if (stop || iters >= o.maxiter) break;
            double wt[BK_MAX_BORDER] = {0.0};
            BK_TRY(A->apply_check(x, nt ? xtail : nullptr, alpha0, alpha1, w, wt));
            BK_TRY(v_axpbyz(ctx, n, 1.0, b, -1.0, w, r));
            for (int q = 0; q < nt; ++q) rt[q] = bt[q] - wt[q];
            BK_TRY(vo.nrm2(r, rt, &beta));
            if (beta <= tol) { res->converged = 1; break; }
            BK_TRY(start_cycle());
        }
    }
    res->niter = kk ? numops : iters;
    res->resnorm = beta;
    if (sstep_on) ctx->diag.block_unconsumed += blk_accepted - blk_consumed;
    ctx->gmres_last_steps = iters;
    if (carry && !shifts.empty()) ctx->newton_shifts = shifts;
    if (xt) for (int q = 0; q < nt; ++q) xt[q] = xtail[q];
    return 0;
}

namespace {

// v -> a0 v + a1 Pl^-1 (J v)   (order 0: KrylovKit branch, src/LinearSolver.jl:270-277)
// v -> Pl^-1 (a0 v + a1 J v)   (order 1: IterativeSolvers `Pl`, :198-201)
// v -> a0 v + a1 J v           (no preconditioner; used by the IterativeSolvers flavor)
//
// Stencil-free mode (round 5; option gmres_stencil_free, default on where the transform kernels can take the pointwise work in).
// With the spectral preconditioner of the SAME Swift-Hohenberg problem, Pl = L1 + s I and J = -L1 + diag g(u), so
//     Pl^-1 J = Pl^-1 (-(Pl - s I) + diag g) = -I + T,           T = Pl^-1 diag(g + s)                       (order 0)
//     Pl^-1 (a0 + a1 J) = -a1 I + T',                             T' = Pl^-1 diag(a0 + a1 s + a1 g)           (order 1)
// exactly: the 25-point stencil drops out of the preconditioned operator.  The Arnoldi process then runs on T (T'): ONE
// preconditioner application whose first transform pass multiplies its input by the pointwise factor on the fly (one more
// 8 B/point stream, bk_precond::apply_pw) -- no stencil kernel, no intermediate vector, and on ranks no halo exchange inside GMRES.
// The identity part is a shift of the Hessenberg matrix (bk_op::hessenberg_shift: the Krylov space of alpha0 + alpha1 T is the
// space of T, the iterates are the same), so it costs nothing; a Newton shift of a block step rides in the last transform pass
// (one more 8 B/point stream).  What the Arnoldi vectors lose is the O(1) component along v_j that Gram-Schmidt had to cancel
// (w = Pl^-1 J v = -v + T v): T v is formed without that cancellation.  The explicit residual checks of a solve (apply_check)
// still go through the stencil kernel and the plain preconditioner, so every solve verifies the identity on its own solution.
struct ShiftPrecOp : bk_op {
    bk_op* J;
    bk_precond* P;
    bk_precond* Pr = nullptr;     // right preconditioner (order 1 only): the operator is v -> Pl^-1 (a0 + a1 J) Pr^-1 v
    double* tmp2 = nullptr;
    double a0, a1;
    int order;
    double* tmp;
    // order 0 with the spectral preconditioner of the SAME Swift-Hohenberg problem: a shift of the preconditioned operator can
    // be folded into the stencil kernel (apply below), i.e. costs nothing
    bool fold = false;
    double pl_shift = 0.0;
    // stencil-free mode: apply() is b0 x + b1 T x; (alpha0, alpha1) of the solve are in t_alpha0 / t_alpha1 (linsolve hands them
    // to gmres_core instead of (0, 1))
    bool tmode = false;
    DctFuse pw;
    double t_alpha0 = 0.0, t_alpha1 = 1.0;
    int init_fold() {
        const bool same = P && J->sh_problem() && P->is_l1_plus_shift(J->sh_problem(), &pl_shift);
        fold = same && order == 0 && ctx->opt("gmres_fold_shift", 1.0) != 0.0;
        // 1 (default): where the x passes run as the fused LDS kernel; 2: everywhere (separate pointwise pass: tests); 0: off
        const double sf = ctx->opt("gmres_stencil_free", 1.0);
        const double* u = nullptr;
        double l = 0.0, nu = 0.0;
        tmode = same && !Pr && sf != 0.0 && J->sh_state(&u, &l, &nu);
        if (tmode && sf != 2.0) {
            if (ctx->nranks > 1) {
                // every rank must take the same form (the chain exchanges halos inside GMRES, the stencil-free form does not).  The
                // inputs of the decision are static -- the shape of this rank's part of the plan -- so the ranks agree ONCE per
                // preconditioner and every later solve reads the cached flag; a failed all-reduce is this solve's error, never a silent
                // fall-back to the other form
                if (P->pw_agreed < 0) {
                    double no = P->pw_plan_ok() ? 0.0 : 1.0;
                    BK_TRY(comm_allreduce_host(ctx, &no, 1, 1));
                    P->pw_agreed = no == 0.0 ? 1 : 0;
                }
                tmode = P->pw_agreed == 1;
            } else {
                tmode = P->pw_fused_ok(u, u, u);
            }
        }
        pw.src = nullptr;                     // (nothing armed carries over into a solve: arm_v0)
        mono_first = ctx->opt("gmres_monomial_shift", kMonomialShiftDefault) != 0.0;
        chain = ctx->opt("dct_x_turnaround", 1.0) != 0.0;
        // (options, the communicator and the plan only: every rank takes the same decision)
        spectral_check = ctx->opt("gmres_check_spectral", kCheckSpectralDefault) != 0.0 && P && !Pr && ctx->nranks == 1 && P->nrm2_spectral_ok();
        check_nostore = ctx->opt("gmres_check_nostore", 1.0) != 0.0;
        if (!tmode) return 0;
        // g(u) = l + 2 nu u - 3 u^2 (examples/SH3d.jl:50-53); factor = c0 + cg g = A + u (B + C u)
        const double cg = order == 0 ? 1.0 : a1, c0 = order == 0 ? pl_shift : a0 + a1 * pl_shift;
        pw.u = u; pw.A = c0 + cg * l; pw.B = 2.0 * nu * cg; pw.C = -3.0 * cg;
        t_alpha0 = order == 0 ? a0 - a1 : -a1;
        t_alpha1 = order == 0 ? a1 : 1.0;
        return 0;
    }
    bool shift_is_free() const override { return Pr ? false : (P ? (fold || tmode) : J->shift_is_free()); }
    bool hessenberg_shift() const override { return tmode; }
    // T = W + I (order 0), T' = W' + a1 I (order 1): the first block of a solve runs on powers of W (W'), see bk_op::monomial_shift
    double rearranged_origin() const override { return tmode ? (order == 0 ? 1.0 : a1) : 0.0; }
    double monomial_shift() const override { return mono_first ? rearranged_origin() : 0.0; }
    bool mono_first = false;      // option gmres_monomial_shift, read once per solve (init_fold)
    bool chain = true;            // option dct_x_turnaround, read once per solve (init_fold)
    bool spectral_check = false;  // option gmres_check_spectral and what the preconditioner's plan allows, once per solve (init_fold)
    bool check_nostore = true;    // option gmres_check_nostore, once per solve (init_fold): the check's x-forward pass stores the spectrum only
    const double* rhs = nullptr;  // the solve's UNpreconditioned right-hand side (linsolve): b = Pl^-1 rhs
    // GMRES cycle start (bk_op::arm_v0): in stencil-free mode on a single rank the next application's first transform pass can
    // write V[0] = scale * src itself (DctFuse::src); the preconditioner decides per call whether that pass runs fused and writes
    // V[0] in a pass of its own where it does not (bk_precond::pw_src_first)
    void disarm_v0() override { pw.src = nullptr; }
    bool arm_v0(const double* src, double scale, double* dst) override {
        if (!tmode || ctx->nranks != 1 || src == dst || !P->pw_fused_ok(src, pw.u, dst)) return false;
        pw.src = src; pw.src_scale = scale; pw.src_store = dst;
        return true;
    }
    // the armed source, for one application of x (cleared); an application of anything but the armed vector: its scale pass first
    int take_v0(const double* x, DctFuse* d) {
        *d = pw;
        pw.src = nullptr;
        if (d->src && x != d->src_store) BK_TRY(P->pw_src_first(*d));
        return 0;
    }
    int apply(const double* x, const double*, double b0, double b1, double* out, double*) override {
        // out = b0 x + b1 * W(x)
        tmp_valid = false;
        if (tmode) {                                            // W = T (T'): see above
            DctFuse d;
            BK_TRY(take_v0(x, &d));
            return P->apply_pw(x, d, b0, b1, out);
        }
        return apply_chain(x, b0, b1, out);
    }
    // a Newton-basis block in stencil-free mode: the s applications as ONE preconditioner chain (bk_precond::apply_pw_chain), which
    // lets the spectral preconditioner run each x-inverse pass together with the next application's x-forward pass
    int apply_block(const double* x, int s, double b0, double b1, const double* theta, double* const* outs) override {
        if (!tmode || !chain || s > sstep::kS) return bk_op::apply_block(x, s, b0, b1, theta, outs);
        double cx[sstep::kS];
        for (int i = 0; i < s; ++i) cx[i] = b0 - (theta ? theta[i] : 0.0);
        DctFuse d;
        BK_TRY(take_v0(x, &d));
        return P->apply_pw_chain(x, d, s, cx, b1, outs);
    }
    int apply_check(const double* x, const double*, double c0, double c1, double* out, double*) override {
        tmp_valid = false;
        return check_chain(x, c0, c1, out);
    }
    // apply_check of the x a check_norm has JUST returned done = 1 for: tmp holds the chain's stencil result already
    int apply_check_resume(const double* x, double c0, double c1, double* out) override {
        if (!tmp_valid) return set_error(ctx, "apply_check_resume: no check_norm result to continue from");
        tmp_valid = false;
        have_tmp = true;
        const int e = check_chain(x, c0, c1, out);
        have_tmp = false;
        return e;
    }
    int check_chain(const double* x, double c0, double c1, double* out) {
        int e;
        if (!tmode) e = apply_chain(x, c0, c1, out);
        // c0 x + c1 T x through the stencil: T = I + Pl^-1 J (order 0), T' = a1 I + Pl^-1 (a0 + a1 J) (order 1)
        else e = order == 0 ? chain_order0(x, c0 + c1, c1, out) : chain_order1(x, c0 + c1 * a1, c1, out);
        return e;
    }
    // |b - (c0 + c1 A) x| of apply_check WITHOUT the residual vector.  b = Pl^-1 rhs, so the residual is Pl^-1 (rhs + c tmp) with tmp the
    // intermediate the chain itself forms with its one stencil pass, and its norm comes out of the preconditioner's spectrum
    // (bk_precond::apply_nrm2: Parseval, sum_k sym_k^2 |(Phi' (rhs + c tmp))_k|^2) after the forward passes alone:
    //   order 0, cx == 0:  tmp = J x, c = -ct                    order 0, fold:  tmp = (ct J + cx Pl) x, c = -1  (chain_order0)
    //   order 1, b0 == 0:  tmp = (a0 + a1 J) x, c = -b1
    // Still the original chain -- the stencil kernel's L1 and the spectral symbol -- so a mismatch between the two cannot pass.  tmp
    // holds exactly what apply_check would put there: when the value fails, gmres_core asks for the chain's result through
    // apply_check_resume, which continues from it, so the stencil runs once per check as before (tests/test_gpu_stencil_free.py counts
    // the stencil launches of every solve: at most one per cycle and one).
    // Everything else (no or a right preconditioner, cx != 0 without fold, ranks, plans off the LDS transforms): *done = 0.
    bool tmp_valid = false;               // tmp holds the chain intermediate of the last check_norm; cleared by whatever else writes tmp
    int check_norm(const double* x, double c0, double c1, double* nrm, int* done) override { return check_norm(x, c0, c1, rhs, nrm, done); }
    int check_norm(const double* x, double c0, double c1, const double* rhs_, double* nrm, int* done) {
        *done = 0;
        tmp_valid = false;
        if (!spectral_check || !rhs_ || !tmp) return 0;
        double c;
        if (order == 0) {
            const double cx = tmode ? c0 + c1 : c0 + c1 * a0, ct = tmode ? c1 : c1 * a1;      // (as apply_check hands them to chain_order0)
            if (cx != 0.0 && fold) { BK_TRY(J->apply_parts(x, cx * pl_shift, ct - cx, ct, tmp)); c = -1.0; }
            else if (cx == 0.0) { BK_TRY(J->apply(x, nullptr, 0.0, 1.0, tmp, nullptr)); c = -ct; }
            else return 0;
        } else {
            const double b0 = tmode ? c0 + c1 * a1 : c0, b1 = c1;
            if (b0 != 0.0) return 0;
            BK_TRY(J->apply(x, nullptr, a0, a1, tmp, nullptr));
            c = -b1;
        }
        BK_TRY(P->apply_nrm2(rhs_, c, tmp, nrm, !check_nostore));
        tmp_valid = true;
        *done = 1;
        return 0;
    }
    bool have_tmp = false;        // (apply_check_resume only) the stencil pass of this chain has run: check_norm left its result in tmp
    // out = cx x + ct Pl^-1 J x
    int chain_order0(const double* x, double cx, double ct, double* out) {
        if (have_tmp) {                        // the forms check_norm takes: cx == 0, or the folded shift
            BK_TRY(P->apply(tmp, out));
            return (cx != 0.0 || ct == 1.0) ? 0 : v_scale(ctx, n, ct, out);
        }
        if (cx != 0.0 && fold) {
            // cx x + ct Pl^-1 J x = Pl^-1 (ct J + cx Pl) x with Pl = L1 + s I and J = -L1 + diag(g):
            //   ct J + cx Pl = (ct - cx) (-L1) + diag(ct g + cx s)
            // -- the SAME stencil kernel with its two parts scaled separately, then the preconditioner: no extra pass
            BK_TRY(J->apply_parts(x, cx * pl_shift, ct - cx, ct, tmp));
            return P->apply(tmp, out);
        }
        BK_TRY(J->apply(x, nullptr, 0.0, 1.0, tmp, nullptr));
        if (cx == 0.0) {                       // the common Arnoldi call (a0 = 0): Pl^-1 writes straight into out
            BK_TRY(P->apply(tmp, out));
            return ct == 1.0 ? 0 : v_scale(ctx, n, ct, out);
        }
        BK_TRY(P->apply(tmp, tmp));
        return v_axpbyz(ctx, n, cx, x, ct, tmp, out);
    }
    // out = b0 x + b1 Pl^-1 (a0 x + a1 J x)
    int chain_order1(const double* x, double b0, double b1, double* out) {
        if (!have_tmp) BK_TRY(J->apply(x, nullptr, a0, a1, tmp, nullptr));
        if (b0 == 0.0) {
            BK_TRY(P->apply(tmp, out));
            return b1 == 1.0 ? 0 : v_scale(ctx, n, b1, out);
        }
        BK_TRY(P->apply(tmp, tmp));
        return v_axpbyz(ctx, n, b0, x, b1, tmp, out);
    }
    int apply_chain(const double* x, double b0, double b1, double* out) {
        if (Pr) {
            BK_TRY(Pr->apply(x, tmp2));
            BK_TRY(J->apply(tmp2, nullptr, a0, a1, tmp, nullptr));
            if (P) BK_TRY(P->apply(tmp, tmp));
            return v_axpbyz(ctx, n, b0, x, b1, tmp, out);
        }
        if (!P) return J->apply(x, nullptr, b0 + b1 * a0, b1 * a1, out, nullptr);
        if (order == 0) return chain_order0(x, b0 + b1 * a0, b1 * a1, out);
        return chain_order1(x, b0, b1, out);
    }
};

}  // namespace

// The operator of a left-preconditioned solve as an object of its own, for operators built on top of it (bordered.hip): the
// ShiftPrecOp linsolve would set up for (J, pl, a0, a1) -- order 0: a0 + a1 Pl^-1 J, order 1: Pl^-1 (a0 + a1 J) -- in whichever mode
// init_fold chooses.  tmp: n doubles owned by the caller.
int prec_op_create(bk_ctx* ctx, bk_op* J, bk_precond* pl, double a0, double a1, int order, double* tmp, PrecOpView* out) {
    ShiftPrecOp* W = new ShiftPrecOp;
    W->ctx = ctx; W->n = J->n; W->ntail = 0;
    W->J = J; W->P = pl; W->a0 = a0; W->a1 = a1; W->order = order; W->tmp = tmp;
    const int e = W->init_fold();
    if (e != 0) { delete W; return e; }
    out->op = W;
    out->tmode = W->tmode;
    out->alpha0 = W->tmode ? W->t_alpha0 : 0.0;
    out->alpha1 = W->tmode ? W->t_alpha1 : 1.0;
    return 0;
}

// ================================================================== symmetric Krylov.jl solvers (KrylovLS :minres / :cg)
// Paige-Saunders MINRES for the symmetric operator v -> a0 v + a1 J v with the SPD preconditioner M^-1 = Pl^-1
// (src/LinearSolver.jl:336-341 passes Pl as Krylov.jl's centered preconditioner M); restated in oracle/krylov.py
// (minres_krylovjl).  Short recurrences: 8 vectors, no restarts.
static int minres_core(bk_ctx* ctx, bk_op* J, const double* b, double* x, double a0, double a1, const bk_gmres_opts& o,
                       bk_precond* pl, GmresResult* res) {
    // Per iteration: operator, preconditioner, and three streaming passes -- (y += c r1; alfa = z.y), (y += c r2),
    // (beta^2 = r2.z), (w = .., x += phi w) -- the Lanczos vector v = z / beta is never materialised: its scale goes
    // into the operator call and into the update coefficients.  Buffers r1, r2, y and w, w1, w2 rotate.
    // Option minres_fused (default 1): the first of those passes rides in the operator kernel's store stage and the
    // third comes out of the preconditioner's spectrum (apply_axpy_dot / apply_dot: 28 -> 23 array streams per iteration
    // where both are fused, same arithmetic otherwise); 0 keeps the separate passes.
    const size_t n = J->n;
    WsGuard ws(ctx);
    double *r1 = nullptr, *r2 = nullptr, *y = nullptr, *z = nullptr, *w = nullptr, *w1 = nullptr, *w2 = nullptr;
    BK_TRY(ws.get(n, &r1)); BK_TRY(ws.get(n, &r2)); BK_TRY(ws.get(n, &y)); BK_TRY(ws.get(n, &z));
    BK_TRY(ws.get(n, &w)); BK_TRY(ws.get(n, &w1)); BK_TRY(ws.get(n, &w2));
    const bool fused = ctx->opt("minres_fused", 1.0) != 0.0;
    // Round 6 (option minres_pair_update, default 1): the direction / solution update -- the one pass of the iteration that touches
    // neither the operator nor the preconditioner -- is taken TWO iterations at a time: iteration k only keeps its Lanczos vector (one
    // more buffer) and its four scalars, iteration k + 1 writes w_k, w_{k+1} and x in one pass (v_minres_update2: 8 array streams instead
    // of 2 x 6, element for element the arithmetic of the two single updates); a solve that ends on an odd count flushes the pending
    // update alone.  The stopping test only needs the scalar recurrence (phibar), never x.  23 -> 21 streams per iteration.
    const bool pair = ctx->opt("minres_pair_update", 1.0) != 0.0 && (n & 1) == 0;
    double* vh = nullptr;                       // the first Lanczos vector of a pending pair
    if (pair) BK_TRY(ws.get(n, &vh));
    bool pending = false;
    double pa_cz = 0.0, pa_c1 = 0.0, pa_c2 = 0.0, pa_phi = 0.0;
    // out = M^-1 in, *d = in . out
    auto prec_dot = [&](const double* in, double* out, double* d) -> int {
        if (!pl) { BK_TRY(v_copy(ctx, n, in, out)); return v_dot(ctx, n, in, out, d); }
        return fused ? pl->apply_dot(in, out, d) : pl->bk_precond::apply_dot(in, out, d);
    };
    BK_TRY(v_zero(ctx, n, x));
    BK_TRY(v_copy(ctx, n, b, r2));
    double beta1;
    BK_TRY(prec_dot(r2, z, &beta1));
    res->converged = 0; res->niter = 0; res->resnorm = 0.0;
    if (beta1 < 0.0) return set_error(ctx, "minres: the preconditioner is not positive definite");
    if (beta1 == 0.0) { res->converged = 1; return 0; }
    beta1 = std::sqrt(beta1);
    const double eps = 2.220446049250313e-16;
    const double tol = o.atol + o.rtol * beta1;
    const int itmax = o.maxiter > 0 ? o.maxiter : 2 * (int)std::min<size_t>(n, 1u << 30);
    double oldb = 0.0, beta = beta1, dbar = 0.0, epsln = 0.0, phibar = beta1, cs = -1.0, sn = 0.0;
    BK_TRY(v_zero(ctx, n, w)); BK_TRY(v_zero(ctx, n, w2));
    int it = 0;
    bool solved = phibar <= tol;
    const bool trace = ctx->opt("solver_trace", 0.0) != 0.0;
    if (trace) { ctx->hist_solves += 1; ctx->hist.push_back(-(double)ctx->hist_solves); ctx->hist.push_back(phibar); }
    while (!solved && it < itmax) {
        it += 1;
        // y = (a0 + a1 J) v with v = z / beta
        double zy;                                                                   // y -= (beta/oldb) r1 ; alfa = v.y
        {
            const double c = it >= 2 ? -beta / oldb : 0.0;
            const double* r = it >= 2 ? r1 : nullptr;
            if (fused) BK_TRY(J->apply_axpy_dot(z, a0 / beta, a1 / beta, c, r, y, &zy));
            else BK_TRY(J->bk_op::apply_axpy_dot(z, a0 / beta, a1 / beta, c, r, y, &zy));
        }
        const double alfa = zy / beta;
        // y -= (alfa / beta) r2, then z = M^-1 y and b2 = y . z: with the spectral preconditioner the axpy rides in its x-forward
        // transform pass (bk_precond::apply_dot_pre_axpy, round 6: one array stream and one launch fewer per iteration, the same values)
        const double cy = -alfa / beta;
        const double* r2_old = r2;
        // direction / solution update need v = z / beta of THIS iteration: do it before z is overwritten
        const double oldeps = epsln;
        const double delta = cs * dbar + sn * alfa;
        const double gbar = sn * dbar - cs * alfa;
        { double* tmp = r1; r1 = r2; r2 = y; y = tmp; }                             // r1 <- r2, r2 <- y
        // the rotation needs the NEXT beta = sqrt(r2 . M^-1 r2): keep v's vector alive in `y` (free now) meanwhile
        { double* tmp = y; y = z; z = tmp; }                                         // y holds the old z (v * beta), z is free
        double b2;
        if (pl && fused) BK_TRY(pl->apply_dot_pre_axpy(r2, cy, r2_old, z, &b2));
        else { BK_TRY(v_axpby(ctx, n, cy, r2_old, 1.0, r2)); BK_TRY(prec_dot(r2, z, &b2)); }
        const double vbeta = beta;                                                   // scale of the vector kept in y
        oldb = beta;
        if (b2 < 0.0) return set_error(ctx, "minres: the preconditioner is not positive definite");
        beta = std::sqrt(b2);
        epsln = sn * beta;
        dbar = -cs * beta;
        const double gamma = std::max(std::hypot(gbar, beta), eps);
        cs = gbar / gamma; sn = beta / gamma;
        const double phi = cs * phibar;
        phibar = sn * phibar;
        // w = (v - oldeps w1 - delta w2) / gamma ; x += phi w          (w1 = w_{k-2}, w2 = w_{k-1}; v = y / vbeta)
        const double cz = 1.0 / (vbeta * gamma), c1 = -oldeps / gamma, c2 = -delta / gamma;
        if (trace) ctx->hist.push_back(phibar);
        solved = phibar <= tol;
        if (pair && !pending && !solved && it < itmax) {
            // first of a pair: keep the vector (y takes the spare buffer) and the scalars; w1 / w2 / w stay as they are
            { double* tmp = vh; vh = y; y = tmp; }
            pa_cz = cz; pa_c1 = c1; pa_c2 = c2; pa_phi = phi;
            pending = true;
            continue;
        }
        if (pending) {
            // second of the pair (or the solve's last iteration).  The buffers still hold the state before the pending iteration k - 1
            // rotated anything: w = w_{k-2}, w2 = w_{k-3}, w1 = spare.  Pending:  w_{k-1} = pa_cz vh + pa_c1 w2 + pa_c2 w;  this
            // iteration:  w_k = cz y + c1 w + c2 w_{k-1}.
            double* m2 = w2;  double* m1 = w;  double* wa = w1;  double* wb = w2;      // wb overwrites w_{k-3} (element-wise safe)
            const int st2 = v_minres_update2(ctx, n, pa_cz, vh, pa_c1, pa_c2, cz, y, c1, c2, m2, m1, wa, wb, pa_phi, phi, x);
            if (st2 < 0) return st2;                   // a launch error; 1 = shape not covered: the two single updates
            if (st2 > 0) {
                BK_TRY(v_minres_update(ctx, n, pa_cz, vh, pa_c1, m2, pa_c2, m1, wa, pa_phi, x));
                BK_TRY(v_minres_update(ctx, n, cz, y, c1, m1, c2, wa, wb, phi, x));
            }
            // now: wa = w_{k-1} (in the old w1 buffer), wb = w_k (in the old w2 buffer), the old w buffer (w_{k-2}) is free
            { double* freeb = w; w2 = wa; w = wb; w1 = freeb; }                           // (w2, w) = (w_{k-1}, w_k), w1 = free
            pending = false;
            continue;
        }
        { double* tmp = w1; w1 = w2; w2 = w; w = tmp; }                             // w1 <- w2, w2 <- w
        BK_TRY(v_minres_update(ctx, n, cz, y, c1, w1, c2, w2, w, phi, x));
    }
    res->converged = solved ? 1 : 0;
    res->niter = it;
    res->resnorm = phibar;
    return 0;
}

// Preconditioned conjugate gradients (Krylov.jl `cg` semantics: sqrt(r' M^-1 r) <= atol + rtol * its initial value).
static int cg_core(bk_ctx* ctx, bk_op* J, const double* b, double* x, double a0, double a1, const bk_gmres_opts& o,
                   bk_precond* pl, GmresResult* res) {
    const size_t n = J->n;
    WsGuard ws(ctx);
    double *r = nullptr, *z = nullptr, *p = nullptr, *Ap = nullptr;
    BK_TRY(ws.get(n, &r)); BK_TRY(ws.get(n, &z)); BK_TRY(ws.get(n, &p)); BK_TRY(ws.get(n, &Ap));
    const bool fused = ctx->opt("minres_fused", 1.0) != 0.0;       // the same two fused passes as MINRES
    auto prec_dot = [&](const double* in, double* out, double* d) -> int {
        if (!pl) { BK_TRY(v_copy(ctx, n, in, out)); return v_dot(ctx, n, in, out, d); }
        return fused ? pl->apply_dot(in, out, d) : pl->bk_precond::apply_dot(in, out, d);
    };
    BK_TRY(v_zero(ctx, n, x));
    BK_TRY(v_copy(ctx, n, b, r));
    double gamma;
    BK_TRY(prec_dot(r, z, &gamma));
    BK_TRY(v_copy(ctx, n, z, p));
    res->converged = 0; res->niter = 0; res->resnorm = 0.0;
    if (gamma == 0.0) { res->converged = 1; return 0; }
    double rnorm = std::sqrt(std::max(gamma, 0.0));
    const double tol = o.atol + o.rtol * rnorm;
    const int itmax = o.maxiter > 0 ? o.maxiter : 2 * (int)std::min<size_t>(n, 1u << 30);
    int it = 0;
    bool solved = rnorm <= tol;
    while (!solved && it < itmax) {
        double pAp;
        if (fused) BK_TRY(J->apply_axpy_dot(p, a0, a1, 0.0, nullptr, Ap, &pAp));
        else BK_TRY(J->bk_op::apply_axpy_dot(p, a0, a1, 0.0, nullptr, Ap, &pAp));
        if (!(pAp > 0.0)) break;                                                     // not positive definite along p
        const double alpha = gamma / pAp;
        BK_TRY(v_axpby(ctx, n, alpha, p, 1.0, x));
        // r -= alpha Ap, z = M^-1 r, gnext = r . z: the axpy rides in the spectral preconditioner's x-forward pass where it can (as in MINRES)
        double gnext;
        if (pl && fused) BK_TRY(pl->apply_dot_pre_axpy(r, -alpha, Ap, z, &gnext));
        else { BK_TRY(v_axpby(ctx, n, -alpha, Ap, 1.0, r)); BK_TRY(prec_dot(r, z, &gnext)); }
        rnorm = std::sqrt(std::max(gnext, 0.0));
        BK_TRY(v_axpby(ctx, n, 1.0, z, gnext / gamma, p));                           // p = z + beta p
        gamma = gnext;
        it += 1;
        solved = rnorm <= tol;
    }
    res->converged = solved ? 1 : 0;
    res->niter = it;
    res->resnorm = rnorm;
    return 0;
}

int linsolve(bk_ctx* ctx, bk_op* J, const double* rhs, double* x, double a0, double a1, const bk_gmres_opts& o,
             bk_precond* pl, GmresResult* res) {
    if (J->ntail != 0) return set_error(ctx, "linsolve: operator must be unbordered");
    if (x == rhs) return set_error(ctx, "linsolve: x must not alias rhs");
    if (o.flavor == BK_KRYLOV_MINRES) return minres_core(ctx, J, rhs, x, a0, a1, o, pl, res);
    if (o.flavor == BK_KRYLOV_CG) return cg_core(ctx, J, rhs, x, a0, a1, o, pl, res);
    const bool kk = (o.flavor == BK_GMRES_KRYLOVKIT);
    if (kk && o.pr) return set_error(ctx, "GMRESKrylovKit has no right preconditioner (src/LinearSolver.jl:223-250): use the IterativeSolvers or Krylov.jl flavor");
    if (!pl && kk) return gmres_core(ctx, J, rhs, nullptr, x, nullptr, a0, a1, o, res);
    WsGuard ws(ctx);
    ShiftPrecOp W;
    W.ctx = ctx; W.n = J->n; W.ntail = 0;
    W.J = J; W.P = pl; W.a0 = a0; W.a1 = a1; W.order = kk ? 0 : 1; W.tmp = nullptr;
    W.Pr = kk ? nullptr : o.pr;
    BK_TRY(W.init_fold());
    W.rhs = rhs;
    const double* b = rhs;
    if (pl || W.Pr) BK_TRY(ws.get(J->n, &W.tmp));
    if (W.Pr) BK_TRY(ws.get(J->n, &W.tmp2));
    if (pl) {
        double* prhs = nullptr;
        BK_TRY(ws.get(J->n, &prhs));
        BK_TRY(pl->apply(rhs, prhs));            // ldiv!(similar(rhs), Pl, copy(rhs)) :278
        b = prhs;
    }
    // (stencil-free mode: W applies T, and the identity part of the operator is the solve's (alpha0, alpha1))
    BK_TRY(gmres_core(ctx, &W, b, nullptr, x, nullptr, W.tmode ? W.t_alpha0 : 0.0, W.tmode ? W.t_alpha1 : 1.0, o, res));
    // right preconditioner: the iteration ran on y = Pr x; x = Pr^-1 y (IterativeSolvers update_solution!, Krylov.jl N)
    if (W.Pr) BK_TRY(W.Pr->apply(x, x));
    return 0;
}

// Two independent solves with the same operator and preconditioner -- the R and dF/dp solves of BorderingBLS, ls(J, rhs1,
// rhs2) (src/LinearSolver.jl:15-19) -- on TWO LANES: the second runs on the context's second lane (own stream, reduction
// buffers, workspace, scratch of the preconditioner; a host thread drives it) while the first runs where it always did.
// Each solve's arithmetic is untouched, so results and counters are bitwise those of the sequential calls; what changes is
// that the device always has the other solve's kernels to run while one solve waits for its host (a synchronisation per
// Arnoldi chunk), fills the tail of a short kernel, or -- later, with a second communicator -- sits in a collective.
// Used for vectors that do not saturate HBM by themselves (option two_lanes; default: single rank, n <= 2^24): there a
// launch-bound 2-D corrector nearly doubles its rate; at 512^3 both solves are bandwidth-bound and nothing would be gained.
// Supported operators: the PDE Jacobian with no or a single-GPU spectral preconditioner; everything else runs sequentially.
int linsolve2(bk_ctx* ctx, bk_op* J, const double* rhs1, double* x1, const double* rhs2, double* x2, double a0, double a1,
              const bk_gmres_opts& o, bk_precond* pl, GmresResult* r1, GmresResult* r2) {
    PdeJacobian* PJ = dynamic_cast<PdeJacobian*>(J);
    // ranks: opt-in (two_lanes = 1).  With two lanes every rank drives two independent sequences of blocking collectives (two host
    // threads, two communicators, collectives that wait on the device); see the warm-up below for the hang that cost rounds 3-5 a coin
    // toss per suite run.  The decision itself only looks at options, the communicator and the GLOBAL problem: every rank takes the same one
    const bool want = ctx->opt("two_lanes", (ctx->nranks == 1 && J->n <= ((size_t)1 << 24)) ? 1.0 : 0.0) != 0.0;
    bk_ctx* lane = (want && PJ && J->ntail == 0 && !o.pr) ? ctx_lane(ctx) : nullptr;     // (a right preconditioner lives on ctx)
    bk_precond* pl2 = nullptr;
    if (lane && pl) {
        pl2 = precond_lane_shadow(pl, lane);
        if (!pl2) lane = nullptr;
    }
    // both solves start from the context's state as it is on entry (speculation ramp, carried shifts), whichever way they run,
    // and the first solve's is what the context keeps: the two lanes reproduce the sequential calls bitwise
    const int entry_steps = ctx->gmres_last_steps;
    const std::vector<double> entry_shifts = ctx->newton_shifts;
    if (!lane) {
        BK_TRY(linsolve(ctx, J, rhs1, x1, a0, a1, o, pl, r1));
        const int keep_steps = ctx->gmres_last_steps;
        const std::vector<double> keep_shifts = ctx->newton_shifts;
        ctx->gmres_last_steps = entry_steps; ctx->newton_shifts = entry_shifts;
        const int s2 = linsolve(ctx, J, rhs2, x2, a0, a1, o, pl, r2);
        ctx->gmres_last_steps = keep_steps; ctx->newton_shifts = keep_shifts;
        return s2;
    }
    lane->gmres_last_steps = entry_steps;
    lane->newton_shifts = entry_shifts;
    bk_problem prob2 = *PJ->prob;              // the problem on the lane, with its own halo planes on ranks
    prob2.ctx = lane;
    prob2.halo_lo = prob2.halo_hi = nullptr;
    WsGuard lws(lane);
    if (PJ->prob->halo_lo) {
        if (lws.get(2 * prob2.plane, &prob2.halo_lo) != 0 || lws.get(2 * prob2.plane, &prob2.halo_hi) != 0) {
            delete pl2;
            return set_error(ctx, "linsolve2: halo buffers of the second lane: %s", lane->err.c_str());
        }
    }
    PdeJacobian J2 = *PJ;
    J2.ctx = lane;
    J2.prob = &prob2;
    // the lane's stream starts after everything already enqueued on the context's stream (its inputs), and the context's
    // stream continues after the lane has finished (the thread synchronises the lane's stream before it returns)
    hipEvent_t ev = nullptr;
    int s2 = 0;
    if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess || hipEventRecord(ev, ctx->stream) != hipSuccess ||
        hipStreamWaitEvent(lane->stream, ev, 0) != hipSuccess) {
        if (ev) (void)hipEventDestroy(ev);
        delete pl2;
        return set_error(ctx, "linsolve2: lane hand-over failed");
    }
    // RANKS: no runtime call that synchronises the whole device may run inside a lane while the other lane can sit in a collective --
    // hipFree / hipHostFree (the proxy's staging buffers growing, a workspace pool miss) wait for EVERY stream of the process, the
    // other lane's collective among them, and two ranks that do so in different lanes at the same moment wait for each other for
    // ever (the intermittent two-lane hang found in round 6: 7 hangs in 72 runs with two to four ranks sharing a GPU before this
    // warm-up, 0 in 72 with it; profiles/r6_dist_two_lane_hang.txt).  So the FIRST
    // pair of solves of a (global size, Krylov dimension) runs one solve after the other, each on its own lane: every pool of both
    // lanes then holds what the concurrent pairs that follow ask for.  Same arithmetic either way (the lanes reproduce sequential calls).
    const bk_problem_desc& gd = PJ->prob->desc;
    const std::pair<size_t, int> wkey{(size_t)gd.n[0] * (size_t)std::max(gd.n[1], 1) * (size_t)std::max(gd.n[2], 1), o.dim};
    const bool cold = ctx->nranks > 1 && ctx->lanes_warm.count(wkey) == 0;
    int s1 = 0;
    if (cold) {
        s1 = linsolve(ctx, J, rhs1, x1, a0, a1, o, pl, r1);
        if (s1 == 0 && hipStreamSynchronize(ctx->stream) != hipSuccess) s1 = set_error(ctx, "linsolve2: synchronisation failed");
        if (s1 == 0) {
            s2 = linsolve(lane, &J2, rhs2, x2, a0, a1, o, pl2, r2);
            if (hipStreamSynchronize(lane->stream) != hipSuccess && s2 == 0) s2 = set_error(lane, "linsolve2: lane synchronisation failed");
        }
        if (s1 == 0 && s2 == 0) ctx->lanes_warm.insert(wkey);
    } else {
    std::thread th([&]() {
        (void)hipSetDevice(lane->device);
        s2 = linsolve(lane, &J2, rhs2, x2, a0, a1, o, pl2, r2);
        if (hipStreamSynchronize(lane->stream) != hipSuccess && s2 == 0) s2 = set_error(lane, "linsolve2: lane synchronisation failed");
    });
    s1 = linsolve(ctx, J, rhs1, x1, a0, a1, o, pl, r1);
    th.join();
    }
    (void)hipEventDestroy(ev);
    delete pl2;
    ctx_lane_merge(ctx, lane);
    if (s1 != 0) return s1;
    if (s2 != 0) return set_error(ctx, "second lane: %s", lane->err.c_str());
    return 0;
}

}  // namespace bk

using namespace bk;

// ================================================================== C ABI: linear solves
extern "C" {

void bk_gmres_default_opts(bk_gmres_opts* o, int flavor) {
    if (!o) return;
    o->flavor = flavor;
    o->pr = nullptr;
    if (flavor == BK_KRYLOV_MINRES || flavor == BK_KRYLOV_CG) {   // Krylov.jl: atol = rtol = sqrt(eps), itmax = 0 -> 2n
        o->dim = 0; o->maxiter = 0; o->atol = 1.4901161193847656e-08; o->rtol = 1.4901161193847656e-08;
    } else if (flavor == BK_GMRES_KRYLOVJL) {       // Krylov.jl gmres defaults: memory 20, atol = rtol = sqrt(eps)
        o->dim = 20; o->maxiter = 2000; o->atol = 1.4901161193847656e-08; o->rtol = 1.4901161193847656e-08;
    } else if (flavor == BK_GMRES_ITERATIVESOLVERS) {      // src/LinearSolver.jl:151-160
        o->dim = 200 > kMaxBasis - 1 ? kMaxBasis - 1 : 200;
        o->maxiter = 100; o->atol = 0.0; o->rtol = 1e-8;
    } else {                                        // KrylovDefaults, src/LinearSolver.jl:225-234
        o->dim = 30; o->maxiter = 100; o->atol = 1e-12; o->rtol = 1e-12;
    }
}

int bk_gmres(bk_ctx* ctx, bk_op* J, const double* rhs, double* x, double a0, double a1, const bk_gmres_opts* opts,
             bk_precond* pl, int* converged, int* niter, double* resnorm) {
    if (!ctx || !J || !rhs || !x || !opts) return -1;
    GmresResult r;
    BK_TRY(linsolve(ctx, J, rhs, x, a0, a1, *opts, pl, &r));
    if (converged) *converged = r.converged;
    if (niter) *niter = r.niter;
    if (resnorm) *resnorm = r.resnorm;
    return 0;
}

int bk_precond_op_apply(bk_ctx* ctx, bk_precond* pl, bk_op* J, const double* x, double a0, double a1, double* out, int* stencil_free) {
    if (!ctx || !pl || !J || !x || !out) return -1;
    if (J->ntail != 0) return set_error(ctx, "bk_precond_op_apply: operator must be unbordered");
    if (out == x) return set_error(ctx, "bk_precond_op_apply: out must not alias x");
    WsGuard ws(ctx);
    ShiftPrecOp W;
    W.ctx = ctx; W.n = J->n; W.ntail = 0;
    W.J = J; W.P = pl; W.a0 = a0; W.a1 = a1; W.order = 0; W.tmp = nullptr;
    BK_TRY(W.init_fold());
    BK_TRY(ws.get(J->n, &W.tmp));
    if (stencil_free) *stencil_free = W.tmode ? 1 : 0;
    // tmode: W.apply(b0, b1) = b0 x + b1 T x and a0 + a1 Pl^-1 J = (a0 - a1) + a1 T; else the chain a0 x + a1 Pl^-1 (J x)
    return W.tmode ? W.apply(x, nullptr, W.t_alpha0, W.t_alpha1, out, nullptr) : W.apply(x, nullptr, 0.0, 1.0, out, nullptr);
}

int bk_precond_check_norm(bk_ctx* ctx, bk_precond* pl, bk_op* J, const double* x, const double* rhs, double a0, double a1, int flavor,
                          double* nrm, int* spectral) {
    if (!ctx || !pl || !J || !x || !rhs || !nrm) return -1;
    if (J->ntail != 0) return set_error(ctx, "bk_precond_check_norm: operator must be unbordered");
    if (flavor != BK_GMRES_KRYLOVKIT && flavor != BK_GMRES_ITERATIVESOLVERS && flavor != BK_GMRES_KRYLOVJL)
        return set_error(ctx, "bk_precond_check_norm: a GMRES flavor");
    // the operator exactly as linsolve sets it up, then the check of gmres_core on x
    WsGuard ws(ctx);
    ShiftPrecOp W;
    W.ctx = ctx; W.n = J->n; W.ntail = 0;
    W.J = J; W.P = pl; W.a0 = a0; W.a1 = a1; W.order = flavor == BK_GMRES_KRYLOVKIT ? 0 : 1; W.tmp = nullptr;
    BK_TRY(W.init_fold());
    W.rhs = rhs;
    BK_TRY(ws.get(J->n, &W.tmp));
    const double alpha0 = W.tmode ? W.t_alpha0 : 0.0, alpha1 = W.tmode ? W.t_alpha1 : 1.0;
    int have = 0;
    BK_TRY(W.check_norm(x, alpha0, alpha1, nrm, &have));
    if (spectral) *spectral = have;
    if (have) return 0;
    double *b = nullptr, *w = nullptr;
    BK_TRY(ws.get(J->n, &b));
    BK_TRY(ws.get(J->n, &w));
    BK_TRY(pl->apply(rhs, b));
    BK_TRY(W.apply_check(x, nullptr, alpha0, alpha1, w, nullptr));
    return v_diff_nrm2(ctx, J->n, b, w, nrm);
}

int bk_abi_version(void) { return BK_ABI_VERSION; }

int bk_gmres2(bk_ctx* ctx, bk_op* J, const double* rhs1, const double* rhs2, double* x1, double* x2, double a0,
              double a1, const bk_gmres_opts* opts, bk_precond* pl, int* converged, int niter[2]) {
    if (!ctx || !J || !rhs1 || !rhs2 || !x1 || !x2 || !opts) return -1;
    if (x1 == x2) return set_error(ctx, "bk_gmres2: x1 and x2 must be distinct buffers");
    GmresResult r1, r2;
    BK_TRY(linsolve2(ctx, J, rhs1, x1, rhs2, x2, a0, a1, *opts, pl, &r1, &r2));
    if (converged) *converged = r1.converged & r2.converged;
    if (niter) { niter[0] = r1.niter; niter[1] = r2.niter; }
    return 0;
}

}  // extern "C"

// ================================================================== bordered solvers
namespace bk {

struct BorderingState {          // caches dx = (shift + J)^-1 dR between BEC passes
    double* dx = nullptr;
    bool have_dx = false;
    int it_dx = 0;
    int cv_dx = 1;
};

namespace {

// The bordered tail and the Newton update as ONE pass (option palc_fuse_update): t = a dx + x1, then x = x - t, element by element
// what the two v_axpby calls  x1 <- a dx + 1 x1  and  x <- -1 x1 + 1 x  compute (their products by +-1 are exact) -- the product and
// the two sums rounded on their own, a zero a skips the dx term as v_axpbyz skips an operand (0.0 + x1) -- without the store and the
// reload of x1: three read streams and one write instead of 2 x (2 + 1).  The third operand is read from xs and the result written
// to x: xs == x is the update in place, xs != x (the corrector's first iteration, bk_newton_palc_from) leaves the predictor as it
// is and saves the copy of it (no __restrict__ on either); every lane reads its elements of xs before it writes them to x.  dx and
// x1 are only read and must not alias x.
template <int VEC, bool NTH>
__global__ void __launch_bounds__(kThreads) palc_update_kernel(size_t n, double a, const double* __restrict__ dx,
                                                               const double* __restrict__ x1, const double* xs, double* x, int has_dx) {
    auto one = [&](double d, double v, double xv) {
        double t = 0.0;
        if (has_dx) t = __dmul_rn(a, d);
        t = __dadd_rn(t, v);
        return __dadd_rn(-t, xv);
    };
    if (VEC == 2) {
        stream_loop<4>(n >> 1, [&](auto uc, size_t i0, size_t st) {
            constexpr int UU = decltype(uc)::value;
            double2 dv[UU], vv[UU], xv[UU];
#pragma unroll
            for (int u = 0; u < UU; ++u) {
                dv[u] = ld2<NTH>(dx, i0 + u * st);
                vv[u] = ld2<NTH>(x1, i0 + u * st);
                xv[u] = ld2<NTH>(xs, i0 + u * st);
            }
#pragma unroll
            for (int u = 0; u < UU; ++u) {
                const double rx = one(dv[u].x, vv[u].x, xv[u].x), ry = one(dv[u].y, vv[u].y, xv[u].y);
                if (NTH) {
                    nt_d2 r; r.x = rx; r.y = ry;
                    __builtin_nontemporal_store(r, reinterpret_cast<nt_d2*>(x) + (i0 + u * st));
                } else {
                    reinterpret_cast<double2*>(x)[i0 + u * st] = make_double2(rx, ry);
                }
            }
        });
        if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) x[n - 1] = one(dx[n - 1], x1[n - 1], xs[n - 1]);
    } else {
        for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kThreads) x[i] = one(dx[i], x1[i], xs[i]);
    }
}

}  // namespace

// x <- xs - (x1 - dl dx), xs == x or a vector that does not overlap x: the launches v_axpby(-dl, dx, 1, x1) and v_axpby(-1, x1, 1, x)
// as one (x1 is left as it is)
int palc_update(bk_ctx* ctx, size_t n, double dl, const double* dx, const double* x1, const double* xs, double* x) {
    if (n == 0) return 0;
    ProfScope ps(ctx, "blas1", 32.0 * n);
    const bool vec = aligned16(dx) && aligned16(x1) && aligned16(xs) && aligned16(x);
    const int grid = grid_for(n, vec ? 2 : 1, 4096);
    const double a = -dl;
    const int has_dx = a != 0.0 ? 1 : 0;
    if (vec && nt_hint(ctx, n))
        hipLaunchKernelGGL((palc_update_kernel<2, true>), dim3(grid), dim3(kThreads), 0, ctx->stream, n, a, dx, x1, xs, x, has_dx);
    else if (vec)
        hipLaunchKernelGGL((palc_update_kernel<2, false>), dim3(grid), dim3(kThreads), 0, ctx->stream, n, a, dx, x1, xs, x, has_dx);
    else
        hipLaunchKernelGGL((palc_update_kernel<1, false>), dim3(grid), dim3(kThreads), 0, ctx->stream, n, a, dx, x1, xs, x, has_dx);
    BK_HIP(ctx, hipGetLastError());
    return 0;
}

// BEC, src/LinearBorderSolver.jl:125-144.  x1 <- (shift+J)^-1 R - dl * dx.
// xnew != NULL (bk_newton_palc, option palc_fuse_update): the tail pass is palc_update, xnew <- xsrc - (x1 - dl dx) (xsrc = NULL:
// xnew itself), and x1 is left holding (shift+J)^-1 R WITHOUT the dl term -- only for callers that do not read x1 afterwards.
static int bec(bk_ctx* ctx, bk_op* J, const double* dR, const double* dzu, double dzp, const double* R, double nn,
               double xiu, double xip, bool has_shift, double shift, double dotscale, const bk_gmres_opts& ls,
               bk_precond* pl, BorderingState& st, double* x1, double* dl, int* cv, int it[2], double* xnew = nullptr,
               const double* xsrc = nullptr) {
    const size_t n = J->n;
    GmresResult r1;
    const double a0 = has_shift ? shift : 0.0;
    if (!st.have_dx) {
        GmresResult r2;                        // the two solves of the first BEC pass are independent: two lanes
        BK_TRY(linsolve2(ctx, J, R, x1, dR, st.dx, a0, 1.0, ls, pl, &r1, &r2));
        st.have_dx = true; st.it_dx = r2.niter; st.cv_dx = r2.converged;
    } else {
        BK_TRY(linsolve(ctx, J, R, x1, a0, 1.0, ls, pl, &r1));
    }
    double d[2];
    BK_TRY(v_dot2(ctx, n, dzu, x1, st.dx, d));
    d[0] *= dotscale; d[1] *= dotscale;
    *dl = (nn - d[0] * xiu) / (dzp * xip - d[1] * xiu);
    if (xnew) BK_TRY(palc_update(ctx, n, *dl, st.dx, x1, xsrc ? xsrc : xnew, xnew));
    else BK_TRY(v_axpby(ctx, n, -(*dl), st.dx, 1.0, x1));
    *cv = r1.converged & st.cv_dx;
    it[0] = r1.niter; it[1] = st.it_dx;
    return 0;
}

int bls_bordering(bk_ctx* ctx, bk_op* J, const double* dR, const double* dzu, double dzp, const double* R, double nn,
                  double xiu, double xip, bool has_shift, double shift, double dotscale, const bk_bordering_opts& bo,
                  const bk_gmres_opts& ls, bk_precond* pl, double* dX, double* dl, int* converged, int itlinear[2],
                  double* xnew, const double* xsrc) {
    // xnew (optional; needs check_precision off): the Newton update xnew <- xsrc - dX (xsrc = NULL: xnew) rides in the tail pass of
    // the one BEC pass, and dX is left holding x1 = (shift+J)^-1 R without the dl term (see bec)
    if (xnew && bo.check_precision) return set_error(ctx, "bls_bordering: the fused update needs check_precision off");
    const size_t n = J->n;
    WsGuard ws(ctx);
    BorderingState st;
    BK_TRY(ws.get(n, &st.dx));
    int cv = 0, it[2] = {0, 0};
    BK_TRY(bec(ctx, J, dR, dzu, dzp, R, nn, xiu, xip, has_shift, shift, dotscale, ls, pl, st, dX, dl, &cv, it, xnew, xsrc));
    int k = 0;
    bool fail = true;
    double *dXr = nullptr, *dX1 = nullptr;
    while (bo.check_precision && k < bo.k && fail) {
        // residualBEC, :146-166: dXr = R - (shift + J) dX - dl dR ; dlr = n - xip dzp dl - xiu dotp(dzu, dX)
        if (!dXr) { BK_TRY(ws.get(n, &dXr)); BK_TRY(ws.get(n, &dX1)); }
        BK_TRY(J->apply(dX, nullptr, has_shift ? shift : 0.0, 1.0, dXr, nullptr));
        BK_TRY(v_axpby(ctx, n, *dl, dR, 1.0, dXr));
        BK_TRY(v_axpby(ctx, n, 1.0, R, -1.0, dXr));
        double dd, nr;
        BK_TRY(v_dot(ctx, n, dzu, dX, &dd));
        const double dlr = nn - xip * dzp * (*dl) - xiu * dotscale * dd;
        BK_TRY(v_nrm2(ctx, n, dXr, &nr));
        fail = nr > bo.tol || std::fabs(dlr) > bo.tol;
        if (fail) {
            double dl1 = 0.0;
            BK_TRY(bec(ctx, J, dR, dzu, dzp, dXr, dlr, xiu, xip, has_shift, shift, dotscale, ls, pl, st, dX1, &dl1, &cv, it));
            BK_TRY(v_axpby(ctx, n, 1.0, dX1, 1.0, dX));
            *dl += dl1;
            k += 1;
        }
    }
    if (converged) *converged = cv;
    if (itlinear) { itlinear[0] = it[0]; itlinear[1] = it[1]; }
    return 0;
}

// MatrixFreeBLSmap on BorderedArray, src/LinearBorderSolver.jl:326-335 (scalar border) and :338-352 (m-column border:
// a, b tuples of m vectors, c an m x m matrix): out.u = J x.u + shift x.u + sum_i x.p[i] a_i,
// out.p = c x.p + [dot(b_i, x.u)]_i.
struct BorderedMapOp : bk_op {
    bk_op* J;
    const double* a[BK_MAX_BORDER];      // columns (dR for the PALC system)
    const double* bvec[BK_MAX_BORDER];   // rows (dzu, scaled by xiu * dotscale through `bscale`)
    double bscale;
    double c[BK_MAX_BORDER * BK_MAX_BORDER];     // row-major m x m
    bool has_shift;
    double shift;
    int apply(const double* x, const double* xt, double b0, double b1, double* out, double* outt) override {
        // out.u = b0 x + b1 (J x + shift x + sum xt_i a_i) ; out.p = b0 xt + b1 (bscale <b_i, x> + c xt)
        const int m = ntail;
        BK_TRY(J->apply(x, nullptr, b0 + b1 * (has_shift ? shift : 0.0), b1, out, nullptr));
        for (int i = 0; i < m; ++i)
            if (xt[i] != 0.0 && b1 != 0.0) BK_TRY(v_axpby(ctx, n, b1 * xt[i], a[i], 1.0, out));
        for (int i = 0; i < m; ++i) {
            double d;
            BK_TRY(v_dot(ctx, n, bvec[i], x, &d));
            double cx = 0.0;
            for (int j = 0; j < m; ++j) cx += c[i * m + j] * xt[j];
            outt[i] = b0 * xt[i] + b1 * (bscale * d + cx);
        }
        return 0;
    }
};

// MatrixFreeBLS (src/LinearBorderSolver.jl:424-437): ONE GMRES on the (N + 1) operator MatrixFreeBLSmap over BorderedArray(u, p)
int bls_matrixfree(bk_ctx* ctx, bk_op* J, const double* dR, const double* dzu, double dzp, const double* R, double n, double xiu,
                   double xip, bool has_shift, double shift, double dotscale, const bk_gmres_opts& ls, double* dX, double* dl,
                   int* converged, int* itlinear) {
    if (ls.flavor >= BK_KRYLOV_MINRES) return set_error(ctx, "bk_bls_matrixfree: the bordered operator is not symmetric (use a GMRES flavor)");
    BorderedMapOp M;
    M.ctx = ctx; M.n = J->n; M.ntail = 1;
    M.J = J; M.a[0] = dR; M.bvec[0] = dzu; M.bscale = xiu * dotscale; M.c[0] = dzp * xip;
    M.has_shift = has_shift; M.shift = shift;
    GmresResult r;
    BK_TRY(gmres_core(ctx, &M, R, &n, dX, dl, 0.0, 1.0, ls, &r));
    if (converged) *converged = r.converged;
    if (itlinear) *itlinear = r.niter;
    return 0;
}

}  // namespace bk

extern "C" {

int bk_bls_bordering(bk_ctx* ctx, bk_op* J, const double* dR, const double* dzu, double dzp, const double* R,
                     double n, double xiu, double xip, int has_shift, double shift, double dotscale,
                     const bk_bordering_opts* bopts, const bk_gmres_opts* lsopts, bk_precond* pl, double* dX,
                     double* dl, int* converged, int itlinear[2]) {
    if (!ctx || !J || !dR || !dzu || !R || !bopts || !lsopts || !dX || !dl) return -1;
    if (dX == R || dX == dR || dX == dzu) return set_error(ctx, "bk_bls_bordering: dX must be a fresh buffer");
    if (bopts->k < 1) return set_error(ctx, "BorderingBLS: number of recursions must be positive");
    return bls_bordering(ctx, J, dR, dzu, dzp, R, n, xiu, xip, has_shift != 0, shift, dotscale, *bopts, *lsopts, pl, dX,
                         dl, converged, itlinear);
}

int bk_palc_update(bk_ctx* ctx, size_t n, double dl, const double* dx, const double* x1, double* x) {
    if (!ctx || !dx || !x1 || !x) return -1;
    if (x == dx || x == x1) return set_error(ctx, "bk_palc_update: x must not alias dx or x1");
    return palc_update(ctx, n, dl, dx, x1, x, x);
}

int bk_bls_matrixfree(bk_ctx* ctx, bk_op* J, const double* dR, const double* dzu, double dzp, const double* R,
                      double n, double xiu, double xip, int has_shift, double shift, double dotscale,
                      const bk_gmres_opts* lsopts, double* dX, double* dl, int* converged, int* itlinear) {
    if (!ctx || !J || !dR || !dzu || !R || !lsopts || !dX || !dl) return -1;
    if (dX == R || dX == dR || dX == dzu) return set_error(ctx, "bk_bls_matrixfree: dX must be a fresh buffer");
    return bls_matrixfree(ctx, J, dR, dzu, dzp, R, n, xiu, xip, has_shift != 0, shift, dotscale, *lsopts, dX, dl, converged, itlinear);
}

// solve_bls_block(::BorderingBLS, J, b::NTuple{M}, c::NTuple{M}, d::Matrix, rhst, rhsb), src/LinearBorderSolver.jl:173-206:
//   [ J   b ] [u1]   [rhst]        x1 = J^-1 rhst, x2_j = J^-1 b_j,  S_ij = d_ij - <c_i, x2_j>,  h_i = rhsb_i - <c_i, x1>,
//   [ c'  d ] [u2] = [rhsb]        u2 = S \ h,  u1 = x1 - sum_j u2_j x2_j.
// As in the reference the convergence flag of the x1 solve is dropped (`cv = true` after it, :186-189): only the m
// border solves are AND-ed; their iteration counts are returned.
int bk_bls_block_bordering(bk_ctx* ctx, bk_op* J, int m, const double* const* b, const double* const* c, const double* d,
                           const double* rhst, const double* rhsb, const bk_gmres_opts* lsopts, bk_precond* pl,
                           double* u1, double* u2, int* converged, int* itlinear) {
    if (!ctx || !J || !b || !c || !d || !rhst || !rhsb || !lsopts || !u1 || !u2) return -1;
    if (m < 1 || m > BK_MAX_BORDER) return set_error(ctx, "Linear bordered solver, wrong sizes! (1 <= m <= %d)", BK_MAX_BORDER);
    if (u1 == rhst) return set_error(ctx, "bk_bls_block_bordering: u1 must be a fresh buffer");
    const size_t n = J->n;
    WsGuard ws(ctx);
    double* x2[BK_MAX_BORDER];
    GmresResult g;
    BK_TRY(linsolve(ctx, J, rhst, u1, 0.0, 1.0, *lsopts, pl, &g));
    int cv = 1;
    for (int j = 0; j < m; ++j) {
        if (!b[j] || !c[j]) return -1;
        BK_TRY(ws.get(n, &x2[j]));
        BK_TRY(linsolve(ctx, J, b[j], x2[j], 0.0, 1.0, *lsopts, pl, &g));
        cv &= g.converged;
        if (itlinear) itlinear[j] = g.niter;
    }
    double S[BK_MAX_BORDER][BK_MAX_BORDER + 1];          // augmented [S | h]
    for (int i = 0; i < m; ++i) {
        double t;
        for (int j = 0; j < m; ++j) {
            BK_TRY(v_dot(ctx, n, c[i], x2[j], &t));
            S[i][j] = d[i * m + j] - t;
        }
        BK_TRY(v_dot(ctx, n, c[i], u1, &t));
        S[i][m] = rhsb[i] - t;
    }
    for (int k = 0; k < m; ++k) {                          // S \ h: LU with partial pivoting
        int piv = k;
        for (int i = k + 1; i < m; ++i)
            if (std::fabs(S[i][k]) > std::fabs(S[piv][k])) piv = i;
        if (S[piv][k] == 0.0) return set_error(ctx, "bk_bls_block_bordering: singular Schur complement");
        if (piv != k)
            for (int j = 0; j <= m; ++j) std::swap(S[k][j], S[piv][j]);
        for (int i = k + 1; i < m; ++i) {
            const double f = S[i][k] / S[k][k];
            for (int j = k; j <= m; ++j) S[i][j] -= f * S[k][j];
        }
    }
    for (int i = m - 1; i >= 0; --i) {
        double t = S[i][m];
        for (int j = i + 1; j < m; ++j) t -= S[i][j] * u2[j];
        u2[i] = t / S[i][i];
    }
    for (int j = 0; j < m; ++j) BK_TRY(v_axpby(ctx, n, -u2[j], x2[j], 1.0, u1));
    if (converged) *converged = cv;
    return 0;
}

// solve_bls_block(::MatrixFreeBLS, J, a, b, c, rhst, rhsb; shift, dotp), src/LinearBorderSolver.jl:440-450: ONE GMRES
// on the (N + m) operator MatrixFreeBLSmap (:338-352) over BorderedArray(u, p::Vector) -- the m border scalars live on
// the host next to the Krylov basis tails.
int bk_bls_block_matrixfree(bk_ctx* ctx, bk_op* J, int m, const double* const* a, const double* const* b, const double* c,
                            const double* rhst, const double* rhsb, int has_shift, double shift, double dotscale,
                            const bk_gmres_opts* lsopts, double* u1, double* u2, int* converged, int* itlinear) {
    if (!ctx || !J || !a || !b || !c || !rhst || !rhsb || !lsopts || !u1 || !u2) return -1;
    if (m < 1 || m > BK_MAX_BORDER) return set_error(ctx, "Linear bordered solver, wrong sizes! (1 <= m <= %d)", BK_MAX_BORDER);
    if (u1 == rhst) return set_error(ctx, "bk_bls_block_matrixfree: u1 must be a fresh buffer");
    if (lsopts->flavor >= BK_KRYLOV_MINRES) return set_error(ctx, "bk_bls_block_matrixfree: the bordered operator is not symmetric (use a GMRES flavor)");
    BorderedMapOp M;
    M.ctx = ctx; M.n = J->n; M.ntail = m;
    M.J = J; M.bscale = dotscale;
    for (int i = 0; i < m; ++i) {
        if (!a[i] || !b[i]) return -1;
        M.a[i] = a[i]; M.bvec[i] = b[i];
        for (int j = 0; j < m; ++j) M.c[i * m + j] = c[i * m + j];
    }
    M.has_shift = has_shift != 0; M.shift = shift;
    GmresResult r;
    BK_TRY(gmres_core(ctx, &M, rhst, rhsb, u1, u2, 0.0, 1.0, *lsopts, &r));
    if (converged) *converged = r.converged;
    if (itlinear) *itlinear = r.niter;
    return 0;
}

}  // extern "C"

// ================================================================== Newton correctors
namespace bk {

static int norm_of(bk_ctx* ctx, size_t n, const double* x, bool inf, double* out) {
    return inf ? v_nrminf(ctx, n, x, out) : v_nrm2(ctx, n, x, out);
}

// callback(state; fromNewton): the built-in cbMaxNorm veto first, then the user's function pointer
int newton_cb(const bk_newton_opts* no, const double* x, const double* fx, double residual, int step, int itlinear,
              double p, const double* z0u, double z0p, int from_newton) {
    if (no->max_residual > 0.0 && !(residual < no->max_residual)) return 0;      // cbMaxNorm, src/Newton.jl:156-159
    if (no->callback) return no->callback(no->callback_user, x, fx, residual, step, itlinear, p, z0u, z0p, from_newton) != 0;
    return 1;
}

// x <- x0 for a corrector that has to run in place, or whose loop never ran.  Accounted under a profiling scope of its own: whether a
// corrector call copied its predictor is read off "entry_copy", and "blas1" keeps counting the passes of the iterations alone.
static int palc_entry_copy(bk_ctx* ctx, size_t n, const double* x0, double* x) {
    if (n == 0) return 0;
    ProfScope ps(ctx, "entry_copy", 16.0 * n);
    BK_HIP(ctx, hipMemcpyAsync(x, x0, n * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    return 0;
}

}  // namespace bk

extern "C" {

int bk_newton(bk_ctx* ctx, bk_problem* prob, double* x, const double* params, int nparams, const bk_newton_opts* no,
              const bk_gmres_opts* lsopts, bk_precond* pl, bk_newton_result* res) {
    if (!ctx || !prob || !x || !params || !no || !lsopts || !res) return -1;
    if (no->max_iterations > BK_MAX_NEWTON_ITER) return set_error(ctx, "max_iterations > %d", BK_MAX_NEWTON_ITER);
    const size_t n = prob->nloc;
    WsGuard ws(ctx);
    double *fx = nullptr, *u = nullptr;
    BK_TRY(ws.get(n, &fx));
    BK_TRY(ws.get(n, &u));
    BK_TRY(bk_residual(prob, x, params, nparams, fx));
    double r;
    BK_TRY(norm_of(ctx, n, fx, no->norm_inf != 0, &r));
    int step = 0, itlin = 0;
    res->residuals[0] = r;
    int compute = newton_cb(no, x, fx, r, 0, 0, NAN, nullptr, NAN, 1);               // src/Newton.jl:88
    while (step < no->max_iterations && r > no->tol && compute) {
        bk_op* J = nullptr;
        BK_TRY(bk_jacobian(prob, x, params, nparams, &J));
        GmresResult g;
        int s = linsolve(ctx, J, fx, u, 0.0, 1.0, *lsopts, pl, &g);
        bk_op_destroy(J);
        if (s != 0) return s;
        itlin += g.niter;
        BK_TRY(v_axpby(ctx, n, -1.0, u, 1.0, x));            // minus!!(x, u), src/Newton.jl:97
        BK_TRY(bk_residual(prob, x, params, nparams, fx));
        BK_TRY(norm_of(ctx, n, fx, no->norm_inf != 0, &r));
        step += 1;
        res->residuals[step] = r;
        compute = newton_cb(no, x, fx, r, step, g.niter, NAN, nullptr, NAN, 1);     // :111
    }
    res->converged = (res->residuals[step] < no->tol) & newton_cb(no, x, fx, r, step, 0, NAN, nullptr, NAN, 1);   // :114
    res->itnewton = step;
    res->itlinear = itlin;
    return 0;
}

int bk_newton_palc(bk_ctx* ctx, bk_problem* prob, double* x, double* p, const double* z0u, double z0p,
                   const double* tauu, double taup, double ds, double theta, const double* params, int nparams,
                   int ipar, double p_min, double p_max, const bk_newton_opts* no, const bk_bordering_opts* bo,
                   const bk_gmres_opts* lsopts, bk_precond* pl, bk_newton_result* res) {
    return bk_newton_palc_from(ctx, prob, x, x, p, z0u, z0p, tauu, taup, ds, theta, params, nparams, ipar, p_min, p_max, no, bo,
                               lsopts, pl, res);
}

// The corrector from a predictor x0 that stays as it is (x0 == x: in place, bk_newton_palc).  Where the Newton update rides in the
// bordering solve's tail pass (fuse_update below) the first iteration reads x0 -- entry residual, arc-length equation, dF/dp, the
// Jacobian handle, both solves -- and its update writes x = x0 - u; the later iterations run in place on x.  No copy of x0 then
// (option palc_entry_copy = 1 makes it first, as every other path does: line search, check_precision, MatrixFreeBLS).
int bk_newton_palc_from(bk_ctx* ctx, bk_problem* prob, const double* x0, double* x, double* p, const double* z0u, double z0p,
                        const double* tauu, double taup, double ds, double theta, const double* params, int nparams,
                        int ipar, double p_min, double p_max, const bk_newton_opts* no, const bk_bordering_opts* bo,
                        const bk_gmres_opts* lsopts, bk_precond* pl, bk_newton_result* res) {
    if (!ctx || !prob || !x0 || !x || !p || !z0u || !tauu || !params || !no || !bo || !lsopts || !res) return -1;
    if (ipar < 0 || ipar >= nparams || nparams > BK_MAX_PARAMS) return set_error(ctx, "bad parameter index");
    if (no->max_iterations > BK_MAX_NEWTON_ITER) return set_error(ctx, "max_iterations > %d", BK_MAX_NEWTON_ITER);
    const size_t n = prob->nloc;
    // length(x) of the reference's NormalisedDot (Palc.jl:1-6) = GLOBAL number of unknowns
    double Nglob = 1.0;
    for (int a = 0; a < prob->desc.ndim; ++a) Nglob *= prob->desc.n[a];
    if (prob->desc.pde == BK_PDE_CGL2D) Nglob *= 2.0;
    const double dotscale = 1.0 / Nglob;
    const double eps = 1.4901161193847656e-08;             // sqrt(eps(Float64)): src/Problems.jl:69-70
    WsGuard ws(ctx);
    double *res_f = nullptr, *dFdp = nullptr, *u = nullptr, *x_pred = nullptr;
    BK_TRY(ws.get(n, &res_f));
    BK_TRY(ws.get(n, &dFdp));
    BK_TRY(ws.get(n, &u));
    const bool linesearch = no->linesearch != 0;
    if (linesearch) BK_TRY(ws.get(n, &x_pred));
    const double alpha0 = no->alpha > 0.0 ? no->alpha : 1.0;                        // NewtonPar defaults, src/Newton.jl:29-31
    const double alpha_min = no->alpha_min > 0.0 ? no->alpha_min : 1e-3;
    double alpha = alpha0;
    double par[BK_MAX_PARAMS];
    for (int i = 0; i < nparams; ++i) par[i] = params[i];
    const bool inf = no->norm_inf != 0;
    double dz0;                                            // <z0.u, tau.u>: second term of arc_length_eq, Palc.jl:51-55
    BK_TRY(v_dot(ctx, n, z0u, tauu, &dz0));
    auto Nfun = [&](const double* xx, double pp, double* out) -> int {       // Palc.jl:212
        double d;
        BK_TRY(v_dot(ctx, n, xx, tauu, &d));
        *out = (d * dotscale * theta + (pp - z0p) * taup * (1.0 - theta) - ds) - (dz0 * dotscale * theta);
        return 0;
    };
    // option palc_fuse_update (read once per corrector call): BorderingBLS without check_precision and no line search -- nobody reads
    // u after the update, so x <- x - u rides in the tail pass of the bordering solve (bls_bordering: xnew)
    const bool fuse_update = bo->kind == 0 && bo->check_precision == 0 && !linesearch && ctx->opt("palc_fuse_update", 1.0) != 0.0;
    // cur = the current iterate: the predictor x0 itself until the first fused update has written x
    const double* cur = x;
    if (x0 != x) {
        if (fuse_update && ctx->opt("palc_entry_copy", 0.0) == 0.0) cur = x0;
        else BK_TRY(palc_entry_copy(ctx, n, x0, x));
    }
    double pc = *p;
    par[ipar] = pc;
    BK_TRY(bk_residual(prob, cur, par, nparams, res_f));
    double res_n, rf;
    BK_TRY(Nfun(cur, pc, &res_n));
    BK_TRY(norm_of(ctx, n, res_f, inf, &rf));
    double r = std::max(rf, std::fabs(res_n));
    int step = 0, itlin = 0;
    res->residuals[0] = r;
    bool line_step = true;
    int compute = newton_cb(no, cur, res_f, r, 0, 0, pc, z0u, z0p, 0);              // Palc.jl:235
    while (step < no->max_iterations && r > no->tol && line_step && compute) {
        par[ipar] = pc;                                    // dFdp = (F(x, p + eps) - res_f)/eps, Palc.jl:239-240
        BK_TRY(prob->dparam(cur, par, nparams, ipar, eps, res_f, dFdp));
        bk_op* J = nullptr;
        BK_TRY(bk_jacobian(prob, cur, par, nparams, &J));
        double up = 0.0;
        int cv = 0, it[2] = {0, 0};
        int s;
        if (bo->kind == 1) {                                  // MatrixFreeBLS: one GMRES on the (N + 1) operator, no preconditioner
            int itm = 0;
            s = bls_matrixfree(ctx, J, dFdp, tauu, taup, res_f, res_n, theta, 1.0 - theta, false, 0.0, dotscale, *lsopts, u, &up, &cv, &itm);
            it[0] = itm; it[1] = 0;
        } else {
            s = bls_bordering(ctx, J, dFdp, tauu, taup, res_f, res_n, theta, 1.0 - theta, false, 0.0, dotscale, *bo,
                              *lsopts, pl, u, &up, &cv, it, fuse_update ? x : nullptr, cur);
        }
        bk_op_destroy(J);
        if (s != 0) return s;
        cur = x;                                             // (cur != x only with fuse_update: the tail pass has written x = x0 - u)
        itlin += it[0] + it[1];
        if (linesearch) {                                    // Palc.jl:254-281
            line_step = false;
            while (!line_step && alpha > alpha_min) {
                BK_TRY(v_axpbyz(ctx, n, 1.0, x, -alpha, u, x_pred));                // x_pred = x - alpha u
                const double p_pred = pc - alpha * up;
                par[ipar] = p_pred;
                BK_TRY(bk_residual(prob, x_pred, par, nparams, res_f));
                BK_TRY(Nfun(x_pred, p_pred, &res_n));
                BK_TRY(norm_of(ctx, n, res_f, inf, &rf));
                r = std::max(rf, std::fabs(res_n));
                if (r < res->residuals[step]) {
                    if (r < res->residuals[step] / 4.0 && alpha < 1.0) alpha *= 2.0;
                    line_step = true;
                    BK_TRY(v_copy(ctx, n, x_pred, x));
                    pc = std::min(std::max(p_pred, p_min), p_max);
                } else {
                    alpha /= 2.0;
                }
            }
            alpha = alpha0;                                  // "we put back the initial value"
            par[ipar] = pc;
        } else {
            if (!fuse_update) BK_TRY(v_axpby(ctx, n, -1.0, u, 1.0, x));        // x = minus!!(x, u), Palc.jl:282
            pc = std::min(std::max(pc - up, p_min), p_max);  // clamp, :283
            par[ipar] = pc;
            BK_TRY(bk_residual(prob, x, par, nparams, res_f));
            BK_TRY(Nfun(x, pc, &res_n));
            BK_TRY(norm_of(ctx, n, res_f, inf, &rf));
            r = std::max(rf, std::fabs(res_n));
        }
        step += 1;
        res->residuals[step] = r;
        compute = newton_cb(no, x, res_f, r, step, it[0] + it[1], pc, z0u, z0p, 0);   // Palc.jl:294
    }
    if (cur != x) BK_TRY(palc_entry_copy(ctx, n, x0, x));  // no iteration ran: the result is the predictor
    *p = pc;
    res->converged = (res->residuals[step] < no->tol) & newton_cb(no, x, res_f, r, step, 0, pc, z0u, z0p, 0);   // :297
    res->itnewton = step;
    res->itlinear = itlin;
    return 0;
}

}  // extern "C"
