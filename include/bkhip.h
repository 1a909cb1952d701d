/*
 * bkhip.h -- C ABI of the MI355X-native Newton-Krylov corrector for BifurcationKit.jl's
 * pseudo-arclength continuation (PALC).
 *
 * This is the drop-in boundary: plain pointers and sizes, no torch / C++ types.  Each entry
 * point cites the reference interface (paths relative to the BifurcationKit.jl checkout) it
 * replaces.  Julia reaches it with `ccall` (julia/BifurcationKitHIP.jl); the
 * parity tests reach it with Python `ctypes` using the same call sequence.
 *
 * Conventions
 *   - every function returns an int status: 0 = ok, <0 = error (bk_last_error() has the text).
 *     Non-convergence of an iterative solver is NOT an error: it is reported through the
 *     `converged` out-parameter, like the reference which only `@debug`s it
 *     (src/Newton.jl:93, src/LinearSolver.jl:289).
 *   - `double*` vector arguments are DEVICE pointers (HIP) to fp64 data of the problem's LOCAL
 *     length (bk_problem_nlocal); scalars travel by value / host pointers.
 *   - all work is enqueued on the context's HIP stream; functions that return host scalars
 *     synchronise that stream before returning, the others are asynchronous.
 *   - state layout: flat index = i + Nx*(j + Ny*k), x fastest -- the order the reference's
 *     `kron` assembly and `vec` of an [x,y,z] comprehension produce (examples/SH3d.jl:38-39,77).
 *     Multi-GPU (3-D Swift-Hohenberg): z-slabs of contiguous planes, one slab per rank.
 */
#ifndef BKHIP_H
#define BKHIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bk_ctx bk_ctx;         /* device, stream, scratch, (optional) communicator        */
typedef struct bk_problem bk_problem; /* a stencil PDE on a grid: residual F(u,p) and J(u,p)      */
typedef struct bk_op bk_op;           /* a linear operator handle = what `jacobian(prob,x,p)` returns */
typedef struct bk_precond bk_precond; /* a left preconditioner Pl (GMRESKrylovKit.Pl)              */

/* ------------------------------------------------------------------ context ---------------- */

#define BK_UNIQUE_ID_BYTES 128

int bk_version(void);
/* Layout version of the option structs below (bk_gmres_opts, bk_bordering_opts, bk_eig_opts, ...).  A binding compares it with
 * the BK_ABI_VERSION it was written against before its first call: the structs carry no size field, and a client built against
 * an older header would hand over shorter ones.                                                                  */
#define BK_ABI_VERSION 6
int bk_abi_version(void);
/* Create a single-GPU context on `device`; `stream` is the hipStream_t all work is enqueued on
 * (NULL = the default stream, which orders the library with the caller's own default-stream work). */
int bk_ctx_create(bk_ctx** ctx, int device, void* stream);
/* Multi-GPU context: one process per GPU, RCCL communicator built from a unique id that rank 0
 * obtained with bk_comm_unique_id() and broadcast out-of-band (torch.distributed / MPI).
 * No reference counterpart: the reference is single-process.             */
int bk_comm_unique_id(void* id128);
int bk_ctx_create_dist(bk_ctx** ctx, int device, void* stream, int rank, int nranks,
                       const void* id128);
/* Test-only communicator: collectives staged through host buffers and user callbacks (lets two
 * ranks share one GPU, or run over gloo).  allreduce(user, buf, n, op) with op 0=sum 1=max acts
 * in place on a host buffer; sendrecv(user, sendbuf, nsend, dst, recvbuf, nrecv, src) exchanges
 * host buffers with neighbour ranks (dst/src = -1: no peer).                                     */
typedef int (*bk_allreduce_fn)(void* user, double* buf, int n, int op);
typedef int (*bk_sendrecv_fn)(void* user, const double* sendbuf, size_t nsend, int dst,
                              double* recvbuf, size_t nrecv, int src);
int bk_ctx_create_hostcomm(bk_ctx** ctx, int device, void* stream, int rank, int nranks,
                           bk_allreduce_fn allreduce, bk_sendrecv_fn sendrecv, void* user);
/* THREADING of the callbacks.  A host-staged context ENQUEUES its collectives in the stream like an RCCL context does
 * (device-resident Arnoldi chunks, halo exchange under the interior z-chunks): each one is a stream-ordered hand-over to a
 * proxy thread the library owns, and the callbacks run ON THAT THREAD, never on the caller's (a Julia client needs
 * @cfunction callbacks that may be entered from a foreign thread: Julia >= 1.9).  `user` is passed through untouched.
 * Second lane (option two_lanes, solver: ls(J, rhs1, rhs2) with both solves in flight): its collectives are issued
 * concurrently with the context's own and must never be matched against them, so it needs a communicator of its own:
 * register one with bk_ctx_set_lane_comm (same callback types, its own `user`; e.g. a second gloo / MPI group).  Without
 * a registered lane communicator a host-staged context simply runs one lane.  RCCL contexts split their communicator
 * themselves (ncclCommSplit).  No reference counterpart.                                                              */
int bk_ctx_set_lane_comm(bk_ctx* ctx, bk_allreduce_fn allreduce, bk_sendrecv_fn sendrecv, void* user);
/* What the communicator of this context is: *kind 0 = none, 1 = RCCL, 2 = host-staged test communicator; *rank /
 * *nranks as the communicator itself reports them (RCCL: ncclCommUserRank / ncclCommCount -- the number of ranks RCCL
 * actually connected, bench.py prints it next to a multi-GPU number).  No reference counterpart.                    */
int bk_comm_info(bk_ctx* ctx, int* kind, int* rank, int* nranks);
/* Time the two collectives of the hot path on this context's communicator (collective call: every rank must make it):
 * what 0 = in-stream all-reduce (sum) of `count` doubles (count <= 256: the projections of one Arnoldi step),
 * what 1 = halo exchange of `count` doubles with each z-neighbour (ncclSend/ncclRecv group).  `reps` back-to-back calls
 * between two stream synchronisations; *us_per_call = host wall time / reps.  No reference counterpart.               */
int bk_comm_probe(bk_ctx* ctx, int what, size_t count, int reps, double* us_per_call);
int bk_ctx_destroy(bk_ctx* ctx);
const char* bk_last_error(bk_ctx* ctx);
int bk_ctx_sync(bk_ctx* ctx);
/* Tuning knobs ("sh_kernel": 0 gather / 1 streaming; "sh_zchunk"; "dgks_eta"; "dct_fft"; "dct_roundtrip";
 * "dct_gemm"; "halo_overlap"; ...): experiments and cross-checks, the defaults are the measured optimum.
 * One key is no knob: "solver_state_hold".  Set to 1 it puts aside the state a GMRES solve hands to the next one on this
 * context (the Arnoldi step count of the last solve, from which the next sizes its first block, and with "gmres_newton_carry"
 * the carried shifts); set to 0 it puts that state back.  Solves made in between leave no trace, so the solves after them run
 * exactly as they would have without them (continuation_hopf's codim-2 detection between curve steps).  One level: a second 1
 * before the 0 overwrites what is held; 0 with nothing held does nothing.  Reading it gives 1 while a state is held.  */
int bk_ctx_set_option(bk_ctx* ctx, const char* key, double value);
int bk_ctx_get_option(bk_ctx* ctx, const char* key, double* value);
/* Per-kernel timing with HIP events on the context's stream (bench.py's roofline leg):
 * names: "jvp", "residual", "multidot", "multiaxpy", "dct_pass", "blas1", "combine"; multi-GPU also "halo",
 * "alltoall", "transpose".                                                                       */
int bk_prof_enable(bk_ctx* ctx, int on);
int bk_prof_reset(bk_ctx* ctx);
int bk_prof_get(bk_ctx* ctx, const char* name, double* total_ms, long long* calls,
                double* alg_bytes);

/* Diagnostics: with option "solver_trace" != 0 every Krylov linear solve appends its residual-estimate history (one
 * value per iteration: GMRES |y_k+1|, MINRES phibar) to a per-context log; a negative entry -(k) opens the k-th solve
 * and is followed by the initial residual norm.  Copies up to cap entries into buf (may be NULL), *n = entries
 * available; reset != 0 clears the log.  The reference's counterpart is the `verbose` / `log = true` switch of the
 * Krylov packages (src/LinearSolver.jl:169,202,244).                                                              */
int bk_solver_history(bk_ctx* ctx, double* buf, size_t cap, size_t* n, int reset);
/* Block log of the GMRES solves (ABI 6; option "gmres_block_log" != 0): one record of 11 doubles per Arnoldi block -- solve number
 * (from 1, since the last reset), first Hessenberg column j of the block, operator applications issued, steps the host algebra
 * accepted (fewer: the block was truncated at a small pivot), last pivot ratio of the block's Cholesky factor (the conditioning
 * margin against the truncation threshold 1e-8), the block's Newton shifts theta[0..3] (NaN: slot unused), residual estimate and
 * tolerance when the block was issued.  Same calling convention as bk_solver_history.  The library never writes to stderr.
 * Reference counterpart: `verbose` of the Krylov packages (src/LinearSolver.jl:169,202,244).                              */
int bk_solver_block_log(bk_ctx* ctx, double* buf, size_t cap, size_t* n, int reset);

/* ------------------------------------------------------------------ memory ----------------- */

int bk_malloc(bk_ctx* ctx, size_t n, double** out);
int bk_free(bk_ctx* ctx, double* p);
int bk_upload(bk_ctx* ctx, double* dst_dev, const double* src_host, size_t n);
int bk_download(bk_ctx* ctx, double* dst_host, const double* src_dev, size_t n);

/* ---------------------------------------- BLAS-1: the VectorInterface methods ---------------
 * of src/BorderedArrays.jl:86-217 on the `.u` part (the scalar `.p` part stays on the host).
 * Dots / norms are global (all-reduced over the communicator) and deterministic run-to-run.     */
int bk_vec_copy(bk_ctx* ctx, size_t n, const double* x, double* y);              /* _copyto!    :34 */
int bk_vec_zero(bk_ctx* ctx, size_t n, double* x);                               /* zerovector! :97 */
int bk_vec_scale(bk_ctx* ctx, size_t n, double a, double* x);                    /* scale!     :118 */
int bk_vec_axpby(bk_ctx* ctx, size_t n, double a, const double* x, double b, double* y);
                                                     /* y = a x + b y : VI.add!(y,x,a,b) :180-196 */
int bk_vec_dot(bk_ctx* ctx, size_t n, const double* x, const double* y, double* out); /* inner :213 */
int bk_vec_nrm2(bk_ctx* ctx, size_t n, const double* x, double* out);            /* norm     :55-70 */
int bk_vec_nrminf(bk_ctx* ctx, size_t n, const double* x, double* out);  /* norminf LinearSolver.jl:4 */
/* Fused Krylov-basis primitives (what the Gram-Schmidt loops inside KrylovKit / IterativeSolvers do with
 * k separate VI.inner / VI.add! passes).  V holds k vectors, V_i = V + i*ldv, k <= 64.
 *   multidot : out[i] = <V_i, w> (i < k), out[k] = <w, w>           -- one pass over V and w
 *   multiaxpy: dst = scale * (src + sum_i c[i] V_i); src may be NULL; *nrm2sq (may be NULL) = ||dst||^2 */
int bk_krylov_multidot(bk_ctx* ctx, size_t n, const double* V, size_t ldv, int k, const double* w,
                       double* out_host);
int bk_krylov_multiaxpy(bk_ctx* ctx, size_t n, const double* V, size_t ldv, int k, const double* c_host,
                        const double* src, double scale, double* dst, double* nrm2sq);

/* ------------------------------------------------------------------ problems --------------- */

enum {
    BK_PDE_SH = 1,    /* Swift-Hohenberg 2-D/3-D, Neumann-ghost: examples/SH3d.jl:16-53,
                         examples/SH2d-fronts.jl:13-34.  params = {l, nu}                           */
    BK_PDE_SH1D = 2,  /* 1-D cubic-quintic SH, Dirichlet: examples/SHpde_snaking.jl:16-25.
                         params = {lambda, nu}                                                      */
    BK_PDE_CGL2D = 3  /* 2-D complex Ginzburg-Landau, 2 stacked real fields, Dirichlet:
                         examples/cGL2d.jl:6-54,281-318.  params = {r, mu, nu, c3, c5, gamma}       */
};
#define BK_MAX_PARAMS 8

typedef struct {
    int pde;            /* BK_PDE_*                                                              */
    int ndim;           /* 1, 2 or 3                                                             */
    int n[3];           /* GLOBAL Nx, Ny, Nz (unused dims = 1)                                   */
    double l[3];        /* half-widths lx, ly, lz: h = 2 l / N (examples/SH3d.jl:18-20)           */
} bk_problem_desc;

int bk_problem_create(bk_ctx* ctx, const bk_problem_desc* desc, bk_problem** out);
int bk_problem_destroy(bk_problem* prob);
/* local (this rank's) vector length and the slab [lo, hi) of the slowest grid index it owns     */
int bk_problem_nlocal(bk_problem* prob, size_t* nlocal, int* slab_lo, int* slab_hi);
/* out = F(u, params): F_sh examples/SH3d.jl:44-47, R_SH SHpde_snaking.jl:19-23,
 * Fcgl! examples/cGL2d.jl:44-47                                                                  */
int bk_residual(bk_problem* prob, const double* u, const double* params, int nparams, double* out);
/* out = (F(u, p + eps) - F(u, p)) / eps for params[ipar] -- the finite-difference dF/dp of newton_palc and the Bordered
 * tangent (src/continuation/Palc.jl:239-240, src/continuation/Tangents.jl:77-82).  Every parameter of these problems
 * multiplies a pointwise term and the stencil part cancels identically, so the quotient is evaluated as
 * ((p + eps) - p)/eps * phi_p(u) in one pass without the ~1e-8 white rounding noise of the two-residual form (context
 * option "fd_dparam" = 0 selects the literal two-residual form).  out must not alias u.                            */
int bk_residual_dparam(bk_problem* prob, const double* u, const double* params, int nparams, int ipar, double eps,
                       double* out);
/* J(u, params) as an operator handle: the closure `dx -> dF_sh(x, p, dx)` of
 * examples/SH3d.jl:119 / the opaque Jacobian object of src/Problems.jl:98-101.  Like the Julia
 * closure it REFERENCES u (no copy): u must stay alive and unchanged while the handle is used. */
int bk_jacobian(bk_problem* prob, const double* u, const double* params, int nparams, bk_op** out);
/* the adjoint Jacobian J(u, p)' (JAd_at_xp of src/codim2/MinAugHopf.jl:66-80): the transposed pointwise block for
 * cGL2d, J itself for the (symmetric) Swift-Hohenberg problems.                                                   */
int bk_jacobian_adjoint(bk_problem* p, const double* u, const double* params, int nparams, bk_op** out);
int bk_op_destroy(bk_op* op);
/* out = a0*v + a1*J*v : _axpy_op, src/LinearSolver.jl:46-64 (a0=0,a1=1: apply, src/Utils.jl:191) */
int bk_op_apply(bk_op* op, const double* v, double a0, double a1, double* out);

/* ------------------------------------------------------------------ preconditioner ---------
 * Pl^-1 = ((I + Lap)^2 + shift I)^-1 applied exactly through the DCT-II diagonalisation of the
 * Neumann-ghost Laplacian.  shift = 0 is `Pl = cholesky(Symmetric(L1))` of examples/SH3d.jl:88;
 * shift = 1 is `lu(L1 + I)` of examples/SH2d-fronts.jl:121.                                      */
int bk_precond_sh_create(bk_problem* prob, double shift, bk_precond** out);
/* Pl^-1 = (Lap - c I)^-1 on both fields of a BK_PDE_CGL2D problem (Dirichlet 5-point Laplacian of
 * examples/cGL2d.jl:6-22, diagonalised by the DST-I), c > 0.  The reference has no iterative counterpart here: its
 * cGL2d runs use sparse LU (DefaultLS, and `EigArpack(1.0, :LM)` factorises J - sigma I inside ARPACK,
 * examples/cGL2d.jl:96, src/EigSolver.jl:85); this is the matrix-free replacement that keeps GMRES mesh-independent. */
int bk_precond_lap_create(bk_problem* prob, double c, bk_precond** out);
/* Pl^-1 = (Lap (x) I_2 + [[a, -b], [b, a]])^-1 on the stacked fields (u1, u2) of a BK_PDE_CGL2D problem: the 2x2 block is
 * inverted per sine mode.  With a = r, b = nu this IS the Jacobian of the trivial state u = 0 (Jcgl, examples/cGL2d.jl:57-79:
 * f1u = r, f1v = -nu, f2u = nu, f2v = r), i.e. the exact solve the reference gets from its sparse LU there; a = r - sigma
 * gives the shift-inverted operator of `EigArpack(sigma, :LM)` (cGL2d.jl:96).  b != 0 keeps every block invertible
 * (also at a Hopf point, where Lap + r I is singular); b = 0 requires a < 0.                                          */
int bk_precond_cgl_create(bk_problem* prob, double a, double b, bk_precond** out);
int bk_precond_destroy(bk_precond* pc);
int bk_precond_apply(bk_precond* pc, const double* v, double* out);   /* out = Pl \ v             */
/* out = a0 x + a1 Pl \ (J x): the `_linmap` closure GMRESKrylovKit hands to KrylovKit when it has a left preconditioner
 * (src/LinearSolver.jl:270-277), i.e. the operator every Arnoldi step of a preconditioned solve applies.  When `pl` is the
 * spectral preconditioner of J's own Swift-Hohenberg problem (Pl = L1 + s I, J = -L1 + diag g(u)) it is evaluated WITHOUT the
 * stencil, as (a0 - a1) x + a1 Pl \ ((g(u) + s) .* x) -- the form the solvers' Arnoldi steps use (context option
 * "gmres_stencil_free": 1 = where the transform kernels take the pointwise factor in, 2 = everywhere, 0 = never: stencil kernel,
 * then Pl).  *stencil_free (optional) reports which form ran.  out must not alias x.                                        */
int bk_precond_op_apply(bk_ctx* ctx, bk_precond* pl, bk_op* J, const double* x, double a0, double a1, double* out,
                        int* stencil_free);
/* Its twin for the explicit residual check of a left-preconditioned GMRES solve of (a0 + a1 J) x = rhs in `flavor`
 * (BK_GMRES_KRYLOVKIT / _ITERATIVESOLVERS / _KRYLOVJL): *nrm = the value the solve compares with its tolerance once the Arnoldi
 * estimate has converged, |Pl \ rhs - a0 x - a1 Pl \ (J x)| (KrylovKit), |Pl \ (rhs - (a0 + a1 J) x)| (the others).  With the
 * spectral preconditioner on the LDS transform kernels (single rank, round trip on) the norm comes out of the spectrum --
 * Pl \ of ONE vector rhs - (...) x formed from the chain's own stencil pass, forward transforms only, sum_k sym_k^2 |.^_k|^2 -- instead of
 * the residual vector through the whole chain (context option "gmres_check_spectral", default 1; 0 = the chain).  *spectral
 * (optional) reports which path ran.                                                                                          */
int bk_precond_check_norm(bk_ctx* ctx, bk_precond* pl, bk_op* J, const double* x, const double* rhs, double a0, double a1, int flavor,
                          double* nrm, int* spectral);

/* ------------------------------------------------------------------ linear solver ----------
 * (ls::AbstractLinearSolver)(J, rhs; a0, a1) -> (x, success, niter): src/LinearSolver.jl:12.   */
enum {
    BK_GMRES_KRYLOVKIT = 0,        /* GMRESKrylovKit semantics, src/LinearSolver.jl:223-291:
                                      maxiter = restart cycles, tol = max(atol, rtol*||b||),
                                      niter = numops (operator applications)                       */
    BK_GMRES_ITERATIVESOLVERS = 1, /* GMRESIterativeSolvers semantics, :149-206: maxiter = inner
                                      iterations, tol = max(rtol*||r0||, atol), niter = iterations */
    BK_KRYLOV_MINRES = 3,          /* KrylovLS(KrylovAlg = :minres), :336-341 (symmetric solvers, "centered" SPD
                                      preconditioner M = Pl): Paige-Saunders MINRES on a0 + a1 J, stop on the
                                      estimated M^-1-norm of the residual <= atol + rtol*beta1; dim unused;
                                      maxiter = itmax; 8 vectors instead of a Krylov basis                        */
    BK_KRYLOV_CG = 4,              /* KrylovLS(KrylovAlg = :cg): preconditioned CG for SPD a0 + a1 J; stops without
                                      success on non-positive curvature                                            */
    BK_GMRES_KRYLOVJL = 2          /* KrylovLS / KrylovLSInplace with :gmres, :316-414: Krylov.jl stopping rule
                                      ||r|| <= atol + rtol*||r0||, dim = `memory` used as restart length,
                                      maxiter = itmax (inner iterations), niter = iterations; Pl = `M`      */
};
typedef struct {
    int flavor;      /* BK_GMRES_*                                                               */
    int dim;         /* Krylov dimension / restart (GMRESKrylovKit.dim, GMRESIterativeSolvers.restart) */
    int maxiter;
    double atol;
    double rtol;
    bk_precond* pr;  /* right preconditioner or NULL: GMRESIterativeSolvers.Pr (src/LinearSolver.jl:178,201 -- the solver iterates
                        on Pl^-1 (a0 I + a1 J) Pr^-1 y = Pl^-1 rhs and returns x = Pr^-1 y) and KrylovLS's `N = Pr` for the
                        non-symmetric methods (:343); an error with the KrylovKit flavor (GMRESKrylovKit has no such field,
                        :223-250); ignored by :minres / :cg exactly as the reference does ("we only pass centered
                        preconditioner", :339-341).  bk_gmres_default_opts sets NULL.                                      */
} bk_gmres_opts;
void bk_gmres_default_opts(bk_gmres_opts* o, int flavor);   /* the reference's defaults           */
/* Solve (a0 I + a1 J) x = rhs, x0 = 0.  `pl` may be NULL.  With `pl` the KrylovKit flavor solves
 * (a0 I + a1 Pl^-1 J) x = Pl^-1 rhs -- shift applied after the preconditioner, exactly the
 * reference's branch src/LinearSolver.jl:268-288.  x must not alias rhs; rhs is not modified.   */
int bk_gmres(bk_ctx* ctx, bk_op* J, const double* rhs, double* x, double a0, double a1,
             const bk_gmres_opts* opts, bk_precond* pl, int* converged, int* niter,
             double* resnorm);
/* (ls)(J, rhs1, rhs2): two sequential solves, flags ANDed, src/LinearSolver.jl:15-19.           */
int bk_gmres2(bk_ctx* ctx, bk_op* J, const double* rhs1, const double* rhs2, double* x1,
              double* x2, double a0, double a1, const bk_gmres_opts* opts, bk_precond* pl,
              int* converged, int niter[2]);

/* ------------------------------------------------------------------ bordered solvers -------
 * (lbs)(J, dR, dzu, dzp, R, n, xi_u, xi_p; shift, dotp) -> (dX, dl, success, itlinear):
 * src/LinearBorderSolver.jl:3-6.  Solves
 *     [ shift I + J      dR     ] [dX]   [R]
 *     [ xi_u dzu' S   xi_p dzp  ] [dl] = [n]       with dotp(x,y) = dotscale * <x,y>
 * (PALC passes dotscale = 1/N, xi_u = theta, xi_p = 1-theta: solve_bls_palc :16-36).            */
typedef struct {
    double tol;            /* BorderingBLS.tol             (:63)                                  */
    int check_precision;   /* BorderingBLS.check_precision (:66)                                  */
    int k;                 /* BorderingBLS.k               (:69)                                  */
    int kind;              /* which bordered solver the correctors (bk_newton_palc, bk_cont_*) use: 0 = BorderingBLS (the
                              fields above), 1 = MatrixFreeBLS (:326-335,424-437: ONE GMRES on the (N+1) operator; tol,
                              check_precision, k and the preconditioner are not used by it, as in the reference).
                              bk_bls_bordering itself ignores the field.                                           */
} bk_bordering_opts;
int bk_bls_bordering(bk_ctx* ctx, bk_op* J, const double* dR, const double* dzu, double dzp,
                     const double* R, double n, double xiu, double xip, int has_shift,
                     double shift, double dotscale, const bk_bordering_opts* bopts,
                     const bk_gmres_opts* lsopts, bk_precond* pl, double* dX, double* dl,
                     int* converged, int itlinear[2]);                   /* BorderingBLS :88-166 */
/* Iteration accounting with check_precision (k refinement passes, :111-121): the reference's BEC solves
 * (shift I + J) x = dR again on every pass (:134) and returns the counts of the LAST pass.  dR does not change between
 * the passes, so this implementation solves it once and reports that solve's count and flag for every pass -- the same
 * numbers the repeated (deterministic) solve would return, at one solve less per pass; itlinear[0] is the last pass's
 * solve with the refreshed right-hand side, as in the reference.                                                      */
/* Probe of the pass bk_newton_palc runs instead of the bordered tail x1 <- x1 - dl dx and the Newton update x <- x - x1 when
 * nobody reads x1 afterwards (BorderingBLS without check_precision, no line search; context option "palc_fuse_update",
 * default 1): x <- x - (x1 - dl dx) in ONE pass over dx, x1 and x, rounded exactly as bk_vec_axpby(-dl, dx, 1, x1) followed by
 * bk_vec_axpby(-1, x1, 1, x).  x1 and dx are only read; x must not alias them.                                         */
int bk_palc_update(bk_ctx* ctx, size_t n, double dl, const double* dx, const double* x1, double* x);
int bk_bls_matrixfree(bk_ctx* ctx, bk_op* J, const double* dR, const double* dzu, double dzp,
                      const double* R, double n, double xiu, double xip, int has_shift,
                      double shift, double dotscale, const bk_gmres_opts* lsopts, double* dX,
                      double* dl, int* converged, int* itlinear);        /* MatrixFreeBLS :424-437 */

/* solve_bls_block(::BorderingBLS, ...) for an m-column border (normal forms, Bogdanov-Takens; :173-206):
 *     [ J   b ] [u1]   [rhst]      b, c: m device vectors each; d: m x m host, row-major d[i*m + j];
 *     [ c'  d ] [u2] = [rhsb]      plain inner products (VI.inner), no shift.
 * u1 (device, fresh buffer) and u2[m] (host) receive the solution, itlinear[m] the iteration counts of the m
 * border solves, *converged their AND (the flag of the J u = rhst solve is dropped, as in the reference).      */
#define BK_MAX_BORDER 8
int bk_bls_block_bordering(bk_ctx* ctx, bk_op* J, int m, const double* const* b, const double* const* c,
                           const double* d, const double* rhst, const double* rhsb,
                           const bk_gmres_opts* lsopts, bk_precond* pl, double* u1, double* u2,
                           int* converged, int* itlinear);

/* solve_bls_block(::MatrixFreeBLS, J, a, b, c, rhst, rhsb; shift, dotp) (:440-450): ONE GMRES on the (N + m) operator
 * MatrixFreeBLSmap (:338-352) acting on BorderedArray(u, p::Vector{m}):
 *     out.u = (J + shift) u + sum_i p_i a_i ,   out.p = c p + [dotscale <b_i, u>]_i          c: m x m row-major.   */
int bk_bls_block_matrixfree(bk_ctx* ctx, bk_op* J, int m, const double* const* a, const double* const* b,
                            const double* c, const double* rhst, const double* rhsb, int has_shift,
                            double shift, double dotscale, const bk_gmres_opts* lsopts, double* u1,
                            double* u2, int* converged, int* itlinear);

/* MatrixFreeBLS with the solver's LEFT preconditioner carried into the bordered system as diag(Pl, 1): the arguments of
 * bk_bls_matrixfree / bk_bls_block_matrixfree plus pl (required).  ONE GMRES on
 *     out.u = Pl^-1 ((J + shift I) x.u) + sum_j x.p[j] (Pl^-1 a_j) ,   out.p = c x.p + [xi_u dotscale <b_i, x.u>]_i
 * (MatrixFreeBLSmap, src/LinearBorderSolver.jl:326-352, under the preconditioned map of src/LinearSolver.jl:270-278) with the
 * right-hand side (Pl^-1 R, n): the top preconditioned, the tail untouched.  The unbordered part runs as the preconditioned
 * operator of bk_gmres does (stencil-free where the plan allows it, option gmres_stencil_free); stopping rules and the explicit
 * residual check are those of the GMRES flavor, on the BorderedArray norm of the PRECONDITIONED system.  MINRES / CG flavors, a
 * right preconditioner and ranks > 1 are refused.  Regular where J itself is singular (folds, branch points).             */
int bk_bls_matrixfree_pl(bk_ctx* ctx, bk_op* J, const double* dR, const double* dzu, double dzp,
                         const double* R, double n, double xiu, double xip, int has_shift,
                         double shift, double dotscale, const bk_gmres_opts* lsopts, bk_precond* pl,
                         double* dX, double* dl, int* converged, int* itlinear);
int bk_bls_block_matrixfree_pl(bk_ctx* ctx, bk_op* J, int m, const double* const* a, const double* const* b,
                               const double* c, const double* rhst, const double* rhsb, int has_shift,
                               double shift, double dotscale, const bk_gmres_opts* lsopts, bk_precond* pl,
                               double* u1, double* u2, int* converged, int* itlinear);
/* The per-application pass of that operator, exposed for exact tests: y[i] += sum_j coef[j] atil[j][i] in place (every product
 * and every sum rounded on its own, in j order) and dots[j] = <b[j], x> (deterministic two-stage sum, all-reduced), j < m <=
 * BK_MAX_BORDER, in ONE pass over y, x, the m atil and the m b: (3 + 2 m) 8 n bytes.  y must not alias another operand.   */
int bk_bordered_tail(bk_ctx* ctx, size_t n, int m, double* y, const double* x, const double* const* atil,
                     const double* const* b, const double* coef, double* dots);

/* ------------------------------------------------------------------ eigensolver ------------
 * (eig::ShiftInvert)(J, nev) -> (vals, vecs, converged, niter): src/EigSolver.jl:246-266 with a
 * Krylov-Schur (KrylovKit.eigsolve-style) outer iteration; the SH3dEig of examples/SH3d.jl:96-113.
 * Eigenvalues come back sorted by decreasing real part (__sort_spectrum, src/EigSolver.jl:16-19).
 * vals_re / vals_im hold nev + 1 entries: *nvals = nev, or nev + 1 when the cut would split a complex-conjugate
 * pair (as ARPACK / KrylovKit do); entries that did not converge to max(tol, sqrt(eps)|mu|) are NaN.
 * vecs (may be NULL) receives up to nev + 1 device vectors of local length, stride ldvecs, real parts of
 * the eigenvectors (imaginary parts in vecs_im when not NULL; symmetric problems: zero).        */
typedef struct {
    double sigma;      /* shift                                                                    */
    int krylovdim;     /* examples/SH3d.jl:109: max(30, nev+30)                                   */
    int maxiter;       /* restarts                                                                 */
    double tol;        /* Ritz residual tolerance                                                  */
    int hermitian;     /* ishermitian = true -> Lanczos-like symmetric Rayleigh quotient          */
    unsigned long long seed;   /* start vector: rand(N) in the reference (SH3d.jl:109)            */
} bk_eig_opts;
int bk_eig_shiftinvert(bk_ctx* ctx, bk_op* J, int nev, const bk_eig_opts* eopts,
                       const bk_gmres_opts* lsopts, bk_precond* pl, double* vals_re,
                       double* vals_im, double* vecs, double* vecs_im, size_t ldvecs, int* nvals,
                       int* nconv, int* numops);
/* Start vector of the NEXT bk_eig_shiftinvert / bk_eig_krylovkit call on this context (one-shot; NULL restores the
 * default rand(N) of examples/SH3d.jl:109): the x0 argument of KrylovKit.eigsolve, EigKrylovKit.x0 (src/EigSolver.jl:
 * 143,160).  x0 (device, local length) must stay valid until that call returns.                                    */
int bk_eig_set_start_vector(bk_ctx* ctx, const double* x0);
/* (eig::EigKrylovKit)(J, nev), which = :LR (src/EigSolver.jl:117-166): Krylov-Schur on J itself, rightmost eigenvalues,
 * no inner solves (sigma ignored); same output conventions as bk_eig_shiftinvert; *numops = operator applications.   */
int bk_eig_krylovkit(bk_ctx* ctx, bk_op* J, int nev, const bk_eig_opts* eopts, double* vals_re, double* vals_im,
                     double* vecs, double* vecs_im, size_t ldvecs, int* nvals, int* nconv, int* numops);

/* ------------------------------------------------------------------ Newton correctors ------ */
/* Newton callback, the reference's `callback(state; fromNewton, kwargs...) -> Bool` (src/Newton.jl:88,111-113,
 * src/continuation/Palc.jl:235,294-297; e.g. cbMaxNorm src/Newton.jl:156-159): called before the first iteration
 * (step = 0, itlinear = 0), after every iteration, and once more when the loop has ended (its value is AND-ed into
 * `converged`).  x / fx are device vectors of the current iterate and residual; p the current continuation parameter
 * (newton_palc) or NaN (_newton); z0u / z0p the previous point of the branch (newton_palc) or NULL / NaN.
 * Return 0 to stop the iteration (a veto), non-zero to go on.                                                        */
typedef int (*bk_newton_callback)(void* user, const double* x, const double* fx, double residual, int step,
                                  int itlinear, double p, const double* z0u, double z0p, int from_newton);
typedef struct {
    double tol;           /* NewtonPar.tol            src/Newton.jl:19                            */
    int max_iterations;   /* NewtonPar.max_iterations :21                                         */
    int norm_inf;         /* normN: 1 = norminf (examples/SH3d.jl:166), 0 = 2-norm                */
    /* the remaining fields may be left zero (= the reference defaults)                                              */
    int linesearch;       /* NewtonPar.linesearch (:27): Armijo-type damping in newton_palc, Palc.jl:254-281        */
    double alpha;         /* NewtonPar.alpha  (:29), <= 0 -> 1                                                       */
    double alpha_min;     /* NewtonPar.alphamin (:31), <= 0 -> 1e-3                                                  */
    double max_residual;  /* > 0: built-in cbMaxNorm(max_residual) veto (src/Newton.jl:156-159), no host round trip  */
    bk_newton_callback callback;   /* may be NULL                                                                    */
    void* callback_user;
} bk_newton_opts;
#define BK_MAX_NEWTON_ITER 64
typedef struct {
    int converged;
    int itnewton;
    int itlinear;                                /* itlineartot, src/Newton.jl:60                 */
    double residuals[BK_MAX_NEWTON_ITER + 1];    /* NonLinearSolution.residuals                   */
} bk_newton_result;
/* _newton, src/Newton.jl:66-114: x is the initial guess on entry, the solution on exit.         */
int bk_newton(bk_ctx* ctx, bk_problem* prob, double* x, const double* params, int nparams,
              const bk_newton_opts* nopts, const bk_gmres_opts* lsopts, bk_precond* pl,
              bk_newton_result* res);
/* newton_palc, src/continuation/Palc.jl:187-305 (linesearch = false) with BorderingBLS:
 * (x, *p) = predictor on entry, corrected point on exit; (z0u, z0p) last point, (tauu, taup)
 * tangent; the continuation parameter is params[ipar].                                          */
int bk_newton_palc(bk_ctx* ctx, bk_problem* prob, double* x, double* p, const double* z0u,
                   double z0p, const double* tauu, double taup, double ds, double theta,
                   const double* params, int nparams, int ipar, double p_min, double p_max,
                   const bk_newton_opts* nopts, const bk_bordering_opts* bopts,
                   const bk_gmres_opts* lsopts, bk_precond* pl, bk_newton_result* res);
/* The same corrector from a predictor x0 that is only read: x receives the corrected point (x0 itself when no iteration runs)
 * and must not overlap x0 unless x == x0, which is bk_newton_palc.  With BorderingBLS, check_precision off and no line search the
 * first iteration reads x0 and its update writes x, so the predictor is never copied (context option "palc_entry_copy" = 1, or
 * "palc_fuse_update" = 0: copy first and run in place; so do the line search, check_precision and MatrixFreeBLS).  Same results
 * bit for bit either way.                                                                                                      */
int bk_newton_palc_from(bk_ctx* ctx, bk_problem* prob, const double* x0, double* x, double* p,
                        const double* z0u, double z0p, const double* tauu, double taup, double ds,
                        double theta, const double* params, int nparams, int ipar, double p_min,
                        double p_max, const bk_newton_opts* nopts, const bk_bordering_opts* bopts,
                        const bk_gmres_opts* lsopts, bk_precond* pl, bk_newton_result* res);

/* ------------------------------------------------------------------ complex shifts (Hopf) ----------
 * The Hopf normal form and the minimally augmented Hopf system call the same plugin surface with a COMPLEX shift on
 * complex vectors and a real Jacobian: ls(L, rhs; a0 = Complex(0, 2w), a1 = -1) (src/NormalForms.jl:1053),
 * bls(J, a, b, 0, 0, 1; shift = Complex(0, -w)) (src/codim2/MinAugHopf.jl:17, 72-76).  Complex device vectors are
 * (re, im) pairs; *_im inputs may be NULL (= 0).  The solve runs on the real-equivalent 2N system with the real GMRES
 * (iteration counts can differ from a complex-arithmetic GMRES; same residual tolerance).  SURVEY section 8(f) item 3. */
int bk_gmres_cshift(bk_ctx* ctx, bk_op* J, const double* rhs_re, const double* rhs_im, double* x_re,
                    double* x_im, double a0_re, double a0_im, double a1, const bk_gmres_opts* opts,
                    bk_precond* pl, int* converged, int* niter, double* resnorm);
/* BorderingBLS, one BEC pass (check_precision = false), dotp(x, y) = dotscale * conj(x).y; dl[2] = (re, im).           */
int bk_bls_bordering_cshift(bk_ctx* ctx, bk_op* J, const double* dR_re, const double* dR_im,
                            const double* dzu_re, const double* dzu_im, double dzp_re, double dzp_im,
                            const double* R_re, const double* R_im, double n_re, double n_im, double xiu,
                            double xip, double shift_re, double shift_im, double dotscale,
                            const bk_gmres_opts* lsopts, bk_precond* pl, double* dX_re, double* dX_im,
                            double dl[2], int* converged, int itlinear[2]);
/* MatrixFreeBLS (src/LinearBorderSolver.jl:326-352, :424-437) for the same arguments with the solver's LEFT preconditioner carried
 * into the bordered system as diag(Pl, 1): the complex counterpart of bk_bls_matrixfree_pl.  ONE real GMRES on the real-equivalent
 * (2N + 2) system of
 *     out.u = Pl^-1 ((shift + J) x.u) + x.p (Pl^-1 dR) ,   out.p = dzp xip x.p + xiu dotscale dzu^H x.u
 * with the right-hand side (Pl^-1 R, n); Pl^-1 acts on each half, the shift sits under Pl^-1 in every GMRES flavor.  Regular where
 * shift + J is singular (the bordered systems of src/codim2/MinAugHopf.jl:17, 72-76 at a Hopf point).  One itlinear.  MINRES / CG
 * flavors, a right preconditioner, a missing pl, an odd local length and ranks > 1 are refused.                              */
int bk_bls_matrixfree_pl_cshift(bk_ctx* ctx, bk_op* J, const double* dR_re, const double* dR_im,
                                const double* dzu_re, const double* dzu_im, double dzp_re, double dzp_im,
                                const double* R_re, const double* R_im, double n_re, double n_im, double xiu,
                                double xip, double shift_re, double shift_im, double dotscale,
                                const bk_gmres_opts* lsopts, bk_precond* pl, double* dX_re, double* dX_im,
                                double dl[2], int* converged, int* itlinear);
/* The per-application pass of that operator, exposed for exact tests: on (re, im) pairs of length n, y += xi at in place with
 * xi = coef[0] + i coef[1] (every product and sum rounded on its own, y_re + xi_r at_re - xi_i at_im, y_im + xi_r at_im + xi_i at_re)
 * and dots = b^H x = (b_re.x_re + b_im.x_im, b_re.x_im - b_im.x_re) (four deterministic two-stage sums, one host read), in ONE pass:
 * eight read streams, two written, 80 n bytes.  y_re, y_im must not alias each other or another operand.                     */
int bk_cbordered_tail(bk_ctx* ctx, size_t n, double* y_re, double* y_im, const double* x_re, const double* x_im,
                      const double* at_re, const double* at_im, const double* b_re, const double* b_im,
                      const double coef[2], double dots[2]);

/* ------------------------------------------------------------------ continuation step -----------
 * The body of `iterate` (src/Continuation.jl:458-504) as one call: corrector! (newton_palc), compute_eigenvalues!
 * + is_stable (src/Utils.jl:67-104, src/Bifurcations.jl:5-19), _step_size_control! (src/continuation/Contbase.jl:77-102),
 * gettangent! (Secant / Bordered, src/continuation/Tangents.jl:28-104) and the predictor (addtangent!, :8-15).
 * bk_cont_create takes the two converged points of src/Continuation.jl:349-456 ((u0, p0) and (u1, p1 = p0 + ds/eta))
 * and performs initialize! (Palc.jl:112-123): secant tangent, first predictor and, with detect != 0, the eigenvalues
 * at (u0, p0) (returned in *init).  SURVEY section 8(f) item 2.                                                   */
#define BK_MAX_NEV 62
typedef struct {
    double ds, dsmin, dsmax;   /* ContinuationPar.ds / dsmin / dsmax   (src/ContParameters.jl)                      */
    double a;                  /* step-size aggressiveness ContinuationPar.a                                        */
    double theta;              /* PALC.theta                                                                         */
    double p_min, p_max;       /* ContinuationPar.p_min / p_max                                                      */
    int tangent;               /* 0: Secant(), 1: Bordered()                                                         */
    int detect;                /* detect_bifurcation > 0: eigenvalues after every converged step                    */
    int nev;                   /* ContinuationPar.nev                                                                */
    double tol_stability;      /* ContinuationPar.tol_stability                                                      */
} bk_cont_opts;
typedef struct {
    int converged, itnewton, itlinear;           /* corrector (NonLinearSolution)                                   */
    double residuals[BK_MAX_NEWTON_ITER + 1];
    double p;                                    /* parameter of the current point z after the step                  */
    double ds_used, ds_next;                     /* arclength step of this corrector / of the next predictor         */
    int step;                                    /* number of accepted steps so far                                  */
    int stop;                                    /* 0 continue, 1 |ds| <= dsmin after a failed corrector, 2 the previous point reached
                                                    the boundary of [p_min, p_max]: nothing was done (`done`, Continuation.jl:254) */
    int n_unstable, n_imag, bifurcation;         /* is_stable counts; bifurcation = 1 when n_unstable changed        */
    int nvals, eig_converged, eig_numops;        /* eigensolver return values; vals sorted by decreasing real part   */
    double vals_re[BK_MAX_NEV + 1], vals_im[BK_MAX_NEV + 1];
    int tangent_converged;                       /* Bordered(): convergence flag of the tangent's bordered solve     */
    int natural;                                 /* 1: the predictor left [p_min, p_max] and the step was corrected by the Natural
                                                    corrector at the clamped parameter (Palc.jl:157-160, Natural.jl:38-58)      */
} bk_cont_step_result;
typedef struct bk_cont bk_cont;
int bk_cont_create(bk_ctx* ctx, bk_problem* prob, const double* params, int nparams, int ipar,
                   const double* u0, double p0, const double* u1, double p1, const bk_cont_opts* copts,
                   const bk_newton_opts* nopts, const bk_bordering_opts* bopts, const bk_gmres_opts* lsopts,
                   bk_precond* pl, const bk_eig_opts* eopts, const bk_gmres_opts* eig_lsopts,
                   bk_precond* eig_pl, bk_cont_step_result* init, bk_cont** out);
int bk_cont_step(bk_cont* c, bk_cont_step_result* res);
/* copies of the current point / tangent (device buffers of the local length, any may be NULL) */
int bk_cont_get(bk_cont* c, double* u, double* p, double* tauu, double* taup, double* ds);
int bk_cont_destroy(bk_cont* c);
/* copy(state), src/Continuation.jl (ContState copies used by the bisection and by the engine's own bookkeeping)        */
int bk_cont_clone(bk_cont* src, bk_cont** out);
/* locate_bifurcation!(iter, state), src/Bifurcations.jl:159-349: call right after a bk_cont_step whose result has
 * bifurcation = 1.  Bisects with the continuation step itself (step-size control off, ds halved / reversed at every
 * crossing) until n_inversion crossings, max_bisection_steps steps or |ds| < dsmin_bisection; leaves the state next to the
 * bifurcation point with the predictor rebuilt.  status: 0 none, 1 guess, 2 converged, 3 guessL; type: 0 none, 1 bp,
 * 2 hopf, 3 nd (the codim-1 classification of _get_bifurcation_type, :80-130).                                        */
typedef struct {
    double dsmin_bisection;          /* ContinuationPar.dsmin_bisection           (1e-16)                             */
    int n_inversion;                 /* ContinuationPar.n_inversion               (2, must be even)                   */
    int max_bisection_steps;         /* ContinuationPar.max_bisection_steps       (25)                                */
    double tol_bisection_eigenvalue; /* ContinuationPar.tol_bisection_eigenvalue  (1e-16)                             */
    int max_steps;                   /* ContinuationPar.max_steps: `done` also bounds the bisection's own step counter */
} bk_bisection_opts;
typedef struct {
    int status, type;
    double interval[2];              /* parameter interval that contains the bifurcation point                        */
    double p;                        /* parameter of the state on return                                             */
    int n_unstable[2], n_imag[2];    /* (current, previous) pairs of the state on return                              */
    int steps;                       /* continuation steps spent                                                      */
    int nvals;                       /* eigenvalues of the state on return (`_state.eigvals = state.eigvals`, :341)   */
    double vals_re[BK_MAX_NEV + 1], vals_im[BK_MAX_NEV + 1];
} bk_bisection_result;
int bk_cont_locate_bifurcation(bk_cont* c, const bk_bisection_opts* opts, bk_bisection_result* res);

/* ------------------------------------------------------------------ deflated Newton --------------
 * solve(prob, defOp, options, DeflatedProblemCustomLS()) (src/DeflationOperator.jl:340-355): Newton on M(u) F(u) with
 * M(u) = prod_i ( <u - root_i, u - root_i>^-power + alpha ) (accumulator_mean != 0: the mean, Val(:Mean)), dM by finite
 * differences of step delta (:160-169), every linear solve = two solves with the plain Jacobian (ls(J, rhs, Fu)) and the
 * Sherman-Morrison style recombination of :264-312.  x: guess on entry, solution on exit.  SURVEY section 8(f) item 4. */
int bk_newton_deflated(bk_ctx* ctx, bk_problem* prob, double* x, const double* params, int nparams,
                       const double* const* roots, int nroots, double power, double alpha,
                       int accumulator_mean, double delta, const bk_newton_opts* nopts,
                       const bk_gmres_opts* lsopts, bk_precond* pl, bk_newton_result* res);

/* ------------------------------------------------------------------ deflation with the exact derivative ---
 * DeflationOperator(power, dot, alpha, roots; autodiff = true) (src/DeflationOperator.jl:61-169), as multicontinuation uses it
 * for 9 to 27 deflated states (src/bifdiagram/BranchSwitching.jl:325,339).  With t_i = u - root_i, d_i = <t_i, t_i>,
 * e_i = <t_i, h> and m_i = d_i^-power + alpha:
 *   M(u) = prod_i m_i,          dM(u) . h = sum_i (prod_{j != i} m_j) (-2 power d_i^(-power - 1)) e_i        (Val(:Prod), :124-138)
 *   M(u) = (sum_i m_i) / k,     dM(u) . h = (sum_i (-2 power d_i^(-power - 1)) e_i) / k                      (Val(:Mean))
 * which is what :159-169 differentiates.                                                                                       */
/* One streaming pass per 8 roots over u, h and the roots (1 + 1 + 8 streams) that writes nothing: host d[nroots] and
 * e[nroots].  h == NULL (then e == NULL too): the d_i alone; the d_i are the same sums bit for bit with and without h.  A root
 * equal to u gives d_i = 0 exactly.  Deterministic, all-reduced.                                                               */
int bk_deflation_dots(bk_ctx* ctx, size_t n, const double* u, const double* h /* may be NULL */,
                      const double* const* roots, int nroots, double* d, double* e /* NULL iff h is */);
typedef struct {
    int converged;
    int itnewton;
    int itlinear;                                /* one solve per Newton step                                         */
    double residuals[BK_MAX_NEWTON_ITER + 1];    /* of the quantity stopped on: |M F| or |F|                          */
    double M;                                    /* M at the final x                                                  */
    double min_dist;                             /* min_i sqrt(d_i) at the final x, +inf without roots                */
} bk_deflated_result;
/* _newton (src/Newton.jl:66-114) on M(u) F(u) with the exact dM and ONE linear solve per step.  DeflatedProblemCustomLS
 * (src/DeflationOperator.jl:264-312) solves h1 = J^-1 (M F) and h2 = J^-1 F and steps by h = (h1 - z h2) / M,
 * z = dM.h1 / (M + dM.h2); h1 = M h2 by linearity, so with e = dM(u) . h2 the same step is x <- x - M / (M + e) h2
 * (Sherman-Morrison on M J + F grad M').  Per step: one GMRES solve and one pass of bk_deflation_dots with h = h2; the residual
 * evaluation runs the pass without h and its d_i serve the next step.
 * stop_plain == 0: stop on |M F| = |M| |F| < tol, the reference's rule (:340-355); != 0: stop on |F| < tol, which follows from
 * the former whenever alpha >= 1 and does not ask |F| to fall below tol / M (~ tol 1e-5 with several roots 0.2 - 0.4 away).
 * The norm is nopts->norm_inf ? inf : 2; nopts' callback and max_residual are not consulted.
 * A root with d_i = 0 (x on a deflated state) makes M infinite: converged = 0, no error.  x == roots[i] (aliased) is refused with
 * a message.  nroots == 0 is plain Newton.                                                                                     */
int bk_newton_deflated_exact(bk_ctx* ctx, bk_problem* prob, double* x, const double* params, int nparams,
                             const double* const* roots, int nroots, double power, double alpha,
                             int accumulator_mean, int stop_plain, const bk_newton_opts* nopts,
                             const bk_gmres_opts* lsopts, bk_precond* pl, bk_deflated_result* res);

/* ------------------------------------------------------------------ deflated continuation ---------------
 * continuation(prob, DefCont(...), contParams) (src/DeflatedContinuation.jl:196-356; examples/SH2d-fronts.jl:168-181): the loop over
 * steps and branches is host logic (bk_amd.deflated_continuation); these are its device parts.                                     */
/* The normC(u - root) of the acceptance tests (:282, :334) for normC = norm and normC = norminf from ONE streaming pass per 8 roots
 * over u and the roots (1 + 8 streams) that writes nothing: host d2[i] = sum (u - root_i)^2 and dinf[i] = max |u - root_i|.  d2[i] is
 * the d[i] of bk_deflation_dots for the same operands bit for bit (same items per lane, same element order, same two stages).  A NaN
 * in u - root_i makes dinf[i] NaN (norminf, src/LinearSolver.jl:4); a root equal to u gives exactly 0 in both.  Deterministic,
 * all-reduced (sum, max).  nroots == 0 does nothing.                                                                                */
int bk_deflation_dist(bk_ctx* ctx, size_t n, const double* u, const double* const* roots, int nroots, double* d2, double* dinf);
/* perturb_solution of the example, x .+ amp .* rand(length(x)) (examples/SH2d-fronts.jl:181; DefCont.perturb_solution,
 * src/DeflatedContinuation.jl:26, :272), in place with a counter-based uniform: x[i] += amp U(seed, index0 + i), where for the GLOBAL
 * index g, in wrapping 64-bit arithmetic,
 *   z = seed + (g + 1) 0x9E3779B97F4A7C15;  z = (z ^ z >> 30) 0xBF58476D1CE4E5B9;  z = (z ^ z >> 27) 0x94D049BB133111EB;
 *   z ^= z >> 31;  U = (z >> 11) 2^-53 in [0, 1).
 * The product and the sum are rounded one after the other (no fused multiply-add).  The result depends on (seed, g) alone -- not on
 * the grid, the alignment or the load path -- so a rank passes index0 = slab_lo x plane size (bk_problem_nlocal) and the pieces equal
 * the unsplit vector.  Reads and writes x once: 16 n bytes.  n == 0 does nothing.                                                   */
int bk_vec_perturb(bk_ctx* ctx, size_t n, double* x, double amp, unsigned long long seed, unsigned long long index0);
typedef struct {
    int converged;               /* of the deflated Newton                                                             */
    int itnewton;
    int itlinear;                /* one solve per Newton step                                                          */
    int accepted;                /* reason == 0                                                                        */
    int reason;                  /* 0 accepted, 1 Newton not converged, 2 plain residual >= tol, 3 a known root within tol */
    int itnewton_total;          /* entries of the residual history, itnewton + 1; the caller's buffer holds the last
                                    min(residuals_cap, itnewton_total) of them, oldest first                           */
    double M;                    /* M at the final x                                                                   */
    double min_dist;             /* min_i sqrt(d_i) at the final x as the Newton saw it, +inf without roots            */
    double plain_residual;       /* normC(F(x)) at the final x, from the Newton's last evaluation of F                 */
    double min_dist_normC;       /* min_i normC(x - root_i) from bk_deflation_dist, +inf without roots                 */
} bk_defcont_seek_result;
/* _DC_get_new_solution (src/DeflatedContinuation.jl:269-286) and the duplicate test of :334 as one call: the Newton of
 * bk_newton_deflated_exact (the same loop) from the already perturbed guess x with an open iteration count -- the seek runs
 * max_iter_defop x newton.max_iterations iterations (:223), so the residual history goes to the caller's buffer of residuals_cap >= 1
 * doubles -- and then, in the reference's order: the Newton converged (:274); the plain residual normC(F(x)) < tol (:281), taken from
 * the last evaluation of F; min_i normC(x - root_i) >= tol (:282; :334 when the state sought from is among the roots, where the
 * driver keeps it) from one pass of bk_deflation_dist.  normC is norm_inf ? norminf : norm, for the Newton and for the tests.
 * stop_plain as in bk_newton_deflated_exact.  A root with d_i = 0 (x on a deflated state) makes M infinite: reason 1, no error.
 * x == roots[i] (aliased) is refused with a message.  nroots == 0 is plain Newton.                                                  */
int bk_defcont_seek(bk_ctx* ctx, bk_problem* prob, double* x, const double* params, int nparams,
                    const double* const* roots, int nroots, double power, double alpha, int accumulator_mean,
                    int stop_plain, int norm_inf, double tol, int max_iterations, const bk_gmres_opts* lsopts,
                    bk_precond* pl, double* residuals, int residuals_cap, bk_defcont_seek_result* res);

/* ------------------------------------------------------------------ fold points (codim 2) ---------------
 * The minimally augmented fold formulation of src/codim2/MinAugFold.jl, matrix-free (the reference assembles it for MatrixBLS /
 * MinAugMatrixBased): unknowns (x, p = params[ipar]), G(x, p) = (F(x, p), sigma(x, p)) with sigma from
 * [J a; b' 0][v; sigma] = [0; 1] and the adjoint system [J' b; a' 0][w; sigma2] = [0; 1].  Defined for BK_PDE_SH (2-D / 3-D)
 * and BK_PDE_SH1D, whose Jacobians are symmetric (J' = J, :79-84) and whose Hessians are pointwise; any other problem returns
 * an error.  The Newton solve is only as good as the linear solver on the near-singular J: it is demonstrated for SH with the
 * spectral preconditioner; SH1D has no preconditioner here, and unpreconditioned GMRES does not converge on its J (N = 200).
 * Vectors have the problem's local length (ranks: z-slabs); the scalars come from the all-reduced reductions of the BLAS-1 and
 * contraction kernels (not yet exercised on more than one rank).                                                           */
/* out = d2F(u, params)[dx1, dx2] (src/Problems.jl:107,165): SH (2 nu - 6 u) dx1 dx2 (examples/SH2d-fronts.jl:40), SH1D
 * (6 nu u - 20 u^3) dx1 dx2 (examples/SHpde_snaking.jl:26); pointwise, no halo.                                       */
int bk_d2f(bk_problem* prob, const double* u, const double* params, int nparams, const double* dx1, const double* dx2,
           double* out);
/* out = dJ/dp(u) dx for params[ipar]: J depends on the parameter only through the pointwise term, factor SH l: 1, nu: 2u;
 * SH1D lambda: 1, nu: 3u^2 -- the analytic value of the central difference dJvdp of _get_bordered_terms (MinAugFold.jl:93-94). */
int bk_djdp(bk_problem* prob, const double* u, const double* params, int nparams, int ipar, const double* dx, double* out);
/* One streaming pass over u, v, w and m <= 3 device vectors X[k]:  out[k] = <w, d2F(u)[v, X_k]>  (k < m),
 * out[m] = -<w, dJ/dp(u) v> = sigma_p for params[ipar]  (the inner products of foldMALinearSolver, MinAugFold.jl:153-157,
 * and of _get_bordered_terms, :95).  Host out[m + 1]; deterministic, all-reduced.                                    */
int bk_fold_contract(bk_problem* prob, const double* u, const double* params, int nparams, int ipar, const double* v,
                     const double* w, int m, const double* const* X, double* out);
/* _compute_bordered_vectors + the sigma_p of _get_bordered_terms (MinAugFold.jl:54-99) at (x, params): v and sigma from the
 * BorderingBLS solve bls(J, a, b, 0, 0, 1) (bopts / lsopts / pl as bk_bls_bordering), w from bls(J', b, a, 0, 0, 1) -- or
 * w = v with no second solve when a and b are the SAME pointer (newton_fold(br, ind) passes one vector twice, :246-247).
 * sigma_p (may be NULL) = -<w, dJ/dp v> for params[ipar].  itlinear[0] / [1]: GMRES counts of the v / w solves.        */
int bk_fold_terms(bk_ctx* ctx, bk_problem* prob, const double* x, const double* params, int nparams, int ipar,
                  const double* a, const double* b, const bk_bordering_opts* bopts, const bk_gmres_opts* lsopts,
                  bk_precond* pl, double* v, double* w, double* sigma, double* sigma_p, int* converged, int itlinear[2]);
/* foldMALinearSolver, usehessian branch (MinAugFold.jl:119-166) for nrhs = 1 or 2 right-hand sides (rhsu[k] device, rhsp[k]
 * host) at (x, params) with the bordered vectors v, w of that point: x1_k = J \ rhsu_k, ONE x2 = J \ dpF shared by all
 * right-hand sides (dpF analytic), dsigma_k = (rhsp_k - sx1_k) / (sigma_p - sx2) with sx = -<w, d2F[., v]> from one fused pass,
 * dX_k = x1_k - dsigma_k x2.  nrhs + 1 GMRES solves (the reference: 2 nrhs).  *itlinear = their GMRES counts.             */
int bk_fold_linsolve(bk_ctx* ctx, bk_problem* prob, const double* x, const double* params, int nparams, int ipar,
                     const double* v, const double* w, int nrhs, const double* const* rhsu, const double* rhsp,
                     const bk_gmres_opts* lsopts, bk_precond* pl, double* const* dX, double* dsigma, int* converged,
                     int* itlinear);
/* newton_fold (MinAugFold.jl:211-233) under the semantics of _newton (src/Newton.jl:66-114): (x, *p) = guess on entry, fold
 * point on exit; tol applies to |(F, sigma)| in the chosen norm (norm_inf: max(|F|_inf, |sigma|), else the 2-norm of the
 * BorderedArray); callback as bk_newton (p = the fold parameter, z0u = NULL).  Each point's v and w are solved ONCE and serve
 * both its residual sigma and the Newton step taken from it (the reference solves them again for the Jacobian).  On exit
 * v, w, *sigma are those of the returned point; res->itlinear = every GMRES count run (bordered vectors and steps).
 * As in _newton the linear solves' convergence flags do not enter res->converged; each unconverged bordered-vector or step
 * solve adds 1 to the context counter "fold_unconverged_solves" (bk_ctx_get_option; reset with bk_ctx_set_option(.., 0)). */
int bk_newton_fold(bk_ctx* ctx, bk_problem* prob, double* x, double* p, const double* params, int nparams, int ipar,
                   const double* a, const double* b, const bk_newton_opts* nopts, const bk_bordering_opts* bopts,
                   const bk_gmres_opts* lsopts, bk_precond* pl, double* v, double* w, double* sigma,
                   bk_newton_result* res);
/* The border row of the full fold Jacobian as a vector (MinAugFold.jl:136-145, the branch without `usehessian`):
 * sigx[i] = -w[i] h(u[i]) v[i] with h the pointwise Hessian factor of bk_d2f, so that <sigx, X> = -<w, d2F(u)[v, X]> for every
 * X; one streaming pass, sigx must not alias u, v or w.  sigma_p (may be NULL) = -<w, dJ/dp v> for params[ipar] as
 * bk_fold_contract returns it.
 * Context option "fold_bordered" (default 0, read once per call by bk_fold_terms, bk_fold_linsolve and bk_newton_fold; no option
 * struct changes).  At 1 the formulation runs on the system that is REGULAR at the fold instead of on J \ a, J \ F, J \ dpF
 * ("Careful, this method makes the linear system singular", :149):
 *   bk_fold_terms     (v, sigma) from ONE solve [J a; b' 0][v; sigma] = [0; 1] with bk_bls_matrixfree_pl (w: the adjoint system
 *                     the same way, or w = v for a == b); bopts is not read; itlinear[0] / [1] = the two GMRES counts;
 *   bk_fold_linsolve  [J dpF; sigx' sigma_p][dX_k; dsigma_k] = [rhsu_k; rhsp_k], one such solve per right-hand side, all
 *                     sharing Pl^-1 dpF;
 *   bk_newton_fold    runs on both; "fold_unconverged_solves" counts as before.
 * pl must be given (the bordered operator is preconditioned by diag(Pl, 1)).                                               */
int bk_fold_border(bk_problem* prob, const double* u, const double* params, int nparams, int ipar, const double* v,
                   const double* w, double* sigx, double* sigma_p);

/* ------------------------------------------------------------------ Hopf points (codim 2) ---------------
 * The minimally augmented Hopf formulation of src/codim2/MinAugHopf.jl, matrix-free: unknowns (x, p = params[ipar], omega),
 * G = (F(x, p), Re sigma, Im sigma) with sigma from [J - i omega, a; b^H, 0][v; sigma] = [0; 1] and w from the adjoint system
 * [J' + i omega, b; a^H, 0][w; sigma2] = [0; 1].  With w^H a = 1: sigma_x . dx = -w^H d2F[v, dx], sigma_p = -w^H dJ/dp v,
 * sigma_omega = i w^H v.  Defined for BK_PDE_CGL2D only (its nonlinearity is pointwise with an analytic Hessian); any other
 * problem returns an error.  Complex device vectors are (re, im) pairs of real vectors of the problem's local length; an *_im
 * input may be NULL (= 0) where noted.  J is regular at a Hopf point, so the real solves J \ . need no bordering.          */
/* out = d2F(u, params)[dx1, dx2] for real dx1, dx2: per grid point the symmetric 2 x 2 Hessians of the cGL nonlinearity
 * (examples/cGL2d.jl:24-40); complex arguments by linearity.                                                            */
int bk_hopf_d2f(bk_problem* prob, const double* u, const double* params, int nparams, const double* dx1, const double* dx2,
                double* out);
/* out = dJ/dp(u) dx for params[ipar] = (r, mu, nu, c3, c5, gamma): the u-derivative of the pointwise dF/dp (zero for gamma). */
int bk_hopf_djdp(bk_problem* prob, const double* u, const double* params, int nparams, int ipar, const double* dx, double* out);
/* One streaming pass over u, v, w and m <= 3 real device vectors X[k]: host out[2 (m + 2)] = (re, im) pairs of
 * S_k = w^H d2F(u)[v, X_k] (k < m), P = w^H dJ/dp(u) v for params[ipar], Q = w^H v.  Deterministic, all-reduced.           */
int bk_hopf_contract(bk_problem* prob, const double* u, const double* params, int nparams, int ipar, const double* v_re,
                     const double* v_im, const double* w_re, const double* w_im, int m, const double* const* X, double* out);
/* _compute_bordered_vectors + _get_bordered_terms (MinAugHopf.jl) at (x, params, omega): v, sigma from
 * bk_bls_bordering_cshift(J, a, b, 0, 0, 1; shift = -i omega), w from the same on the adjoint handle with a and b exchanged and
 * shift = +i omega (a_im, b_im may be NULL).  sigma[2], and (each may be NULL) sigma_p[2] = -w^H dJ/dp v and
 * sigma_omega[2] = i w^H v.  itlinear[0] / [1]: GMRES counts of the v / w solves.
 * Context option "hopf_bordered" (default 0, read once per call by bk_hopf_terms, bk_newton_hopf and bk_bautin_normal_form; no
 * option struct changes).  J - i omega is singular at a Hopf point, where the two shifted solves of each BEC pass stop unconverged.
 * At 1, (v, sigma) and w each come from ONE solve of their bordered system, which is regular there, with
 * bk_bls_matrixfree_pl_cshift (pl must be given); itlinear[0] / [1] = the two GMRES counts, "hopf_unconverged_solves" counts as
 * before.  The Newton step (bk_hopf_linsolve) stays by elimination: J itself is regular at a Hopf point, and the reference
 * eliminates there too (MinAugHopf.jl:160-197).  The H21 solve of bk_bautin_normal_form goes the same way.                  */
int bk_hopf_terms(bk_ctx* ctx, bk_problem* prob, const double* x, const double* params, int nparams, int ipar, double omega,
                  const double* a_re, const double* a_im, const double* b_re, const double* b_im, const bk_gmres_opts* lsopts,
                  bk_precond* pl, double* v_re, double* v_im, double* w_re, double* w_im, double sigma[2], double sigma_p[2],
                  double sigma_omega[2], int* converged, int itlinear[2]);
/* _hopf_MA_linear_solver, usehessian branch, for nrhs = 1 or 2 right-hand sides (rhsu[k] device, host rhspw[2k], rhspw[2k+1]
 * = the p and omega rows) with the bordered vectors v, w of (x, params): x1_k = J \ rhsu_k, ONE x2 = J \ dpF shared by all
 * right-hand sides (dpF analytic), (dp_k, domega_k) from the complex equation
 * (sigma_p - sigma_x.x2) dp + sigma_omega domega = (rhsp + i rhsomega) - sigma_x.x1 as a 2 x 2 real system, dX_k = x1_k - dp_k x2.
 * Host dpw[2k], dpw[2k+1] = (dp_k, domega_k).  nrhs + 1 real GMRES solves (the reference: 2 nrhs).                        */
int bk_hopf_linsolve(bk_ctx* ctx, bk_problem* prob, const double* x, const double* params, int nparams, int ipar,
                     const double* v_re, const double* v_im, const double* w_re, const double* w_im, int nrhs,
                     const double* const* rhsu, const double* rhspw, const bk_gmres_opts* lsopts, bk_precond* pl,
                     double* const* dX, double* dpw, int* converged, int* itlinear);
/* newton_hopf under the semantics of _newton (src/Newton.jl:66-114), as bk_newton_fold: (x, *p, *omega) = guess on entry, Hopf
 * point on exit; tol applies to BorderedArray(F, [Re sigma, Im sigma]) in the chosen norm; callback as bk_newton (p = the
 * Hopf parameter).  Each point's v and w are solved once and serve its residual and its Newton step.  On exit v, w and sigma
 * are those of the returned point.  Each unconverged bordered-vector or step solve adds 1 to the context counter
 * "hopf_unconverged_solves".                                                                                            */
int bk_newton_hopf(bk_ctx* ctx, bk_problem* prob, double* x, double* p, double* omega, const double* params, int nparams,
                   int ipar, const double* a_re, const double* a_im, const double* b_re, const double* b_im,
                   const bk_newton_opts* nopts, const bk_gmres_opts* lsopts, bk_precond* pl, double* v_re, double* v_im,
                   double* w_re, double* w_im, double sigma[2], bk_newton_result* res);

/* ------------------------------------------------------------------ Hopf normal form ---------------------
 * __hopf_normal_form (src/NormalForms.jl:1009-1076) and the orbit of predictor(::Hopf, ds) (:1227-1281), matrix-free, for
 * BK_PDE_CGL2D (any other problem: the error of the Hopf entries above).  At a Hopf point (x, params, omega) with zeta the
 * eigenvector of J for i omega and zeta* that of J' for -i omega -- the v and w bk_newton_hopf returns, scaled to |zeta| = 1 and
 * <zeta, zeta*> = 1 with inner(x, y) = sum conj(x) y -- the coefficients of z' = z (i omega + a dp + b |z|^2) are
 *   a = < dJ/dp zeta + d2F[zeta, Psi001], zeta* >,
 *   b = < d2F[zeta, Psi110] + d2F[conj zeta, Psi200] + d3F[zeta, zeta, conj zeta] / 2, zeta* >,
 *   Psi001 = -J \ dpF,  Psi110 = -J \ d2F[zeta, conj zeta],  Psi200 = (2 i omega - J) \ (d2F[zeta, zeta] / 2).
 * dpF and dJ/dp are analytic where the reference differentiates (:1032-1047).  Complex vectors are (re, im) pairs.          */
/* out = d3F(u, params)[dx1, dx2, dx3] for real arguments (the d3F of R3, :1029): per grid point and field the symmetric
 * 2 x 2 x 2 third derivative of the cGL nonlinearity (examples/cGL2d.jl:24-40); complex arguments by linearity.           */
int bk_hopf_d3f(bk_problem* prob, const double* u, const double* params, int nparams, const double* dx1, const double* dx2,
                const double* dx3, double* out);
/* One pass over u and zeta: (r20_re, r20_im) = d2F[zeta, zeta] / 2 = R2(zeta, zeta) (:1052) and r11 = d2F[zeta, conj zeta]
 * = 2 R2(zeta, conj zeta) (:1057; real).  The outputs are distinct and alias no input.                                     */
int bk_hopf_nf_rhs(bk_problem* prob, const double* u, const double* params, int nparams, const double* z_re, const double* z_im,
                   double* r20_re, double* r20_im, double* r11);
/* One streaming pass over u, zeta, zeta*, Psi001, Psi110 and Psi200: host out[4] = (Re a, Im a, Re b, Im b), the two inner
 * products of :1049 and :1063 for params[ipar].  Deterministic, all-reduced.                                              */
int bk_hopf_nf_contract(bk_problem* prob, const double* u, const double* params, int nparams, int ipar, const double* z_re,
                        const double* z_im, const double* zs_re, const double* zs_im, const double* psi001, const double* psi110,
                        const double* psi200_re, const double* psi200_im, double out[4]);
/* The whole of __hopf_normal_form (:1009-1076) at (x, params, omega) for params[ipar]: analytic dpF, the pass of
 * bk_hopf_nf_rhs, the two real solves as one two-lane pair (as bk_gmres2), the shifted solve (bk_gmres_cshift with
 * a0 = 2 i omega, a1 = -1, :1053) and the pass of bk_hopf_nf_contract.  zeta and zeta* come normalised; unless
 * |<zeta, zeta*> - 1| <= 1e-8 the call is an error (:1186-1189).  ab[4] = (Re a, Im a, Re b, Im b); the four Psi vectors are
 * outputs, distinct from each other and from the inputs.  *converged = all three solves converged; itlinear[3] = GMRES counts
 * of the Psi001, Psi110 and Psi200 solves.  An unconverged solve is no error (the reference logs it, :1039): each adds 1 to the
 * context counter "hopf_nf_unconverged_solves".                                                                            */
int bk_hopf_normal_form(bk_ctx* ctx, bk_problem* prob, const double* x, const double* params, int nparams, int ipar, double omega,
                        const double* z_re, const double* z_im, const double* zs_re, const double* zs_im,
                        const bk_gmres_opts* lsopts, bk_precond* pl, double* psi001, double* psi110, double* psi200_re,
                        double* psi200_im, double ab[4], int* converged, int itlinear[3]);
/* The orbit of predictor(::Hopf, ds) (:1262-1271) at the M phases t[0..M) (host): device vectors of length n
 *   out[m] = x0 + 2 Re(zeta A_m) + ds Psi001 + |A_m|^2 Psi110 + 2 Re(A_m^2 Psi200),   A_m = amp e^{i t[m]},
 * up to eight phases per pass over the seven inputs.  The outputs are distinct and alias no input.                         */
int bk_hopf_orbit(bk_ctx* ctx, size_t n, const double* x0, const double* z_re, const double* z_im, const double* psi001,
                  const double* psi110, const double* psi200_re, const double* psi200_im, double ds, double amp, int M,
                  const double* t, double* const* out);

/* ------------------------------------------------------------------ Bautin normal form -------------------
 * bautin_normal_form (src/codim2/NormalForms.jl:642-829, detailed = false), matrix-free, for BK_PDE_CGL2D (any other problem:
 * the error of the Hopf entries above).  At a Hopf point (x, params, omega) with q = zeta, p0 = zeta*, <zeta, zeta*> = 1,
 * dot(p0, h) = sum conj(p0) h and B, C, D, E the 2nd .. 5th derivatives of the right-hand side at x:
 *   H20 = (2 i omega - J) \ B(q, q) = 2 Psi200,  H11 = -J \ B(q, conj q) = Psi110,  G21 = 2 conj(b)   (bk_hopf_normal_form)
 *   H30 = (3 i omega - J) \ (C(q, q, q) + 3 B(q, H20))
 *   H21 : [J - i omega, q; p0^H, 0][H21; s] = [G21 q - (C(q, q, conj q) + B(conj q, H20) + 2 B(q, H11)); 0]
 *   H31 = (2 i omega - J) \ (D(q, q, q, conj q) + 3 C(q, q, H11) + 3 C(q, conj q, H20) + 3 B(H20, H11) + B(conj q, H30)
 *                            + 3 B(q, H21) - 3 G21 H20)
 *   H22 = -J \ (D(q, q, conj q, conj q) + 4 C(q, conj q, H11) + C(conj q, conj q, H20) + C(q, q, conj H20) + 2 B(H11, H11)
 *               + 2 B(q, conj H21) + 2 B(conj q, H21) + B(conj H20, H20) - 4 Re(G21) H11)               (real)
 *   G32 = dot(p0, E(q, q, q, conj q, conj q) + D(q, q, q, conj H20) + 3 D(q, conj q, conj q, H20) + 6 D(q, q, conj q, H11)
 *                 + C(conj q, conj q, H30) + 3 C(q, q, conj H21) + 6 C(q, conj q, H21) + 3 C(q, conj H20, H20)
 *                 + 6 C(q, H11, H11) + 6 C(conj q, H20, H11) + 2 B(conj q, H31) + 3 B(q, H22) + B(conj H20, H30)
 *                 + 3 B(conj H21, H20) + 6 B(H11, H21)),        l2 = Re G32 / 12  (the second Lyapunov coefficient).
 * D and E are analytic (only the quintic term of cGL contributes) where the reference nests central differences of d3F
 * (:757-794).  Complex vectors are (re, im) pairs; H11 and H22 are real.                                                   */
/* One pass over u, q, H20, H11: (h30_re, h30_im) = C(q, q, q) + 3 B(q, H20) and (h21_re, h21_im) = G21 q - (C(q, q, conj q) +
 * B(conj q, H20) + 2 B(q, H11)) with the host scalar g21 = (Re G21, Im G21).  The outputs are distinct and alias no input.  */
int bk_bautin_rhs3(bk_problem* prob, const double* u, const double* params, int nparams, const double* q_re, const double* q_im,
                   const double* h20_re, const double* h20_im, const double* h11, const double g21[2], double* h30_re,
                   double* h30_im, double* h21_re, double* h21_im);
/* One pass over u, q, H20, H11, H30, H21: (h31_re, h31_im) and the real h22, the right-hand sides of the H31 and H22 solves
 * above (h22 before the sign: H22 = -J \ h22).  The outputs are distinct and alias no input.                              */
int bk_bautin_rhs4(bk_problem* prob, const double* u, const double* params, int nparams, const double* q_re, const double* q_im,
                   const double* h20_re, const double* h20_im, const double* h11, const double* h30_re, const double* h30_im,
                   const double* h21_re, const double* h21_im, const double g21[2], double* h31_re, double* h31_im, double* h22);
/* One streaming pass over the fifteen vectors u, q, p0, H20, H11, H30, H21, H31, H22: host out[2] = (Re G32, Im G32).
 * Deterministic, all-reduced.                                                                                             */
int bk_bautin_contract(bk_problem* prob, const double* u, const double* params, int nparams, const double* q_re, const double* q_im,
                       const double* p_re, const double* p_im, const double* h20_re, const double* h20_im, const double* h11,
                       const double* h30_re, const double* h30_im, const double* h21_re, const double* h21_im,
                       const double* h31_re, const double* h31_im, const double* h22, double out[2]);
/* The whole computation at (x, params, omega) from the outputs of bk_hopf_normal_form at the same point (psi110, psi200 and
 * ab[4] = (Re a, Im a, Re b, Im b); none is modified): the pass of bk_bautin_rhs3, H30 by bk_gmres_cshift (a0 = 3 i omega,
 * a1 = -1), H21 by bk_bls_bordering_cshift(J, q, p0, 0, h21, 0; shift = -i omega), the pass of bk_bautin_rhs4, H31 by
 * bk_gmres_cshift (a0 = 2 i omega, a1 = -1), H22 by the real solve, negated, and the pass of bk_bautin_contract.
 * g[5] = (Re G21, Im G21, Re G32, Im G32, l2).  The four H vectors (seven real arrays) are outputs, distinct from each other and from the inputs.
 * zeta and zeta* come normalised; unless |<zeta, zeta*> - 1| <= 1e-8 the call is an error.  *converged = all four solves
 * converged; itlinear[4] = GMRES counts of the H30, H21 (both solves of the bordering), H31 and H22 solves.  J - i omega is
 * singular at a Hopf point by construction, so an unconverged solve is no error: each adds 1 to the context counter
 * "bautin_unconverged_solves".                                                                                            */
int bk_bautin_normal_form(bk_ctx* ctx, bk_problem* prob, const double* x, const double* params, int nparams, double omega,
                          const double* z_re, const double* z_im, const double* zs_re, const double* zs_im, const double* psi110,
                          const double* psi200_re, const double* psi200_im, const double ab[4], const bk_gmres_opts* lsopts,
                          bk_precond* pl, double* h30_re, double* h30_im, double* h21_re, double* h21_im, double* h31_re,
                          double* h31_im, double* h22, double g[5], int* converged, int itlinear[4]);

/* ------------------------------------------------------------------ normal form, 1-D kernel -------------
 * get_normal_form1d (src/NormalForms.jl:189-353) and the vectors of its predictors (:389-531), matrix-free, for BK_PDE_SH
 * (2-D / 3-D) and BK_PDE_SH1D (any other problem: the error of the fold entries above).  At a simple branch point or fold
 * (x, params) with the kernel vector zeta of J and zeta* of J' = J, |zeta| = 1 and <zeta, zeta*> = 1 (zeta* = zeta /
 * <zeta, zeta> in the is_symmetric branch, :261-263; the two pointers may be equal), E(r) = r - <r, zeta*> zeta:
 *   a01 = <dpF, zeta*>,  b11 = <dJ/dp zeta + d2F[zeta, Psi01], zeta*>,  a02 = <2 dJ/dp Psi01 + d2F[Psi01, Psi01], zeta*>,
 *   b20 = <d2F[zeta, zeta], zeta*>,  b30 = <d3F[zeta, zeta, zeta] + 3 d2F[zeta, Psi20], zeta*>,
 *   [J zeta*; zeta' 0][Psi01; s] = [E(-dpF); 0],   [J zeta*; zeta' 0][Psi20; s] = [E(-d2F[zeta, zeta]); 0]   (:299-336)
 * in a01 dp + a02 dp^2 / 2 + b11 x dp + b20 x^2 / 2 + b30 x^3 / 6.  dpF, dJ/dp, d2F and d3F are pointwise and analytic and
 * d2F/dp2 = 0, where the reference uses ForwardDiff or central differences (:289-321).                                    */
/* out = d3F(u, params)[dx1, dx2, dx3] (the R3 of :283): SH -6 dx1 dx2 dx3, SH1D (6 nu - 60 u^2) dx1 dx2 dx3; pointwise.   */
int bk_d3f(bk_problem* prob, const double* u, const double* params, int nparams, const double* dx1, const double* dx2,
           const double* dx3, double* out);
/* One streaming pass over u, zeta, zeta* that writes nothing: host out[3] = (a01, b20, <zeta, zeta*>) for params[ipar]
 * (:299, :329, :275).  Deterministic, all-reduced.                                                                         */
int bk_nf1d_dots(bk_problem* prob, const double* u, const double* params, int nparams, int ipar, const double* zeta,
                 const double* zeta_star, double out[3]);
/* One pass over u and zeta: the projected right-hand sides r01 = E(-dpF) = a01 zeta - dpF and r20 = E(-d2F[zeta, zeta]) =
 * b20 zeta - d2F[zeta, zeta] of the two bordered solves (:303, :333) with the a01, b20 of bk_nf1d_dots.  The outputs are
 * distinct and alias no input.                                                                                              */
int bk_nf1d_rhs(bk_problem* prob, const double* u, const double* params, int nparams, int ipar, const double* zeta, double a01,
                double b20, double* r01, double* r20);
/* One streaming pass over u, zeta, zeta*, Psi01, Psi20: host out[3] = (b11, a02, b30) for params[ipar] (:313, :323, :336).
 * Deterministic, all-reduced.                                                                                                */
int bk_nf1d_contract(bk_problem* prob, const double* u, const double* params, int nparams, int ipar, const double* zeta,
                     const double* zeta_star, const double* psi01, const double* psi20, double out[3]);
/* The vectors of the predictors (:410-419 Transcritical, :480 Pitchfork, :524 BranchPoint): M <= 4 device vectors of length n
 *   out[k] = ((x0 + alpha[k] zeta) + beta[k] Psi01) + gamma[k] tau
 * in one pass over the inputs (host coefficients).  psi01 and tau may be NULL with zero coefficients; such a stream is not
 * read.  The outputs are distinct and alias no input.                                                                       */
int bk_nf1d_predict(bk_ctx* ctx, size_t n, const double* x0, const double* zeta, const double* psi01, const double* tau, int M,
                    const double* alpha, const double* beta, const double* gamma, double* const* out);
/* The whole of get_normal_form1d's computation (:281-337) at (x, params) for params[ipar]: the pass of bk_nf1d_dots, the pass
 * of bk_nf1d_rhs, the two bordered solves and the pass of bk_nf1d_contract.  bopts->kind == 0 (BorderingBLS,
 * src/LinearBorderSolver.jl:88-166): the systems share their matrix, so x1_k = J \ r_k run as one two-lane pair (as bk_gmres2)
 * and x2 = J \ zeta* is solved ONCE -- three GMRES solves where the reference's two bls calls run four -- then
 * Psi_k = x1_k - s_k x2 with s_k = <zeta, x1_k> / <zeta, x2>; check_precision / k / tol as bk_bls_bordering, every correction
 * reusing x2.  kind == 1: two solves as bk_bls_matrixfree.  zeta and zeta* come normalised; unless |<zeta, zeta*> - 1| <= 1e-8
 * the call is an error.  coef[5] = (a01, a02, b11, b20, b30); psi01 and psi20 are outputs, distinct from each other and from
 * the inputs.  itlinear[3] = GMRES counts of the Psi01, Psi20 and J \ zeta* solves (kind 1: the two solves, 0).  J is
 * singular by construction at these points, so an unconverged solve is no error (the reference logs it, :304, :334):
 * *converged = the AND over all solves, and each unconverged one adds 1 to the context counter "nf1d_unconverged_solves".  */
int bk_normal_form_1d(bk_ctx* ctx, bk_problem* prob, const double* x, const double* params, int nparams, int ipar,
                      const double* zeta, const double* zeta_star, const bk_bordering_opts* bopts, const bk_gmres_opts* lsopts,
                      bk_precond* pl, double* psi01, double* psi20, double coef[5], int* converged, int itlinear[3]);

/* ------------------------------------------------------------------ cusp points on fold curves -------------
 * The cusp test value along continuation_fold and cusp_normal_form (src/codim2/NormalForms.jl:15-123; Kuznetsov 1999), matrix-free,
 * for BK_PDE_SH (2-D / 3-D) and BK_PDE_SH1D (any other problem: the error of the fold entries above).  At a fold (x, params) with
 * q = zeta spanning ker J, p = zeta* spanning ker J' = J, |q| = 1 and <q, p> = 1 (the two pointers may be equal), B = d2F and
 * C = d3F pointwise and analytic:
 *   b2 = <p, B(q, q)>,   [J q; p' 0][H2; s] = [b2 q - B(q, q); 0]  (:107-109),   c = (<p, C(q, q, q)> + 3 <p, B(q, H2)>) / 6  (:112-113).
 * b2 vanishes at a cusp; c is the coefficient of the cusp normal form.                                                       */
/* One streaming pass over u, v, w that writes nothing: host out[4] = (<w, d2F(u)[v, v]>, <v, v>, <w, w>, <v, w>).  For the
 * unnormalised bordered vectors v, w of a fold-curve point b2 = out[0] / (sqrt(out[1]) out[3]) (q = v / |v|, p = w / <q, w>).
 * Deterministic, all-reduced.                                                                                               */
int bk_cusp_dots(bk_problem* prob, const double* u, const double* params, int nparams, const double* v, const double* w,
                 double out[4]);
/* One pass over u and q: out = b2 q - d2F(u)[q, q], the right-hand side of the H2 solve (:107-108).  out aliases no input.   */
int bk_cusp_rhs(bk_problem* prob, const double* u, const double* params, int nparams, const double* q, double b2, double* out);
/* One streaming pass over u, q, p, H2 (32 N bytes): host out[2] = (<p, d3F(u)[q, q, q]>, <p, d2F(u)[q, H2]>);
 * c = (out[0] + 3 out[1]) / 6 (:112-113).  Deterministic, all-reduced.                                                       */
int bk_cusp_contract(bk_problem* prob, const double* u, const double* params, int nparams, const double* q, const double* p,
                     const double* H2, double out[2]);
/* The whole of cusp_normal_form's computation at (x, params): the pass of bk_cusp_dots on (x, q, p), the pass of bk_cusp_rhs,
 * ONE bordered solve bls(J, q, p, 0, rhs, 0) (:109) and the pass of bk_cusp_contract.  bopts->kind == 0: BorderingBLS as
 * bk_bls_bordering (two GMRES solves, J \ rhs and J \ q; check_precision / k / tol as there); kind == 1: as bk_bls_matrixfree;
 * context option "fold_bordered" = 1 (read once per call; bopts->kind is then not read): as bk_bls_matrixfree_pl, pl must be
 * given.  q and p come normalised; unless |<q, p> - 1| <= 1e-8 the call is an error.  coef[2] = (b2, c); H2 is an output and
 * aliases no input.  itlinear[2] = the GMRES counts (one solve: the second is 0).  J alone is singular at the point, so an
 * unconverged solve is no error (the reference logs it, :110): *converged = 0 and the context counter
 * "cusp_unconverged_solves" grows by 1.                                                                                     */
int bk_cusp_normal_form(bk_ctx* ctx, bk_problem* prob, const double* x, const double* params, int nparams, const double* q,
                        const double* p, const bk_bordering_opts* bopts, const bk_gmres_opts* lsopts, bk_precond* pl, double* H2,
                        double coef[2], int* converged, int itlinear[2]);

/* ------------------------------------------------------------------ normal form, 2-d and 3-d kernels -------------
 * get_normal_formNd (src/NormalForms.jl:648-896), matrix-free, for BK_PDE_SH (2-D / 3-D) and BK_PDE_SH1D (any other problem:
 * the error of the fold entries above) at a branch point (x, params) whose kernel has dimension N = 2 or 3.  J' = J, the
 * is_symmetric branch (:741-743): zeta*_i = zeta_i, and the N kernel vectors zeta[0..N) come orthonormal in l2 (what
 * biorthogonalise, :752, leaves).  With E(r) = r - sum_i <r, zeta_i> zeta_i and the bordered matrix B = [J Z; Z' 0],
 * Z = (zeta_0 ... zeta_{N-1}):
 *   a01[i]        = <dpF, zeta_i>                                         B [Psi01; s] = [E(-dpF); 0]                    (:783, :798)
 *   b20[i,(j,k)]  = <d2F[zeta_j, zeta_k], zeta_i>            j <= k        B [Psijk; s] = [E(-d2F[zeta_j, zeta_k]); 0]    (:822-826, :844-857)
 *   b11[i,j]      = <dJ/dp zeta_j + d2F[zeta_j, Psi01], zeta_i>                                                          (:800-803)
 *   a02[i]        = <2 dJ/dp Psi01 + d2F[Psi01, Psi01], zeta_i>                                                          (:812-813)
 *   b30[i,(j,k,l)]= <d3F[zeta_j, zeta_k, zeta_l] + d2F[zeta_j, Psikl] + d2F[zeta_k, Psijl] + d2F[zeta_l, Psijk], zeta_i>,  j <= k <= l  (:842-871)
 * in a01 dp + a02 dp^2 / 2 + b11 x dp + b20 x x / 2 + b30 x x x / 6 (:541-574).  P = N (N + 1) / 2 pairs (j <= k) and T =
 * N (N + 1) (N + 2) / 6 triples (j <= k <= l), both in lexicographic order; packed layouts a01[i], a02[i], b11[i N + j],
 * b20[i P + jk], b30[i T + jkl].  The tensors are pointwise and analytic and d2F/dp2 = 0 (the reference: ForwardDiff or central
 * differences, :771-780); the border has all N columns (the reference: the first two, :759-760); every Psijk is solved once
 * (the reference re-solves three systems per triple) and a02 is computed once per i.                                         */
/* One streaming pass over u and the N zeta that writes nothing: host out[N + N P + N N] = (a01 | b20 | <zeta_i, zeta_j>) for
 * params[ipar] (12 values for N = 2, 30 for N = 3).  Deterministic, all-reduced.                                             */
int bk_nfnd_dots(bk_problem* prob, const double* u, const double* params, int nparams, int ipar, int N,
                 const double* const* zeta, double* out);
/* One pass over u and the N zeta: the 1 + P projected right-hand sides r[0] = E(-dpF) = sum_i a01[i] zeta_i - dpF and
 * r[1 + jk] = sum_i b20[i P + jk] zeta_i - d2F[zeta_j, zeta_k] (:798, :844-857) with the a01, b20 of bk_nfnd_dots.  The sum
 * over i runs left to right and every product and sum is rounded on its own.  The outputs are distinct and alias no input.   */
int bk_nfnd_rhs(bk_problem* prob, const double* u, const double* params, int nparams, int ipar, int N,
                const double* const* zeta, const double* a01, const double* b20, double* const* r);
/* One streaming pass over u, the N zeta, Psi01 and the P Psijk (7 streams for N = 2, 11 for N = 3): host
 * out[N N + N + N T] = (b11 | a02 | b30) for params[ipar] (14 | 42 values).  Deterministic, all-reduced.                    */
int bk_nfnd_contract(bk_problem* prob, const double* u, const double* params, int nparams, int ipar, int N,
                     const double* const* zeta, const double* psi01, const double* const* psi2, double* out);
/* The whole computation at (x, params) for params[ipar]: the pass of bk_nfnd_dots, the pass of bk_nfnd_rhs, 1 + P solves as
 * bk_bls_block_matrixfree_pl (m = N, a = b = zeta, c = 0, bottom right-hand side 0; Pl^-1 zeta_j is formed once for all of
 * them) and the pass of bk_nfnd_contract.  Errors: N outside {2, 3}; a problem without the fold formulation; pl == NULL; an
 * output (psi01, psi2[0..P)) that aliases another output, x or a zeta; |<zeta_i, zeta_j> - delta_ij| > 1e-8.
 * coef[2 N + N N + N P + N T] = [a01 | a02 | b11 | b20 | b30] (22 values for N = 2, 63 for N = 3); itlinear[1 + P] = GMRES
 * counts of the Psi01 and Psijk solves.  The bordered system is regular at the point itself; an unconverged solve is still a
 * flag and no error (the reference logs it, :799, :846): *converged = the AND over all solves, and each unconverged one adds 1
 * to the context counter "nfnd_unconverged_solves".  The predictor vectors x0 + sum_i x_i zeta_i (:576-582) are
 * bk_nf1d_predict with zeta_0, zeta_1, zeta_2 in its (zeta, psi01, tau) slots.                                               */
int bk_normal_form_nd(bk_ctx* ctx, bk_problem* prob, const double* x, const double* params, int nparams, int ipar, int N,
                      const double* const* zeta, const bk_gmres_opts* lsopts, bk_precond* pl, double* psi01,
                      double* const* psi2, double* coef, int* converged, int* itlinear);

/* ------------------------------------------------------------------ periodic orbits, trapezoid rule --------
 * The functional Trapeze of src/periodicorbit/PeriodicOrbitTrapeze.jl as examples/cGL2d.jl:166-260 uses it (jacobian =
 * FullMatrixFree()), for BK_PDE_CGL2D on one rank; any other problem kind gets the error of the Hopf entries.  Orbit vector
 * (:139-142): M slices of N = 2 n doubles on the device, slice i = [u1; u2], and the period entry T as ONE host scalar.  With
 * K = M - 1, prev(0) = K - 1, prev(i) = i - 1:
 *     G_i = u_i - u_prev(i) - (h / 2) (F(u_i) + F(u_prev(i))), i < K;   G_K = u_K - u_0;   G_T = <u - xpi, phi>.
 * h = T (1 / M) on each of the M - 1 intervals (get_time_step of an integer TimeMesh, src/TimeMesh.jl:21): the entry called T
 * is M / (M - 1) times the orbit's period, as in every guess and result of the reference.                                   */
typedef struct bk_potrap bk_potrap;
typedef struct {
    int converged;
    int niter;       /* operator applications (KrylovKit flavor) / iterations, as bk_gmres reports them */
    double resnorm;
} bk_solve_result;
/* Trapeze(prob, phi, xpi, M, 2n) (:67-110): M >= 3.  The section is set by one of the two calls below.                      */
int bk_potrap_create(bk_problem* prob, int M, bk_potrap** out);
int bk_potrap_destroy(bk_potrap* h);
/* phi, xpi: M N doubles each (the constructor's arguments, cGL2d.jl:177-181); copied.                                       */
int bk_potrap_set_section(bk_potrap* h, const double* phi, const double* xpi);
/* The section in force (trap.ϕ, trap.xπ, :67-110), copied into M N doubles each; an error before a section is set.          */
int bk_potrap_get_section(bk_potrap* h, double* phi, double* xpi);
/* po_residual! (:249-269) with po_residual_bare! (:272-287): out = G(u, T)[0 .. M N), *out_tail = the phase condition
 * <u, phi> - <xpi, phi> (:262).  One marching pass: every slice's stencil is evaluated once, nothing but out is written, the
 * phase dot rides in the same pass (deterministic).  Context option "potrap_chunks": 0 (default) = the chunk count follows
 * the device's compute units, k > 0 = k chunks of the time axis (clamped to [1, M - 1]); out has the same bits for every
 * chunk count.  out must not alias u.                                                                                        */
int bk_potrap_residual(bk_potrap* h, const double* u, double T, const double* params, int nparams, double* out, double* out_tail);
/* po_jvp! (:294-330): the cyclic part Jc (:362-386), the period column -(dT / M / 2) (F(u_i) + F(u_prev(i))) (:309-317), the
 * closure du_K - du_0 and *out_tail = <du, phi> (:323).  One marching pass as above.  out must not alias u or du.           */
int bk_potrap_jvp(bk_potrap* h, const double* u, double T, const double* params, int nparams, const double* du, double dT,
                  double* out, double* out_tail);
/* dG(u, T) as an operator handle with one host tail scalar (the FullMatrixFree Jacobian, :330): REFERENCES u.               */
int bk_potrap_op_create(bk_potrap* h, const double* u, double T, const double* params, int nparams, bk_op** out);
/* updatesection! (:665-681): xpi <- u, phi_i <- F(u_i) / M for every slice.                                                 */
int bk_potrap_update_section(bk_potrap* h, const double* u, double T, const double* params, int nparams);
/* d_p G(u, T) for params[ipar], analytic where the reference differences the functional (src/continuation/Palc.jl:239-240):
 * rows i < K are -(h / 2) (dpF(u_i) + dpF(u_prev(i))), the closure row and the tail are zero.  out must not alias u.        */
int bk_potrap_dparam(bk_potrap* h, const double* u, double T, const double* params, int nparams, int ipar, double* out);
/* The space-time spectral preconditioner P = diag(A0, 1) in the place of the ILU of the assembled Jacobian (cGL2d.jl:209-213):
 * A0 is the cyclic-plus-closure matrix above with every J_i replaced by L0 = Lap (x) I_2 + [[a, -b], [b, a]], the operator of
 * bk_precond_cgl_create (a = r, b = nu: the linearisation at the trivial state).  Applied exactly: the DST-I of all 2 M fields,
 * per sine mode the scalar complex cyclic bidiagonal system in time by one recurrence, the DST-I back.  bk_precond_apply and
 * bk_precond_destroy work on it; the period must be set first.                                                               */
int bk_precond_potrap_create(bk_potrap* h, double a, double b, bk_precond** out);
/* h = T / M of the preconditioner.  Refuses, naming the sine mode, when min_k |1 - (h/2) mu_k| or min_k |1 - rho_k^(M-1)| is
 * below 1e-8 (mu_k = a + lam_k + i b, rho_k = (1 + (h/2) mu_k) / (1 - (h/2) mu_k)): a mode that is Hopf-critical for (a, b) at
 * this period makes A0 singular -- move a.  An error for a preconditioner of another kind.                                  */
int bk_precond_potrap_set_period(bk_precond* pl, double T);
/* Which kernel the transform passes of the LAST application dispatched to, as the dispatch itself recorded it, per axis (x, y):
 * 1 the matrix-core product, 0 one thread per output, 2 rocBLAS (option dct_gemm), -1 no application yet.  A diagnostic
 * (the reference has no counterpart).                                                                                        */
int bk_precond_potrap_transform_paths(bk_precond* pl, int paths[2]);
/* ONE GMRES on diag(A0^-1, 1) dG [x; x_tail] = [A0^-1 rhs; rhs_tail] (the linear solve of newton(poTrapMF, ...),
 * cGL2d.jl:213-219): op from bk_potrap_op_create, pl from bk_precond_potrap_create.  x must not alias rhs.                   */
int bk_potrap_solve(bk_ctx* ctx, bk_op* op, bk_precond* pl, const double* rhs, double rhs_tail, double* x, double* x_tail,
                    const bk_gmres_opts* opts, bk_solve_result* result);

/* ------------------------------------------------------------------ the adjoint of the orbit Jacobian (pofold.hip) --
 * dG(u, T)^T on (w, tau), what the left null vector of the fold of limit cycles is computed with (src/codim2/MinAugFold.jl:15-69
 * on the Trapeze functional, cGL2d.jl:347-392).  With next(j) = j + 1, next(K - 1) = 0, s_j = w_j + w_next(j), q_j = J_j^T s_j:
 *     out_j = (w_j - w_next(j)) - (h / 2) q_j - [j = 0] w_K + tau phi_j (j < K),   out_K = w_K + tau phi_K,
 *     *out_tail = -(1 / (2 M)) sum_{j < K} <F(u_j), s_j>.
 * One marching pass, one adjoint stencil evaluation per slice; option "potrap_chunks" as for bk_potrap_residual, out has the same
 * bits for every chunk count.  out must not alias u, w or the section.                                                       */
int bk_potrap_jvp_adjoint(bk_potrap* h, const double* u, double T, const double* params, int nparams, const double* w, double tau,
                          double* out, double* out_tail);
/* dG(u, T)^T as an operator handle with one host tail scalar: REFERENCES u.                                                  */
int bk_potrap_op_adjoint_create(bk_potrap* h, const double* u, double T, const double* params, int nparams, bk_op** out);
/* diag(A0^T, 1): the DST-I is symmetric and L0^T multiplies a sine mode by conj(mu_k), so per mode w_K = f_K, f_0 <- f_0 + f_K and
 * the cyclic recurrence runs backwards in time, w_j = conj(rho) w_next(j) + f_j / conj(alpha).  bk_precond_potrap_set_period (the
 * same guards: the moduli are equal), bk_precond_apply, bk_precond_potrap_transform_paths and bk_precond_destroy work on it.
 * bk_potrap_solve takes the adjoint operator with the adjoint preconditioner and refuses a mixed pair.                        */
int bk_precond_potrap_adjoint_create(bk_potrap* h, double a, double b, bk_precond** out);
/* ONE GMRES on the doubly bordered system
 *     [A a; b' c][x; x_border] = [rhs; rhs_border],    A = dG or dG^T with its T entry (op of either kind, pl of the same kind),
 * left-preconditioned by diag(A0^-1, 1, 1) (A0^-T for the adjoint): regular where dG is singular, i.e. at a fold of limit
 * cycles.  a, b, rhs, x: M N doubles on the device, each with a host T entry (*_tail); c, rhs_border, *x_border the border
 * scalars.  A0^-1 a is formed once per solve; per application the column update and the row dot are one pass.  x must not alias
 * rhs, a or b.                                                                                                               */
int bk_potrap_bordered_solve(bk_ctx* ctx, bk_op* op, bk_precond* pl, const double* a, double a_tail, const double* b, double b_tail,
                             double c, const double* rhs, double rhs_tail, double rhs_border, double* x, double* x_tail,
                             double* x_border, const bk_gmres_opts* opts, bk_solve_result* result);
/* The border row of the Jacobian of the fold system of the orbit functional (MinAugFold.jl:90-97, :131, :136-145) for params[ipar]
 * from the bordered vectors v (with its T entry v_T) and w, in ONE pass over u, v, w:
 *     <(sigx, *sigx_T), X> = -<w, d2G(u, T)[v, X]> for every X,      *sigma_p = -<w, d_p(dG) v>,
 * with the section frozen.  Through s_j = w_j + w_next(j), q_j = J_j^T s_j: sigx_j = (h / 2) (B_j[v_j, .])^T s_j + (v_T / (2 M)) q_j,
 * sigx_K = 0, sigx_T = (1 / (2 M)) sum <q_j, v_j>, sigma_p = sum <s_j, (h / 2) D_p(u_j) v_j + (v_T / (2 M)) d_pF(u_j)>.
 * sigx must not alias u, v or w.                                                                                             */
int bk_potrap_fold_border(bk_potrap* h, const double* u, double T, const double* params, int nparams, int ipar, const double* v,
                          double v_T, const double* w, double* sigx, double* sigx_T, double* sigma_p);
/* The bordered vectors of the fold of limit cycles (MinAugFold.jl:15-69 on the Trapeze functional) at (u, T, params):
 *     [dG a; b' 0][v; sigma] = [0; 1],      [dG^T b; a' 0][w; sigma2] = [0; 1],
 * one bk_potrap_bordered_solve each (pl forward, pl_adjoint of bk_precond_potrap_adjoint_create, periods set).  a, b, v, w carry
 * a T entry.  itlinear[0] / [1]: the GMRES counts of the v / w solve.                                                         */
int bk_potrap_fold_terms(bk_potrap* h, const double* u, double T, const double* params, int nparams, const double* a, double a_T,
                         const double* b, double b_T, bk_precond* pl, bk_precond* pl_adjoint, const bk_gmres_opts* opts, double* v,
                         double* v_T, double* w, double* w_T, double* sigma, int* converged, int itlinear[2]);
/* The linear solver of the fold system of the orbit functional (FoldLinearSolverMinAug, MinAugFold.jl:136-145, :168-178) at
 * (u, T, params) with the bordered vectors v (T entry v_T) and w of that point, for nrhs = 1 or 2 right-hand sides (rhsu[k] device,
 * rhsT[k] and rhsp[k] host: the T entry and the sigma row):  [dG d_pG; sigx' sigma_p][dX_k; dsigma_k] = [rhs_k; rhsp_k] with the
 * border of bk_potrap_fold_border for params[ipar], ONE bk_potrap_bordered_solve per right-hand side (pl forward, period set).
 * dX[k] device, dXT[k] and dsigma[k] host; *itlinear = the GMRES counts summed.  dX must not alias a right-hand side, u, v or w. */
int bk_potrap_fold_linsolve(bk_potrap* h, const double* u, double T, const double* params, int nparams, int ipar, const double* v,
                            double v_T, const double* w, bk_precond* pl, int nrhs, const double* const* rhsu, const double* rhsT,
                            const double* rhsp, const bk_gmres_opts* opts, double* const* dX, double* dXT, double* dsigma,
                            int* converged, int* itlinear);
/* newton_fold on the orbit functional (cGL2d.jl:347-370; MinAugFold.jl:211-233) under the semantics of _newton: (u, *T, *p) =
 * guess on entry, the fold of limit cycles on exit; params[ipar] is the fold parameter; the section of h and (a, b) stay frozen.
 * Per point the two solves of bk_potrap_fold_terms, per step [dG d_pG; sigx' sigma_p][dX; dp] = [G; sigma] as one
 * bk_potrap_bordered_solve (the branch :136-145).  tol applies to max(|G|_inf, |G_T|, |sigma|) (norm_inf) or the 2-norm.  On exit
 * v, w, *sigma are those of the returned point.  itlinear_steps (may be NULL; 3 (max_iterations + 1) ints): per point the
 * counts of the v and w solves, then of the step taken from it.                                                              */
int bk_potrap_newton_fold(bk_potrap* h, double* u, double* T, double* p, const double* params, int nparams, int ipar, const double* a,
                          double a_T, const double* b, double b_T, bk_precond* pl, bk_precond* pl_adjoint, const bk_newton_opts* no,
                          const bk_gmres_opts* opts, double* v, double* v_T, double* w, double* w_T, double* sigma,
                          bk_newton_result* res, int* itlinear_steps);

/* ------------------------------------------------------------------ Floquet multipliers of trapezoid orbits --------
 * The matrix-free monodromy of FloquetQaD (src/periodicorbit/Floquet.jl:48-85), MonodromyQaD_matrix_free(::Trapeze, ...)
 * (:285-315): K = M - 1 sequential steps x <- (I - hh J_i)^-1 (I + hh J_prev(i)) x, hh = T (1 / M) / 2.  Here the same vector is
 * the last slice of ONE block lower-bidiagonal initial-value system over all K slices,
 *     A_i y_i - B_{i-1} y_{i-1} = 0 (i >= 1),  A_0 y_0 = B_{K-1} x,  A_i = I - hh J_i,  B_i = I + hh J_i,  M x = y_{K-1},
 * solved by one left-preconditioned GMRES.  BK_PDE_CGL2D on one rank, as the other bk_potrap_* entries.                     */
/* The initial-value operator on K slices y (K N doubles): out_0 = y_0 - hh J_0 y_0, out_i = (y_i - hh J_i y_i) - (y_{i-1} +
 * hh J_{i-1} y_{i-1}), J_i the cGL Jacobian at orbit slice i of u (M N doubles).  One marching pass; option "potrap_chunks" as
 * for bk_potrap_residual, the same bits for every chunk count.  out must not alias y or u.                                  */
int bk_potrap_ivp_march(bk_potrap* h, const double* u, double T, const double* params, int nparams, const double* y, double* out);
/* The preconditioner of that system on K N doubles: every J_i replaced by L0 = Lap (x) I_2 + [[a, -b], [b, a]], applied exactly
 * (DST-I of all 2 K fields, per sine mode w_i = rho w_{i-1} + f_i / alpha from w_{-1} = 0, DST-I back; alpha, rho as in
 * bk_precond_potrap_set_period).  The period is fixed at creation.  Refuses, naming the sine mode, when min_k |alpha_k| is below
 * 1e-8.  bk_precond_apply and bk_precond_destroy work on it.                                                                 */
int bk_precond_potrap_ivp_create(bk_potrap* h, double a, double b, double T, bk_precond** out);
/* As bk_precond_potrap_transform_paths, for a preconditioner of bk_precond_potrap_ivp_create.                               */
int bk_precond_potrap_ivp_transform_paths(bk_precond* pl, int paths[2]);
/* dx -> MonodromyQaD_matrix_free(trap, u0, par, dx) (Floquet.jl:63, :285-315) as an unbordered operator of length N:
 * apply(x, a0, a1, out) = a0 x + a1 y_{K-1}, one GMRES (opts: a GMRES flavor, left preconditioner (a, b) only) per application.
 * A solve that does not converge is counted, not fatal.  REFERENCES u; owns its preconditioner and work vectors; destroy with
 * bk_op_destroy.                                                                                                             */
int bk_potrap_monodromy_create(bk_potrap* h, const double* u, double T, const double* params, int nparams, double a, double b,
                               const bk_gmres_opts* opts, bk_op** out);
/* One application that also returns all K slices y_0 .. y_{K-1} (K N doubles): for a Floquet eigenvector x the space-time
 * eigenfunction of the Val(:ExtractEigenVector) method (Floquet.jl:319-355), out of the same solve.                          */
int bk_potrap_monodromy_solve(bk_op* op, const double* x, double* y_all, int* converged, int* niter);
/* Counters since creation: solves, those that did not converge, GMRES iterations summed; paths: the transform kernels of the
 * last preconditioner application (bk_precond_potrap_transform_paths).  Any pointer may be NULL.                             */
int bk_potrap_monodromy_stats(bk_op* op, int* solves, int* failed, int* inner_its, int paths[2]);
/* (eig::EigKrylovKit)(op, nev) with which = :LM, what _check_floquet_options forces for Floquet work (Floquet.jl:4-17):
 * Krylov-Schur on the operator itself, Ritz values ordered by modulus, no back-transform; values come back by decreasing
 * modulus.  Arguments and output conventions of bk_eig_krylovkit (sigma ignored).                                            */
int bk_eig_krylovkit_lm(bk_ctx* ctx, bk_op* op, int nev, const bk_eig_opts* eopts, double* vals_re, double* vals_im,
                        double* vecs, double* vecs_im, size_t ldvecs, int* nvals, int* nconv, int* numops);

/* ------------------------------------------------------------------ the spectral ETDRK2 flow of cGL (flow.hip) --------
 * The flow that examples/cGL2d-shooting.jl builds from SplitODEProblem(Lap, NL) and ETDRK2 (:108-113, :123-128), for BK_PDE_CGL2D on
 * one rank; any other problem kind gets the error of the Hopf entries.  Fixed-step Cox-Matthews ETDRK2, h = tau / nsteps, with the
 * Dirichlet Laplacian exact in sine space (batched DST-I) and every pointwise term in N:
 *     a^ = e^z u_n^ + h phi1(z) N^(u_n),   u_{n+1}^ = a^ + h phi2(z) (N^(a) - N^(u_n)),   z_k = h (lam_x[i] + lam_y[j]).
 * Deviations from the example: its krylov = true approximates the phi functions and takes dt = 0.1; here they are exact per mode
 * and the step count is the caller's.  B trajectories advance in lock-step; trajectory i is [u1; u2], N = 2 n doubles, at i N.  */
typedef struct bk_flow bk_flow;
int bk_flow_create(bk_problem* prob, int B, bk_flow** out);
int bk_flow_destroy(bk_flow* flow);
/* evolve(flow, x, par, tau).u (src/periodicorbit/Flow.jl) for B states: out = Phi(x, tau).  A step is four batched transforms, two
 * pointwise passes and two spectral passes.  Errors: nsteps < 1, tau not finite, out aliasing x.                              */
int bk_flow_evolve(bk_flow* flow, const double* x, double tau, int nsteps, const double* params, int nparams, double* out);
/* jvp(flow, x, par, dx, tau) (Flow.jl): out = Phi(x, tau) and dout = dPhi(x, tau) dx from ONE march of state and tangent.  The
 * tangent is the exact derivative of the discrete map where the example differences the flow (FiniteDifferencesMF, :127).
 * Errors: as bk_flow_evolve; out aliasing x or dx; dout aliasing x, dx or out.                                                */
int bk_flow_jvp(bk_flow* flow, const double* x, const double* dx, double tau, int nsteps, const double* params, int nparams,
                double* out, double* dout);
/* The three tables of a step h, n HOST doubles each in natural mode order: E = e^z, P1 = h phi1(z), P2 = h phi2(z).  phi2 is
 * summed as a series for |z| < 1; z -> -inf gives E = 0 and finite P1, P2.  A diagnostic (the reference has no counterpart).   */
int bk_flow_coefficients(bk_flow* flow, double h, double* E, double* P1, double* P2);
/* Which kernel the transform passes of the last march dispatched to, per axis (x, y): as
 * bk_precond_potrap_transform_paths.                                                                                          */
int bk_flow_transform_paths(bk_flow* flow, int paths[2]);
/* Counters since creation: marches that advanced the state, and the kernels the marches launched as the march itself adds them
 * up (12 per step -- two per transform --, 2 for the first transform, the copies): a derived figure.  Either may be NULL.     */
int bk_flow_stats(bk_flow* flow, long long* base_marches, long long* launches);

/* ------------------------------------------------------------------ periodic orbits, standard shooting (shooting.hip) --------
 * Shooting of src/periodicorbit/StandardShooting.jl (:138-257) with ds = 1 / M on the flow above and SectionSS of
 * src/periodicorbit/Sections.jl:6-58, as examples/cGL2d-shooting.jl:123-150 uses them; BK_PDE_CGL2D on one rank.  Orbit vector: M
 * states of N doubles on the device and the period T as ONE host scalar.  With next(i) = i + 1, next(M - 1) = 0:
 *     G_i = Phi(x_i, T / M) - x_next(i),      G_T = (<x_0, normal> - <center, normal>) T            (Sections.jl:13).
 * The M segments advance in lock-step (the reference's parallel = true); each takes nsteps steps of h = T / M / nsteps.       */
typedef struct bk_shooting bk_shooting;
/* Shooting(M, prob_sp, ETDRK2()) (:160-174; M = 1: simple shooting, :123-128).  Errors: more than one rank (asked first: a
 * BK_PDE_CGL2D problem does not exist on several ranks), another problem kind, M < 1, nsteps < 1.                             */
int bk_shooting_create(bk_problem* prob, int M, int nsteps, bk_shooting** out);
int bk_shooting_destroy(bk_shooting* sh);
/* SectionSS(normal, center): N doubles each, copied.                                                                          */
int bk_shooting_set_section(bk_shooting* sh, const double* normal, const double* center);
int bk_shooting_get_section(bk_shooting* sh, double* normal, double* center);
/* updatesection! (:116-122): normal = F(x_0) / |F(x_0)|_2, center = x_0.                                                      */
int bk_shooting_update_section(bk_shooting* sh, const double* x, double T, const double* params, int nparams);
/* po_residual (:138-165): one march of the M segments, then the closure and the section dot in ONE pass (deterministic).  out
 * must not alias x.                                                                                                           */
int bk_shooting_residual(bk_shooting* sh, const double* x, double T, const double* params, int nparams, double* out, double* out_tail);
/* po_jvp (:190-228): out_i = dPhi_i dx_i + F(Phi_i) (dT / M) - dx_next(i), *out_tail = (<x_0, normal> - <center, normal>) dT +
 * <dx_0, normal> T (Sections.jl:43-45).  The period column is vector_field(flow, Phi_i) ds dT (:217), not the tau-derivative of
 * the discrete map.  One march of state and tangent, then one pass.  out must not alias x or dx.                              */
int bk_shooting_jvp(bk_shooting* sh, const double* x, double T, const double* params, int nparams, const double* dx, double dT,
                    double* out, double* out_tail);
/* dG(x, T) as an operator handle with one host tail scalar: REFERENCES x; the section in force is copied, so a later
 * bk_shooting_set_section / update_section does not reach an existing operator.  Context option "shooting_store" (default 1): the
 * base trajectory is marched once, here, u_n and the stage value a_n of every step are kept (2 nsteps M N doubles), and every
 * application marches the tangent alone -- four transforms of 2 M fields per step instead of 4 M and no base nonlinearity.  0:
 * state and tangent are marched together in every application.  Both give the same bits.  The record is one block that goes back
 * to the handle sh when the operator is destroyed and is reused by the next operator (Newton creates one per step; only the first
 * allocates), so sh must outlive its operators.  The budget: the workspace pool of the context has no limit of its own to take one
 * from, so it is the option "shooting_store_max" (doubles, default 2^28); a record above it falls back to recomputation.      */
int bk_shooting_op_create(bk_shooting* sh, const double* x, double T, const double* params, int nparams, bk_op** out);
/* One application of an operator of bk_shooting_op_create: (out, *out_tail) = dG(x, T) (dx, dT), what bk_shooting_jvp returns,
 * on the operator's route (stored or recomputed base).  out must not alias dx or the operator's x.                             */
int bk_shooting_op_apply(bk_op* op, const double* dx, double dT, double* out, double* out_tail);
/* For an operator of bk_shooting_op_create or bk_shooting_monodromy_create: whether it keeps the base trajectory, the base marches
 * it has run and its applications, since creation.  Any pointer may be NULL.                                                  */
int bk_shooting_op_stats(bk_op* op, int* stored, long long* base_marches, long long* applications);
/* The transform kernels of the functional's last march, as bk_flow_transform_paths.                                           */
int bk_shooting_transform_paths(bk_shooting* sh, int paths[2]);
/* ONE unpreconditioned GMRES on dG [x; x_tail] = [rhs; rhs_tail] (the linear solve of newton(probSh, ...), cGL2d-shooting.jl
 * :135-137): op from bk_shooting_op_create.  GMRES flavors only; x must not alias rhs.                                        */
int bk_shooting_solve(bk_ctx* ctx, bk_op* op, const double* rhs, double rhs_tail, double* x, double* x_tail,
                      const bk_gmres_opts* opts, bk_solve_result* result);
/* dx -> MonodromyQaD_matrix_free(sh, x, par, dx) (src/periodicorbit/Floquet.jl:89-108) as an unbordered operator of length N:
 * the M segment tangents applied in sequence on the base trajectory, which is marched and kept at creation (an error when it
 * exceeds "shooting_store_max"); apply(x, a0, a1, out) = a0 x + a1 M x.  Copies what it needs of x; destroy with bk_op_destroy.
 * The multipliers come from bk_eig_krylovkit_lm.                                                                              */
int bk_shooting_monodromy_create(bk_shooting* sh, const double* x, double T, const double* params, int nparams, bk_op** out);

/* ------------------------------------------------------------------ Bogdanov-Takens points ---------------
 * The minimally augmented Bogdanov-Takens formulation (src/codim2/MinAugBT.jl), matrix-free, for BK_PDE_CGL2D on one rank (any
 * other problem: the error of the Hopf entries).  Unknowns (x, p1, p2) for the two lenses ipar1 != ipar2,
 *   G = (F, sigma1, sigma2),  [J a; b' 0][v1; sigma1] = [0; 1],  [J a; b' 0][v2; sigma2] = [v1; 0],
 *                             [J' b; a' 0][w1; .] = [0; 1],      [J' b; a' 0][w2; .] = [w1; 0].
 * J has a double zero eigenvalue at the point, so every solve is ONE GMRES on its bordered system with the left preconditioner
 * diag(Pl, 1) (bk_bls_matrixfree_pl semantics): pl for J, pl_adj for J' (bk_precond_cgl_create with the sign of b flipped).   */
/* One streaming pass over u and four real device vectors: row1 = s B(u)[v1, .]' w1, row2 = s (B(u)[v1, .]' w2 + B(u)[v2, .]' w1)
 * (B = d2F, so <row, y> = s <w, d2F(u)[v, y]>), host sums[4] = s <w1, D_k v1> (sums[k]) and s (<w2, D_k v1> + <w1, D_k v2>)
 * (sums[2 + k]) with D_k = dJ/dp for ipar1 (k = 0) and ipar2 (k = 1).  s = -1 with the bordered vectors: sigma1_x, sigma2_x and
 * the row-major 2 x 2 block sigma_p.  row1, row2 must not alias an input or each other.  Deterministic.                      */
int bk_bt_border(bk_problem* prob, const double* u, const double* params, int nparams, int ipar1, int ipar2, double s,
                 const double* v1, const double* v2, const double* w1, const double* w2, double* row1, double* row2,
                 double sums[4]);
/* The bordered vectors at (x, params): (v1, v2, sigma[2]) when v1, v2 are given (pl required), (w1, w2) when w1, w2 are given
 * (pl_adj required); each pair both or neither, at least one pair.  converged[4], itlinear[4] (each may be NULL): per solve in
 * the order v1, v2, w1, w2 (1 and 0 for a pair that is not solved).                                                          */
int bk_bt_terms(bk_ctx* ctx, bk_problem* prob, const double* x, const double* params, int nparams, const double* a,
                const double* b, const bk_gmres_opts* lsopts, bk_precond* pl, bk_precond* pl_adj, double* v1, double* v2,
                double* w1, double* w2, double sigma[2], int converged[4], int itlinear[4]);
/* btMALinearSolver (:118-228) with the bordered vectors of (x, params) given: [J dpF; sigma_x sigma_p][dX; dp] = [rhsu; rhsp]
 * as ONE block-bordered solve with m = 2 (bk_bls_block_matrixfree_pl semantics): columns dF/dp1, dF/dp2 (analytic), rows and
 * block from bk_bt_border with s = -1.  dX must be a fresh buffer.                                                           */
int bk_bt_linsolve(bk_ctx* ctx, bk_problem* prob, const double* x, const double* params, int nparams, int ipar1, int ipar2,
                   const double* v1, const double* v2, const double* w1, const double* w2, const double* rhsu,
                   const double rhsp[2], const bk_gmres_opts* lsopts, bk_precond* pl, double* dX, double dp[2], int* converged,
                   int* itlinear);
/* newton_bt under the semantics of _newton (src/Newton.jl:66-114), as bk_newton_hopf: (x, p[2]) = guess on entry, the
 * Bogdanov-Takens point on exit; tol applies to BorderedArray(F, [sigma1, sigma2]) in the chosen norm; callback as bk_newton
 * (p = p[0]).  Each point's v1, v2 are solved once and serve its residual and its Newton step; w1, w2 are solved per step.  On
 * exit v1, v2 and sigma are those of the returned point, w1, w2 those of the last step taken.  itsolves[5] (may be NULL): GMRES
 * iterations summed per solve, v1, v2, w1, w2 and the block solve; *unconverged (may be NULL): solves that returned unconverged. */
int bk_newton_bt(bk_ctx* ctx, bk_problem* prob, double* x, double p[2], const double* params, int nparams, int ipar1, int ipar2,
                 const double* a, const double* b, const bk_newton_opts* nopts, const bk_gmres_opts* lsopts, bk_precond* pl,
                 bk_precond* pl_adj, double* v1, double* v2, double* w1, double* w2, double sigma[2], bk_newton_result* res,
                 int itsolves[5], int* unconverged);

/* The streaming passes of the Bogdanov-Takens normal form (src/codim2/NormalForms.jl:180-272) at (u, params) with the Jordan chains
 * J q0 = 0, J q1 = q0, J' p1 = 0, J' p0 = p1, B = d2F:
 *   bk_bt_nf_dots  host out[6] = <p1, B(q0, q0)>, <p0, B(q0, q0)>, <p1, B(q0, q1)>, <p0, B(q0, q1)>, <p1, B(q1, q1)>, <p0, B(q1, q1)>
 *   bk_bt_nf_rhs   mode 0: out = k q1 - B(q0, q0) (H unused); mode 1: out = k q1 + H - B(q0, q1); out must not alias an input
 *   bk_bt_nf_k2    host out[3] = <p1, B(H0001, H0001)>, <p1, D_1 H0001>, <p1, D_2 H0001>, D_k = dJ/dp for ipar1, ipar2
 * One pass each, deterministic.                                                                                              */
int bk_bt_nf_dots(bk_problem* prob, const double* u, const double* params, int nparams, const double* q0, const double* q1,
                  const double* p0, const double* p1, double out[6]);
int bk_bt_nf_rhs(bk_problem* prob, const double* u, const double* params, int nparams, int mode, double k, const double* q0,
                 const double* q1, const double* H, double* out);
int bk_bt_nf_k2(bk_problem* prob, const double* u, const double* params, int nparams, int ipar1, int ipar2, const double* p1,
                const double* H0001, double out[3]);
/* bogdanov_takens_normal_form (:141-335) through K2.  Host nf[10] = (a, b, gamma, c, K10[2], K11[2], K2[2]) with
 *   a = <p1, B(q0, q0)> / 2,  b = <p0, B(q0, q0)> + <p1, B(q0, q1)>;   detailed = 0 returns after these (the rest NaN, no solve).
 * detailed: H2000 and H1100 from two bordered solves [J p1; q0' 0] (Ainv, :205-213), H0010 / K10 and H0001 / K11 from two
 * block-bordered solves with m = 2 of [J dpF; A12 A22] (:258-262; A12, A22 analytic from the bk_bt_border pass with s = +1), K2
 * from bk_bt_nf_k2.  Every parameter of BK_PDE_CGL2D enters F linearly, so the second parameter derivatives of :234-246 vanish.
 * converged[4], itlinear[4] (each may be NULL): per solve in the order H2000, H1100, (H0010, K10), (H0001, K11).  The
 * coefficients of the homoclinic predictor (d, e, a1, b1 and their vectors) are not computed.                                */
int bk_bt_normal_form(bk_ctx* ctx, bk_problem* prob, const double* x, const double* params, int nparams, int ipar1, int ipar2,
                      const double* q0, const double* q1, const double* p0, const double* p1, int detailed,
                      const bk_gmres_opts* lsopts, bk_precond* pl, double* H2000, double* H1100, double* H0010, double* H0001,
                      double nf[10], int converged[4], int itlinear[4]);

#ifdef __cplusplus
}
#endif
#endif /* BKHIP_H */
