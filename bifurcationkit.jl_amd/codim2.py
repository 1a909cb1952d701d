"""Fold and Hopf points: refinement and two-parameter continuation with the minimally augmented formulations of
src/codim2/MinAugFold.jl and MinAugHopf.jl (Hopf: the second half of this module; the Hopf normal form and the periodic-orbit
predictor of src/NormalForms.jl and the Bautin normal form of src/codim2/NormalForms.jl: its last sections), matrix-free on the preconditioned GMRES
path (the reference assembles the systems for MatrixBLS / MinAugMatrixBased, which cannot run at the sizes of this library).

  FoldProblem              FoldMinimallyAugmentedFormulation + FoldMAProblem: G(X, p2) = (F(x, p1), sigma(x, p1)), X = (x, p1)
  FoldLinearSolverMinAug   foldMALinearSolver, usehessian branch (:119-166): one or two right-hand sides, one shared J \\ dpF
  fold_point               fold_point(br, ind) (:6-13) on a Python branch record, with the start vector a = b = tau
  newton_fold              newton_fold (:211-278) written out call by call on HipVecs (bk_d2f, bk_djdp, ls(J, r1, r2), BorderingBLS)
  newton_fold_native       the same as one library call (bk_newton_fold)
  continuation_fold        continuation_fold (:369-536): PALC on G(X, p2), BorderingBLS(solver = FoldLinearSolverMinAug,
                           check_precision = false) as wired at :445-453, Secant tangent, a / b updated after every step
                           (update!, :280-313), BT = <zeta*, zeta> and CP = tau.p recorded (test_bt_cusp, :551-576);
                           detect_codim2 = 1 | 2: b2 = <p, B(q, q)> per point, the sign changes of CP as "cusp" points,
                           bisected (_locate_event)
  cusp_normal_form         cusp_normal_form (src/codim2/NormalForms.jl:15-123) call by call; cusp_normal_form_native: the same
                           as one library call (bk_cusp_normal_form); get_normal_form on a "cusp" point of a FoldBranch

Problems: SwiftHohenberg (2-D / 3-D) and SwiftHohenberg1D -- symmetric, J' = J (:79-84).  sigma_p, dpF and sigma_x are analytic
(the Jacobians depend on the parameters only through their pointwise term), where the reference takes central differences.
The bordered vectors v, w of a point are solved once and serve both its residual and its Newton step.
With ``bls = MatrixFreeBLS(ls, use_pl=True)`` the fold entries run the branch without `usehessian` (:54-69, :136-145) on the
preconditioned bordered solver: [J a; b' 0] for (v, sigma) and w, [J dpF; sigma_x' sigma_p] per Newton step -- systems that stay
regular at the fold, where J \\ a and J \\ F do not converge (context option fold_bordered).

Codim-2 points: on Hopf curves generalised Hopf (Bautin) points are detected, bisected and given their normal form
(continuation_hopf(..., detect_codim2 = 1 | 2), get_normal_form on a "gh" point); on fold curves cusp points, the same way
(continuation_fold(..., detect_codim2 = 1 | 2), get_normal_form on a "cusp" point).  A Hopf curve that stops near omega = 0 records
a Bogdanov-Takens guess ("bt"), which newton_bt refines and get_normal_form unfolds (a, b, K10, K11, K2; the last section of this
module); the Hopf curve restarts from it with continuation_hopf_from_bt.  Zero-Hopf and Hopf-Hopf points are not located, nor
Bogdanov-Takens points on fold curves; for the Swift-Hohenberg problems J' = J, so BT = <zeta*, zeta> = 1 and a fold curve has no
Bogdanov-Takens point.

What the two formulations have in common is written once: _MinAugProblem (the cached bordered vectors and the problem surface),
_MinAugLinearSolver, _continuation_minaug (the PALC loop) and _newton_minaug_mirror (the Newton loop of the mirrors).
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _lib as L
from . import continuation as Cn
from .hip import BorderedArray, BorderingBLS, HipJacobian, HipVec, MatrixFreeBLS, _GMRES, _ptr, newton_opts


def _nanmax(*vals):
    """max that propagates a NaN from any argument (Python's max drops it depending on the argument order)."""
    vals = [float(v) for v in vals]
    return math.nan if any(v != v for v in vals) else max(vals)


def _norm_fold(F, sigma, norm_inf):
    """normN of BorderedArray(F, sigma): norminf = max(|F|_inf, |sigma|), norm = sqrt(|F|^2 + sigma^2); a NaN in either
    component gives NaN in both norms, as norm_fold of fold.hip."""
    return _nanmax(F.norminf(), abs(sigma)) if norm_inf else math.sqrt(F.norm() ** 2 + sigma ** 2)


def _carr(pars):
    """The parameter list as the double array of the C API."""
    return (C.c_double * len(pars))(*pars)


def _vptrs(vecs):
    """The device pointers of HipVecs as an array of const double* (one unused slot when there are none)."""
    return (C.c_void_p * max(len(vecs), 1))(*[v.t.data_ptr() for v in vecs])


def _into_similar(prob, fn: str, x: HipVec, pars, *args) -> HipVec:
    """out = the library's ``fn``(prob, x, pars, len(pars), *args, out) with a new vector ``out`` like x."""
    ctx, out = prob.ctx, x.similar()
    ctx.check(getattr(ctx.lib, fn)(prob.h, _ptr(x.t), _carr(pars), len(pars), *args, _ptr(out.t)), fn)
    return out


def _params(prob, **vals):
    pv = dict(prob.params)
    pv.update({k: float(v) for k, v in vals.items()})
    return [float(pv[k]) for k in prob.param_names]


def d2F(prob, x: HipVec, pars, dx1: HipVec, dx2: HipVec) -> HipVec:
    """d2F(prob, x, par, dx1, dx2) (src/Problems.jl:107,165) on the device (bk_d2f)."""
    return _into_similar(prob, "bk_d2f", x, pars, _ptr(dx1.t), _ptr(dx2.t))


def dJdp(prob, x: HipVec, pars, ipar: int, dx: HipVec) -> HipVec:
    """dJ/dp(x) dx for params[ipar] (bk_djdp): the analytic value of dJvdp in _get_bordered_terms (:93-94)."""
    return _into_similar(prob, "bk_djdp", x, pars, int(ipar), _ptr(dx.t))


def fold_contract(prob, x: HipVec, pars, ipar: int, v: HipVec, w: HipVec, X=()):
    """One fused pass (bk_fold_contract): ([<w, d2F(x)[v, X_k]> for X_k in X], -<w, dJ/dp v>)."""
    ctx = prob.ctx
    m = len(X)
    xp = _vptrs(X)
    out = (C.c_double * (m + 1))()
    ctx.check(ctx.lib.bk_fold_contract(prob.h, _ptr(x.t), _carr(pars), len(pars), int(ipar), _ptr(v.t), _ptr(w.t), m, xp, out),
              "bk_fold_contract")
    return [out[k] for k in range(m)], out[m]


def residual(prob, x: HipVec, pars) -> HipVec:
    """F(x, pars) with every parameter given (bk_residual)."""
    return _into_similar(prob, "bk_residual", x, pars)


def dpF(prob, x: HipVec, pars, ipar: int) -> HipVec:
    """Analytic dF/dp for params[ipar].  bk_residual_dparam evaluates ((p + eps) - p) / eps * phi_p(x) and phi_p does not
    depend on the parameters, so with p = 0 and eps = 1 the scalar is exactly 1."""
    pv = list(pars)
    pv[ipar] = 0.0
    return _into_similar(prob, "bk_residual_dparam", x, pv, int(ipar), 1.0)


def _bls_opts(bls):
    if isinstance(bls, MatrixFreeBLS):          # the entry points take the struct; with fold_bordered = 1 they do not read it
        return L.BorderingOpts(1e-12, 0, 1, 1)
    return L.BorderingOpts(bls.tol, 1 if bls.check_precision else 0, bls.k, 0)


def _bordered_path(bls) -> bool:
    """True when ``bls`` selects the fold formulation on the system that is regular at the fold (context option fold_bordered):
    MatrixFreeBLS(ls, use_pl=True), every solve ONE GMRES on [J a; b' c] left-preconditioned by diag(Pl, 1)."""
    if isinstance(bls, MatrixFreeBLS):
        if not bls.use_pl:
            raise TypeError("the fold formulation takes BorderingBLS or MatrixFreeBLS(ls, use_pl=True)")
        return True
    return False


class _fold_bordered:
    """Context option fold_bordered set to 1 around a native call and put back afterwards (the library reads it once per call).
    With ``on`` false nothing is touched.  An option cannot be unset: on a context that never had it, it is left at 0, which the
    library reads as the default path (tests/test_gpu_fold_bordered.py: unset and 0 give the same bits)."""
    option = "fold_bordered"

    def __init__(self, ctx, on: bool):
        self.ctx, self.on = ctx, bool(on)
        self.prev = None

    def __enter__(self):
        if self.on:
            try:
                self.prev = self.ctx.get_option(self.option)
            except L.BkHipError:
                self.prev = 0.0
            self.ctx.set_option(self.option, 1.0)
        return self

    def __exit__(self, *exc):
        if self.on:
            self.ctx.set_option(self.option, self.prev)
        return False


class _hopf_bordered(_fold_bordered):
    """The same for the context option hopf_bordered (tests/test_gpu_hopf_bordered.py: unset and 0 give the same bits)."""
    option = "hopf_bordered"


def _hopf_bordered_path(bls) -> bool:
    """True when ``bls`` selects the Hopf bordered vectors (and the H21 solve of the Bautin normal form) on the system that is
    regular at the Hopf point (context option hopf_bordered): MatrixFreeBLS(ls, use_pl=True), each bordered vector ONE GMRES on
    [J - i omega, a; b^H, 0] left-preconditioned by diag(Pl, 1).  None or a BorderingBLS: block elimination, two shifted solves."""
    if isinstance(bls, MatrixFreeBLS):
        if not bls.use_pl:
            raise TypeError("the Hopf formulation takes BorderingBLS or MatrixFreeBLS(ls, use_pl=True)")
        return True
    return False


def fold_border(prob, x: HipVec, pars, ipar: int, v: HipVec, w: HipVec):
    """(sigx, sigma_p) of bk_fold_border: sigx = -w h(x) v as a vector, <sigx, X> = -<w, d2F(x)[v, X]>; sigma_p = -<w, dJ/dp v>."""
    ctx, out = prob.ctx, x.similar()
    sp = C.c_double()
    ctx.check(ctx.lib.bk_fold_border(prob.h, _ptr(x.t), _carr(pars), len(pars), int(ipar), _ptr(v.t), _ptr(w.t), _ptr(out.t),
                                     C.byref(sp)), "bk_fold_border")
    return out, sp.value


def _solve2(ls: _GMRES, J, rhs1: HipVec, rhs2: HipVec):
    """ls(J, rhs1, rhs2) (src/LinearSolver.jl:15-19) as the library runs it inside its own solves (bk_gmres2: both solves start
    from the same solver state), so that the call-by-call path reproduces the native one."""
    ctx = rhs1.ctx
    x1, x2 = rhs1.similar(), rhs2.similar()
    cv = C.c_int()
    it = (C.c_int * 2)()
    o = ls._opts()
    ctx.check(ctx.lib.bk_gmres2(ctx.h, J.h, _ptr(rhs1.t), _ptr(rhs2.t), _ptr(x1.t), _ptr(x2.t), 0.0, 1.0, C.byref(o), ls._pl(),
                                C.byref(cv), it), "bk_gmres2")
    return x1, x2, bool(cv.value), (it[0], it[1])


# ------------------------------------------------------------------------------------------ what fold and Hopf share
def _newton_minaug_mirror(point, step, norm, tol, max_iterations):
    """_newton (src/Newton.jl:66-114) on G: ``point()`` -> (F, sigma, v, w) at the current unknowns, ``step(F, sigma, v, w)``
    one update of them with the bordered vectors of that point.  Returns (last point, residuals, steps)."""
    pt = point()
    res = [norm(pt[0], pt[1])]
    n = 0
    while n < max_iterations and res[-1] > tol:
        step(*pt)
        pt = point()
        res.append(norm(pt[0], pt[1]))
        n += 1
    return pt, res, n


class _MinAugProblem:
    """G(X, p2) = (F(x, p1), sigma) of a minimally augmented formulation with lens2: X = (x, scalar unknowns), p1 = the
    problem's lens, parameter p2 = ``lens2``.  ``residual`` / ``jacobian`` / ``residual_dparam`` are the BifurcationProblem
    surface continuation.newton_palc drives; the bordered vectors of a point are cached and solved once per point.  A
    formulation supplies ``_p1`` (p1 of X), ``_solve_terms`` (v, w, sigma and the GMRES counts of the bordered solves), ``_vec``
    (a residual vector from its x part and sigma), ``_sigma_p`` and ``update``."""

    def __init__(self, prob, lens2: str, a, b, ls: _GMRES):
        if lens2 == prob.lens:
            raise ValueError(f"Please choose 2 different parameters. You only passed {lens2}")
        self.prob, self.ctx = prob, prob.ctx
        self.lens1, self.lens2 = prob.lens, lens2
        self.ipar1, self.ipar2 = prob.param_names.index(prob.lens), prob.param_names.index(lens2)
        self.ls = ls
        self.a, self.b = a, b
        self.delta = prob.delta
        self.itlinear = 0                       # GMRES counts of the bordered-vector solves (the linear solver counts its own)
        self._cache = None

    def pvec(self, p1, p2):
        return _params(self.prob, **{self.lens1: p1, self.lens2: p2})

    def terms(self, X, p2: float):
        """(v, w, sigma) of _compute_bordered_vectors at (X, p2), solved once per point."""
        c = self._cache
        if c is not None and np.array_equal(c[1], X.p) and c[2] == p2 and torch.equal(c[0].t, X.u.t):
            return c[3]
        v, w, sigma, *_, it = self._solve_terms(X, p2)      # fold_terms / hopf_terms: (v, w, sigma, ..., (itv, itw))
        self.itlinear += it[0] + it[1]
        t = (v, w, sigma)
        self._cache = (X.u.copy(), np.array(X.p, dtype=np.float64), p2, t)
        return t

    def residual(self, X, p2: float):
        _, _, sigma = self.terms(X, p2)
        return self._vec(residual(self.prob, X.u, self.pvec(self._p1(X), p2)), sigma)

    def residual_dparam(self, X, p2: float, eps=None):
        """dG/dp2 = (dF/dp2, sigma_p2), analytic (the reference differentiates G by finite differences)."""
        v, w, _ = self.terms(X, p2)
        pv = self.pvec(self._p1(X), p2)
        sp2 = self._sigma_p(X.u, pv, self.ipar2, v, w)
        return self._vec(dpF(self.prob, X.u, pv, self.ipar2), sp2)

    def jacobian(self, X, p2: float):
        return _JacobianMinAug(self, X, p2)


@dataclass
class _JacobianMinAug:
    """What jacobian(FoldMAProblem | HopfMAProblem, X, p2) hands to the linear solver: the point (no matrix)."""
    ma: _MinAugProblem
    X: object
    p2: float


def _linsolve_args(J: _JacobianMinAug, rhs):
    """What bk_fold_linsolve and bk_hopf_linsolve take alike: (problem, v, w, params, nparams, outputs dX, pointers of the x
    parts of ``rhs``, pointers of dX); v, w are the cached bordered vectors of the point."""
    P = J.ma
    v, w, _ = P.terms(J.X, J.p2)
    pv = P.pvec(P._p1(J.X), J.p2)
    dX = [J.X.u.similar() for _ in rhs]
    return P, v, w, _carr(pv), len(pv), dX, _vptrs([r.u for r in rhs]), _vptrs(dX)


class _MinAugLinearSolver:
    """The linear solver of a minimally augmented problem; ``_run(J, [rhs...])`` -> (solutions, converged, GMRES iterations).
    ``solve2`` serves both right-hand sides of the BorderingBLS BEC with ONE J \\ dpF solve: three GMRES solves where the
    reference runs four."""

    def __call__(self, J: _JacobianMinAug, rhs, a0=0.0, a1=1.0):
        out, cv, it = self._run(J, [rhs])
        return out[0], cv, it

    def solve2(self, J: _JacobianMinAug, rhs1, rhs2, a0=0.0, a1=1.0):
        out, cv, it = self._run(J, [rhs1, rhs2])
        return out[0], out[1], cv, (it, 0)


@dataclass
class _MinAugBranch:
    """What the records of continuation_fold and continuation_hopf share, one entry per point."""
    p1: list = field(default_factory=list)
    p2: list = field(default_factory=list)
    ds: list = field(default_factory=list)
    itnewton: list = field(default_factory=list)
    itlinear: list = field(default_factory=list)
    residuals: list = field(default_factory=list)
    sol: list = field(default_factory=list)


def _continuation_minaug(P: _MinAugProblem, lin: _MinAugLinearSolver, what: str, br: _MinAugBranch, guess, p2: float, cp, theta,
                         normC, update_minaug_every_step, save_sol, ds_sequence, verbosity, record_x, skipped, describe,
                         stop_after=None, after_record=None) -> bool:
    """PALC on G(X, p2) with a Secant tangent through continuation.newton_palc and BorderingBLS(solver = lin, check_precision =
    false): the two starting points of continuation (Continuation.jl:349-456) by newton on G, step-size control of
    continuation.py or the prescribed ``ds_sequence``.  Every converged point goes into ``br``; its formulation's own fields by
    ``record_x(X, val, tau)`` with val = P.update(...) (a, b renewed) or ``skipped(X)`` when update_minaug_every_step skips it.
    The run ends when ``stop_after(val)`` holds, and True is returned then.  ``after_record(z, z_old, tau, ds, nopt, bls)``
    (optional) sees every recorded step of the loop with the state the next step starts from and the step ``ds`` that led from
    z_old to z (not the one the step-size control chose for the next step); it must leave that state as it is."""
    def record(z, sol, ds_, val, tau):
        record_x(z.u, val, tau)
        br.p2.append(z.p); br.ds.append(ds_)
        br.itnewton.append(sol.itnewton); br.itlinear.append(sol.itlineartot); br.residuals.append(list(sol.residuals))
        if save_sol:
            br.sol.append(z.copy())

    nopt = Cn.NewtonPar(tol=cp.newton_options.tol, max_iterations=cp.newton_options.max_iterations, linsolver=lin)
    bls = BorderingBLS(lin, check_precision=False)
    sol0 = Cn.newton(P, guess, p2, nopt, normC)
    if not sol0.converged:
        raise RuntimeError(f"Newton failed to converge for the initial {what} guess")
    ds = cp.ds if ds_sequence is None else ds_sequence[0]
    p2b = p2 + ds / cp.eta
    sol1 = Cn.newton(P, sol0.u, p2b, nopt, normC)
    if not sol1.converged:
        raise RuntimeError("Newton failed to converge. Required for the computation of the initial tangent")
    z0, z1 = BorderedArray(sol0.u, p2), BorderedArray(sol1.u, p2b)
    tau = Cn.secant_tangent(z1, z0, ds, theta)
    z, z_old = z0.copy(), z0.copy()
    record(z, sol0, ds, P.update(z.u, z.p), tau)
    z_pred = z.copy().add_(tau, ds)
    step = 0
    while step < cp.max_steps and (cp.p_min < z.p < cp.p_max or step == 0):
        it0 = P.itlinear
        sol = Cn.newton_palc(P, z, tau, z_pred, ds, theta, bls, nopt, cp.p_min, cp.p_max, normC)
        sol.itlineartot += P.itlinear - it0
        if verbosity:
            print(f"{what.lower()} step {step:3d} ds={ds:+.3e} p2={sol.u.p:+.8f} {describe(sol.u.u)} conv={sol.converged} "
                  f"itnewton={sol.itnewton} itlinear={sol.itlineartot}")
        if sol.converged:
            z_old.copyto_(z)
            z.copyto_(sol.u)
            step += 1
        if ds_sequence is not None:
            if not sol.converged:
                raise RuntimeError(f"{what} continuation step {step} did not converge with the prescribed ds")
            ds_next, stop = (ds_sequence[step] if step < len(ds_sequence) else ds), step >= len(ds_sequence)
        else:
            ds_next, stop = Cn.step_size_control(ds, sol.converged, sol.itnewton, cp)
        if sol.converged:
            tau = Cn.secant_tangent(z, z_old, ds_next, theta)
            val = P.update(z.u, z.p) if Cn.mod_counter(step, update_minaug_every_step) else skipped(z.u)
            record(z, sol, ds, val, tau)
            if after_record is not None:
                after_record(z, z_old, tau, ds, nopt, bls)
            if stop_after is not None and stop_after(val):
                return True
        ds = ds_next
        if stop:
            break
        z_pred = z.copy().add_(tau, ds)
    return False


# ------------------------------------------------------------------------------------------ fold point guesses
def _saved(br, i):
    """(x, p) of the i-th recorded point of a branch from continuation.continuation (save_sol = True: one vector per point;
    save_sol_every_step: dicts with the step number)."""
    for s in br.sol:
        if isinstance(s, dict) and s["step"] == i:
            return s["x"], s["p"]
    if len(br.sol) == len(br.param) and not isinstance(br.sol[i], dict):
        return br.sol[i], br.param[i]
    raise ValueError(f"the branch kept no solution for point {i} (continuation(..., save_sol=True))")


def fold_point(br, ind: int, normN=Cn.norm2):
    """fold_point(br, index) (:6-13) and the start vector of newton_fold(br, ind) (:246-247): the branch records a fold guess
    (continuation.locate_fold) without state or tangent, so both come from the saved solutions -- x and p of the middle point
    of the three whose parameter turned, tau = the difference of its neighbours.  Returns (BorderedArray(x, p), zeta) with
    zeta = tau.u / normN(tau.u)."""
    sp = br.specialpoint[ind]
    if sp.get("type") not in ("bp", "nd", "fold"):
        raise ValueError(f"This should be a Fold / BP point.\nYou passed a {sp.get('type')} point.")
    i = sp["idx"]
    x, p = _saved(br, i)
    xl, _ = _saved(br, i - 1)
    xr, _ = _saved(br, i + 1)
    tau = xr.copy().add_(xl, -1.0)
    return BorderedArray(x.copy(), float(p)), tau.scale_(1.0 / normN(tau))


def start_vector_eigen(prob, x: HipVec, p: float, eig):
    """start_with_eigen = true (:251-266): the eigenvector of the eigenvalue of J(x, p) nearest 0 (e.g. ShiftInvert(sigma = 0)
    with ``save_vectors``); J' = J for the problems here, so it serves as a and b."""
    vals, vecs, _, _ = eig(prob.jacobian(x, p), 4)
    k = int(np.argmin(np.abs(np.asarray(vals))))
    z = vecs[k][0].copy()
    return z.scale_(1.0 / z.norm())


# ------------------------------------------------------------------------------------------ newton_fold
def newton_fold(prob, x0: HipVec, p0: float, a: HipVec, b: HipVec, ls: _GMRES, bls: BorderingBLS | MatrixFreeBLS | None = None,
                tol=1e-12, max_iterations=25, norm_inf=False):
    """newton_fold (:211-233) with FoldLinearSolverMinAug under _newton (src/Newton.jl:66-114), call by call on the plugin
    surface: the residual (:16-38) solves bls(J, a, b, 0, 0, 1) for (v, sigma) and bls(J', b, a, 0, 0, 1) for w (no second
    solve when ``a is b``: J' = J); each Newton step is foldMALinearSolver's usehessian branch (:146-164) with ls(J, F, dpF),
    d2F + inner for sigma_x and dJ/dp v + inner for sigma_p.  v, w of a point serve its residual and its step.

    ``bls = MatrixFreeBLS(ls, use_pl=True)``: the same two calls of the residual go to the preconditioned bordered solver, and each
    Newton step is the branch without ``usehessian`` (:136-145): sigma_x as a vector (fold_border) and ONE solve
    bls(J, dpF, sigma_x, sigma_p, F, sigma) -- regular at the fold, where J \\ F is not."""
    bls = bls if bls is not None else BorderingBLS(ls, check_precision=False)
    bordered = _bordered_path(bls)
    ipar = prob.ipar
    x, p = x0.copy(), float(p0)
    itlin, bad = 0, 0

    def point():
        nonlocal itlin, bad
        J = prob.jacobian(x, p)
        zero = x.zerovector()
        v, sigma, cv, itv = bls(J, a, b, 0.0, zero, 1.0)
        itlin += int(np.sum(itv))
        if a is b:
            w = v
        else:
            w, _, cv2, itw = bls(J, b, a, 0.0, zero, 1.0)      # J' = J (:79-84)
            itlin += int(np.sum(itw))
            cv = cv and cv2
        bad += 0 if cv else 1
        F = prob.residual(x, p)
        return F, sigma, v, w

    def update(F, sigma, v, w):
        nonlocal p, itlin, bad
        pars = prob._pvec(p)
        J = prob.jacobian(x, p)
        if bordered:
            sigx, sp = fold_border(prob, x, pars, ipar, v, w)
            dX, dsig, cv, it = bls(J, dpF(prob, x, pars, ipar), sigx, sp, F, sigma)
            itlin += int(it)
            bad += 0 if cv else 1
            x.add_(dX, -1.0)
            p -= dsig
            return
        x1, x2, cv, it = _solve2(ls, J, F, dpF(prob, x, pars, ipar))
        itlin += int(np.sum(it))
        bad += 0 if cv else 1
        sx1 = -w.inner(d2F(prob, x, pars, x1, v))
        sx2 = -w.inner(d2F(prob, x, pars, x2, v))
        sp = -w.inner(dJdp(prob, x, pars, ipar, v))
        dsig = (sigma - sx1) / (sp - sx2)
        dX = x1.copy().add_(x2, -dsig)
        x.add_(dX, -1.0)
        p -= dsig

    (F, sigma, v, w), res, step = _newton_minaug_mirror(point, update, lambda F, sg: _norm_fold(F, sg, norm_inf), tol,
                                                        max_iterations)
    return dict(u=BorderedArray(x, p), converged=res[-1] < tol, itnewton=step, itlineartot=itlin, residuals=res, v=v,
                w=w.copy() if w is v else w, sigma=sigma, unconverged_solves=bad)


def newton_fold_native(prob, x0: HipVec, p0: float, a: HipVec, b: HipVec, ls: _GMRES,
                       bls: BorderingBLS | MatrixFreeBLS | None = None, tol=1e-12, max_iterations=25, norm_inf=False, callback=None):
    """The same as one library call (bk_newton_fold); with ``bls = MatrixFreeBLS(ls, use_pl=True)`` under the context option
    fold_bordered = 1, set and put back around the call."""
    bls = bls if bls is not None else BorderingBLS(ls, check_precision=False)
    ctx = prob.ctx
    x = x0.copy()
    p = C.c_double(float(p0))
    pv = prob._pvec(p0)
    v, w = x.similar(), x.similar()
    sigma = C.c_double()
    no = newton_opts(tol, max_iterations, norm_inf, callback=callback)
    bo, lo = _bls_opts(bls), ls._opts()
    res = L.NewtonResult()
    bad0 = ctx.get_option("fold_unconverged_solves")
    with _fold_bordered(ctx, _bordered_path(bls)):
        ctx.check(ctx.lib.bk_newton_fold(ctx.h, prob.h, _ptr(x.t), C.byref(p), _carr(pv), len(pv), prob.ipar, _ptr(a.t), _ptr(b.t),
                                         C.byref(no), C.byref(bo), C.byref(lo), ls._pl(), _ptr(v.t), _ptr(w.t), C.byref(sigma),
                                         C.byref(res)), "bk_newton_fold")
    return dict(u=BorderedArray(x, p.value), converged=bool(res.converged), itnewton=res.itnewton, itlineartot=res.itlinear,
                residuals=[res.residuals[i] for i in range(res.itnewton + 1)], v=v, w=w, sigma=sigma.value,
                unconverged_solves=int(ctx.get_option("fold_unconverged_solves") - bad0))


# ------------------------------------------------------------------------------------------ the fold problem G(X, p2)
def fold_terms(prob, x: HipVec, pars, ipar: int, a: HipVec, b: HipVec, ls: _GMRES, bls: BorderingBLS | MatrixFreeBLS):
    """bk_fold_terms: (v, w, sigma, converged, (itv, itw)); w is v itself when ``a is b`` (J' = J: no second solve).  With
    ``bls = MatrixFreeBLS(ls, use_pl=True)`` each of (v, sigma) and w is ONE preconditioned bordered solve (option fold_bordered)."""
    ctx = prob.ctx
    v = x.similar()
    w = v if a is b else x.similar()
    sigma, cv = C.c_double(), C.c_int()
    it = (C.c_int * 2)()
    bo, lo = _bls_opts(bls), ls._opts()
    with _fold_bordered(ctx, _bordered_path(bls)):
        ctx.check(ctx.lib.bk_fold_terms(ctx.h, prob.h, _ptr(x.t), _carr(pars), len(pars), int(ipar), _ptr(a.t), _ptr(b.t),
                                        C.byref(bo), C.byref(lo), ls._pl(), _ptr(v.t), _ptr(w.t), C.byref(sigma), None, C.byref(cv),
                                        it), "bk_fold_terms")
    return v, w, sigma.value, bool(cv.value), (it[0], it[1])


class FoldProblem(_MinAugProblem):
    """FoldMinimallyAugmentedFormulation(prob, a, b, ...) + FoldMAProblem with lens2 (src/codim2/MinAugFold.jl,
    continuation_fold :407-453): unknown X = BorderedArray(x, p1), the bordered vectors from bk_fold_terms."""

    def __init__(self, prob, lens2: str, a: HipVec, b: HipVec, ls: _GMRES, bls: BorderingBLS | MatrixFreeBLS | None = None):
        super().__init__(prob, lens2, a, b, ls)
        self.bls = bls if bls is not None else BorderingBLS(ls, check_precision=False)
        self.bordered = _bordered_path(self.bls)     # MatrixFreeBLS(ls, use_pl=True): bordered vectors AND linear solver on that path

    _p1 = staticmethod(lambda X: X.p)
    _vec = staticmethod(BorderedArray)
    keep_vw = False                                 # detection on: update keeps the bordered vectors of the point in last_vw
    last_vw = None

    def _solve_terms(self, X: BorderedArray, p2: float):
        return fold_terms(self.prob, X.u, self.pvec(X.p, p2), self.ipar1, self.a, self.b, self.ls, self.bls)

    def _sigma_p(self, x, pv, ipar, v, w):
        """-<w, dJ/dp v>"""
        return fold_contract(self.prob, x, pv, ipar, v, w)[1]

    def update(self, X: BorderedArray, p2: float):
        """update!(probma, iter, state) (:280-313) after a converged step: a = w/|w|, b = v/|v| from the bordered vectors of the
        new point; returns BT = <zeta*, zeta> with zeta = v/|v|, zeta* = w/|w| (test_bt_cusp, :551-576)."""
        v, w, _ = self.terms(X, p2)
        zs = w.copy().scale_(1.0 / w.norm())
        z = zs if w is v else v.copy().scale_(1.0 / v.norm())
        bt = zs.inner(z)
        self.a = zs
        self.b = zs if w is v else z
        self._cache = None
        if self.keep_vw:
            self.last_vw = (v, w, p2)               # the null vectors of the point: b2 reuses them
        return bt


class FoldLinearSolverMinAug(_MinAugLinearSolver):
    """FoldLinearSolverMinAug (:168-178) -> foldMALinearSolver as bk_fold_linsolve: the usehessian branch (:146-164), or -- for a
    FoldProblem built with MatrixFreeBLS(ls, use_pl=True) -- the full system [J dpF; sigma_x' sigma_p] (:136-145), one
    preconditioned bordered solve per right-hand side (option fold_bordered)."""

    def _run(self, J: _JacobianMinAug, rhs):
        F, v, w, arr, npar, dX, ru, dxp = _linsolve_args(J, rhs)
        ctx, m = F.ctx, len(rhs)
        rp = (C.c_double * m)(*[float(r.p) for r in rhs])
        ds = (C.c_double * m)()
        cv, it = C.c_int(), C.c_int()
        lo = F.ls._opts()
        with _fold_bordered(ctx, getattr(F, "bordered", False)):
            ctx.check(ctx.lib.bk_fold_linsolve(ctx.h, F.prob.h, _ptr(J.X.u.t), arr, npar, F.ipar1, _ptr(v.t), _ptr(w.t), m, ru, rp,
                                               C.byref(lo), F.ls._pl(), dxp, ds, C.byref(cv), C.byref(it)), "bk_fold_linsolve")
        return [BorderedArray(dX[k], ds[k]) for k in range(m)], bool(cv.value), it.value


JacobianFold = _JacobianMinAug


# ------------------------------------------------------------------------------------------ continuation_fold
@dataclass
class FoldBranch(_MinAugBranch):
    """The record of continuation_fold (record_from_solution, :330-346): p1 (lens1), p2 (lens2), BT, CP per point; with
    detect_codim2 > 0 also b2 = <p, B(q, q)> per point (the quadratic coefficient of the fold, zero at a cusp) and the points
    where CP changed sign in ``specialpoint`` (type "cusp").

    A special point carries type, idx, step, p1, p2 (the point: the one after the crossing, or the located one), ``end_points``
    = the (p1, p2) of the two states the sign change lies between, CP and CP_interval (the event there), b2, x = the state
    BorderedArray(x, p1), a, b, bisection_steps, n_inversion, status, reach (what the point can be off by along the curve, in
    PALC arclength: the ds of the last step that passed the sign change).  ``end_points`` is NOT a bracket of the point in p2: a
    cusp is an extremum of p2 along the curve, so the p2 of both end states lie on the same side of it -- the point lies between
    them along the curve (in arclength), not between their parameter values.

    CP = tau.p2 changes sign at every turning point of the curve in p2.  Where b2 vanishes with it the point is a cusp; where
    b2 != 0 it is <p, dF/dp1> that vanishes instead (the fold curve turns without the fold degenerating).  The reference labels
    both :cusp (codim2.jl:559-570); so does this record, and b2 tells them apart."""
    BT: list = field(default_factory=list)
    CP: list = field(default_factory=list)
    b2: list = field(default_factory=list)
    specialpoint: list = field(default_factory=list)
    lens2: str | None = None


def _norminf_fold(z):
    return _nanmax(z.u.norminf(), abs(z.p))


def cusp_dots(prob, x: HipVec, pars, v: HipVec, w: HipVec):
    """One pass that writes nothing (bk_cusp_dots): (<w, d2F(x)[v, v]>, <v, v>, <w, w>, <v, w>)."""
    ctx = prob.ctx
    out = (C.c_double * 4)()
    ctx.check(ctx.lib.bk_cusp_dots(prob.h, _ptr(x.t), _carr(pars), len(pars), _ptr(v.t), _ptr(w.t), out), "bk_cusp_dots")
    return out[0], out[1], out[2], out[3]


def cusp_b2(prob, x: HipVec, pars, v: HipVec, w: HipVec) -> float:
    """b2 = <p, B(q, q)> with q = v / |v|, p = w / <q, w> from the unnormalised bordered vectors v, w of a fold-curve point:
    <w, B(v, v)> / (|v| <v, w>), one cusp_dots pass and no vector written."""
    d = cusp_dots(prob, x, pars, v, w)
    return d[0] / (math.sqrt(d[1]) * d[3])


def continuation_fold(prob, fold_guess: BorderedArray, p2: float, lens2: str, a: HipVec, b: HipVec, ls: _GMRES,
                      cp: Cn.ContinuationPar, theta=0.5, norm_inf=True, update_minaug_every_step=1, save_sol=False,
                      ds_sequence=None, verbosity=0, bls: BorderingBLS | MatrixFreeBLS | None = None,
                      detect_codim2=0) -> FoldBranch:
    """continuation_fold(prob, alg = PALC(tangent = Secant()), foldpointguess, par, lens1, lens2, a, b, options_cont) (:369-453):
    PALC on G(X, p2) through continuation.newton_palc with BorderingBLS(solver = FoldLinearSolverMinAug(), check_precision =
    false) (:445-453), Secant tangent only (the reference warns against Bordered on folds, :390-392), the two starting points of
    continuation (Continuation.jl:349-456) by newton on G, step-size control of continuation.py.  After every converged step a, b
    are updated (update_minaug_every_step = 1) and BT, CP recorded.  ``ds_sequence`` (optional) replaces the step-size control by
    a fixed list of steps (comparisons with a restatement).
    ``bls`` (optional): the bordered solver of the formulation's OWN solves -- MatrixFreeBLS(ls, use_pl=True) runs the bordered
    vectors and the fold linear solver on the preconditioned bordered system; the outer PALC solve stays BorderingBLS over the fold
    linear solver, as in the reference (:449).

    ``detect_codim2`` (the test_bt_cusp event, :432, :551-576, with the semantics of continuation_hopf): 0 locates nothing and
    issues exactly the library calls of the plain curve.  1: after every converged step b2 of the new point is recorded from the
    bordered vectors the step solved (cusp_b2: one reducing pass), and every sign change of CP between consecutive points goes
    to br.specialpoint as type "cusp" with status "guess".  2: each sign change is bisected along the curve (_locate_event; the
    event is the p2 component of the orientation-keeping secant tangent) and the special point keeps the located state; the
    curve continues from the state it had before the bisection, so the recorded points are those of detect_codim2 = 1.  The
    secant of a point spans the step that led to it, so a sign change of CP between the points i - 1 and i places the extremum
    of p2 between the points i - 2 and i: the bisection is handed that bracket and the sum of the two steps (the loop itself is
    the one the Hopf curve uses); as the bisection states close in, their secant becomes the local tangent.  See
    FoldBranch for the fields of a special point, for why its ``end_points`` are no bracket in p2, and for the sign changes of CP
    with b2 != 0.  Bogdanov-Takens and zero-Hopf points are not located."""
    br = FoldBranch(lens2=lens2)
    P = FoldProblem(prob, lens2, a, b, ls, bls)
    P.keep_vw = bool(detect_codim2)
    if detect_codim2 and update_minaug_every_step != 1:
        raise ValueError("detect_codim2 needs the bordered vectors of every point (update_minaug_every_step = 1)")
    normC = _norminf_fold if norm_inf else (lambda z: z.norm())

    def b2_at(X, vw):
        v, w, p2_ = vw
        return cusp_b2(prob, X.u, P.pvec(X.p, p2_), v, w)

    def record_x(X, bt, tau):
        br.p1.append(X.p); br.BT.append(bt); br.CP.append(tau.p)
        if detect_codim2:
            with _solver_state_kept(prob.ctx):
                br.b2.append(b2_at(X, P.last_vw))

    def coords(s):
        return (float(s.u.p), float(s.p))

    before = []                                     # (z_old, ds) of the previous step: the state two points back

    def after_record(z, z_old, tau, ds_taken, nopt, bls_):
        # record() has appended the point: CP[-1] belongs to z, CP[-2] to z_old.  CP of a point is the secant over the step that
        # led to it, so a sign change between the points i - 1 and i puts the extremum of p2 between the points i - 2 and i:
        # the bisection starts from that bracket, with the two steps that span it
        z_far, ds_far = before.pop() if before else (z_old, 0.0)
        if detect_codim2 > 1:
            before.append((z_old.copy(), ds_taken))
        if len(br.CP) < 2 or not _sign_change(br.CP[-2], br.CP[-1]):
            return
        i = len(br.CP) - 1
        sp = dict(type="cusp", idx=i, step=i, p1=float(z.u.p), p2=float(z.p), end_points=(coords(z_old), coords(z)),
                  CP=br.CP[-1], CP_interval=(br.CP[-2], br.CP[-1]), b2=br.b2[-1], x=z.u.copy(), a=P.a, b=P.b, bisection_steps=0,
                  n_inversion=0, status="guess", reach=abs(ds_taken))
        if detect_codim2 > 1:
            b2 = [br.b2[-1]]

            def event(zc, tau_b, previous):
                # the corrector's last residual left the bordered vectors of zc in the cache: b2 costs one reducing pass
                v, w, _ = P.terms(zc.u, zc.p)
                b2[0] = b2_at(zc.u, (v, w, zc.p))
                return float(tau_b.p)

            with _solver_state_kept(prob.ctx):
                r = _locate_event(P, z, z_far, tau, ds_taken + ds_far, br.CP[-1], event, coords, cp, theta, nopt, bls_, normC)
            zc, vals = r["z"], [br.CP[-2] if v != v else v for v in r["values"]]
            sp.update(p1=float(zc.u.p), p2=float(zc.p), end_points=tuple(r["ends"]), CP=r["value"], CP_interval=tuple(vals),
                      b2=b2[0], x=zc.u.copy(), bisection_steps=r["bisection_steps"], n_inversion=r["n_inversion"],
                      status=r["status"], reach=r["reach"])
        br.specialpoint.append(sp)

    _continuation_minaug(P, FoldLinearSolverMinAug(), "fold", br, fold_guess, p2, cp, theta, normC, update_minaug_every_step,
                         save_sol, ds_sequence, verbosity, record_x, skipped=lambda X: float("nan"),
                         describe=lambda X: f"p1={X.p:+.8f}", after_record=after_record if detect_codim2 else None)
    return br


# ================================================================================================== Hopf points
# The minimally augmented Hopf formulation of src/codim2/MinAugHopf.jl, matrix-free, for CGL2d (the one problem here whose
# Jacobian is not symmetric):
#
#   HopfVec                  the unknown X = (x, [p1, omega]); BorderedArray holds a scalar p only
#   HopfProblem              HopfMinimallyAugmentedFormulation + HopfMAProblem: G(X, p2) = (F(x, p1), Re sigma, Im sigma)
#   HopfLinearSolverMinAug   _hopf_MA_linear_solver, usehessian branch: one or two right-hand sides, one shared J \ dpF
#   hopf_point               hopf_point(br, ind) on a native branch record (save_sol = True)
#   hopf_start_vectors       the reference's default start vectors (random a, b, then the bordered vectors) or, with an
#                            eigensolver, start_with_eigen (zeta from the eigensolver, zeta* from the adjoint bordered solve)
#   newton_hopf              newton_hopf written out call by call (BorderingBLS.solve_complex, bk_gmres2, hopf_contract)
#   newton_hopf_native       the same as one library call (bk_newton_hopf)
#   continuation_hopf        PALC on G(X, p2), Secant tangent, BorderingBLS(HopfLinearSolverMinAug, check_precision = false),
#                            a / b updated after every step, stop at |omega| < 100 tol (threshBT of update!); detect_codim2 = 1 | 2:
#                            the first Lyapunov coefficient per point, its sign changes as "gh" points, bisected (_locate_gh)
#
# Complex device vectors are (re, im) pairs of HipVecs.  With w^H a = 1:  sigma_x . dx = -w^H d2F[v, dx],
# sigma_p = -w^H dJ/dp v, sigma_omega = i w^H v.
class HopfVec:
    """(u, p) with p = [p1, omega]: the VectorInterface subset PALC and the bordered solvers use."""
    __slots__ = ("u", "p")

    def __init__(self, u, p):
        self.u = u
        self.p = np.array(p, dtype=np.float64).reshape(2)

    def copy(self):
        return HopfVec(self.u.copy(), self.p.copy())

    def zerovector(self):
        return HopfVec(self.u.zerovector(), np.zeros(2))

    def copyto_(self, src):
        self.u.copyto_(src.u)
        self.p[:] = src.p
        return self

    def scale_(self, a):
        self.u.scale_(a)
        self.p *= a
        return self

    def add_(self, x, a=1.0, b=1.0):
        self.u.add_(x.u, a, b)
        self.p = b * self.p + a * x.p
        return self

    def inner(self, y):
        return self.u.inner(y.u) + float(self.p @ y.p)

    def norm(self):
        return math.sqrt(self.u.norm() ** 2 + float(self.p @ self.p))

    def norminf(self):
        return _nanmax(self.u.norminf(), *np.abs(self.p))

    def __len__(self):
        return len(self.u) + 2


def _cptr(z):
    return _ptr(z.t) if z is not None else None


def cnorm(z):
    """|z| of a complex (re, im) pair."""
    re, im = z
    return math.sqrt(re.norm() ** 2 + (im.norm() ** 2 if im is not None else 0.0))


def cinner(x, y):
    """x^H y of (re, im) pairs (VI.inner on complex vectors)."""
    (xr, xi), (yr, yi) = x, y
    re = xr.inner(yr) + (xi.inner(yi) if xi is not None and yi is not None else 0.0)
    im = (xr.inner(yi) if yi is not None else 0.0) - (xi.inner(yr) if xi is not None else 0.0)
    return complex(re, im)


def _cscale(z, c: complex):
    """c z for a complex pair, as a new pair."""
    re, im = z
    im = im if im is not None else re.zerovector()
    return (re.copy().scale_(c.real).add_(im, -c.imag), im.copy().scale_(c.real).add_(re, c.imag))


def hopf_d2F(prob, x: HipVec, pars, dx1: HipVec, dx2: HipVec) -> HipVec:
    """d2F(x)[dx1, dx2] of CGL2d for real dx1, dx2 (bk_hopf_d2f)."""
    return _into_similar(prob, "bk_hopf_d2f", x, pars, _ptr(dx1.t), _ptr(dx2.t))


def hopf_dJdp(prob, x: HipVec, pars, ipar: int, dx: HipVec) -> HipVec:
    """dJ/dp(x) dx of CGL2d for params[ipar] (bk_hopf_djdp)."""
    return _into_similar(prob, "bk_hopf_djdp", x, pars, int(ipar), _ptr(dx.t))


def hopf_contract(prob, x: HipVec, pars, ipar: int, v, w, X=()):
    """One fused pass (bk_hopf_contract): ([w^H d2F(x)[v, X_k] for X_k in X], w^H dJ/dp v, w^H v) as complex numbers."""
    ctx = prob.ctx
    m = len(X)
    xp = _vptrs(X)
    out = (C.c_double * (2 * (m + 2)))()
    ctx.check(ctx.lib.bk_hopf_contract(prob.h, _ptr(x.t), _carr(pars), len(pars), int(ipar), _ptr(v[0].t), _ptr(v[1].t),
                                       _ptr(w[0].t), _ptr(w[1].t), m, xp, out), "bk_hopf_contract")
    z = [complex(out[2 * k], out[2 * k + 1]) for k in range(m + 2)]
    return z[:m], z[m], z[m + 1]


def hopf_terms(prob, x: HipVec, pars, ipar: int, omega: float, a, b, ls: _GMRES, bls: BorderingBLS | MatrixFreeBLS | None = None):
    """bk_hopf_terms: (v, w, sigma, sigma_p, sigma_omega, converged, (itv, itw)); v, w as (re, im) pairs.  With
    ``bls = MatrixFreeBLS(ls, use_pl=True)`` each of (v, sigma) and w is ONE preconditioned bordered solve (option hopf_bordered)."""
    ctx = prob.ctx
    vr, vi, wr, wi = x.similar(), x.similar(), x.similar(), x.similar()
    sg, spp, sw = (C.c_double * 2)(), (C.c_double * 2)(), (C.c_double * 2)()
    cv = C.c_int()
    it = (C.c_int * 2)()
    lo = ls._opts()
    with _hopf_bordered(ctx, _hopf_bordered_path(bls)):
        ctx.check(ctx.lib.bk_hopf_terms(ctx.h, prob.h, _ptr(x.t), _carr(pars), len(pars), int(ipar), float(omega), _cptr(a[0]),
                                        _cptr(a[1]), _cptr(b[0]), _cptr(b[1]), C.byref(lo), ls._pl(), _ptr(vr.t), _ptr(vi.t),
                                        _ptr(wr.t), _ptr(wi.t), sg, spp, sw, C.byref(cv), it), "bk_hopf_terms")
    return ((vr, vi), (wr, wi), complex(sg[0], sg[1]), complex(spp[0], spp[1]), complex(sw[0], sw[1]), bool(cv.value),
            (it[0], it[1]))


def _hopf_2x2(S1: complex, S2: complex, P: complex, Q: complex, rp: float, rw: float):
    """(dp, domega) of (sigma_p + S2) dp + sigma_omega domega = (rp + i rw) + S1 with sigma_p = -P, sigma_omega = i Q: the same
    2 x 2 real system and operation order as bk_hopf_linsolve."""
    spr, spi = -P.real, -P.imag
    swr, swi = -Q.imag, Q.real
    a11, a12, a21, a22 = spr + S2.real, swr, spi + S2.imag, swi
    det = a11 * a22 - a12 * a21
    b1, b2 = rp + S1.real, rw + S1.imag
    return (b1 * a22 - a12 * b2) / det, (a11 * b2 - a21 * b1) / det


def _norm_hopf(F, sigma: complex, norm_inf):
    if norm_inf:
        return _nanmax(F.norminf(), abs(sigma.real), abs(sigma.imag))
    return math.sqrt(F.norm() ** 2 + sigma.real ** 2 + sigma.imag ** 2)


# ------------------------------------------------------------------------------------------ Hopf point guesses
def hopf_point(br, ind: int) -> HopfVec:
    """hopf_point(br, index) (MinAugHopf.jl:6-13) on a branch of continuation.continuation_native(..., bisection = True,
    save_sol = True): x = the saved (bisected) state of the special point, p its parameter, omega = |Im lambda| of the pair that
    crossed, i.e. of the eigenvalue with non-zero imaginary part nearest the imaginary axis in br.eig of that point."""
    sp = br.specialpoint[ind]
    if sp.get("type") != "hopf":
        raise ValueError("The provided index does not refer to a Hopf point")
    i = sp["step"]
    x, p = _saved(br, i)
    vals = np.asarray(br.eig[i])
    cand = vals[np.abs(vals.imag) > 0]
    if cand.size == 0:
        raise ValueError("no complex eigenvalue recorded at the Hopf point")
    lam = cand[np.argmin(np.abs(cand.real))]
    return HopfVec(x.copy(), [float(sp["param"]), abs(float(lam.imag))])


def hopf_start_vectors(prob, X: HopfVec, ls: _GMRES, eig=None, nev=4, seed=0, bls=None):
    """(a, b) for newton_hopf / continuation_hopf at the guess X.  Default (continuation_hopf, :566-585): random complex a, b, then
    the bordered vectors of the guess, a = w/|w|, b = v/|v|.  With an eigensolver (start_with_eigen): b = zeta, the eigenvector
    of J(x, p) whose eigenvalue lambda is nearest i omega (``save_vectors``), a = zeta* from the adjoint bordered solve, scaled so
    that a^H b = 1.  The eigensolver keeps one (re, im) pair per conjugate pair; which member it describes is checked on J itself:
    J zr = Re(lambda) zr - Im(lambda) zi holds for the eigenvector of lambda, J zr = Re(lambda) zr + Im(lambda) zi for its
    conjugate, whose imaginary part is then negated.  ``bls``: as in hopf_terms."""
    x, (p, omega) = X.u, X.p
    pv = prob._pvec(p)
    if eig is None:
        rng = np.random.default_rng(seed)
        n = x.n
        a = tuple(HipVec.from_numpy(prob.ctx, rng.random(n), x.nglobal) for _ in range(2))
        b = tuple(HipVec.from_numpy(prob.ctx, rng.random(n), x.nglobal) for _ in range(2))
        v, w, *_ = hopf_terms(prob, x, pv, prob.ipar, omega, a, b, ls, bls)
        return _cscale(w, 1.0 / cnorm(w)), _cscale(v, 1.0 / cnorm(v))
    J = prob.jacobian(x, p)
    vals, vecs, _, _ = eig(J, nev)
    if vecs is None:
        raise ValueError("start_with_eigen needs the eigenvectors (an eigensolver with save_vectors = True)")
    k = int(np.argmin(np.abs(np.asarray(vals) - 1j * omega)))
    lam = complex(vals[k])
    zr, zi = vecs[k]
    zeta = (zr.copy(), zi.copy() if zi is not None else zr.zerovector())
    Jzr = J(zeta[0])
    own = Jzr.copy().add_(zeta[0], -lam.real).add_(zeta[1], lam.imag).norm()          # J zr - (Re l zr - Im l zi)
    conj = Jzr.add_(zeta[0], -lam.real).add_(zeta[1], -lam.imag).norm()               # J zr - (Re l zr + Im l zi)
    if conj < own:
        zeta[1].scale_(-1.0)
    zeta = _cscale(zeta, 1.0 / cnorm(zeta))
    _, w, *_ = hopf_terms(prob, x, pv, prob.ipar, omega, zeta, zeta, ls, bls)
    c = cinner(w, zeta)
    return _cscale(w, 1.0 / c.conjugate()), zeta


# ------------------------------------------------------------------------------------------ newton_hopf
def newton_hopf(prob, X0: HopfVec, a, b, ls: _GMRES, tol=1e-12, max_iterations=25, norm_inf=False,
                bls: BorderingBLS | MatrixFreeBLS | None = None):
    """newton_hopf with HopfLinearSolverMinAug under _newton (src/Newton.jl:66-114), call by call on the plugin surface: the
    residual solves bls(J, a, b, 0, 0, 1; shift = -i omega) for (v, sigma) and bls(J', b, a, 0, 0, 1; shift = +i omega) for w
    (BorderingBLS.solve_complex); each Newton step is _hopf_MA_linear_solver's usehessian branch with ls(J, F, dpF) (bk_gmres2)
    and one hopf_contract pass for S(x1), S(x2), w^H dJ/dp v and w^H v.  v, w of a point serve its residual and its step.

    ``bls = MatrixFreeBLS(ls, use_pl=True)``: the same two calls of the residual go to the preconditioned bordered solver
    (MatrixFreeBLS.solve_complex), regular at the Hopf point, where J - i omega is not.  The Newton step is unchanged: J itself is
    regular there."""
    if not _hopf_bordered_path(bls):
        bls = BorderingBLS(ls, check_precision=False)
    ipar = prob.ipar
    x, p, om = X0.u.copy(), float(X0.p[0]), float(X0.p[1])
    itlin, bad = 0, 0

    def point():
        nonlocal itlin, bad
        J, Jt = prob.jacobian(x, p), prob.jacobian_adjoint(x, p)
        zero = x.zerovector()
        v, sigma, cv, itv = bls.solve_complex(J, a, b, 0.0, (zero, None), 1.0, shift=complex(0.0, -om))
        w, _, cv2, itw = bls.solve_complex(Jt, b, a, 0.0, (zero, None), 1.0, shift=complex(0.0, om))
        itlin += int(np.sum(itv)) + int(np.sum(itw))
        bad += 0 if (cv and cv2) else 1
        return prob.residual(x, p), sigma, v, w

    def update(F, sigma, v, w):
        nonlocal p, om, itlin, bad
        pars = prob._pvec(p)
        J = prob.jacobian(x, p)
        x1, x2, cv, it = _solve2(ls, J, F, dpF(prob, x, pars, ipar))
        itlin += int(np.sum(it))
        bad += 0 if cv else 1
        (S1, S2), P, Q = hopf_contract(prob, x, pars, ipar, v, w, [x1, x2])
        dp, dw = _hopf_2x2(S1, S2, P, Q, sigma.real, sigma.imag)
        x1.add_(x2, -dp)
        x.add_(x1, -1.0)
        p -= dp
        om -= dw

    (F, sigma, v, w), res, step = _newton_minaug_mirror(point, update, lambda F, sg: _norm_hopf(F, sg, norm_inf), tol,
                                                        max_iterations)
    return dict(u=HopfVec(x, [p, om]), converged=res[-1] < tol, itnewton=step, itlineartot=itlin, residuals=res, v=v, w=w,
                sigma=sigma, unconverged_solves=bad)


def newton_hopf_native(prob, X0: HopfVec, a, b, ls: _GMRES, tol=1e-12, max_iterations=25, norm_inf=False, callback=None,
                       bls: BorderingBLS | MatrixFreeBLS | None = None):
    """The same as one library call (bk_newton_hopf); with ``bls = MatrixFreeBLS(ls, use_pl=True)`` under the context option
    hopf_bordered = 1, set and put back around the call."""
    ctx = prob.ctx
    x = X0.u.copy()
    p, om = C.c_double(float(X0.p[0])), C.c_double(float(X0.p[1]))
    pv = prob._pvec(p.value)
    vr, vi, wr, wi = x.similar(), x.similar(), x.similar(), x.similar()
    sigma = (C.c_double * 2)()
    no = newton_opts(tol, max_iterations, norm_inf, callback=callback)
    lo = ls._opts()
    res = L.NewtonResult()
    bad0 = ctx.get_option("hopf_unconverged_solves")
    with _hopf_bordered(ctx, _hopf_bordered_path(bls)):
        ctx.check(ctx.lib.bk_newton_hopf(ctx.h, prob.h, _ptr(x.t), C.byref(p), C.byref(om), _carr(pv), len(pv), prob.ipar,
                                         _cptr(a[0]), _cptr(a[1]), _cptr(b[0]), _cptr(b[1]), C.byref(no), C.byref(lo), ls._pl(),
                                         _ptr(vr.t), _ptr(vi.t), _ptr(wr.t), _ptr(wi.t), sigma, C.byref(res)), "bk_newton_hopf")
    return dict(u=HopfVec(x, [p.value, om.value]), converged=bool(res.converged), itnewton=res.itnewton,
                itlineartot=res.itlinear, residuals=[res.residuals[i] for i in range(res.itnewton + 1)], v=(vr, vi), w=(wr, wi),
                sigma=complex(sigma[0], sigma[1]),
                unconverged_solves=int(ctx.get_option("hopf_unconverged_solves") - bad0))


# ------------------------------------------------------------------------------------------ the Hopf problem G(X, p2)
class HopfProblem(_MinAugProblem):
    """HopfMinimallyAugmentedFormulation(prob, a, b, ...) + HopfMAProblem with lens2: unknown X = HopfVec(x, [p1, omega]), a, b,
    v, w complex (re, im) pairs, the bordered vectors from bk_hopf_terms."""

    _p1 = staticmethod(lambda X: X.p[0])
    _vec = staticmethod(lambda u, s: HopfVec(u, [s.real, s.imag]))
    keep_vw = False                                 # detection on: update keeps the bordered vectors of the point in last_vw
    last_vw = None

    def __init__(self, prob, lens2: str, a, b, ls: _GMRES, bls: BorderingBLS | MatrixFreeBLS | None = None):
        super().__init__(prob, lens2, a, b, ls)
        _hopf_bordered_path(bls)                    # refuses an unpreconditioned MatrixFreeBLS up front
        self.bls = bls                              # MatrixFreeBLS(ls, use_pl=True): the bordered vectors on that path

    def _solve_terms(self, X: HopfVec, p2: float):
        return hopf_terms(self.prob, X.u, self.pvec(X.p[0], p2), self.ipar1, X.p[1], self.a, self.b, self.ls, self.bls)

    def _sigma_p(self, x, pv, ipar, v, w):
        """-w^H dJ/dp v"""
        return -hopf_contract(self.prob, x, pv, ipar, v, w)[1]

    def update(self, X: HopfVec, p2: float):
        """update!(probma, iter, state) after a converged step: a = w/|w|, b = v/|v| from the bordered vectors of the new
        point; returns omega (BT test function: the curve is stopped when |omega| < threshBT)."""
        v, w, _ = self.terms(X, p2)
        self.a, self.b = _cscale(w, 1.0 / cnorm(w)), _cscale(v, 1.0 / cnorm(v))
        self._cache = None
        if self.keep_vw:
            self.last_vw = (v, w, p2)               # the null vectors of the point: the first Lyapunov coefficient reuses them
        return float(X.p[1])


class HopfLinearSolverMinAug(_MinAugLinearSolver):
    """HopfLinearSolverMinAug -> _hopf_MA_linear_solver, usehessian branch, as bk_hopf_linsolve (real GMRES solves)."""

    def _run(self, J: _JacobianMinAug, rhs):
        H, v, w, arr, npar, dX, ru, dxp = _linsolve_args(J, rhs)
        ctx, m = H.ctx, len(rhs)
        rp = (C.c_double * (2 * m))(*[float(c) for r in rhs for c in r.p])
        ds = (C.c_double * (2 * m))()
        cv, it = C.c_int(), C.c_int()
        lo = H.ls._opts()
        ctx.check(ctx.lib.bk_hopf_linsolve(ctx.h, H.prob.h, _ptr(J.X.u.t), arr, npar, H.ipar1, _ptr(v[0].t), _ptr(v[1].t),
                                           _ptr(w[0].t), _ptr(w[1].t), m, ru, rp, C.byref(lo), H.ls._pl(), dxp, ds,
                                           C.byref(cv), C.byref(it)), "bk_hopf_linsolve")
        return [HopfVec(dX[k], [ds[2 * k], ds[2 * k + 1]]) for k in range(m)], bool(cv.value), it.value


JacobianHopf = _JacobianMinAug


# ------------------------------------------------------------------------------------------ continuation_hopf
@dataclass
class HopfBranch(_MinAugBranch):
    """The record of continuation_hopf (record_from_solution): p1 (lens1), p2 (lens2), omega and BT = omega per point; with
    detect_codim2 > 0 also l1 (the first Lyapunov coefficient b of the Hopf normal form) and GH = Re b per point, and the
    generalised Hopf points in ``specialpoint`` (type "gh")."""
    omega: list = field(default_factory=list)
    BT: list = field(default_factory=list)
    stopped_at_bt: bool = False
    l1: list = field(default_factory=list)
    GH: list = field(default_factory=list)
    specialpoint: list = field(default_factory=list)
    lens2: str | None = None


def continuation_hopf(prob, hopf_guess: HopfVec, p2: float, lens2: str, a, b, ls: _GMRES, cp: Cn.ContinuationPar, theta=0.5,
                      norm_inf=True, update_minaug_every_step=1, save_sol=False, ds_sequence=None, verbosity=0,
                      detect_codim2=0, bls: BorderingBLS | MatrixFreeBLS | None = None) -> HopfBranch:
    """continuation_hopf(prob, alg = PALC(tangent = Secant()), hopfpointguess, par, lens1, lens2, a, b, options_cont) with
    jacobian_ma = MinAug(): PALC on G(X, p2) through continuation.newton_palc with BorderingBLS(solver = HopfLinearSolverMinAug(),
    check_precision = false), Secant tangent, the two starting points of continuation by newton on G, step-size control of
    continuation.py.  After every converged step a, b are updated (update!) and the run stops once |omega| < 100 tol
    (threshBT: the curve is near a Bogdanov-Takens point).  ``ds_sequence`` (optional) replaces the step-size control by a fixed
    list of steps.

    ``detect_codim2`` (detect_codim2_bifurcation, MinAugHopf.jl:598-634): 0 locates nothing and issues exactly the library calls
    of the plain curve.  1: after every converged step the first Lyapunov coefficient of the new point is computed as test_bt_gh
    does -- zeta = v / |v|, zeta* = w / <zeta, w> from the bordered vectors the step solved, then hopf_normal_form_native -- into
    br.l1 (b) and br.GH (Re b; the previous value when |Re b| >= 1e5, :632), and every sign change of GH between consecutive
    points goes to br.specialpoint as type "gh" with the bracketing p2 interval.  2: each sign change is bisected along the curve
    (_locate_gh) and the special point keeps the located state; the curve continues from the state it had before the bisection,
    so the recorded points are those of detect_codim2 = 1.  With 1 or 2, a run that ends at |omega| < 100 tol appends a special
    point of type "bt" with the stop state (x, p1, omega), p2, the step index and the current a, b: a fold point NEAR the
    Bogdanov-Takens point, the guess newton_bt refines (bt_point).  Zero-Hopf and Hopf-Hopf points are not located.

    ``bls`` (optional): the bordered solver of the formulation's bordered vectors -- MatrixFreeBLS(ls, use_pl=True) takes each from
    ONE preconditioned bordered solve (option hopf_bordered).  The PALC border and the Newton step of G stay as they are."""
    br = HopfBranch(lens2=lens2)
    P = HopfProblem(prob, lens2, a, b, ls, bls)
    P.keep_vw = bool(detect_codim2)
    if detect_codim2 and update_minaug_every_step != 1:
        raise ValueError("detect_codim2 needs the bordered vectors of every point (update_minaug_every_step = 1)")

    last = {}

    def record_x(X, om, tau):
        br.p1.append(float(X.p[0])); br.omega.append(float(X.p[1])); br.BT.append(om)
        if detect_codim2:
            last["X"] = X                           # the state of the loop, read once more if the curve stops at omega = 0
            with _solver_state_kept(prob.ctx):
                l1 = _first_lyapunov(P, X)
            br.l1.append(l1)
            br.GH.append(_gh_value(l1, br.GH[-1] if br.GH else math.nan))

    def after_record(z, z_old, tau, ds_taken, nopt, bls):
        # record() has appended the point: GH[-1] belongs to z, GH[-2] to z_old
        if len(br.GH) < 2 or not _sign_change(br.GH[-2], br.GH[-1]):
            return
        sp = dict(type="gh", idx=len(br.GH) - 1, step=len(br.GH) - 1, p2=float(z.p), interval=tuple(sorted((z_old.p, z.p))),
                  GH=br.GH[-1], GH_interval=(br.GH[-2], br.GH[-1]), x=z.u.copy(), a=P.a, b=P.b, bisection_steps=0, status="guess")
        if detect_codim2 > 1:
            with _solver_state_kept(prob.ctx):
                sp.update(_locate_gh(P, z, z_old, tau, ds_taken, br.GH[-1], cp, theta, nopt, bls, normC))
        br.specialpoint.append(sp)

    normC = (lambda z: z.norminf()) if norm_inf else (lambda z: z.norm())
    thresh_bt = 100 * cp.newton_options.tol
    br.stopped_at_bt = _continuation_minaug(
        P, HopfLinearSolverMinAug(), "Hopf", br, hopf_guess, p2, cp, theta, normC, update_minaug_every_step, save_sol, ds_sequence,
        verbosity, record_x, skipped=lambda X: float(X.p[1]), describe=lambda X: f"p1={X.p[0]:+.8f} omega={X.p[1]:+.8f}",
        stop_after=lambda om: abs(om) < thresh_bt, after_record=after_record if detect_codim2 else None)
    if br.stopped_at_bt and detect_codim2:
        # the :bt point of the reference (src/events/Event.jl:27-40, MinAugHopf.jl:353-367): the state at which the event value
        # fell below threshBT.  The Hopf Newton has collapsed onto omega = 0 there, so this is a fold point NEAR the
        # Bogdanov-Takens point and the guess of newton_bt (bt_point), not the point itself.
        X, i = last["X"], len(br.p2) - 1
        br.specialpoint.append(dict(type="bt", idx=i, step=i, p1=float(X.p[0]), p2=float(br.p2[i]), omega=float(X.p[1]),
                                    x=X.u.copy(), a=tuple(v.copy() for v in P.a), b=tuple(v.copy() for v in P.b), status="guess"))
    return br


# ------------------------------------------------------------------------------------------ generalised Hopf points on the curve
class _lens2_at:
    """with _lens2_at(prob, lens2, p2): the problem's parameter ``lens2`` is p2 inside the block (prob._pvec fills the other
    parameters from prob.params), and what it was afterwards."""

    def __init__(self, prob, lens2, p2):
        self.prob, self.lens2, self.p2 = prob, lens2, float(p2)

    def __enter__(self):
        self.old = self.prob.params[self.lens2]
        self.prob.params[self.lens2] = self.p2

    def __exit__(self, *exc):
        self.prob.params[self.lens2] = self.old
        return False


class _solver_state_kept:
    """with _solver_state_kept(ctx): GMRES solves inside the block leave no trace in the state one solve hands to the next on
    the context (the step count of the last solve, from which the next one sizes its first Arnoldi block, and the carried Newton
    shifts: the context's "solver_state_hold"), so the solves after the block run exactly as they would have without it."""

    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        self.ctx.set_option("solver_state_hold", 1)

    def __exit__(self, *exc):
        self.ctx.set_option("solver_state_hold", 0)
        return False


def _gh_value(l1: complex, previous: float) -> float:
    """GH of test_bt_gh (MinAugHopf.jl:632): Re l1, or the previous value when |Re l1| >= 1e5."""
    return float(l1.real) if abs(l1.real) < 1e5 else previous


def _sign_change(g0: float, g1: float) -> bool:
    return g0 * g1 < 0


def _first_lyapunov(P: HopfProblem, X: HopfVec, vw=None) -> complex:
    """b of the Hopf normal form at the point X of the curve from its bordered vectors (test_bt_gh, :598-634): those P.update
    has just kept, or ``vw`` = (v, w, p2)."""
    v, w, p2 = vw if vw is not None else P.last_vw
    zeta = _cscale(v, 1.0 / cnorm(v))
    zeta_star = _cscale(w, 1.0 / cinner(zeta, w))
    with _lens2_at(P.prob, P.lens2, p2):
        return complex(hopf_normal_form_native(P.prob, X, zeta, zeta_star, P.ls).nf.b)


def _locate_event(P: _MinAugProblem, z, z_old, tau, ds, ev_after: float, event, coords, cp, theta, nopt, bls, normC) -> dict:
    """locate_event! (src/events/EventDetection.jl:28-175) for the sign change of an event between z_old and z, on copies of the
    state: ds, the step that led from z_old to z, is reversed and halved (the first point is the middle of the crossing step), then
    PALC corrector steps are taken with the step-size control off, ds halved after every step and its sign flipped whenever the
    event changed sign, until cp.max_bisection_steps, cp.n_inversion, |ds| < cp.dsmin_bisection or an unconverged corrector.  The
    tangent keeps the orientation of the curve (Secant with the sign of the ds of the step), a and b stay those of the point after
    the crossing, and the problem's a, b, cache, GMRES count and kept bordered vectors are restored on exit.
    ``event(zc, tau_b, previous)`` -> the event value at the new state zc with its tangent tau_b; ``coords(z)`` -> what is kept of
    the two end states.  Returns dict(z = the last state, value = its event value, ends = [coords of the state before the
    crossing, coords of the state after it] as the bisection moved them, values = the event values there, bisection_steps,
    n_inversion, status = why the bisection ended, reach = |ds| of the last step that passed the crossing -- the first, halved,
    step when none did: the halved steps after it add up to no more than this, so it is what the last state can still be off by
    along the curve)."""
    keep = (P.a, P.b, P._cache, P.itlinear, getattr(P, "last_vw", None))
    zc, zp_ = z.copy(), z_old.copy()
    tau_b = tau.copy()
    ends = [coords(z_old), coords(z)]
    values = [math.nan, ev_after]
    ind = 1                                          # the end the current state replaces
    sign = ev_after > 0
    ds_b = -ds / 2.0
    ev, steps, n_inv, status = ev_after, 0, 0, "max_bisection_steps"
    reach = abs(ds_b)
    try:
        while steps < cp.max_bisection_steps:
            if n_inv >= cp.n_inversion:
                status = "n_inversion"
                break
            if abs(ds_b) < cp.dsmin_bisection:
                status = "dsmin_bisection"
                break
            sol = Cn.newton_palc(P, zc, tau_b, zc.copy().add_(tau_b, ds_b), ds_b, theta, bls, nopt, cp.p_min, cp.p_max, normC)
            if not sol.converged:
                status = "unconverged"
                break
            zp_.copyto_(zc)
            zc.copyto_(sol.u)
            steps += 1
            tau_b = Cn.secant_tangent(zc, zp_, ds_b, theta)
            ev = event(zc, tau_b, ev)
            if (ev > 0) == sign:
                ds_b /= 2.0
            else:
                reach = abs(ds_b)
                ds_b /= -2.0
                n_inv += 1
                ind = 1 - ind
                sign = ev > 0
            ends[ind] = coords(zc)
            values[ind] = ev
    finally:
        P.a, P.b, P._cache, P.itlinear = keep[:4]
        if hasattr(P, "last_vw"):
            P.last_vw = keep[4]
    return dict(z=zc, value=ev, ends=ends, values=values, bisection_steps=steps, n_inversion=n_inv, status=status, reach=reach)


def _locate_gh(P: HopfProblem, z, z_old, tau, ds, gh_after: float, cp, theta, nopt, bls, normC) -> dict:
    """_locate_event for the sign change of GH between z_old and z: the event is the first Lyapunov coefficient from the bordered
    vectors of the new state.  Returns the fields of the special point: the last state, its p2 and GH, the bracket, the steps
    taken and why the bisection ended."""
    def event(zc, tau_b, previous):
        v, w, _ = P.terms(zc.u, zc.p)
        return _gh_value(_first_lyapunov(P, zc.u, (v, w, zc.p)), previous)

    r = _locate_event(P, z, z_old, tau, ds, gh_after, event, lambda s: float(s.p), cp, theta, nopt, bls, normC)
    return dict(x=r["z"].u.copy(), p2=float(r["z"].p), GH=r["value"], interval=tuple(sorted(r["ends"])),
                bisection_steps=r["bisection_steps"], n_inversion=r["n_inversion"], status=r["status"])


# ================================================================================================== Hopf normal form
# __hopf_normal_form (src/NormalForms.jl:1009-1076) and predictor(::Hopf, ds) (:1227-1281) for CGL2d, matrix-free:
#
#   hopf_d3F, hopf_nf_rhs, hopf_nf_contract, hopf_orbit   the device passes (bk_hopf_d3f, bk_hopf_nf_rhs, bk_hopf_nf_contract,
#                                                         bk_hopf_orbit)
#   hopf_eigenpair            zeta, zeta* from the null vectors v, w of a newton_hopf result, |zeta| = 1, <zeta, zeta*> = 1
#   hopf_normal_form          the computation call by call on the plugin surface (ls(J, rhs1, rhs2), ls.solve_complex)
#   hopf_normal_form_native   the same as one library call (bk_hopf_normal_form)
#   get_normal_form           get_normal_form(br, ind) for a Hopf point of a native branch: refine, then the normal form ("bp" and
#                             "fold" points of the Swift-Hohenberg problems: normal_form1d.py)
#   predictor                 the second-order guess of the periodic orbit that branches off
#
# z' = z (i omega + a dp + b |z|^2); inner(x, y) = sum conj(x) y = cinner(x, y), so a = cinner(av, zeta*), b = cinner(bv, zeta*).
# dpF and dJ/dp are analytic where the reference differentiates (ForwardDiff / central differences).
@dataclass
class HopfNormalForm:
    """HopfNormalForm(a, b, Psi110, Psi001, Psi200) (src/NormalForms.jl:1066); Psi200 is a (re, im) pair."""
    a: complex | None = None
    b: complex | None = None
    Psi110: object = None
    Psi001: object = None
    Psi200: object = None


@dataclass
class Hopf:
    """The reference's Hopf record (x0, p, omega, zeta, zeta_star, nf, type; params and lens as there) plus what the solves
    reported: ``converged`` (all three), ``itlinear`` (GMRES counts of the Psi001, Psi110, Psi200 solves) and, from the native
    call, ``unconverged_solves``."""
    x0: object
    p: float
    omega: float
    zeta: object
    zeta_star: object
    nf: HopfNormalForm = field(default_factory=HopfNormalForm)
    type: str = "?"
    params: list | None = None
    lens: str | None = None
    converged: bool | None = None
    itlinear: tuple = ()
    unconverged_solves: int | None = None


def hopf_type(b: complex) -> str:
    """:1067-1073"""
    return "SuperCritical" if b.real < 0 else ("SubCritical" if b.real > 0 else "Singular")


def hopf_d3F(prob, x: HipVec, pars, dx1: HipVec, dx2: HipVec, dx3: HipVec) -> HipVec:
    """d3F(x)[dx1, dx2, dx3] of CGL2d for real arguments (bk_hopf_d3f)."""
    return _into_similar(prob, "bk_hopf_d3f", x, pars, _ptr(dx1.t), _ptr(dx2.t), _ptr(dx3.t))


def hopf_nf_rhs(prob, x: HipVec, pars, zeta):
    """One fused pass (bk_hopf_nf_rhs): (d2F[zeta, zeta] / 2 as a (re, im) pair, d2F[zeta, conj zeta])."""
    ctx = prob.ctx
    rr, ri, r11 = x.similar(), x.similar(), x.similar()
    ctx.check(ctx.lib.bk_hopf_nf_rhs(prob.h, _ptr(x.t), _carr(pars), len(pars), _ptr(zeta[0].t), _ptr(zeta[1].t), _ptr(rr.t),
                                     _ptr(ri.t), _ptr(r11.t)), "bk_hopf_nf_rhs")
    return (rr, ri), r11


def hopf_nf_contract(prob, x: HipVec, pars, ipar: int, zeta, zeta_star, Psi001: HipVec, Psi110: HipVec, Psi200):
    """One fused pass (bk_hopf_nf_contract): the coefficients (a, b) as complex numbers."""
    ctx = prob.ctx
    out = (C.c_double * 4)()
    ctx.check(ctx.lib.bk_hopf_nf_contract(prob.h, _ptr(x.t), _carr(pars), len(pars), int(ipar), _ptr(zeta[0].t), _ptr(zeta[1].t),
                                          _ptr(zeta_star[0].t), _ptr(zeta_star[1].t), _ptr(Psi001.t), _ptr(Psi110.t),
                                          _ptr(Psi200[0].t), _ptr(Psi200[1].t), out), "bk_hopf_nf_contract")
    return complex(out[0], out[1]), complex(out[2], out[3])


def hopf_orbit(x0: HipVec, zeta, Psi001: HipVec, Psi110: HipVec, Psi200, ds: float, amp: float, ts):
    """[x0 + 2 Re(zeta A) + ds Psi001 + |A|^2 Psi110 + 2 Re(A^2 Psi200) for A = amp e^{i t}, t in ts] (bk_hopf_orbit: eight
    phases per pass over the inputs)."""
    ctx = x0.ctx
    ts = [float(t) for t in ts]
    outs = [x0.similar() for _ in ts]
    ctx.check(ctx.lib.bk_hopf_orbit(ctx.h, x0.n, _ptr(x0.t), _ptr(zeta[0].t), _ptr(zeta[1].t), _ptr(Psi001.t), _ptr(Psi110.t),
                                    _ptr(Psi200[0].t), _ptr(Psi200[1].t), float(ds), float(amp), len(ts),
                                    (C.c_double * max(len(ts), 1))(*ts), _vptrs(outs)), "bk_hopf_orbit")
    return outs


def hopf_eigenpair(prob, sol):
    """(zeta, zeta*) of the normal form from a newton_hopf / newton_hopf_native result: its v spans ker(J - i omega) and its w
    ker(J' + i omega) (the start_with_eigen = Val(false) branch, :1173-1179).  zeta = v / |v|, zeta* = w / cinner(zeta, w), so that
    cinner(zeta, zeta_star) == 1; cinner(x, y) = x^H y conjugates its FIRST argument (:1186-1187)."""
    v, w = sol["v"], sol["w"]
    zeta = _cscale(v, 1.0 / cnorm(v))
    return zeta, _cscale(w, 1.0 / cinner(zeta, w))


def _hopf_record(prob, X: HopfVec, zeta, zeta_star, a, b, P001, P110, P200, cv, it, bad=None) -> Hopf:
    p, om = float(X.p[0]), float(X.p[1])
    return Hopf(x0=X.u, p=p, omega=om, zeta=zeta, zeta_star=zeta_star, nf=HopfNormalForm(a, b, P110, P001, P200),
                type=hopf_type(b), params=prob._pvec(p), lens=prob.lens, converged=bool(cv), itlinear=tuple(int(i) for i in it),
                unconverged_solves=bad)


def hopf_normal_form(prob, X: HopfVec, zeta, zeta_star, ls: _GMRES) -> Hopf:
    """__hopf_normal_form (:1009-1076) call by call on the plugin surface at the Hopf point X = (x, [p, omega]) with
    zeta, zeta* normalised (hopf_eigenpair): Psi001 = ls(J, -dpF) and Psi110 = ls(J, -d2F[zeta, conj zeta]) as one
    ls(J, rhs1, rhs2) (bk_gmres2), Psi200 = ls.solve_complex(J, d2F[zeta, zeta] / 2, a0 = 2 i omega, a1 = -1) (:1053), the
    right-hand sides from hopf_nf_rhs and (a, b) from hopf_nf_contract."""
    x, p, om = X.u, float(X.p[0]), float(X.p[1])
    pv, ipar = prob._pvec(p), prob.ipar
    nrm = hopf_contract(prob, x, pv, ipar, zeta, zeta_star)[2].conjugate()         # <zeta, zeta*> = conj(zeta*^H zeta)
    if not abs(nrm - 1) <= 1e-8:
        raise ValueError(f"Error of precision in normalization: <zeta, zeta*> = {nrm}, expected 1")
    J = prob.jacobian(x, p)
    r20, r11 = hopf_nf_rhs(prob, x, pv, zeta)
    P001, P110, cv, it = _solve2(ls, J, dpF(prob, x, pv, ipar).scale_(-1.0), r11.scale_(-1.0))
    P200, cv2, it2 = ls.solve_complex(J, r20, a0=complex(0.0, 2.0 * om), a1=-1.0)
    a, b = hopf_nf_contract(prob, x, pv, ipar, zeta, zeta_star, P001, P110, P200)
    return _hopf_record(prob, X, zeta, zeta_star, a, b, P001, P110, P200, cv and cv2, (it[0], it[1], it2))


def hopf_normal_form_native(prob, X: HopfVec, zeta, zeta_star, ls: _GMRES) -> Hopf:
    """The same as one library call (bk_hopf_normal_form)."""
    ctx = prob.ctx
    x, p, om = X.u, float(X.p[0]), float(X.p[1])
    pv = prob._pvec(p)
    P001, P110, P200 = x.similar(), x.similar(), (x.similar(), x.similar())
    ab = (C.c_double * 4)()
    cv = C.c_int()
    it = (C.c_int * 3)()
    lo = ls._opts()
    bad0 = ctx.get_option("hopf_nf_unconverged_solves")
    ctx.check(ctx.lib.bk_hopf_normal_form(ctx.h, prob.h, _ptr(x.t), _carr(pv), len(pv), prob.ipar, om, _ptr(zeta[0].t),
                                          _ptr(zeta[1].t), _ptr(zeta_star[0].t), _ptr(zeta_star[1].t), C.byref(lo), ls._pl(),
                                          _ptr(P001.t), _ptr(P110.t), _ptr(P200[0].t), _ptr(P200[1].t), ab, C.byref(cv), it),
              "bk_hopf_normal_form")
    return _hopf_record(prob, X, zeta, zeta_star, complex(ab[0], ab[1]), complex(ab[2], ab[3]), P001, P110, P200, cv.value,
                        (it[0], it[1], it[2]), int(ctx.get_option("hopf_nf_unconverged_solves") - bad0))


# ------------------------------------------------------------------------------------------ Bautin normal form
# bautin_normal_form (src/codim2/NormalForms.jl:642-829, detailed = false) for CGL2d, matrix-free, on top of a Hopf record:
# H11 = Psi110, H20 = 2 Psi200 and G21 = 2 conj(b) come from the Hopf normal form (b = cinner(bv, zeta*) conjugates bv, the
# reference's G21 = dot(p0, .) conjugates p0).  D = d4F and E = d5F are analytic (the reference nests central differences).
#
#   bautin_rhs3, bautin_rhs4, bautin_contract   the device passes (bk_bautin_rhs3, bk_bautin_rhs4, bk_bautin_contract)
#   bautin_normal_form                          the computation call by call on the plugin surface (ls.solve_complex,
#                                               BorderingBLS.solve_complex, ls(J, rhs))
#   bautin_normal_form_native                   the same as one library call (bk_bautin_normal_form)
@dataclass
class BautinNormalForm:
    """The reference's nf = (omega, G21, G32, l2) plus the vectors of the computation (complex ones as (re, im) pairs)."""
    omega: float | None = None
    G21: complex | None = None
    G32: complex | None = None
    l2: float | None = None
    H20: object = None
    H11: object = None
    H30: object = None
    H21: object = None
    H31: object = None
    H22: object = None


@dataclass
class Bautin:
    """The reference's Bautin record (x0, params, lens = (lens1, lens2), zeta, zeta_star, nf, type) plus what the four solves
    reported: ``converged`` (all of them), ``itlinear`` (GMRES counts of the H30, H21, H31, H22 solves) and, from the native call,
    ``unconverged_solves``."""
    x0: object
    params: list
    lens: tuple
    zeta: object
    zeta_star: object
    nf: BautinNormalForm = field(default_factory=BautinNormalForm)
    type: str = "?"
    converged: bool | None = None
    itlinear: tuple = ()
    unconverged_solves: int | None = None


def bautin_type(l2: float) -> str:
    """type(::Bautin): the sign of the second Lyapunov coefficient."""
    return "Subcritical" if l2 > 0 else "Supercritical"


def _c2(z):
    return _ptr(z[0].t), _ptr(z[1].t)


def bautin_rhs3(prob, x: HipVec, pars, q, H20, H11: HipVec, G21: complex):
    """One fused pass (bk_bautin_rhs3): (h30, h21) as (re, im) pairs -- C(q, q, q) + 3 B(q, H20) and
    G21 q - (C(q, q, conj q) + B(conj q, H20) + 2 B(q, H11))."""
    ctx = prob.ctx
    h30, h21 = (x.similar(), x.similar()), (x.similar(), x.similar())
    g = (C.c_double * 2)(complex(G21).real, complex(G21).imag)
    ctx.check(ctx.lib.bk_bautin_rhs3(prob.h, _ptr(x.t), _carr(pars), len(pars), *_c2(q), *_c2(H20), _ptr(H11.t), g, *_c2(h30),
                                     *_c2(h21)), "bk_bautin_rhs3")
    return h30, h21


def bautin_rhs4(prob, x: HipVec, pars, q, H20, H11: HipVec, H30, H21, G21: complex):
    """One fused pass (bk_bautin_rhs4): (h31 as a (re, im) pair, the real h22), the right-hand sides of the H31 and H22 solves."""
    ctx = prob.ctx
    h31, h22 = (x.similar(), x.similar()), x.similar()
    g = (C.c_double * 2)(complex(G21).real, complex(G21).imag)
    ctx.check(ctx.lib.bk_bautin_rhs4(prob.h, _ptr(x.t), _carr(pars), len(pars), *_c2(q), *_c2(H20), _ptr(H11.t), *_c2(H30),
                                     *_c2(H21), g, *_c2(h31), _ptr(h22.t)), "bk_bautin_rhs4")
    return h31, h22


def bautin_contract(prob, x: HipVec, pars, q, p0, H20, H11: HipVec, H30, H21, H31, H22: HipVec) -> complex:
    """One fused pass over the fifteen vectors (bk_bautin_contract): G32."""
    ctx = prob.ctx
    out = (C.c_double * 2)()
    ctx.check(ctx.lib.bk_bautin_contract(prob.h, _ptr(x.t), _carr(pars), len(pars), *_c2(q), *_c2(p0), *_c2(H20), _ptr(H11.t),
                                         *_c2(H30), *_c2(H21), *_c2(H31), _ptr(H22.t), out), "bk_bautin_contract")
    return complex(out[0], out[1])


def _bautin_record(hopf: Hopf, lens2, G21, G32, H20, H30, H21, H31, H22, cv, it, bad=None) -> Bautin:
    l2 = G32.real / 12.0
    nf = BautinNormalForm(hopf.omega, G21, G32, l2, H20, hopf.nf.Psi110, H30, H21, H31, H22)
    return Bautin(x0=hopf.x0, params=list(hopf.params), lens=(hopf.lens, lens2), zeta=hopf.zeta, zeta_star=hopf.zeta_star, nf=nf,
                  type=bautin_type(l2), converged=bool(cv), itlinear=tuple(int(i) for i in it), unconverged_solves=bad)


def bautin_normal_form(prob, hopf: Hopf, ls: _GMRES, lens2=None, bls: BorderingBLS | MatrixFreeBLS | None = None) -> Bautin:
    """bautin_normal_form (:642-829, detailed = false) call by call on the plugin surface at the Hopf point of the record ``hopf``
    (hopf_normal_form / hopf_normal_form_native: x0, params, omega, zeta, zeta*, Psi110, Psi200, b): H30 =
    ls.solve_complex(J, h30, a0 = 3 i omega, a1 = -1), H21 = BorderingBLS(ls, check_precision = false).solve_complex(J, q, p0, 0,
    h21, 0; shift = -i omega), H31 = ls.solve_complex(J, h31, a0 = 2 i omega, a1 = -1), H22 = -ls(J, h22); the right-hand sides
    from bautin_rhs3 / bautin_rhs4 and G32 from bautin_contract.  ``bls = MatrixFreeBLS(ls, use_pl=True)`` takes H21, whose
    J - i omega is singular, from ONE preconditioned bordered solve (MatrixFreeBLS.solve_complex)."""
    from .hip import HipJacobian
    x, om, pv = hopf.x0, float(hopf.omega), list(hopf.params)
    q, p0 = hopf.zeta, hopf.zeta_star
    nrm = hopf_contract(prob, x, pv, 0, q, p0)[2].conjugate()
    if not abs(nrm - 1) <= 1e-8:
        raise ValueError(f"Error of precision in normalization: <zeta, zeta*> = {nrm}, expected 1")
    H11 = hopf.nf.Psi110
    H20 = tuple(v.copy().scale_(2.0) for v in hopf.nf.Psi200)
    G21 = 2.0 * complex(hopf.nf.b).conjugate()
    J = HipJacobian(prob, x, pv)
    h30, h21 = bautin_rhs3(prob, x, pv, q, H20, H11, G21)
    H30, cv30, it30 = ls.solve_complex(J, h30, a0=complex(0.0, 3.0 * om), a1=-1.0)
    bls21 = bls if _hopf_bordered_path(bls) else BorderingBLS(ls, check_precision=False)
    H21, _, cv21, it21 = bls21.solve_complex(J, q, p0, 0.0, h21, 0.0, shift=complex(0.0, -om))
    h31, h22 = bautin_rhs4(prob, x, pv, q, H20, H11, H30, H21, G21)
    H31, cv31, it31 = ls.solve_complex(J, h31, a0=complex(0.0, 2.0 * om), a1=-1.0)
    H22, cv22, it22 = ls(J, h22)
    H22.scale_(-1.0)
    G32 = bautin_contract(prob, x, pv, q, p0, H20, H11, H30, H21, H31, H22)
    return _bautin_record(hopf, lens2, G21, G32, H20, H30, H21, H31, H22, cv30 and cv21 and cv31 and cv22,
                          (it30, int(np.sum(it21)), it31, it22))


def bautin_normal_form_native(prob, hopf: Hopf, ls: _GMRES, lens2=None, bls: BorderingBLS | MatrixFreeBLS | None = None) -> Bautin:
    """The same as one library call (bk_bautin_normal_form); with ``bls = MatrixFreeBLS(ls, use_pl=True)`` under the context option
    hopf_bordered = 1, set and put back around the call."""
    ctx = prob.ctx
    x, om, pv = hopf.x0, float(hopf.omega), list(hopf.params)
    H30, H21, H31, H22 = (x.similar(), x.similar()), (x.similar(), x.similar()), (x.similar(), x.similar()), x.similar()
    b = complex(hopf.nf.b)
    a = complex(hopf.nf.a) if hopf.nf.a is not None else 0j
    ab = (C.c_double * 4)(a.real, a.imag, b.real, b.imag)
    g = (C.c_double * 5)()
    cv = C.c_int()
    it = (C.c_int * 4)()
    lo = ls._opts()
    bad0 = ctx.get_option("bautin_unconverged_solves")
    with _hopf_bordered(ctx, _hopf_bordered_path(bls)):
        ctx.check(ctx.lib.bk_bautin_normal_form(ctx.h, prob.h, _ptr(x.t), _carr(pv), len(pv), om, *_c2(hopf.zeta),
                                                *_c2(hopf.zeta_star), _ptr(hopf.nf.Psi110.t), *_c2(hopf.nf.Psi200), ab, C.byref(lo),
                                                ls._pl(), *_c2(H30), *_c2(H21), *_c2(H31), _ptr(H22.t), g, C.byref(cv), it),
                  "bk_bautin_normal_form")
    H20 = tuple(v.copy().scale_(2.0) for v in hopf.nf.Psi200)
    return _bautin_record(hopf, lens2, complex(g[0], g[1]), complex(g[2], g[3]), H20, H30, H21, H31, H22, cv.value,
                          (it[0], it[1], it[2], it[3]), int(ctx.get_option("bautin_unconverged_solves") - bad0))


def _bautin_from_branch(br, ind: int, prob, ls: _GMRES, tol, max_iterations, norm_inf, bls=None) -> Bautin:
    """A "gh" point of a HopfBranch: newton_hopf_native at the located p2 from the located state -> hopf_eigenpair ->
    hopf_normal_form_native -> bautin_normal_form_native (the normal form at the REFINED Hopf point of the located p2)."""
    sp = br.specialpoint[ind]
    with _lens2_at(prob, br.lens2, sp["p2"]):
        s = newton_hopf_native(prob, sp["x"], sp["a"], sp["b"], ls, tol=tol, max_iterations=max_iterations, norm_inf=norm_inf,
                               bls=bls)
        if not s["converged"]:
            raise RuntimeError(f"get_normal_form: newton_hopf did not converge from the located point (residuals {s['residuals']})")
        zeta, zeta_star = hopf_eigenpair(prob, s)
        hp = hopf_normal_form_native(prob, s["u"], zeta, zeta_star, ls)
        return bautin_normal_form_native(prob, hp, ls, lens2=br.lens2, bls=bls)


# ------------------------------------------------------------------------------------------ cusp normal form
# cusp_normal_form (src/codim2/NormalForms.jl:15-123; Kuznetsov 1999) for the Swift-Hohenberg problems, matrix-free, at a fold
# (x, params) with q = zeta, p = zeta*, |q| = 1, <q, p> = 1 (J' = J: p may be q itself):
#
#   b2 = <p, B(q, q)>,   [J q; p' 0][H2; s] = [b2 q - B(q, q); 0]   (:107-109),   c = (<p, C(q, q, q)> + 3 <p, B(q, H2)>) / 6   (:112-113)
#
#   cusp_dots, cusp_rhs, cusp_contract   the device passes (bk_cusp_dots, bk_cusp_rhs, bk_cusp_contract)
#   cusp_normal_form                     the computation call by call on the plugin surface (d2F, bk_d3f, inner products, bls)
#   cusp_normal_form_native              the same as one library call (bk_cusp_normal_form)
@dataclass
class CuspNormalForm:
    """The reference's nf = (c = c,) plus the vector of the computation."""
    c: float | None = None


@dataclass
class Cusp:
    """The reference's Cusp record (x0, params, lens = (lens1, lens2), zeta, zeta_star, nf = (c,)) plus b2 = <zeta*, B(zeta, zeta)>
    (zero at a cusp; not small: the point is a turning point of the fold curve in lens2 that is no cusp, see FoldBranch), H2 and
    what the one bordered solve reported: ``converged``, ``itlinear`` and, from the native call, ``unconverged_solves``."""
    x0: object
    params: list
    lens: tuple
    zeta: object
    zeta_star: object
    nf: CuspNormalForm = field(default_factory=CuspNormalForm)
    b2: float | None = None
    H2: object = None
    converged: bool | None = None
    itlinear: tuple = ()
    unconverged_solves: int | None = None


def cusp_rhs(prob, x: HipVec, pars, q: HipVec, b2: float) -> HipVec:
    """One pass over (x, q) (bk_cusp_rhs): b2 q - d2F(x)[q, q], the right-hand side of the H2 solve."""
    return _into_similar(prob, "bk_cusp_rhs", x, pars, _ptr(q.t), float(b2))


def cusp_contract(prob, x: HipVec, pars, q: HipVec, p: HipVec, H2: HipVec):
    """One pass over (x, q, p, H2) (bk_cusp_contract): (<p, d3F(x)[q, q, q]>, <p, d2F(x)[q, H2]>)."""
    ctx = prob.ctx
    out = (C.c_double * 2)()
    ctx.check(ctx.lib.bk_cusp_contract(prob.h, _ptr(x.t), _carr(pars), len(pars), _ptr(q.t), _ptr(p.t), _ptr(H2.t), out),
              "bk_cusp_contract")
    return out[0], out[1]


def _cusp_lens(prob, lens2):
    return (prob.lens, lens2)


def cusp_normal_form(prob, x: HipVec, pars, q: HipVec, p: HipVec, ls: _GMRES, bls: BorderingBLS | MatrixFreeBLS | None = None,
                     lens2=None) -> Cusp:
    """cusp_normal_form (:100-123) call by call on the plugin surface at the fold (x, pars) with q, p normalised (|q| = 1,
    <q, p> = 1; they may be the same vector): h2 = d2F(q, q), b2 = <p, h2>, H2 = bls(J, q, p, 0, b2 q - h2, 0) and
    c = (<p, d3F(q, q, q)> + 3 <p, d2F(q, H2)>) / 6, every tensor materialised and every inner product its own pass.
    ``bls``: BorderingBLS (default, check_precision = false), MatrixFreeBLS(ls) or MatrixFreeBLS(ls, use_pl=True)."""
    from .normal_form1d import d3F
    bls = bls if bls is not None else BorderingBLS(ls, check_precision=False)
    pars = [float(v) for v in pars]
    nrm = q.inner(p)
    if not abs(nrm - 1) <= 1e-8:
        raise ValueError(f"Error of precision in normalization: <q, p> = {nrm}, expected 1")
    h2 = d2F(prob, x, pars, q, q)
    b2 = p.inner(h2)
    rhs = q.copy().scale_(b2).add_(h2, -1.0)
    J = HipJacobian(prob, x, pars)
    H2, _, cv, it = bls(J, q, p, 0.0, rhs, 0.0)
    c = (p.inner(d3F(prob, x, pars, q, q, q)) + 3.0 * p.inner(d2F(prob, x, pars, q, H2))) / 6.0
    it = tuple(int(i) for i in np.atleast_1d(it))
    return Cusp(x0=x, params=pars, lens=_cusp_lens(prob, lens2), zeta=q, zeta_star=p, nf=CuspNormalForm(c), b2=b2, H2=H2,
                converged=bool(cv), itlinear=it)


def cusp_normal_form_native(prob, x: HipVec, pars, q: HipVec, p: HipVec, ls: _GMRES,
                            bls: BorderingBLS | MatrixFreeBLS | None = None, lens2=None) -> Cusp:
    """The same as one library call (bk_cusp_normal_form); with ``bls = MatrixFreeBLS(ls, use_pl=True)`` under the context option
    fold_bordered = 1, set and put back around the call."""
    bls = bls if bls is not None else BorderingBLS(ls, check_precision=False)
    ctx = prob.ctx
    pars = [float(v) for v in pars]
    H2 = x.similar()
    coef = (C.c_double * 2)()
    cv = C.c_int()
    it = (C.c_int * 2)()
    bordered = isinstance(bls, MatrixFreeBLS) and bls.use_pl
    bo, lo = _bls_opts(bls), ls._opts()
    bad0 = ctx.get_option("cusp_unconverged_solves")
    with _fold_bordered(ctx, bordered):
        ctx.check(ctx.lib.bk_cusp_normal_form(ctx.h, prob.h, _ptr(x.t), _carr(pars), len(pars), _ptr(q.t), _ptr(p.t), C.byref(bo),
                                              C.byref(lo), ls._pl(), _ptr(H2.t), coef, C.byref(cv), it), "bk_cusp_normal_form")
    return Cusp(x0=x, params=pars, lens=_cusp_lens(prob, lens2), zeta=q, zeta_star=p, nf=CuspNormalForm(coef[1]), b2=coef[0], H2=H2,
                converged=bool(cv.value), itlinear=(it[0], it[1]) if not isinstance(bls, MatrixFreeBLS) else (it[0],),
                unconverged_solves=int(ctx.get_option("cusp_unconverged_solves") - bad0))


def _cusp_from_branch(br, ind: int, prob, ls: _GMRES, tol, max_iterations, norm_inf, bls=None) -> Cusp:
    """A "cusp" point of a FoldBranch: newton_fold_native in lens1 at the located p2 from the located state -> q = v / |v|,
    p = w / <q, w> -> cusp_normal_form_native (the normal form at the REFINED fold point of the located p2)."""
    sp = br.specialpoint[ind]
    X = sp["x"]
    with _lens2_at(prob, br.lens2, sp["p2"]):
        s = newton_fold_native(prob, X.u, X.p, sp["a"], sp["b"], ls, bls, tol=tol, max_iterations=max_iterations,
                               norm_inf=norm_inf)
        if not s["converged"]:
            raise RuntimeError(f"get_normal_form: newton_fold did not converge from the located point (residuals {s['residuals']})")
        q = s["v"].copy().scale_(1.0 / s["v"].norm())
        p = s["w"].copy().scale_(1.0 / q.inner(s["w"]))
        return cusp_normal_form_native(prob, s["u"].u, prob._pvec(s["u"].p), q, p, ls, bls, lens2=br.lens2)


def get_normal_form(br, ind: int, prob, ls: _GMRES, eig=None, nev=4, tol=1e-10, max_iterations=15, norm_inf=False, seed=0,
                    bls=None, refine=True, ls_adj=None, detailed=True):
    """get_normal_form(br, ind) (src/NormalForms.jl:1102-1204) for a point of type "hopf" of a branch of
    continuation.continuation_native(..., bisection = True, save_sol = True): hopf_point -> hopf_start_vectors (the reference's
    random start, or start_with_eigen when ``eig`` is given) -> newton_hopf_native -> hopf_eigenpair -> hopf_normal_form_native.
    The normal form is taken at the REFINED point (the reference takes the bisected one).  For a Swift-Hohenberg problem a point of
    type "bp" or "fold" goes to normal_form1d.get_normal_form1d (``bls``, ``refine`` as there) and returns its SimpleBranchPoint;
    "nd" points, and "bp" / "fold" points of any other problem, have no normal form here.  A point of type "gh" of a HopfBranch
    (continuation_hopf(..., detect_codim2 > 0)) returns its Bautin record: newton_hopf_native at the located p2 ->
    hopf_eigenpair -> hopf_normal_form_native -> bautin_normal_form_native.  For "hopf" and "gh" points ``bls`` is the bordered
    solver of newton_hopf_native and bautin_normal_form_native (MatrixFreeBLS(ls, use_pl=True): option hopf_bordered).  A point of
    type "cusp" of a FoldBranch (continuation_fold(..., detect_codim2 > 0)) returns its Cusp record: newton_fold_native in lens1 at
    the located p2 -> q = v / |v|, p = w / <q, w> -> cusp_normal_form_native, ``bls`` the bordered solver of both
    (MatrixFreeBLS(ls, use_pl=True): option fold_bordered).  A point of type "bt" of a HopfBranch (a curve of
    continuation_hopf(..., detect_codim2 > 0) that stopped at omega = 0) returns its BogdanovTakens record: newton_bt_native from
    the recorded state -> bt_jordan_basis -> bogdanov_takens_normal_form_native (``detailed = False``: a and b only); ``ls_adj`` is
    the solver with the preconditioner of the adjoint operator (bt_adjoint_solver), required there."""
    from . import normal_form1d as N1
    sh = N1.is_sh_problem(prob)                     # decided before the branch is looked at
    kind = br.specialpoint[ind].get("type")
    if kind == "gh" and isinstance(br, HopfBranch):
        return _bautin_from_branch(br, ind, prob, ls, tol, max_iterations, norm_inf, bls)
    if kind == "bt" and isinstance(br, HopfBranch):
        return _bt_from_branch(br, ind, prob, ls, ls_adj, tol, max_iterations, norm_inf, seed=seed, detailed=detailed)
    if kind == "cusp" and isinstance(br, FoldBranch):
        return _cusp_from_branch(br, ind, prob, ls, tol, max_iterations, norm_inf, bls)
    if sh and kind in ("bp", "fold"):
        return N1.get_normal_form1d(br, ind, prob, ls, bls=bls, eig=eig, nev=nev, refine=refine, tol=tol,
                                    max_iterations=max_iterations, norm_inf=norm_inf)
    if kind != "hopf":
        raise NotImplementedError(f"get_normal_form: point {ind} is of type {kind!r}; only the Hopf normal form (hopf_normal_form) is "
                                  "available -- fold and branch points have refinement (newton_fold) and fold-curve continuation "
                                  "(continuation_fold), no normal form")
    X = hopf_point(br, ind)
    a, b = hopf_start_vectors(prob, X, ls, eig=eig, nev=nev, seed=seed, bls=bls)
    s = newton_hopf_native(prob, X, a, b, ls, tol=tol, max_iterations=max_iterations, norm_inf=norm_inf, bls=bls)
    if not s["converged"]:
        raise RuntimeError(f"get_normal_form: newton_hopf did not converge from the bisected point (residuals {s['residuals']})")
    zeta, zeta_star = hopf_eigenpair(prob, s)
    return hopf_normal_form_native(prob, s["u"], zeta, zeta_star, ls)


class HopfOrbit:
    """t -> x0 + 2 Re(zeta A(t)) + ds Psi001 + |A(t)|^2 Psi110 + 2 Re(A(t)^2 Psi200), A(t) = amp e^{i t} (:1262-1271), 2 pi
    periodic.  ``orbit(t)`` is one HipVec; ``orbit.slices(M)`` the M equidistant phases t_m = 2 pi m / M, eight per pass over the
    inputs -- the initial guess of a time-discretised periodic orbit."""

    def __init__(self, hopf: Hopf, ds, amp, Psi001, Psi110, Psi200):
        self.hopf, self.ds, self.amp = hopf, float(ds), float(amp)
        self.Psi = (Psi001, Psi110, Psi200)

    def _psi(self):
        P001, P110, P200 = self.Psi
        if P001 is None:                            # no coefficients: the guess from the eigenvector alone (:1253-1260)
            z = self.hopf.x0.zerovector()
            P001, P110, P200 = z, z, (z, z)
        return P001, P110, P200

    def at(self, ts):
        h = self.hopf
        return hopf_orbit(h.x0, h.zeta, *self._psi(), self.ds, self.amp, ts)

    def __call__(self, t: float) -> HipVec:
        return self.at([t])[0]

    def slices(self, M: int):
        return self.at([2.0 * math.pi * m / M for m in range(int(M))])


def predictor(point, *args, **kw):
    """predictor(bp, ds; ampfactor) for a SimpleBranchPoint or Hopf record (below), predictor(bt, "HopfCurve" | "FoldCurve", ds) for
    a BogdanovTakens record (bt_predictor)."""
    if isinstance(point, BogdanovTakens):
        return bt_predictor(point, *args, **kw)
    return _predictor_codim1(point, *args, **kw)


def _predictor_codim1(hopf, ds: float, ampfactor=1.0):
    """predictor(bp, ds; ampfactor).  A SimpleBranchPoint record goes to normal_form1d.predictor (:389-531).  For a Hopf record,
    predictor(hp::Hopf, ds; ampfactor) (:1227-1281): dict(orbit, Psi001, amp, omega, period, p, dsfactor).  With the
    coefficients a, b the side of the Hopf point where the orbits live is dsfactor = +1 when Re a Re b < 0, else -1,
    p = hopf.p + |ds| dsfactor, the amplitude solves Re a dp + Re b amp^2 = 0 and omega is corrected to
    omega + (Im a - Im b Re a / Re b) ds; the returned ``amp`` is twice the one the orbit uses, as in the reference (:1276)."""
    if not isinstance(hopf, Hopf):
        from . import normal_form1d as N1
        return N1.predictor(hopf, ds, ampfactor=ampfactor)
    nf = hopf.nf
    if nf is not None and nf.a is not None and nf.b is not None:
        a, b = complex(nf.a), complex(nf.b)
        if b.real == 0.0:
            raise ValueError(f"The Lyapunov coefficient is zero (b = {b}): the Hopf point is singular, no predictor")
        dsfactor = 1 if a.real * b.real < 0 else -1
        dsnew = abs(ds) * dsfactor
        pnew = hopf.p + dsnew
        amp = ampfactor * math.sqrt(-dsnew * a.real / b.real)
        omega = hopf.omega + (a.imag - b.imag * a.real / b.real) * ds
        P001, P110, P200 = nf.Psi001, nf.Psi110, nf.Psi200
    else:
        amp, omega, pnew, dsfactor = ampfactor, hopf.omega, hopf.p + ds, 1
        P001 = P110 = P200 = None
    return dict(orbit=HopfOrbit(hopf, ds, amp, P001, P110, P200), Psi001=P001, amp=2 * amp, omega=omega,
                period=abs(2 * math.pi / omega), p=pnew, dsfactor=dsfactor)


# ------------------------------------------------------------------------------------------ Bogdanov-Takens points
# src/codim2/MinAugBT.jl and the Bogdanov-Takens part of src/codim2/NormalForms.jl on CGL2d, matrix-free.  J has a double zero
# eigenvalue at the point, so every solve is ONE preconditioned bordered GMRES (MatrixFreeBLS(ls, use_pl=True) semantics); the
# solves with J' take ``ls_adj``, the same solver with the preconditioner of the adjoint operator (bt_adjoint_solver).
#
#   bt_point / bt_start_vectors   the guess a Hopf curve records where it stops at omega = 0, and the reference's default a, b
#   bt_terms, bt_border           the bordered vectors (bk_bt_terms) and the fused pass for sigma_x, sigma_p / A12, A22 (bk_bt_border)
#   newton_bt / newton_bt_native  newton_bt call by call, and as one library call (bk_newton_bt)
#   bt_jordan_basis               (q0, q1), (p0, p1) of NormalForms.jl:603-622
#   bogdanov_takens_normal_form / _native    a, b, gamma, c, K10, K11, K2 (:180-272), call by call and as bk_bt_normal_form
#   predictor(bt, "HopfCurve" | "FoldCurve", ds)   (:342-434);  continuation_hopf_from_bt: the Hopf curve restarted from the point
BTVec = HopfVec                                  # (u, p) with p = [p1, p2]


def bt_adjoint_solver(prob, ls: _GMRES, a: float, b: float):
    """``ls`` with the left preconditioner of the adjoint operator: L0' = Lap (x) I_2 + [[a, b], [-b, a]], the cGL block of
    CGLBlockPreconditioner(prob, a, b) with the sign of its rotation part flipped."""
    import copy
    from .hip import CGLBlockPreconditioner
    out = copy.copy(ls)
    out.Pl = CGLBlockPreconditioner(prob, a, -b)
    return out


def _bt_lenses(prob, lens2):
    if lens2 == prob.lens:
        raise ValueError(f"Please choose 2 different parameters. You only passed {lens2}")
    return prob.param_names.index(prob.lens), prob.param_names.index(lens2)


def _bt_pvec(prob, lens2, p):
    return _params(prob, **{prob.lens: float(p[0]), lens2: float(p[1])})


def bt_border(prob, x: HipVec, pars, ipar1: int, ipar2: int, s: float, v1: HipVec, v2: HipVec, w1: HipVec, w2: HipVec):
    """One fused pass (bk_bt_border): (row1, row2, block) with row1 = s B(x)[v1, .]' w1, row2 = s (B(x)[v1, .]' w2 + B(x)[v2, .]' w1)
    and block[i, k] = s <w1, D_k v1> (i = 0), s (<w2, D_k v1> + <w1, D_k v2>) (i = 1) for the lenses k = (ipar1, ipar2)."""
    ctx = prob.ctx
    r1, r2 = x.similar(), x.similar()
    out = (C.c_double * 4)()
    ctx.check(ctx.lib.bk_bt_border(prob.h, _ptr(x.t), _carr(pars), len(pars), int(ipar1), int(ipar2), float(s), _ptr(v1.t),
                                   _ptr(v2.t), _ptr(w1.t), _ptr(w2.t), _ptr(r1.t), _ptr(r2.t), out), "bk_bt_border")
    return r1, r2, np.array(list(out)).reshape(2, 2)


def bt_terms(prob, x: HipVec, pars, a: HipVec, b: HipVec, ls: _GMRES, ls_adj: _GMRES | None, which="vw"):
    """bk_bt_terms: dict(v1, v2, sigma, w1, w2, converged, itlinear) -- the pair (v1, v2) with sigma when ``which`` has "v", the
    pair (w1, w2) when it has "w" (needs ``ls_adj``, refused with a message when missing); converged / itlinear per solve in the
    order v1, v2, w1, w2."""
    ctx = prob.ctx
    v = (x.similar(), x.similar()) if "v" in which else (None, None)
    w = (x.similar(), x.similar()) if "w" in which else (None, None)
    sg = (C.c_double * 2)()
    cv, it = (C.c_int * 4)(), (C.c_int * 4)()
    lo = ls._opts()
    ctx.check(ctx.lib.bk_bt_terms(ctx.h, prob.h, _ptr(x.t), _carr(pars), len(pars), _ptr(a.t), _ptr(b.t), C.byref(lo), ls._pl(),
                                  ls_adj._pl() if ls_adj is not None else None, _cptr(v[0]), _cptr(v[1]), _cptr(w[0]),
                                  _cptr(w[1]), sg, cv, it), "bk_bt_terms")
    return dict(v1=v[0], v2=v[1], w1=w[0], w2=w[1], sigma=(sg[0], sg[1]) if "v" in which else None,
                converged=[bool(c) for c in cv], itlinear=list(it))


def bt_point(br, ind: int) -> BTVec:
    """bt_point(br, index) (MinAugBT.jl:59-65): the recorded stop state of the Hopf curve as BTVec(x, [p1, p2])."""
    sp = br.specialpoint[ind]
    if sp.get("type") != "bt":
        raise ValueError(f"This should be a BT point.\nYou passed a {sp.get('type')} point.")
    return BTVec(sp["x"].copy(), [sp["p1"], sp["p2"]])


def bt_start_vectors(prob, X: BTVec, lens2: str, ls: _GMRES, ls_adj: _GMRES, seed=0):
    """(a, b) of newton_bt(br, ind) without start_with_eigen (:417-435): random a, b, then a = w1 / |w1|, b = v1 / |v1| of the
    bordered solves at the guess."""
    rng = np.random.default_rng(seed)
    x = X.u
    a = HipVec.from_numpy(prob.ctx, rng.random(x.n), x.nglobal)
    b = HipVec.from_numpy(prob.ctx, rng.random(x.n), x.nglobal)
    t = bt_terms(prob, x, _bt_pvec(prob, lens2, X.p), a, b, ls, ls_adj)
    return t["w1"].scale_(1.0 / t["w1"].norm()), t["v1"].scale_(1.0 / t["v1"].norm())


def _norm_bt(F, sigma, norm_inf):
    if norm_inf:
        return _nanmax(F.norminf(), abs(sigma[0]), abs(sigma[1]))
    return math.sqrt(F.norm() ** 2 + sigma[0] ** 2 + sigma[1] ** 2)


def newton_bt(prob, guess: BTVec, lens2: str, a: HipVec, b: HipVec, ls: _GMRES, ls_adj: _GMRES, tol=1e-10, max_iterations=25,
              norm_inf=False):
    """newton_bt with BTLinearSolverMinAug under _newton, call by call: per point bk_bt_terms for (v1, v2, sigma) and the residual;
    per step bk_bt_terms for (w1, w2), one bk_bt_border pass (s = -1) for sigma_x and sigma_p, and ONE block-bordered solve
    MatrixFreeBLS(ls, use_pl=True).solve_block(J, (dp1F, dp2F), (sigma1_x, sigma2_x), sigma_p, F, sigma)."""
    i1, i2 = _bt_lenses(prob, lens2)
    if ls_adj is None or ls_adj._pl() is None:
        raise TypeError("newton_bt needs ls_adj, the solver with the left preconditioner of the adjoint operator (bt_adjoint_solver)")
    bls = MatrixFreeBLS(ls, use_pl=True)
    x, p = guess.u.copy(), np.array(guess.p, dtype=np.float64)
    its, bad = [0] * 5, 0
    state = {}

    def point():
        nonlocal bad
        pv = _bt_pvec(prob, lens2, p)
        t = bt_terms(prob, x, pv, a, b, ls, None, "v")
        its[0] += t["itlinear"][0]; its[1] += t["itlinear"][1]
        bad += sum(not c for c in t["converged"][:2])
        state["pv"] = pv
        return residual(prob, x, pv), t["sigma"], t["v1"], t["v2"]

    def update(F, sigma, v1, v2):
        nonlocal bad
        pv = state["pv"]
        t = bt_terms(prob, x, pv, a, b, ls, ls_adj, "w")
        r1, r2, sp = bt_border(prob, x, pv, i1, i2, -1.0, v1, v2, t["w1"], t["w2"])
        J = HipJacobian(prob, x, pv)
        dX, dp, cv, it = bls.solve_block(J, (dpF(prob, x, pv, i1), dpF(prob, x, pv, i2)), (r1, r2), sp, F, sigma)
        its[2] += t["itlinear"][2]; its[3] += t["itlinear"][3]; its[4] += it
        bad += sum(not c for c in t["converged"][2:]) + (0 if cv else 1)
        state["w"] = (t["w1"], t["w2"])
        x.add_(dX, -1.0)
        p[0] -= dp[0]
        p[1] -= dp[1]

    (F, sigma, v1, v2), res, step = _newton_minaug_mirror(point, update, lambda F, sg: _norm_bt(F, sg, norm_inf), tol, max_iterations)
    w1, w2 = state.get("w", (None, None))
    return dict(u=BTVec(x, p), converged=res[-1] < tol, itnewton=step, itlineartot=sum(its), itsolves=its, residuals=res, v1=v1,
                v2=v2, w1=w1, w2=w2, sigma=sigma, unconverged_solves=bad)


def newton_bt_native(prob, guess: BTVec, lens2: str, a: HipVec, b: HipVec, ls: _GMRES, ls_adj: _GMRES, tol=1e-10,
                     max_iterations=25, norm_inf=False, callback=None):
    """The same as one library call (bk_newton_bt).  The double zero eigenvalue of J at the returned point moves like the square
    root of what the last update leaves, the error of the linear solves included: give ``ls`` an rtol well below ``tol`` (the tests
    run 1e-13 under tol = 1e-10 and find |lambda| <= 5e-7)."""
    i1, i2 = _bt_lenses(prob, lens2)
    ctx = prob.ctx
    x = guess.u.copy()
    p = (C.c_double * 2)(float(guess.p[0]), float(guess.p[1]))
    pv = _bt_pvec(prob, lens2, guess.p)
    v1, v2, w1, w2 = x.similar(), x.similar(), x.similar(), x.similar()
    sigma = (C.c_double * 2)()
    its, bad = (C.c_int * 5)(), C.c_int()
    no = newton_opts(tol, max_iterations, norm_inf, callback=callback)
    lo = ls._opts()
    res = L.NewtonResult()
    ctx.check(ctx.lib.bk_newton_bt(ctx.h, prob.h, _ptr(x.t), p, _carr(pv), len(pv), i1, i2, _ptr(a.t), _ptr(b.t), C.byref(no),
                                   C.byref(lo), ls._pl(), ls_adj._pl() if ls_adj is not None else None, _ptr(v1.t), _ptr(v2.t),
                                   _ptr(w1.t), _ptr(w2.t), sigma, C.byref(res), its, C.byref(bad)), "bk_newton_bt")
    return dict(u=BTVec(x, [p[0], p[1]]), converged=bool(res.converged), itnewton=res.itnewton, itlineartot=res.itlinear,
                itsolves=list(its), residuals=[res.residuals[i] for i in range(res.itnewton + 1)], v1=v1, v2=v2,
                w1=w1 if res.itnewton else None, w2=w2 if res.itnewton else None, sigma=(sigma[0], sigma[1]),
                unconverged_solves=bad.value)


@dataclass
class BogdanovTakens:
    """BogdanovTakens (src/NormalForms.jl): x0, params, lens = (lens1, lens2), ipars = the indices of the two lenses in params, zeta = (q0, q1),
    zeta_star = (p0, p1), newton = the result of the refinement that led here (get_normal_form), nf =
    dict(a, b[, gamma, c, K10, K11, K2, H2000, H1100, H0010, H0001]) or None, converged / itlinear per solve of the normal form,
    ``basis`` = the Gram matrices of the Jordan basis (<p_i, q_j>, <p_i, J q_j>)."""
    x0: HipVec
    params: list
    lens: tuple
    ipars: tuple
    zeta: tuple
    zeta_star: tuple
    nf: dict | None = None
    converged: list = field(default_factory=list)
    itlinear: list = field(default_factory=list)
    basis: tuple | None = None
    newton: dict | None = None

    @property
    def p(self):
        return np.array([self.params[i] for i in self.ipars])


def bt_jordan_basis(prob, X: BTVec, lens2: str, vr: HipVec, vl: HipVec, ls: _GMRES, ls_adj: _GMRES) -> BogdanovTakens:
    """The basis (q0, q1), (p0, p1) of NormalForms.jl:603-622 at X from guesses vr, vl of the right and left null vectors: four
    bordered solves (two with J, two with J') and the normalisation, J q0 = 0, J q1 = q0, J' p1 = 0, J' p0 = p1,
    <p_i, q_j> = delta_ij.  Warns, as the reference does (:174-178), when a Gram matrix is off by more than 1e-5."""
    import warnings
    i1, i2 = _bt_lenses(prob, lens2)
    pv = _bt_pvec(prob, lens2, X.p)
    x = X.u
    J, Jt = HipJacobian(prob, x, pv), HipJacobian(prob, x, pv, adjoint=True)
    bl, bla = MatrixFreeBLS(ls, use_pl=True), MatrixFreeBLS(ls_adj, use_pl=True)
    zero = x.zerovector()
    cvs, its = [], []

    def run(b_, *args):
        y, _, cv, it = b_(*args)
        cvs.append(cv); its.append(it)
        return y

    q0 = run(bl, J, vl, vr, 0.0, zero, 1.0)
    p1 = run(bla, Jt, vr, vl, 0.0, zero, 1.0)
    q1 = run(bl, J, p1, q0, 0.0, q0, 0.0)
    p0 = run(bla, Jt, q0, p1, 0.0, p1, 0.0)
    mu = math.sqrt(abs(q0.inner(q0)))
    q0.scale_(1.0 / mu)
    q1.scale_(1.0 / mu)
    q1.add_(q0, -q0.inner(q1))
    nu = q0.inner(p0)
    p1.scale_(1.0 / nu)
    p0.add_(p1, -p0.inner(q1))
    p0.scale_(1.0 / nu)
    G = np.array([[ps.inner(q) for q in (q0, q1)] for ps in (p0, p1)])
    Jq = [J(q0), J(q1)]
    GJ = np.array([[ps.inner(jq) for jq in Jq] for ps in (p0, p1)])
    if np.abs(G - np.eye(2)).max() > 1e-5:
        warnings.warn(f"G == I(2) is not valid. We built a basis such that G = {G}")
    if np.abs(GJ - np.array([[0.0, 1.0], [0.0, 0.0]])).max() > 1e-5:
        warnings.warn(f"G is not close to the Jordan block of size 2. We built a basis such that G = {GJ}")
    return BogdanovTakens(x.copy(), pv, (prob.lens, lens2), (i1, i2), (q0, q1), (p0, p1), None, cvs, its, (G, GJ))


def bt_nf_dots(prob, x: HipVec, pars, q0, q1, p0, p1):
    """One pass (bk_bt_nf_dots): <p1, B00>, <p0, B00>, <p1, B01>, <p0, B01>, <p1, B11>, <p0, B11> with Bij = d2F(x)[qi, qj]."""
    ctx = prob.ctx
    out = (C.c_double * 6)()
    ctx.check(ctx.lib.bk_bt_nf_dots(prob.h, _ptr(x.t), _carr(pars), len(pars), _ptr(q0.t), _ptr(q1.t), _ptr(p0.t), _ptr(p1.t), out),
              "bk_bt_nf_dots")
    return list(out)


def bt_nf_rhs(prob, x: HipVec, pars, mode: int, k: float, q0: HipVec, q1: HipVec, H: HipVec | None = None) -> HipVec:
    """One pass (bk_bt_nf_rhs): mode 0: k q1 - B(q0, q0); mode 1: k q1 + H - B(q0, q1)."""
    return _into_similar(prob, "bk_bt_nf_rhs", x, pars, int(mode), float(k), _ptr(q0.t), _ptr(q1.t), _cptr(H))


def bt_nf_k2(prob, x: HipVec, pars, ipar1: int, ipar2: int, p1: HipVec, H0001: HipVec):
    """One pass (bk_bt_nf_k2): <p1, B(H0001, H0001)>, <p1, D_1 H0001>, <p1, D_2 H0001>."""
    ctx = prob.ctx
    out = (C.c_double * 3)()
    ctx.check(ctx.lib.bk_bt_nf_k2(prob.h, _ptr(x.t), _carr(pars), len(pars), int(ipar1), int(ipar2), _ptr(p1.t), _ptr(H0001.t), out),
              "bk_bt_nf_k2")
    return list(out)


def _bt_nf_dict(vals, H=None):
    nf = dict(a=vals[0], b=vals[1])
    if H is not None:
        nf.update(gamma=vals[2], c=vals[3], K10=np.array(vals[4:6]), K11=np.array(vals[6:8]), K2=np.array(vals[8:10]),
                  H2000=H[0], H1100=H[1], H0010=H[2], H0001=H[3])
    return nf


def bogdanov_takens_normal_form(prob, bt: BogdanovTakens, ls: _GMRES, detailed=True) -> BogdanovTakens:
    """bogdanov_takens_normal_form (NormalForms.jl:141-335) through K2, call by call: bt_nf_dots for a, b (detailed = False returns
    here), then bt_nf_rhs + MatrixFreeBLS(ls, use_pl=True)(J, p1, q0, 0, rhs, 0) for H2000 and H1100, one bt_border pass (s = +1 on
    (q0, q1, p1, p0)) for A12 and A22, two solve_block calls for (H0010, K10) and (H0001, K11), bt_nf_k2 for K2.  a and b keep the
    orientation of the basis as computed.  The coefficients of the homoclinic predictor are not computed."""
    import dataclasses
    x, pv = bt.x0, bt.params
    i1, i2 = bt.ipars
    (q0, q1), (p0, p1) = bt.zeta, bt.zeta_star
    d = bt_nf_dots(prob, x, pv, q0, q1, p0, p1)
    a, b = 0.5 * d[0], d[1] + d[2]
    if not detailed:
        return dataclasses.replace(bt, nf=_bt_nf_dict([a, b]), converged=[], itlinear=[])
    bls = MatrixFreeBLS(ls, use_pl=True)
    J = HipJacobian(prob, x, pv)
    cvs, its = [], []
    H2000, _, cv, it = bls(J, p1, q0, 0.0, bt_nf_rhs(prob, x, pv, 0, 2.0 * a, q0, q1), 0.0)
    cvs.append(cv); its.append(it)
    gamma = (-2.0 * p0.inner(H2000) + 2.0 * d[3] + d[4]) / 2.0
    H2000.add_(q0, gamma)
    H1100, _, cv, it = bls(J, p1, q0, 0.0, bt_nf_rhs(prob, x, pv, 1, b, q0, q1, H2000), 0.0)
    cvs.append(cv); its.append(it)
    c = 3.0 * p0.inner(H1100) - d[5]
    r1, r2, A22 = bt_border(prob, x, pv, i1, i2, 1.0, q0, q1, p1, p0)
    J1s = (dpF(prob, x, pv, i1), dpF(prob, x, pv, i2))
    H0010, K10, cv, it = bls.solve_block(J, J1s, (r1, r2), A22, q1, (d[4] / 2.0, c))
    cvs.append(cv); its.append(it)
    H0001, K11, cv, it = bls.solve_block(J, J1s, (r1, r2), A22, x.zerovector(), (0.0, 1.0))
    cvs.append(cv); its.append(it)
    # every cGL parameter enters F linearly: J2_11 = J2_12 = J2_22 = 0 exactly, so kappa3 (:270-271) is dropped
    k = bt_nf_k2(prob, x, pv, i1, i2, p1, H0001)
    f = -(k[0] + 2.0 * (k[1] * K11[0] + k[2] * K11[1]))
    vals = [a, b, gamma, c, K10[0], K10[1], K11[0], K11[1], f * K10[0], f * K10[1]]
    return dataclasses.replace(bt, nf=_bt_nf_dict(vals, (H2000, H1100, H0010, H0001)), converged=cvs, itlinear=its)


def bogdanov_takens_normal_form_native(prob, bt: BogdanovTakens, ls: _GMRES, detailed=True) -> BogdanovTakens:
    """The same as one library call (bk_bt_normal_form)."""
    import dataclasses
    ctx, x, pv = prob.ctx, bt.x0, bt.params
    i1, i2 = bt.ipars
    (q0, q1), (p0, p1) = bt.zeta, bt.zeta_star
    H = [x.similar() for _ in range(4)] if detailed else [None] * 4
    nf = (C.c_double * 10)()
    cv, it = (C.c_int * 4)(), (C.c_int * 4)()
    lo = ls._opts()
    ctx.check(ctx.lib.bk_bt_normal_form(ctx.h, prob.h, _ptr(x.t), _carr(pv), len(pv), i1, i2, _ptr(q0.t), _ptr(q1.t), _ptr(p0.t),
                                        _ptr(p1.t), 1 if detailed else 0, C.byref(lo), ls._pl(), *[_cptr(h) for h in H], nf, cv,
                                        it), "bk_bt_normal_form")
    if not detailed:
        return dataclasses.replace(bt, nf=_bt_nf_dict(list(nf)), converged=[], itlinear=[])
    return dataclasses.replace(bt, nf=_bt_nf_dict(list(nf), H), converged=[bool(c) for c in cv], itlinear=list(it))


def _bt_from_branch(br, ind: int, prob, ls: _GMRES, ls_adj: _GMRES, tol, max_iterations, norm_inf, seed=0, detailed=True,
                    native=True) -> BogdanovTakens:
    """newton_bt_native from the "bt" point of a Hopf curve -> Jordan basis from the bordered vectors of the refined point ->
    normal form there (the project's convention: the normal form is taken at the REFINED point)."""
    if ls_adj is None:
        raise TypeError('get_normal_form on a "bt" point needs ls_adj, the solver with the left preconditioner of the adjoint '
                        "operator (bt_adjoint_solver)")
    X = bt_point(br, ind)
    with _lens2_at(prob, br.lens2, X.p[1]), _solver_state_kept(prob.ctx):
        a, b = bt_start_vectors(prob, X, br.lens2, ls, ls_adj, seed=seed)
        s = (newton_bt_native if native else newton_bt)(prob, X, br.lens2, a, b, ls, ls_adj, tol=tol, max_iterations=max_iterations,
                                                         norm_inf=norm_inf)
        if not s["converged"]:
            raise RuntimeError(f"get_normal_form: newton_bt did not converge from the recorded point (residuals {s['residuals']})")
        pv = _bt_pvec(prob, br.lens2, s["u"].p)
        w1 = bt_terms(prob, s["u"].u, pv, a, b, ls, ls_adj, "w")["w1"]
        bt = bt_jordan_basis(prob, s["u"], br.lens2, s["v1"], w1, ls, ls_adj)
        f = bogdanov_takens_normal_form_native if native else bogdanov_takens_normal_form
        bt = f(prob, bt, ls, detailed=detailed)
    import dataclasses
    return dataclasses.replace(bt, newton=s)


def _bt_getx(a: float, s: float) -> float:
    return -math.sqrt(abs(s) / a) if a > 0 else math.sqrt(abs(s) / abs(a))


def bt_predictor(bt: BogdanovTakens, curve: str, ds: float):
    """predictor(bt, Val(:HopfCurve), ds) (:342-400) and predictor(bt, Val(:FoldCurve), ds) (:408-434) evaluated at ds:
    dict(pars = the predicted (p1, p2), omega (Hopf curve only), EigenVec, EigenVecAd, x0 = the predicted offset of the state).
    On the Hopf curve the eigenvectors are (re, im) pairs: the eigenvector of [[0, 1], [2 x a, 0]] for +i omega (its adjoint's for
    -i omega) in the basis (q0, q1) ((p0, p1)), formed with axpby calls."""
    nf = bt.nf
    if nf is None or "K10" not in nf:
        raise ValueError("the predictor needs the detailed normal form (K10, K11, K2)")
    a, b = nf["a"], nf["b"]
    (q0, q1), (p0, p1) = bt.zeta, bt.zeta_star
    xx = _bt_getx(a, ds)
    if curve == "FoldCurve":
        pars = bt.p + nf["K11"] * ds + nf["K2"] * (ds ** 2 / 2)
        return dict(pars=pars, EigenVec=q0, EigenVecAd=p1, x0=q0.copy().scale_(xx))
    if curve != "HopfCurve":
        raise ValueError(f'predictor(bt, curve, ds): curve is "HopfCurve" or "FoldCurve" (got {curve!r}); the homoclinic predictor '
                         "is not available")
    beta1 = -abs(ds) if a > 0 else abs(ds)
    beta2 = -b * xx
    pars = bt.p + nf["K10"] * beta1 + nf["K11"] * beta2 + nf["K2"] * (beta2 ** 2 / 2)
    A = np.array([[0.0, 1.0], [2 * xx * a, 0.0]])
    vals, vecs = np.linalg.eig(A)
    h = vecs[:, int(np.argmax(vals.imag))]
    vals, vecs = np.linalg.eig(A.T)
    ha = vecs[:, int(np.argmin(vals.imag))]
    comb = lambda u0, u1, c: (u0.copy().scale_(c[0].real).add_(u1, c[1].real), u0.copy().scale_(c[0].imag).add_(u1, c[1].imag))
    return dict(pars=pars, omega=math.sqrt(-2 * xx * a), EigenVec=comb(q0, q1, h), EigenVecAd=comb(p0, p1, ha),
                x0=q0.copy().scale_(xx))


def continuation_hopf_from_bt(bt: BogdanovTakens, prob, ls: _GMRES, cp: Cn.ContinuationPar, ds: float, newton_tol=None,
                              max_iterations=15, bls=None, **kw):
    """The Hopf curve restarted FROM the Bogdanov-Takens point: the Hopf-curve predictor at ``ds`` -> newton_hopf_native from
    (x0 + predicted offset, p1, omega) with the predicted a = EigenVecAd, b = EigenVec at the predicted p2 -> continuation_hopf in
    lens2 from the point it lands on.  Returns (branch, the newton_hopf_native result, the predictor)."""
    lens1, lens2 = bt.lens
    if prob.lens != lens1:
        raise ValueError(f"the problem's lens is {prob.lens!r}, the first lens of the Bogdanov-Takens point is {lens1!r}")
    pr = bt_predictor(bt, "HopfCurve", ds)
    nrm = lambda z: _cscale(z, 1.0 / cnorm(z))
    a, b = nrm(pr["EigenVecAd"]), nrm(pr["EigenVec"])
    X0 = HopfVec(bt.x0.copy().add_(pr["x0"], 1.0), [pr["pars"][0], pr["omega"]])
    tol = cp.newton_options.tol if newton_tol is None else newton_tol
    with _lens2_at(prob, lens2, pr["pars"][1]):
        s = newton_hopf_native(prob, X0, a, b, ls, tol=tol, max_iterations=max_iterations, bls=bls)
        if not s["converged"]:
            raise RuntimeError(f"continuation_hopf_from_bt: newton_hopf did not converge from the predictor (residuals {s['residuals']})")
        a2, b2 = nrm(s["w"]), nrm(s["v"])
        br = continuation_hopf(prob, s["u"], float(pr["pars"][1]), lens2, a2, b2, ls, cp, bls=bls, **kw)
    return br, s, pr
