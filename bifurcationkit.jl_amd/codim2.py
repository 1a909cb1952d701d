"""Fold points: refinement and two-parameter continuation with the minimally augmented formulation of
src/codim2/MinAugFold.jl, matrix-free on the preconditioned GMRES path (the reference assembles the system for MatrixBLS /
MinAugMatrixBased, which cannot run at the sizes of this library).

  FoldProblem              FoldMinimallyAugmentedFormulation + FoldMAProblem: G(X, p2) = (F(x, p1), sigma(x, p1)), X = (x, p1)
  FoldLinearSolverMinAug   foldMALinearSolver, usehessian branch (:119-166): one or two right-hand sides, one shared J \\ dpF
  fold_point               fold_point(br, ind) (:6-13) on a Python branch record, with the start vector a = b = tau
  newton_fold              newton_fold (:211-278) written out call by call on HipVecs (bk_d2f, bk_djdp, ls(J, r1, r2), BorderingBLS)
  newton_fold_native       the same as one library call (bk_newton_fold)
  continuation_fold        continuation_fold (:369-536): PALC on G(X, p2), BorderingBLS(solver = FoldLinearSolverMinAug,
                           check_precision = false) as wired at :445-453, Secant tangent, a / b updated after every step
                           (update!, :280-313), BT = <zeta*, zeta> and CP = tau.p recorded (test_bt_cusp, :551-576)

Problems: SwiftHohenberg (2-D / 3-D) and SwiftHohenberg1D -- symmetric, J' = J (:79-84).  sigma_p, dpF and sigma_x are analytic
(the Jacobians depend on the parameters only through their pointwise term), where the reference takes central differences.
The bordered vectors v, w of a point are solved once and serve both its residual and its Newton step.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _lib as L
from . import continuation as Cn
from .hip import BorderedArray, BorderingBLS, HipVec, _GMRES, _ptr, newton_opts


def _norm_fold(F, sigma, norm_inf):
    """normN of BorderedArray(F, sigma): norminf = max(|F|_inf, |sigma|), norm = sqrt(|F|^2 + sigma^2)."""
    return max(F.norminf(), abs(sigma)) if norm_inf else math.sqrt(F.norm() ** 2 + sigma ** 2)


def _params(prob, **vals):
    pv = dict(prob.params)
    pv.update({k: float(v) for k, v in vals.items()})
    return [float(pv[k]) for k in prob.param_names]


def d2F(prob, x: HipVec, pars, dx1: HipVec, dx2: HipVec) -> HipVec:
    """d2F(prob, x, par, dx1, dx2) (src/Problems.jl:107,165) on the device (bk_d2f)."""
    ctx, out = prob.ctx, x.similar()
    arr = (C.c_double * len(pars))(*pars)
    ctx.check(ctx.lib.bk_d2f(prob.h, _ptr(x.t), arr, len(pars), _ptr(dx1.t), _ptr(dx2.t), _ptr(out.t)), "bk_d2f")
    return out


def dJdp(prob, x: HipVec, pars, ipar: int, dx: HipVec) -> HipVec:
    """dJ/dp(x) dx for params[ipar] (bk_djdp): the analytic value of dJvdp in _get_bordered_terms (:93-94)."""
    ctx, out = prob.ctx, x.similar()
    arr = (C.c_double * len(pars))(*pars)
    ctx.check(ctx.lib.bk_djdp(prob.h, _ptr(x.t), arr, len(pars), int(ipar), _ptr(dx.t), _ptr(out.t)), "bk_djdp")
    return out


def fold_contract(prob, x: HipVec, pars, ipar: int, v: HipVec, w: HipVec, X=()):
    """One fused pass (bk_fold_contract): ([<w, d2F(x)[v, X_k]> for X_k in X], -<w, dJ/dp v>)."""
    ctx = prob.ctx
    m = len(X)
    arr = (C.c_double * len(pars))(*pars)
    xp = (C.c_void_p * max(m, 1))(*[t.t.data_ptr() for t in X])
    out = (C.c_double * (m + 1))()
    ctx.check(ctx.lib.bk_fold_contract(prob.h, _ptr(x.t), arr, len(pars), int(ipar), _ptr(v.t), _ptr(w.t), m, xp, out),
              "bk_fold_contract")
    return [out[k] for k in range(m)], out[m]


def residual(prob, x: HipVec, pars) -> HipVec:
    """F(x, pars) with every parameter given (bk_residual)."""
    ctx, out = prob.ctx, x.similar()
    arr = (C.c_double * len(pars))(*pars)
    ctx.check(ctx.lib.bk_residual(prob.h, _ptr(x.t), arr, len(pars), _ptr(out.t)), "bk_residual")
    return out


def dpF(prob, x: HipVec, pars, ipar: int) -> HipVec:
    """Analytic dF/dp for params[ipar].  bk_residual_dparam evaluates ((p + eps) - p) / eps * phi_p(x) and phi_p does not
    depend on the parameters, so with p = 0 and eps = 1 the scalar is exactly 1."""
    ctx, out = prob.ctx, x.similar()
    pv = list(pars)
    pv[ipar] = 0.0
    arr = (C.c_double * len(pv))(*pv)
    ctx.check(ctx.lib.bk_residual_dparam(prob.h, _ptr(x.t), arr, len(pv), int(ipar), 1.0, _ptr(out.t)), "bk_residual_dparam")
    return out


def _bls_opts(bls: BorderingBLS):
    return L.BorderingOpts(bls.tol, 1 if bls.check_precision else 0, bls.k, 0)


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
def newton_fold(prob, x0: HipVec, p0: float, a: HipVec, b: HipVec, ls: _GMRES, bls: BorderingBLS | None = None, tol=1e-12,
                max_iterations=25, norm_inf=False):
    """newton_fold (:211-233) with FoldLinearSolverMinAug under _newton (src/Newton.jl:66-114), call by call on the plugin
    surface: the residual (:16-38) solves bls(J, a, b, 0, 0, 1) for (v, sigma) and bls(J', b, a, 0, 0, 1) for w (no second
    solve when ``a is b``: J' = J); each Newton step is foldMALinearSolver's usehessian branch (:146-164) with ls(J, F, dpF),
    d2F + inner for sigma_x and dJ/dp v + inner for sigma_p.  v, w of a point serve its residual and its step."""
    bls = bls if bls is not None else BorderingBLS(ls, check_precision=False)
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

    F, sigma, v, w = point()
    res = [_norm_fold(F, sigma, norm_inf)]
    step = 0
    while step < max_iterations and res[-1] > tol:
        pars = prob._pvec(p)
        J = prob.jacobian(x, p)
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
        F, sigma, v, w = point()
        res.append(_norm_fold(F, sigma, norm_inf))
        step += 1
    return dict(u=BorderedArray(x, p), converged=res[-1] < tol, itnewton=step, itlineartot=itlin, residuals=res, v=v,
                w=w.copy() if w is v else w, sigma=sigma, unconverged_solves=bad)


def newton_fold_native(prob, x0: HipVec, p0: float, a: HipVec, b: HipVec, ls: _GMRES, bls: BorderingBLS | None = None,
                       tol=1e-12, max_iterations=25, norm_inf=False, callback=None):
    """The same as one library call (bk_newton_fold)."""
    bls = bls if bls is not None else BorderingBLS(ls, check_precision=False)
    ctx = prob.ctx
    x = x0.copy()
    p = C.c_double(float(p0))
    pv = prob._pvec(p0)
    arr = (C.c_double * len(pv))(*pv)
    v, w = x.similar(), x.similar()
    sigma = C.c_double()
    no = newton_opts(tol, max_iterations, norm_inf, callback=callback)
    bo, lo = _bls_opts(bls), ls._opts()
    res = L.NewtonResult()
    bad0 = ctx.get_option("fold_unconverged_solves")
    ctx.check(ctx.lib.bk_newton_fold(ctx.h, prob.h, _ptr(x.t), C.byref(p), arr, len(pv), prob.ipar, _ptr(a.t), _ptr(b.t),
                                     C.byref(no), C.byref(bo), C.byref(lo), ls._pl(), _ptr(v.t), _ptr(w.t), C.byref(sigma),
                                     C.byref(res)), "bk_newton_fold")
    return dict(u=BorderedArray(x, p.value), converged=bool(res.converged), itnewton=res.itnewton, itlineartot=res.itlinear,
                residuals=[res.residuals[i] for i in range(res.itnewton + 1)], v=v, w=w, sigma=sigma.value,
                unconverged_solves=int(ctx.get_option("fold_unconverged_solves") - bad0))


# ------------------------------------------------------------------------------------------ the fold problem G(X, p2)
class FoldProblem:
    """FoldMinimallyAugmentedFormulation(prob, a, b, ...) + FoldMAProblem with lens2 (src/codim2/MinAugFold.jl,
    continuation_fold :407-453): unknown X = BorderedArray(x, p1) (p1 = the problem's lens), parameter p2 = ``lens2``.
    ``residual`` / ``jacobian`` / ``residual_dparam`` are the BifurcationProblem surface continuation.newton_palc drives;
    the bordered vectors of a point are cached and solved once per point (bk_fold_terms)."""

    def __init__(self, prob, lens2: str, a: HipVec, b: HipVec, ls: _GMRES, bls: BorderingBLS | None = None):
        if lens2 == prob.lens:
            raise ValueError(f"Please choose 2 different parameters. You only passed {lens2}")
        self.prob, self.ctx = prob, prob.ctx
        self.lens1, self.lens2 = prob.lens, lens2
        self.ipar1, self.ipar2 = prob.param_names.index(prob.lens), prob.param_names.index(lens2)
        self.ls = ls
        self.bls = bls if bls is not None else BorderingBLS(ls, check_precision=False)
        self.a, self.b = a, b
        self.delta = prob.delta
        self.itlinear = 0                       # GMRES counts of the bordered-vector solves (the linear solver counts its own)
        self._cache = None

    def pvec(self, p1, p2):
        return _params(self.prob, **{self.lens1: p1, self.lens2: p2})

    def terms(self, X: BorderedArray, p2: float):
        """(v, w, sigma) of _compute_bordered_vectors at (X, p2), solved once per point."""
        c = self._cache
        if c is not None and c[1] == X.p and c[2] == p2 and torch.equal(c[0].t, X.u.t):
            return c[3]
        ctx = self.ctx
        pv = self.pvec(X.p, p2)
        arr = (C.c_double * len(pv))(*pv)
        v = X.u.similar()
        w = v if self.a is self.b else X.u.similar()
        sigma, cv = C.c_double(), C.c_int()
        it = (C.c_int * 2)()
        bo, lo = _bls_opts(self.bls), self.ls._opts()
        ctx.check(ctx.lib.bk_fold_terms(ctx.h, self.prob.h, _ptr(X.u.t), arr, len(pv), self.ipar1, _ptr(self.a.t),
                                        _ptr(self.b.t), C.byref(bo), C.byref(lo), self.ls._pl(), _ptr(v.t), _ptr(w.t),
                                        C.byref(sigma), None, C.byref(cv), it), "bk_fold_terms")
        self.itlinear += it[0] + it[1]
        t = (v, w, sigma.value)
        self._cache = (X.u.copy(), X.p, p2, t)
        return t

    def residual(self, X: BorderedArray, p2: float) -> BorderedArray:
        _, _, sigma = self.terms(X, p2)
        return BorderedArray(residual(self.prob, X.u, self.pvec(X.p, p2)), sigma)

    def residual_dparam(self, X: BorderedArray, p2: float, eps=None) -> BorderedArray:
        """dG/dp2 = (dF/dp2, -<w, dJ/dp2 v>), analytic (the reference differentiates G by finite differences)."""
        v, w, _ = self.terms(X, p2)
        pv = self.pvec(X.p, p2)
        _, sp2 = fold_contract(self.prob, X.u, pv, self.ipar2, v, w)
        return BorderedArray(dpF(self.prob, X.u, pv, self.ipar2), sp2)

    def jacobian(self, X: BorderedArray, p2: float):
        return JacobianFold(self, X, p2)

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
        return bt


@dataclass
class JacobianFold:
    """What jacobian(FoldMAProblem, X, p2) hands to FoldLinearSolverMinAug: the point (no matrix)."""
    fold: FoldProblem
    X: BorderedArray
    p2: float


class FoldLinearSolverMinAug:
    """FoldLinearSolverMinAug (:168-178) -> foldMALinearSolver, usehessian branch (:146-164) as bk_fold_linsolve.
    ``solve2`` serves both right-hand sides of the BorderingBLS BEC with ONE J \\ dpF solve: three GMRES solves where the
    reference runs four."""

    def _run(self, Jf: JacobianFold, rhs):
        F = Jf.fold
        v, w, _ = F.terms(Jf.X, Jf.p2)
        ctx = F.ctx
        pv = F.pvec(Jf.X.p, Jf.p2)
        arr = (C.c_double * len(pv))(*pv)
        m = len(rhs)
        dX = [Jf.X.u.similar() for _ in range(m)]
        ru = (C.c_void_p * m)(*[r.u.t.data_ptr() for r in rhs])
        rp = (C.c_double * m)(*[float(r.p) for r in rhs])
        dxp = (C.c_void_p * m)(*[d.t.data_ptr() for d in dX])
        ds = (C.c_double * m)()
        cv, it = C.c_int(), C.c_int()
        lo = F.ls._opts()
        ctx.check(ctx.lib.bk_fold_linsolve(ctx.h, F.prob.h, _ptr(Jf.X.u.t), arr, len(pv), F.ipar1, _ptr(v.t), _ptr(w.t), m,
                                           ru, rp, C.byref(lo), F.ls._pl(), dxp, ds, C.byref(cv), C.byref(it)),
                  "bk_fold_linsolve")
        return [BorderedArray(dX[k], ds[k]) for k in range(m)], bool(cv.value), it.value

    def __call__(self, Jf: JacobianFold, rhs: BorderedArray, a0=0.0, a1=1.0):
        out, cv, it = self._run(Jf, [rhs])
        return out[0], cv, it

    def solve2(self, Jf: JacobianFold, rhs1: BorderedArray, rhs2: BorderedArray, a0=0.0, a1=1.0):
        out, cv, it = self._run(Jf, [rhs1, rhs2])
        return out[0], out[1], cv, (it, 0)


# ------------------------------------------------------------------------------------------ continuation_fold
@dataclass
class FoldBranch:
    """The record of continuation_fold (record_from_solution, :330-346): p1 (lens1), p2 (lens2), BT, CP per point."""
    p1: list = field(default_factory=list)
    p2: list = field(default_factory=list)
    BT: list = field(default_factory=list)
    CP: list = field(default_factory=list)
    ds: list = field(default_factory=list)
    itnewton: list = field(default_factory=list)
    itlinear: list = field(default_factory=list)
    residuals: list = field(default_factory=list)
    sol: list = field(default_factory=list)


def _norminf_fold(z):
    return max(z.u.norminf(), abs(z.p))


def continuation_fold(prob, fold_guess: BorderedArray, p2: float, lens2: str, a: HipVec, b: HipVec, ls: _GMRES,
                      cp: Cn.ContinuationPar, theta=0.5, norm_inf=True, update_minaug_every_step=1, save_sol=False,
                      ds_sequence=None, verbosity=0) -> FoldBranch:
    """continuation_fold(prob, alg = PALC(tangent = Secant()), foldpointguess, par, lens1, lens2, a, b, options_cont) (:369-453):
    PALC on G(X, p2) through continuation.newton_palc with BorderingBLS(solver = FoldLinearSolverMinAug(), check_precision =
    false) (:445-453), Secant tangent only (the reference warns against Bordered on folds, :390-392), the two starting points of
    continuation (Continuation.jl:349-456) by newton on G, step-size control of continuation.py.  After every converged step a, b
    are updated (update_minaug_every_step = 1) and BT, CP recorded.  ``ds_sequence`` (optional) replaces the step-size control by
    a fixed list of steps (comparisons with a restatement).  Codim-2 points are not located."""
    F = FoldProblem(prob, lens2, a, b, ls)
    lin = FoldLinearSolverMinAug()
    nopt = Cn.NewtonPar(tol=cp.newton_options.tol, max_iterations=cp.newton_options.max_iterations, linsolver=lin)
    bls = BorderingBLS(lin, check_precision=False)
    normC = _norminf_fold if norm_inf else (lambda z: z.norm())
    br = FoldBranch()
    sol0 = Cn.newton(F, fold_guess, p2, nopt, normC)
    if not sol0.converged:
        raise RuntimeError("Newton failed to converge for the initial fold guess")
    ds = cp.ds if ds_sequence is None else ds_sequence[0]
    p2b = p2 + ds / cp.eta
    sol1 = Cn.newton(F, sol0.u, p2b, nopt, normC)
    if not sol1.converged:
        raise RuntimeError("Newton failed to converge. Required for the computation of the initial tangent")
    z0, z1 = BorderedArray(sol0.u, p2), BorderedArray(sol1.u, p2b)

    def record(z, sol, ds_, bt, cpv):
        br.p1.append(z.u.p); br.p2.append(z.p); br.BT.append(bt); br.CP.append(cpv); br.ds.append(ds_)
        br.itnewton.append(sol.itnewton); br.itlinear.append(sol.itlineartot); br.residuals.append(list(sol.residuals))
        if save_sol:
            br.sol.append(z.copy())

    tau = Cn.secant_tangent(z1, z0, ds, theta)
    z, z_old = z0.copy(), z0.copy()
    record(z, sol0, ds, F.update(z.u, z.p), tau.p)
    z_pred = z.copy().add_(tau, ds)
    step = 0
    while step < cp.max_steps and (cp.p_min < z.p < cp.p_max or step == 0):
        it0 = F.itlinear
        sol = Cn.newton_palc(F, z, tau, z_pred, ds, theta, bls, nopt, cp.p_min, cp.p_max, normC)
        sol.itlineartot += F.itlinear - it0
        if verbosity:
            print(f"fold step {step:3d} ds={ds:+.3e} p2={sol.u.p:+.8f} p1={sol.u.u.p:+.8f} conv={sol.converged} "
                  f"itnewton={sol.itnewton} itlinear={sol.itlineartot}")
        if sol.converged:
            z_old.copyto_(z)
            z.copyto_(sol.u)
            step += 1
        if ds_sequence is not None:
            if not sol.converged:
                raise RuntimeError(f"fold continuation step {step} did not converge with the prescribed ds")
            ds_next, stop = (ds_sequence[step] if step < len(ds_sequence) else ds), step >= len(ds_sequence)
        else:
            ds_next, stop = Cn.step_size_control(ds, sol.converged, sol.itnewton, cp)
        if sol.converged:
            tau = Cn.secant_tangent(z, z_old, ds_next, theta)
            bt = F.update(z.u, z.p) if Cn.mod_counter(step, update_minaug_every_step) else float("nan")
            record(z, sol, ds, bt, tau.p)
        ds = ds_next
        if stop:
            break
        z_pred = z.copy().add_(tau, ds)
    return br
