"""Normal forms at simple branch points and folds, their predictors and automatic branch switching for the Swift-Hohenberg
problems (SwiftHohenberg 2-D / 3-D, SwiftHohenberg1D): get_normal_form1d (src/NormalForms.jl:189-353), predictor (:389-531) and
continuation(br, ind_bif, ...) (src/bifdiagram/BranchSwitching.jl:74-198), matrix-free on the preconditioned GMRES path.

  d3F, nf1d_dots, nf1d_rhs, nf1d_contract, nf1d_predict   the device passes (bk_d3f, bk_nf1d_dots, bk_nf1d_rhs,
                                                          bk_nf1d_contract, bk_nf1d_predict)
  normal_form1d            the computation call by call on the plugin surface (the four passes, ls(J, r1, r2), ls(J, zeta*) and
                           the bordering algebra in Python)
  normal_form1d_native     the same as one library call (bk_normal_form_1d)
  get_normal_form1d        get_normal_form1d(br, ind) for a "bp" or "fold" point of a native branch
  predictor                Transcritical, Pitchfork, Fold (None) and BranchPoint
  continuation_from_branch_point   normal form -> predictor -> optional deflated Newton -> the branch from two points

The reduced equation is  a01 dp + a02 dp^2 / 2 + b11 x dp + b20 x^2 / 2 + b30 x^3 / 6  (:285-287).  With E(r) = r - <r, zeta*> zeta:

  a01 = <dpF, zeta*>                                  Psi01 from [J zeta*; zeta' 0][Psi01; s] = [E(-dpF); 0]
  b11 = <dJ/dp zeta + d2F[zeta, Psi01], zeta*>
  a02 = <2 dJ/dp Psi01 + d2F[Psi01, Psi01], zeta*>     (d2F/dp2 = 0 for these problems)
  b20 = <d2F[zeta, zeta], zeta*>                      Psi20 from the same matrix with E(-d2F[zeta, zeta])
  b30 = <d3F[zeta, zeta, zeta] + 3 d2F[zeta, Psi20], zeta*>

Deviations from the reference, stated once: every tensor is pointwise and analytic (the reference: ForwardDiff or central
differences); the Jacobians are symmetric, so zeta* = zeta / <zeta, zeta> (the is_symmetric branch, :261-263); with BorderingBLS
the two bordered systems share ONE J \\ zeta* solve (three GMRES solves where the reference's two bls calls run four); a point of
type "fold" is refined with newton_fold first (the reference takes the bisected point); the BranchPoint predictor brackets the
zeros of g on the circle by a scan of 4096 angles and bisects each bracket (the reference scans ten million angles and keeps
the first sample past each sign change).
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, replace

import numpy as np

from . import continuation as Cn
from .codim2 import (_bls_opts, _carr, _into_similar, _saved, _solve2, _vptrs, fold_point, newton_fold_native)
from .hip import (BorderedArray, BorderingBLS, DeflationOperator, HipVec, MatrixFreeBLS, SwiftHohenberg, SwiftHohenberg1D, _GMRES,
                  _ptr, newton_deflated_native)

TOL_FOLD = 1e-3


def is_sh_problem(prob) -> bool:
    """The problems the normal form is defined for (symmetric Jacobian, pointwise polynomial nonlinearity)."""
    return isinstance(prob, (SwiftHohenberg, SwiftHohenberg1D))


# ------------------------------------------------------------------------------------------ records
@dataclass
class BranchPointNF:
    """The named tuple nf of :339: (a01, a02, b11, b20, b30, Psi01, Psi20)."""
    a01: float
    a02: float
    b11: float
    b20: float
    b30: float
    Psi01: object = None
    Psi20: object = None


@dataclass
class SimpleBranchPoint:
    """The reference's record of a point with a 1-D kernel (Fold / Transcritical / Pitchfork / BranchPoint: x0, tau, p, params,
    lens, zeta, zeta_star, nf, type; :339) plus what the solves reported: ``converged`` (their AND), ``itlinear`` (GMRES counts of
    the Psi01, Psi20 and J \\ zeta* solves) and, from the native call, ``unconverged_solves``.  ``type`` is one of "Fold",
    "Transcritical", "Pitchfork", "BranchPoint", "NonQuadraticParameter" (a BranchPoint whose a02 vanishes too)."""
    x0: object
    tau: object
    p: float
    params: list
    lens: str
    zeta: object
    zeta_star: object
    nf: BranchPointNF
    type: str
    converged: bool | None = None
    itlinear: tuple = ()
    unconverged_solves: int | None = None


@dataclass
class Branch:
    """Branch(branch, bp) (src/bifdiagram/BranchSwitching.jl:197): the switched branch with the point it left from.  With
    ``bothside`` the run from the second point back through the first is kept in ``backward``."""
    branch: object
    bp: SimpleBranchPoint
    backward: object = None


def classify(a01, a02, b11, b20, b30, tol_fold=TOL_FOLD) -> str:
    """:339-350"""
    if max(abs(a01), abs(b11)) > 1e-10:
        if abs(a01) < tol_fold:
            return "Pitchfork" if 100 * abs(b20 / 2) < abs(b30 / 6) else "Transcritical"
        return "Fold"
    return "NonQuadraticParameter" if abs(a02) < tol_fold else "BranchPoint"


# ------------------------------------------------------------------------------------------ device passes
def d3F(prob, x: HipVec, pars, dx1: HipVec, dx2: HipVec, dx3: HipVec) -> HipVec:
    """d3F(prob, x, par, dx1, dx2, dx3) (the R3 of :283) on the device (bk_d3f)."""
    return _into_similar(prob, "bk_d3f", x, pars, _ptr(dx1.t), _ptr(dx2.t), _ptr(dx3.t))


def nf1d_dots(prob, x: HipVec, pars, ipar: int, zeta: HipVec, zeta_star: HipVec):
    """One pass that writes nothing (bk_nf1d_dots): (a01, b20, <zeta, zeta*>)."""
    ctx = prob.ctx
    out = (C.c_double * 3)()
    ctx.check(ctx.lib.bk_nf1d_dots(prob.h, _ptr(x.t), _carr(pars), len(pars), int(ipar), _ptr(zeta.t), _ptr(zeta_star.t), out),
              "bk_nf1d_dots")
    return out[0], out[1], out[2]


def nf1d_rhs(prob, x: HipVec, pars, ipar: int, zeta: HipVec, a01: float, b20: float):
    """One pass over (x, zeta) (bk_nf1d_rhs): (E(-dpF), E(-d2F[zeta, zeta])) = (a01 zeta - dpF, b20 zeta - d2F[zeta, zeta])."""
    ctx = prob.ctx
    r1, r2 = x.similar(), x.similar()
    ctx.check(ctx.lib.bk_nf1d_rhs(prob.h, _ptr(x.t), _carr(pars), len(pars), int(ipar), _ptr(zeta.t), float(a01), float(b20),
                                  _ptr(r1.t), _ptr(r2.t)), "bk_nf1d_rhs")
    return r1, r2


def nf1d_contract(prob, x: HipVec, pars, ipar: int, zeta: HipVec, zeta_star: HipVec, Psi01: HipVec, Psi20: HipVec):
    """One pass over (x, zeta, zeta*, Psi01, Psi20) (bk_nf1d_contract): (b11, a02, b30)."""
    ctx = prob.ctx
    out = (C.c_double * 3)()
    ctx.check(ctx.lib.bk_nf1d_contract(prob.h, _ptr(x.t), _carr(pars), len(pars), int(ipar), _ptr(zeta.t), _ptr(zeta_star.t),
                                       _ptr(Psi01.t), _ptr(Psi20.t), out), "bk_nf1d_contract")
    return out[0], out[1], out[2]


def nf1d_predict(x0: HipVec, zeta: HipVec, Psi01, tau_u, coefs):
    """[((x0 + a zeta) + b Psi01) + c tau_u for (a, b, c) in coefs] (bk_nf1d_predict: up to four outputs per pass over the
    inputs).  ``Psi01`` / ``tau_u`` may be None when every b / c is zero."""
    ctx = x0.ctx
    m = len(coefs)
    outs = [x0.similar() for _ in coefs]
    arr = lambda j: (C.c_double * max(m, 1))(*[float(c[j]) for c in coefs])
    ctx.check(ctx.lib.bk_nf1d_predict(ctx.h, x0.n, _ptr(x0.t), _ptr(zeta.t), _ptr(Psi01.t) if Psi01 is not None else None,
                                      _ptr(tau_u.t) if tau_u is not None else None, m, arr(0), arr(1), arr(2), _vptrs(outs)),
              "bk_nf1d_predict")
    return outs


# ------------------------------------------------------------------------------------------ the normal form
def _record(prob, x0, p, tau, zeta, zeta_star, coef, Psi01, Psi20, cv, it, bad=None, tol_fold=TOL_FOLD) -> SimpleBranchPoint:
    a01, a02, b11, b20, b30 = (float(c) for c in coef)
    return SimpleBranchPoint(x0=x0, tau=tau, p=float(p), params=prob._pvec(p), lens=prob.lens, zeta=zeta, zeta_star=zeta_star,
                             nf=BranchPointNF(a01, a02, b11, b20, b30, Psi01, Psi20), type=classify(a01, a02, b11, b20, b30, tol_fold),
                             converged=bool(cv), itlinear=tuple(int(i) for i in it), unconverged_solves=bad)


def _default_bls(ls, bls):
    return bls if bls is not None else BorderingBLS(ls, check_precision=False)


def normal_form1d(prob, x0: HipVec, p: float, zeta: HipVec, zeta_star: HipVec, ls: _GMRES, bls=None, tau=None,
                  tol_fold=TOL_FOLD) -> SimpleBranchPoint:
    """The computation of get_normal_form1d (:281-337) call by call on the plugin surface at (x0, p) with zeta, zeta* normalised
    (|zeta| = 1, <zeta, zeta*> = 1; they may be the same vector).  BorderingBLS: ls(J, r1, r2) (bk_gmres2), ONE ls(J, zeta*),
    then the BEC algebra (src/LinearBorderSolver.jl:125-166) for both systems with the shared x2; MatrixFreeBLS: two calls."""
    bls = _default_bls(ls, bls)
    pv, ipar = prob._pvec(p), prob.ipar
    a01, b20, nrm = nf1d_dots(prob, x0, pv, ipar, zeta, zeta_star)
    if not abs(nrm - 1) <= 1e-8:
        raise ValueError(f"Error of precision in normalization: <zeta, zeta*> = {nrm}, expected 1")
    r1, r2 = nf1d_rhs(prob, x0, pv, ipar, zeta, a01, b20)
    J = prob.jacobian(x0, p)
    if isinstance(bls, MatrixFreeBLS):
        Psi01, _, cv1, it1 = bls(J, zeta_star, zeta, 0.0, r1, 0.0)
        Psi20, _, cv2, it2 = bls(J, zeta_star, zeta, 0.0, r2, 0.0)
        cv, it = cv1 and cv2, [it1, it2, 0]
    else:
        Psi01, Psi20, cv, it12 = _solve2(ls, J, r1, r2)
        x2, cv3, it3 = ls(J, zeta_star)
        cv, it = cv and cv3, [it12[0], it12[1], it3]
        dx2 = zeta.inner(x2)
        for k, (Psi, R) in enumerate(((Psi01, r1), (Psi20, r2))):
            s = zeta.inner(Psi) / dx2
            Psi.add_(x2, -s)
            n_pass, fail = 0, True
            while bls.check_precision and n_pass < bls.k and fail:                 # residualBEC, :146-166
                dXr = J(Psi).add_(zeta_star, s).add_(R, 1.0, -1.0)
                sr = 0.0 - zeta.inner(Psi)
                fail = dXr.norm() > bls.tol or abs(sr) > bls.tol
                if fail:
                    dX1, cvc, itc = ls(J, dXr)
                    cv, it[k] = cv and cvc, it[k] + itc
                    s1 = (sr - zeta.inner(dX1)) / (0.0 - dx2)
                    Psi.add_(dX1.add_(x2, -s1), 1.0)
                    s += s1
                    n_pass += 1
    b11, a02, b30 = nf1d_contract(prob, x0, pv, ipar, zeta, zeta_star, Psi01, Psi20)
    return _record(prob, x0, p, tau, zeta, zeta_star, (a01, a02, b11, b20, b30), Psi01, Psi20, cv, it, tol_fold=tol_fold)


def normal_form1d_native(prob, x0: HipVec, p: float, zeta: HipVec, zeta_star: HipVec, ls: _GMRES, bls=None, tau=None,
                         tol_fold=TOL_FOLD) -> SimpleBranchPoint:
    """The same as one library call (bk_normal_form_1d)."""
    bls = _default_bls(ls, bls)
    ctx = prob.ctx
    pv = prob._pvec(p)
    Psi01, Psi20 = x0.similar(), x0.similar()
    coef = (C.c_double * 5)()
    cv = C.c_int()
    it = (C.c_int * 3)()
    if isinstance(bls, MatrixFreeBLS):
        bo = _bls_opts(BorderingBLS(ls, check_precision=False))
        bo.kind = 1
    else:
        bo = _bls_opts(bls)
    lo = ls._opts()
    bad0 = ctx.get_option("nf1d_unconverged_solves")
    ctx.check(ctx.lib.bk_normal_form_1d(ctx.h, prob.h, _ptr(x0.t), _carr(pv), len(pv), prob.ipar, _ptr(zeta.t), _ptr(zeta_star.t),
                                        C.byref(bo), C.byref(lo), ls._pl(), _ptr(Psi01.t), _ptr(Psi20.t), coef, C.byref(cv), it),
              "bk_normal_form_1d")
    return _record(prob, x0, p, tau, zeta, zeta_star, list(coef), Psi01, Psi20, cv.value, (it[0], it[1], it[2]),
                   int(ctx.get_option("nf1d_unconverged_solves") - bad0), tol_fold)


def kernel_vector(prob, x: HipVec, p: float, eig, nev=4) -> HipVec:
    """The eigenvector of the eigenvalue of J(x, p) nearest 0, |zeta| = 1: what the reference recomputes when the branch kept no
    eigenvectors (:244-252).  ``eig`` must return vectors (e.g. ShiftInvert(sigma = 0, save_vectors = True))."""
    vals, vecs, _, _ = eig(prob.jacobian(x, p), nev)
    if vecs is None:
        raise ValueError("get_normal_form1d needs the eigenvectors (an eigensolver with save_vectors = True)")
    vals = np.asarray(vals)
    k = int(np.nanargmin(np.abs(vals)))
    z = vecs[k][0].copy()
    return z.scale_(1.0 / z.norm())


def _tangent(br, i: int) -> BorderedArray:
    """tau of the special point from the saved neighbours of point i (as codim2.fold_point): the difference of the points next to
    it, one-sided at an end of the branch, scaled to unit 2-norm.  Only its direction is used (:410, :414, :521)."""
    lo, hi = max(i - 1, 0), min(i + 1, len(br.param) - 1)
    (xl, pl), (xr, pr) = _saved(br, lo), _saved(br, hi)
    tau = BorderedArray(xr.copy().add_(xl, -1.0), float(pr) - float(pl))
    nrm = tau.norm()
    return tau.scale_(1.0 / nrm) if nrm > 0 else tau


def get_normal_form1d(br, ind: int, prob, ls: _GMRES, bls=None, eig=None, nev=4, refine=True, tol=1e-10, max_iterations=15,
                      norm_inf=False, tol_fold=TOL_FOLD) -> SimpleBranchPoint:
    """get_normal_form1d(br, ind) (:189-353) for a point of type "bp" or "fold" of a branch of continuation.continuation_native(...,
    bisection = True, save_sol = True) in the problem's own lens: x0 and p from the saved (bisected) state, tau from the saved
    neighbours, zeta the eigenvector of the eigenvalue nearest 0 from ``eig`` (:244-252), zeta* = zeta (J' = J, :261-263).  A point
    of type "fold" is, with ``refine``, first refined by newton_fold_native (started from zeta, or from tau without an eigensolver)
    and zeta is the null vector v it returns: the reference takes the bisected point."""
    if not is_sh_problem(prob):
        raise TypeError("get_normal_form1d is available for SwiftHohenberg and SwiftHohenberg1D problems only")
    sp = br.specialpoint[ind]
    kind = sp.get("type")
    if kind not in ("bp", "fold"):
        raise ValueError("The provided index does not refer to a Branch Point with 1d kernel. The type of the bifurcation is "
                         f"{kind}. The bifurcation point is {sp}.")
    i = sp["idx"] if "idx" in sp else sp["step"]
    x, p = _saved(br, i)
    x, p = x.copy(), float(p)
    tau = _tangent(br, i)
    zeta = kernel_vector(prob, x, p, eig, nev) if eig is not None else None
    if kind == "fold" and refine:
        a = zeta if zeta is not None else fold_point(br, ind)[1]
        s = newton_fold_native(prob, x, p, a, a, ls, bls if isinstance(bls, BorderingBLS) else None, tol=tol,
                               max_iterations=max_iterations, norm_inf=norm_inf)
        if not s["converged"]:
            raise RuntimeError(f"get_normal_form1d: newton_fold did not converge from the fold guess (residuals {s['residuals']})")
        x, p = s["u"].u, float(s["u"].p)
        zeta = s["v"].copy().scale_(1.0 / s["v"].norm())
    if zeta is None:
        raise ValueError("get_normal_form1d needs an eigensolver (eig = ...) for the kernel vector of a branch point")
    return normal_form1d_native(prob, x, p, zeta, zeta, ls, bls, tau=tau, tol_fold=tol_fold)


# ------------------------------------------------------------------------------------------ predictors
def _circle_zeros(g, r: float, samples=4096):
    """The zeros of theta -> g(r cos theta, r sin theta) on the circle: sign changes between ``samples`` equidistant angles, each
    bracket bisected to the spacing of doubles.  Returns [(x, p, theta)]."""
    f = lambda t: g(r * math.cos(t), r * math.sin(t))
    th = np.linspace(0.0, 2.0 * math.pi, samples + 1)
    vals = [f(t) for t in th]
    out = []
    for k in range(samples):
        fa, fb = vals[k], vals[k + 1]
        if fa == 0.0:
            out.append((r * math.cos(th[k]), r * math.sin(th[k]), float(th[k])))
            continue
        if fa * fb < 0:
            a, b = float(th[k]), float(th[k + 1])
            for _ in range(200):
                m = 0.5 * (a + b)
                if m == a or m == b:
                    break
                fm = f(m)
                if fm == 0.0:
                    a = b = m
                    break
                if fa * fm < 0:
                    b = m
                else:
                    a, fa = m, fm
            t = 0.5 * (a + b)
            out.append((r * math.cos(t), r * math.sin(t), t))
    return out


def predictor(bp: SimpleBranchPoint, ds: float, ampfactor=1.0):
    """predictor(bp, ds; ampfactor) for Transcritical (:389-435), Pitchfork (:457-487), Fold (None, :489-492) and BranchPoint
    (_predictor, :496-531); a dict with the reference's fields (x0, x1, [xm1], p, [pm1], dsfactor, amp, [p0 | dp]).  The vectors
    come from one bk_nf1d_predict pass."""
    nf, tau = bp.nf, bp.tau
    ds = float(ds)
    if bp.type == "Fold":
        return None
    if bp.type == "Transcritical":
        amp = -2 * ds * nf.b11 / nf.b20 * ampfactor                          # b11 ds + b20 amp / 2 = 0
        ntu = tau.u.norm() if tau is not None else 0.0
        if ntu > 0 and abs(bp.zeta.inner(tau.u)) >= 0.9 * ntu:
            x1, x0 = nf1d_predict(bp.x0, bp.zeta, nf.Psi01, tau.u, [(0.0, ds, 0.0), (0.0, 0.0, ds / tau.p)])
            xm1 = bp.x0.copy()
        else:
            x0 = bp.x0
            x1, xm1 = nf1d_predict(bp.x0, bp.zeta, nf.Psi01, None, [(amp, -ds, 0.0), (-amp, ds, 0.0)])
        if amp == 0:
            amp = abs(ds)
        return dict(x0=x0, x1=x1, xm1=xm1, p=bp.p + ds, pm1=bp.p - ds, dsfactor=1.0, amp=amp, p0=bp.p)
    if bp.type == "Pitchfork":
        dsfactor = 1.0 if nf.b11 * nf.b30 < 0 else -1.0
        amp = ampfactor * math.sqrt(-6 * abs(ds) * dsfactor * nf.b11 / nf.b30)  # b11 dp + b30 amp^2 / 6 = 0
        pnew = bp.p + abs(ds) * dsfactor
        if amp == 0:
            amp = abs(ds)
        (x1,) = nf1d_predict(bp.x0, bp.zeta, None, None, [(amp, 0.0, 0.0)])
        return dict(x0=bp.x0, x1=x1, p=pnew, dsfactor=dsfactor, amp=amp, dp=pnew - bp.p)
    g = lambda x, p: (nf.a01 + nf.a02 * p / 2) * p + (nf.b11 * p + nf.b20 * x / 2 + nf.b30 * x * x / 6) * x
    sols = _circle_zeros(g, abs(ds))
    if len(sols) != 4:
        raise ValueError(f"BranchPoint predictor: {len(sols)} zeros of the reduced equation on the circle of radius {abs(ds)}, "
                         "expected 4 (:520)")
    tz = bp.zeta.inner(tau.u) if tau is not None else 0.0
    tp = tau.p if tau is not None else 0.0
    k = int(np.argmin([abs(tz * s[0] + s[1] * tp) for s in sols]))
    pnew = bp.p + sols[k][1]
    (x1,) = nf1d_predict(bp.x0, bp.zeta, None, None, [(sols[k][0], 0.0, 0.0)])
    return dict(x0=bp.x0, x1=x1, p=pnew, dsfactor=1.0, amp=1.0, dp=pnew - bp.p)


# ------------------------------------------------------------------------------------------ branch switching
def continuation_from_branch_point(br, ind: int, prob, alg: Cn.PALC, cp: Cn.ContinuationPar, delta_p=None, ampfactor=1.0,
                                   use_normal_form=True, usedeflation=False, max_iter_deflation=None, bothside=False, bls=None,
                                   eig=None, nev=None, tol_fold=TOL_FOLD, normC=Cn.norm2, verbosity=0, save_sol=False,
                                   bisection=False, finalise_solution=None, callback_newton=None, filename=None):
    """continuation(br, ind_bif, options_cont; ...) (src/bifdiagram/BranchSwitching.jl:74-198) for a simple branch point of a
    native branch: the normal form (get_normal_form1d) -> the predictor (or x0 + ampfactor zeta at p + ds with use_normal_form =
    False, :148-152) -> with ``usedeflation`` a deflated Newton from pred.x1 with pred.x0 deflated (bk_newton_deflated, :172-186) ->
    the branch from the two points (bp.x0, bp.p), (pred.x1, pred.p) with ds signed by p1 - p0 (:8-32), every step one library call
    as in continuation_native.  ``eig`` (default: the eigensolver of cp.newton_options) supplies the kernel vector.  Returns
    Branch(branch, bp), or None when the point has no predictor (a Fold, :157-160)."""
    kind = br.specialpoint[ind].get("type")
    if kind not in ("bp", "nd"):
        raise ValueError(f"You cannot branch from a :{kind} point using these arguments.")
    if kind == "nd":
        raise NotImplementedError("continuation_from_branch_point: kernels of dimension > 1 (multicontinuation) are not available")
    if normC not in (Cn.norm2, Cn.norminf):
        raise TypeError("continuation_from_branch_point: normC must be norm2 or norminf")
    nopt = cp.newton_options
    ls = nopt.linsolver
    ds = cp.ds if delta_p is None else delta_p
    bp = get_normal_form1d(br, ind, prob, ls, bls=bls, eig=eig if eig is not None else nopt.eigsolver,
                           nev=nev if nev is not None else cp.nev, tol_fold=tol_fold)
    if not use_normal_form:
        (x1,) = nf1d_predict(bp.x0, bp.zeta, None, None, [(float(ampfactor), 0.0, 0.0)])
        pred = dict(x0=bp.x0, x1=x1, p=bp.p + ds, amp=ampfactor)
    else:
        pred = predictor(bp, ds, ampfactor=ampfactor)
    if pred is None:
        return None
    if verbosity:
        print(f"branch switching: type {bp.type}, new p = {pred['p']:+.8f} (dp = {pred['p'] - bp.p:+.3e}), amplitude {pred['amp']:.4e}")
    inf = normC is Cn.norminf
    if usedeflation:
        nmax = max_iter_deflation if max_iter_deflation is not None else min(50, 15 * nopt.max_iterations)
        sol = newton_deflated_native(prob, DeflationOperator(2, 1.0, [pred["x0"]]), pred["x1"], pred["p"], ls, tol=nopt.tol,
                                     max_iterations=nmax, norm_inf=inf)
        if not sol["converged"]:
            import warnings
            warnings.warn("Deflated newton did not converge for the first guess on the bifurcated branch.")
        pred["x1"] = sol["u"]
    dsfactor = math.copysign(1.0, pred["p"] - bp.p) if pred["p"] != bp.p else 0.0
    cp2 = replace(cp, ds=abs(cp.ds) * dsfactor)
    alg = alg.update(cp2)
    first = lambda x: dict(u=x, itnewton=0, itlineartot=0, residuals=[])

    def run(xa, pa, xb, pb, cpx):
        return Cn._continuation_native_from(prob, first(xa), float(pa), dict(u=xb), float(pb), alg, cpx, inf, verbosity, save_sol,
                                            bisection, finalise_solution, callback_newton, None, filename)

    fw = run(bp.x0, bp.p, pred["x1"], pred["p"], cp2)
    bw = run(pred["x1"], pred["p"], bp.x0, bp.p, cp2) if bothside else None          # itbw = deepcopy(itfw), :26-29
    return Branch(fw, bp, bw)
