"""Periodic orbits of the cGL problem by the trapezoid rule: the second half of examples/cGL2d.jl (:166-260) on the device.

  PeriodicOrbitTrap          Trapeze(prob, phi, xpi, M, 2n; jacobian = FullMatrixFree())   src/periodicorbit/PeriodicOrbitTrapeze.jl
  PoTrapPreconditioner       the space-time spectral preconditioner diag(A0, 1) in the place of the example's ILU (:209-213)
  po_guess_from_hopf         the guess of :172-174 and the section of :177-181 from predictor(hopf, ds)
  PoTrapJacobian.adjoint     dG^T, with PoTrapPreconditioner(adjoint=True) the left-null-vector solves of MinAugFold.jl:15-69
  po_bordered_solve          ONE GMRES on [dG a; b' c] (or dG^T), regular at a fold of limit cycles
  po_fold_terms              the bordered vectors v, w and sigma of the fold of orbits         MinAugFold.jl:15-69
  newton_fold_po[_native]    newton_fold(br_po, indfold; prob = probFold) on bordered solves    cGL2d.jl:347-370
  po_fold_point              fold_point(br_po, indfold) and the a = b = tangent of newton_fold  cGL2d.jl:354, MinAugFold.jl:244-247
  PoFoldProblem, PoFoldLinearSolverMinAug, continuation_fold_po   continuation_fold(probFold, br_po, indfold, c5)   cGL2d.jl:381-392
  newton_po_trap             newton(poTrapMF, orbitguess_f, opt_po; normN = norminf)        :213-219
  continuation_po_trap       continuation(poTrapMF, outpo_f.u, PALC(), ...), secant tangent, BorderingBLS, updatesection every step
  get_periodic_orbit         :651-657
  PoTrapMonodromy            MonodromyQaD_matrix_free(::Trapeze) as ONE space-time solve   src/periodicorbit/Floquet.jl:285-315
  floquet_multipliers        compute_eigenvalues(::FloquetQaD, ...), which = :LM            Floquet.jl:59-85 (csrc/floquet.hip)
  floquet_eigenfunction      Val(:ExtractEigenVector)                                        Floquet.jl:319-355
  monodromy_sequential       the call-by-call mirror of :285-315 (yardstick and timing baseline)
  classify_po_bifurcation    _get_bifurcation_type for a Floquet solver                      src/Bifurcations.jl:80-151

An orbit is ``BorderedArray(u, T)``: ``u`` the M slices [u1; u2] on the device, ``T`` the period entry on the host.  The time step
is h = T / M on each of the M - 1 intervals (src/TimeMesh.jl:21), so ``T`` is M / (M - 1) times the orbit's period -- the
reference's convention, kept.  Newton and PALC are the ones of ``continuation.py`` (``newton``, ``newton_palc``, ``secant_tangent``,
``step_size_control``), run on this functional.  The hot path -- functional, Jacobian-vector product, preconditioner, GMRES -- is
``csrc/potrap.hip``; the adjoint pass and the transposed time solve are ``csrc/pofold.hip``.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib as L
from . import continuation as Cn
from .hip import BorderedArray, HipVec, _GMRES, _ptr


def _parr(params):
    return (C.c_double * len(params))(*[float(x) for x in params])


def _norminf(x: BorderedArray):
    r, t = x.u.norminf(), abs(x.p)
    return r if (r != r or r > t) else t


class PeriodicOrbitTrap:
    """The handle of the functional (bk_potrap_create).  ``phi``, ``xpi``: the section, M N doubles each; a ``phi`` of one slice's
    length sits in the first slice (the reference's constructor call, cGL2d.jl:177-181) and ``xpi = None`` is zero."""

    def __init__(self, prob, M: int, phi: HipVec | None = None, xpi: HipVec | None = None):
        self.prob, self.ctx, self.M = prob, prob.ctx, int(M)
        self.N = prob.nlocal
        h = C.c_void_p()
        self.ctx.check(self.ctx.lib.bk_potrap_create(prob.h, self.M, C.byref(h)), "bk_potrap_create")
        self.h = h
        if phi is not None:
            self.set_section(phi, xpi)

    @property
    def n(self):
        return self.N * self.M

    def vec(self, a) -> HipVec:
        return HipVec.from_numpy(self.ctx, np.asarray(a, dtype=np.float64).reshape(-1))

    def set_section(self, phi: HipVec, xpi: HipVec | None = None):
        if phi.n == self.N:
            full = HipVec(self.ctx, self.ctx.empty(self.n)).zerovector()
            full.t[:self.N].copy_(phi.t)
            phi = full
        if xpi is None:
            xpi = phi.zerovector()
        if phi.n != self.n or xpi.n != self.n:
            raise ValueError(f"section vectors must hold M N = {self.n} doubles")
        self.ctx.check(self.ctx.lib.bk_potrap_set_section(self.h, _ptr(phi.t), _ptr(xpi.t)), "bk_potrap_set_section")

    def get_section(self):
        """(phi, xpi), copies of the section in force."""
        phi, xpi = (HipVec(self.ctx, self.ctx.empty(self.n)) for _ in range(2))
        self.ctx.check(self.ctx.lib.bk_potrap_get_section(self.h, _ptr(phi.t), _ptr(xpi.t)), "bk_potrap_get_section")
        return phi, xpi

    def update_section(self, u: HipVec, T: float, params):
        """updatesection! (:665-681)."""
        self.ctx.check(self.ctx.lib.bk_potrap_update_section(self.h, _ptr(u.t), float(T), _parr(params), len(params)),
                       "bk_potrap_update_section")

    def residual(self, u: HipVec, T: float, params) -> BorderedArray:
        out, tail = u.similar(), C.c_double()
        self.ctx.check(self.ctx.lib.bk_potrap_residual(self.h, _ptr(u.t), float(T), _parr(params), len(params), _ptr(out.t),
                                                       C.byref(tail)), "bk_potrap_residual")
        return BorderedArray(out, tail.value)

    def jvp(self, u: HipVec, T: float, params, du: HipVec, dT: float) -> BorderedArray:
        out, tail = u.similar(), C.c_double()
        self.ctx.check(self.ctx.lib.bk_potrap_jvp(self.h, _ptr(u.t), float(T), _parr(params), len(params), _ptr(du.t), float(dT),
                                                  _ptr(out.t), C.byref(tail)), "bk_potrap_jvp")
        return BorderedArray(out, tail.value)

    def jvp_adjoint(self, u: HipVec, T: float, params, w: HipVec, tau: float) -> BorderedArray:
        """dG(u, T)^T (w, tau) (bk_potrap_jvp_adjoint)."""
        out, tail = u.similar(), C.c_double()
        self.ctx.check(self.ctx.lib.bk_potrap_jvp_adjoint(self.h, _ptr(u.t), float(T), _parr(params), len(params), _ptr(w.t),
                                                          float(tau), _ptr(out.t), C.byref(tail)), "bk_potrap_jvp_adjoint")
        return BorderedArray(out, tail.value)

    def fold_border(self, u: HipVec, T: float, params, ipar: int, v: BorderedArray, w: HipVec):
        """The border row of the fold system and sigma_p for params[ipar] (bk_potrap_fold_border) ->
        (BorderedArray(sigma_x, (sigma_x)_T), sigma_p): <sigma_x, X> = -<w, d2G[v, X]>, sigma_p = -<w, d_p(dG) v>."""
        out, st, sp = u.similar(), C.c_double(), C.c_double()
        self.ctx.check(self.ctx.lib.bk_potrap_fold_border(self.h, _ptr(u.t), float(T), _parr(params), len(params), int(ipar),
                                                          _ptr(v.u.t), float(v.p), _ptr(w.t), _ptr(out.t), C.byref(st),
                                                          C.byref(sp)), "bk_potrap_fold_border")
        return BorderedArray(out, st.value), sp.value

    def dparam(self, u: HipVec, T: float, params, ipar: int) -> HipVec:
        out = u.similar()
        self.ctx.check(self.ctx.lib.bk_potrap_dparam(self.h, _ptr(u.t), float(T), _parr(params), len(params), int(ipar),
                                                     _ptr(out.t)), "bk_potrap_dparam")
        return out

    def jacobian(self, u: HipVec, T: float, params) -> "PoTrapJacobian":
        return PoTrapJacobian(self, u, T, params)

    def __del__(self):
        try:
            if self.h.value:
                self.ctx.lib.bk_potrap_destroy(self.h)
        except Exception:
            pass


class PoTrapJacobian:
    """dG(u, T) as an operator handle (bk_potrap_op_create), or dG(u, T)^T (``adjoint=True``: bk_potrap_op_adjoint_create); keeps
    ``u`` alive."""

    def __init__(self, po: PeriodicOrbitTrap, u: HipVec, T: float, params, adjoint: bool = False):
        self.po, self.ctx, self.u, self.T, self.params = po, po.ctx, u, float(T), list(params)
        self.is_adjoint = bool(adjoint)
        name = "bk_potrap_op_adjoint_create" if self.is_adjoint else "bk_potrap_op_create"
        h = C.c_void_p()
        self.ctx.check(getattr(self.ctx.lib, name)(po.h, _ptr(u.t), self.T, _parr(params), len(params), C.byref(h)), name)
        self.h = h

    def __call__(self, dx: BorderedArray) -> BorderedArray:
        if self.is_adjoint:
            return self.po.jvp_adjoint(self.u, self.T, self.params, dx.u, dx.p)
        return self.po.jvp(self.u, self.T, self.params, dx.u, dx.p)

    def adjoint(self) -> "PoTrapJacobian":
        """The transposed operator at the same (u, T, params)."""
        return PoTrapJacobian(self.po, self.u, self.T, self.params, adjoint=not self.is_adjoint)

    def __del__(self):
        try:
            if self.h.value:
                self.ctx.lib.bk_op_destroy(self.h)
        except Exception:
            pass


class PoTrapPreconditioner:
    """P = diag(A0, 1), A0 the orbit Jacobian with every J_i replaced by Lap (x) I_2 + [[a, -b], [b, a]]; the default
    a = r, b = nu is the linearisation at the trivial state.  ``set_period`` refuses a Hopf-critical (a, b).  ``adjoint=True``:
    diag(A0^T, 1), the preconditioner of ``PoTrapJacobian.adjoint()`` (bk_precond_potrap_adjoint_create)."""

    def __init__(self, po: PeriodicOrbitTrap, a: float | None = None, b: float | None = None, params=None, adjoint: bool = False):
        self.po, self.ctx = po, po.ctx
        pv = po.prob._pvec(po.prob.params[po.prob.lens]) if params is None else list(params)
        a = pv[0] if a is None else a
        b = pv[2] if b is None else b
        h = C.c_void_p()
        self.is_adjoint = bool(adjoint)
        name = "bk_precond_potrap_adjoint_create" if self.is_adjoint else "bk_precond_potrap_create"
        self.ctx.check(getattr(self.ctx.lib, name)(po.h, float(a), float(b), C.byref(h)), name)
        self.h = h
        self.a, self.b = float(a), float(b)

    def set_period(self, T: float):
        self.ctx.check(self.ctx.lib.bk_precond_potrap_set_period(self.h, float(T)), "bk_precond_potrap_set_period")
        return self

    def ldiv(self, v: HipVec) -> HipVec:
        out = v.similar()
        self.ctx.check(self.ctx.lib.bk_precond_apply(self.h, _ptr(v.t), _ptr(out.t)), "bk_precond_apply")
        return out

    def transform_paths(self):
        """Per axis (x, y) the kernel the last application's transform passes ran on: 1 matrix cores, 0 one thread per output,
        2 rocBLAS, -1 none yet."""
        p = (C.c_int * 2)()
        self.ctx.check(self.ctx.lib.bk_precond_potrap_transform_paths(self.h, p), "bk_precond_potrap_transform_paths")
        return p[0], p[1]

    def __del__(self):
        try:
            if self.h.value:
                self.ctx.lib.bk_precond_destroy(self.h)
        except Exception:
            pass


def po_solve(J: PoTrapJacobian, pl, rhs: BorderedArray, ls: _GMRES):
    """One GMRES on diag(A0^-1, 1) dG x = diag(A0^-1, 1) rhs (bk_potrap_solve) -> (x, converged, niter).  ``pl``: anything with a
    preconditioner handle ``.h``; the library refuses one that is not a PoTrapPreconditioner of this orbit's size.  An adjoint
    Jacobian goes with an adjoint preconditioner (dG^T and A0^-T); the library refuses a mixed pair."""
    ctx = J.ctx
    x, xt = rhs.u.similar(), C.c_double()
    o = ls._opts()
    res = L.SolveResult()
    ctx.check(ctx.lib.bk_potrap_solve(ctx.h, J.h, pl.h if pl is not None else None, _ptr(rhs.u.t), float(rhs.p), _ptr(x.t),
                                      C.byref(xt), C.byref(o), C.byref(res)), "bk_potrap_solve")
    return BorderedArray(x, xt.value), bool(res.converged), int(res.niter)


def po_bordered_solve(J: PoTrapJacobian, pl, a: BorderedArray, b: BorderedArray, c: float, rhs: BorderedArray, rhs_border: float,
                      ls: _GMRES):
    """ONE GMRES on [A a; b' c][x; s] = [rhs; rhs_border], A = dG or dG^T with its T entry, left-preconditioned by diag(A0^-1, 1, 1)
    (bk_potrap_bordered_solve): regular where dG is singular.  ``a``, ``b``, ``rhs``: BorderedArray(vector, T entry); ``pl`` of the
    kind of ``J``.  Returns (x, s, converged, niter)."""
    ctx = J.ctx
    x, xt, xb = rhs.u.similar(), C.c_double(), C.c_double()
    o = ls._opts()
    res = L.SolveResult()
    ctx.check(ctx.lib.bk_potrap_bordered_solve(ctx.h, J.h, pl.h if pl is not None else None, _ptr(a.u.t), float(a.p), _ptr(b.u.t),
                                               float(b.p), float(c), _ptr(rhs.u.t), float(rhs.p), float(rhs_border), _ptr(x.t),
                                               C.byref(xt), C.byref(xb), C.byref(o), C.byref(res)), "bk_potrap_bordered_solve")
    return BorderedArray(x, xt.value), xb.value, bool(res.converged), int(res.niter)


def po_fold_terms(po: PeriodicOrbitTrap, u: HipVec, T: float, params, a: BorderedArray, b: BorderedArray, pl, pl_adjoint, ls: _GMRES):
    """The bordered vectors of the fold of limit cycles (bk_potrap_fold_terms; MinAugFold.jl:15-69): [dG a; b' 0][v; sigma] = [0; 1]
    and [dG^T b; a' 0][w; .] = [0; 1], one bordered solve each.  Returns dict(v, w (BorderedArrays), sigma, converged, itlinear)."""
    ctx = po.ctx
    v, w = u.similar(), u.similar()
    vT, wT, sg, cv = C.c_double(), C.c_double(), C.c_double(), C.c_int()
    it = (C.c_int * 2)()
    o = ls._opts()
    ctx.check(ctx.lib.bk_potrap_fold_terms(po.h, _ptr(u.t), float(T), _parr(params), len(params), _ptr(a.u.t), float(a.p),
                                           _ptr(b.u.t), float(b.p), pl.h, pl_adjoint.h, C.byref(o), _ptr(v.t), C.byref(vT),
                                           _ptr(w.t), C.byref(wT), C.byref(sg), C.byref(cv), it), "bk_potrap_fold_terms")
    return dict(v=BorderedArray(v, vT.value), w=BorderedArray(w, wT.value), sigma=sg.value, converged=bool(cv.value),
                itlinear=(it[0], it[1]))


def _fold_preconds(po, ls, params, T, pl, pl_adjoint):
    if pl is None:
        pl = _precond_for(po, ls, params).set_period(T)
    if pl_adjoint is None:
        pl_adjoint = PoTrapPreconditioner(po, pl.a, pl.b, adjoint=True).set_period(T)
    return pl, pl_adjoint


def newton_fold_po(po: PeriodicOrbitTrap, orbit: HipVec, T: float, params, lens, a: BorderedArray, b: BorderedArray, ls: _GMRES,
                   tol=1e-10, max_iterations=10, pl=None, pl_adjoint=None):
    """newton_fold(br_po, indfold; prob = probFold) (cGL2d.jl:347-370) call by call: Newton in the sup norm on
    G_fold((u, T), p) = (G, sigma) with the section of ``po`` and (a, b) frozen.  Per point bk_potrap_residual and
    bk_potrap_fold_terms, per step bk_potrap_fold_border, bk_potrap_dparam and ONE bk_potrap_bordered_solve on
    [dG d_pG; sigma_x' sigma_p][dX; dp] = [G; sigma] (MinAugFold.jl:136-145): every linear system is a bordered one, regular at the
    fold.  The preconditioners (default a = r, b = nu, period ``T``) stay fixed.  The yardstick and timing baseline of
    ``newton_fold_po_native``.  Returns dict(u, T, p, residuals, itlinear (per Newton step the GMRES counts of the v solve, the w
    solve and the step taken from that point), last_terms_its (the v and w counts of the returned point), itlineartot (all of
    them summed), v, w, sigma, converged, itnewton)."""
    params = [float(x) for x in params]
    ipar = po.prob.param_names.index(lens) if isinstance(lens, str) else int(lens)
    pl, plT = _fold_preconds(po, ls, params, T, pl, pl_adjoint)
    u, T, pv = orbit.copy(), float(T), list(params)

    def point():
        G = po.residual(u, T, pv)
        t = po_fold_terms(po, u, T, pv, a, b, pl, plT, ls)
        return G, t, max(_norminf(G), abs(t["sigma"]))

    G, t, r = point()
    res, its = [r], []
    while len(res) - 1 < max_iterations and res[-1] > tol:
        sx, sp = po.fold_border(u, T, pv, ipar, t["v"], t["w"].u)
        dpG = BorderedArray(po.dparam(u, T, pv, ipar), 0.0)
        dx, dp, _, it = po_bordered_solve(po.jacobian(u, T, pv), pl, dpG, sx, sp, G, t["sigma"], ls)
        its.append((t["itlinear"][0], t["itlinear"][1], it))
        u.add_(dx.u, -1.0)
        T -= dx.p
        pv[ipar] -= dp
        G, t, r = point()
        res.append(r)
    return dict(u=u, T=T, p=pv[ipar], residuals=res, itlinear=its, v=t["v"], w=t["w"], sigma=t["sigma"], converged=res[-1] < tol,
                itnewton=len(res) - 1, last_terms_its=t["itlinear"],
                itlineartot=sum(sum(k) for k in its) + sum(t["itlinear"]))


def newton_fold_po_native(po: PeriodicOrbitTrap, orbit: HipVec, T: float, params, lens, a: BorderedArray, b: BorderedArray,
                          ls: _GMRES, tol=1e-10, max_iterations=10, pl=None, pl_adjoint=None):
    """``newton_fold_po`` as one library call (bk_potrap_newton_fold); the same results under the same keys."""
    from .hip import newton_opts
    params = [float(x) for x in params]
    ipar = po.prob.param_names.index(lens) if isinstance(lens, str) else int(lens)
    pl, plT = _fold_preconds(po, ls, params, T, pl, pl_adjoint)
    ctx = po.ctx
    u, v, w = orbit.copy(), orbit.similar(), orbit.similar()
    Tc, pc = C.c_double(float(T)), C.c_double(params[ipar])
    vT, wT, sg = C.c_double(), C.c_double(), C.c_double()
    no, o = newton_opts(tol, max_iterations, True), ls._opts()
    res = L.NewtonResult()
    its = (C.c_int * (3 * (int(max_iterations) + 1)))()
    ctx.check(ctx.lib.bk_potrap_newton_fold(po.h, _ptr(u.t), C.byref(Tc), C.byref(pc), _parr(params), len(params), ipar, _ptr(a.u.t),
                                            float(a.p), _ptr(b.u.t), float(b.p), pl.h, plT.h, C.byref(no), C.byref(o), _ptr(v.t),
                                            C.byref(vT), _ptr(w.t), C.byref(wT), C.byref(sg), C.byref(res), its),
              "bk_potrap_newton_fold")
    k = res.itnewton
    return dict(u=u, T=Tc.value, p=pc.value, residuals=[res.residuals[i] for i in range(k + 1)],
                itlinear=[(its[3 * i], its[3 * i + 1], its[3 * i + 2]) for i in range(k)], v=BorderedArray(v, vT.value),
                w=BorderedArray(w, wT.value), sigma=sg.value, converged=bool(res.converged), itnewton=k, itlineartot=res.itlinear,
                last_terms_its=(its[3 * k], its[3 * k + 1]))


def _norminf_nested(z):
    """The sup norm of a (nested) BorderedArray; NaN wins."""
    r = _norminf_nested(z.u) if isinstance(z.u, BorderedArray) else z.u.norminf()
    t = abs(z.p)
    return r if (r != r or r > t) else t


def _po_fold_classes():
    """PoFoldProblem and PoFoldLinearSolverMinAug on the surfaces of codim2.py (imported here: codim2 does not know this module)."""
    from . import codim2 as C2

    class PoFoldProblem(C2._MinAugProblem):
        """FoldMinimallyAugmentedFormulation + FoldMAProblem with lens2 (MinAugFold.jl; continuation_fold :407-453) on the orbit
        functional: the ``_MinAugProblem`` surface on states X = BorderedArray(BorderedArray(u, T), p1), parameter p2 = ``lens2``.
        a, b: BorderedArray(vector, T entry).  The bordered vectors of a point come from bk_potrap_fold_terms (two bordered
        solves), cached per point; the section of ``po`` and the preconditioners stay as they are handed over."""

        def __init__(self, po: PeriodicOrbitTrap, params, lens1, lens2, a: BorderedArray, b: BorderedArray, ls: _GMRES, pl, pl_adjoint):
            names = po.prob.param_names
            self.po, self.prob, self.ctx = po, po.prob, po.ctx
            self.params = [float(x) for x in params]
            self.ipar1 = names.index(lens1) if isinstance(lens1, str) else int(lens1)
            self.ipar2 = names.index(lens2) if isinstance(lens2, str) else int(lens2)
            if self.ipar1 == self.ipar2:
                raise ValueError(f"Please choose 2 different parameters. You only passed {lens2}")
            self.lens1, self.lens2 = names[self.ipar1], names[self.ipar2]
            self.ls, self.pl, self.pl_adjoint = ls, pl, pl_adjoint
            self.a, self.b = a, b
            self.delta = po.prob.delta
            self.itlinear = 0
            self._cache = None

        def pvec(self, p1, p2):
            pv = list(self.params)
            pv[self.ipar1], pv[self.ipar2] = float(p1), float(p2)
            return pv

        def terms(self, X, p2: float):
            """(v, w, sigma) at (X, p2), solved once per point."""
            c = self._cache
            if c is not None and c[1] == (X.u.p, X.p, p2) and torch.equal(c[0].t, X.u.u.t):
                return c[2]
            t = po_fold_terms(self.po, X.u.u, X.u.p, self.pvec(X.p, p2), self.a, self.b, self.pl, self.pl_adjoint, self.ls)
            self.itlinear += t["itlinear"][0] + t["itlinear"][1]
            out = (t["v"], t["w"], t["sigma"])
            self._cache = (X.u.u.copy(), (X.u.p, X.p, p2), out)
            return out

        def residual(self, X, p2: float):
            _, _, sigma = self.terms(X, p2)
            return BorderedArray(self.po.residual(X.u.u, X.u.p, self.pvec(X.p, p2)), sigma)

        def residual_dparam(self, X, p2: float, eps=None):
            """dG/dp2 = ((d_p2 G, 0), sigma_p2), analytic."""
            v, w, _ = self.terms(X, p2)
            pv = self.pvec(X.p, p2)
            _, sp2 = self.po.fold_border(X.u.u, X.u.p, pv, self.ipar2, v, w.u)
            return BorderedArray(BorderedArray(self.po.dparam(X.u.u, X.u.p, pv, self.ipar2), 0.0), sp2)

        def update(self, X, p2: float):
            """update!(probma, iter, state) (:280-313) after a converged step: a <- w / |w|, b <- v / |v| from the bordered vectors
            of the new point (T entries included); returns <a, b>."""
            v, w, _ = self.terms(X, p2)
            self.a = w.copy().scale_(1.0 / w.norm())
            self.b = v.copy().scale_(1.0 / v.norm())
            self._cache = None
            return self.a.inner(self.b)

    class PoFoldLinearSolverMinAug(C2._MinAugLinearSolver):
        """FoldLinearSolverMinAug (:168-178) on the orbit functional as bk_potrap_fold_linsolve: the full system
        [dG d_p1 G; sigma_x' sigma_p1] (:136-145), one bordered solve per right-hand side."""

        def _run(self, J, rhs):
            P, X = J.ma, J.X
            v, w, _ = P.terms(X, J.p2)
            pv = P.pvec(X.p, J.p2)
            ctx, m = P.ctx, len(rhs)
            dX = [X.u.u.similar() for _ in rhs]
            ru = (C.c_void_p * m)(*[r.u.u.t.data_ptr() for r in rhs])
            dxp = (C.c_void_p * m)(*[d.t.data_ptr() for d in dX])
            rT = (C.c_double * m)(*[float(r.u.p) for r in rhs])
            rp = (C.c_double * m)(*[float(r.p) for r in rhs])
            dT, ds = (C.c_double * m)(), (C.c_double * m)()
            cv, it = C.c_int(), C.c_int()
            lo = P.ls._opts()
            ctx.check(ctx.lib.bk_potrap_fold_linsolve(P.po.h, _ptr(X.u.u.t), float(X.u.p), _parr(pv), len(pv), P.ipar1, _ptr(v.u.t),
                                                      float(v.p), _ptr(w.u.t), P.pl.h, m, ru, rT, rp, C.byref(lo), dxp, dT, ds,
                                                      C.byref(cv), C.byref(it)), "bk_potrap_fold_linsolve")
            return [BorderedArray(BorderedArray(dX[k], dT[k]), ds[k]) for k in range(m)], bool(cv.value), it.value

    return PoFoldProblem, PoFoldLinearSolverMinAug, C2


def continuation_fold_po(po: PeriodicOrbitTrap, fold_guess: BorderedArray, p2: float, lens2, a: BorderedArray, b: BorderedArray,
                         ls: _GMRES, cp: Cn.ContinuationPar, params=None, lens1="r", theta=0.5, update_minaug_every_step=1,
                         save_sol=False, ds_sequence=None, verbosity=0, pl=None, pl_adjoint=None):
    """continuation_fold(probFold, br_po, indfold, (@optic _.c5), optcontfold) (cGL2d.jl:381-392; MinAugFold.jl:369-453): PALC on
    G_fold(X, p2) with X = BorderedArray(BorderedArray(u, T), p1) = ``fold_guess`` through the driver the SH fold and Hopf curves
    share (codim2._continuation_minaug: Secant tangent, BorderingBLS over PoFoldLinearSolverMinAug, the two starting points by
    Newton on G_fold).  After every converged step a <- w / |w|, b <- v / |v|.  The section of ``po`` stays frozen; the
    preconditioners (default a = r, b = nu of ``params``, period of the guess) stay fixed.  ``params``: the full parameter list
    (default: the problem's).  Returns a codim2._MinAugBranch (p1, p2, ds, itnewton, itlinear -- the GMRES counts of the step,
    bordered vectors included --, residuals, sol) with T, amplitude and ab = <a, b> per point in addition."""
    PoFoldProblem, PoFoldLinearSolverMinAug, C2 = _po_fold_classes()
    params = po.prob._pvec(po.prob.params[po.prob.lens]) if params is None else [float(x) for x in params]
    pl, plT = _fold_preconds(po, ls, params, fold_guess.u.p, pl, pl_adjoint)
    P = PoFoldProblem(po, params, lens1, lens2, a, b, ls, pl, plT)
    br = C2._MinAugBranch()
    br.T, br.amplitude, br.ab = [], [], []

    def record_x(X, val, tau):
        br.p1.append(X.p); br.T.append(X.u.p); br.amplitude.append(amplitude(X.u.u)); br.ab.append(val)

    C2._continuation_minaug(P, PoFoldLinearSolverMinAug(), "Fold", br, fold_guess, float(p2), cp, theta, _norminf_nested,
                            update_minaug_every_step, save_sol, ds_sequence, verbosity, record_x, lambda X: float("nan"),
                            lambda X: f"p1={X.p:+.8f} T={X.u.p:.6f}")
    return br


def __getattr__(name):
    if name in ("PoFoldProblem", "PoFoldLinearSolverMinAug"):
        return dict(zip(("PoFoldProblem", "PoFoldLinearSolverMinAug"), _po_fold_classes()[:2]))[name]
    raise AttributeError(name)


class _PoFunctional:
    """The functional as the ``prob`` of continuation.newton / newton_palc: states are BorderedArray(u, T), the continuation
    parameter is ``params[ipar]``; d_p G is analytic (bk_potrap_dparam) where the reference differences."""

    def __init__(self, po: PeriodicOrbitTrap, params, ipar: int):
        self.po, self.params, self.ipar = po, [float(x) for x in params], int(ipar)
        # newton_palc reads prob.delta and hands it to residual_dparam as the difference step; d_p G is analytic here and
        # ignores it, the attribute only has to exist
        self.delta = po.prob.delta

    def pv(self, p):
        pv = list(self.params)
        pv[self.ipar] = float(p)
        return pv

    def residual(self, x: BorderedArray, p: float) -> BorderedArray:
        return self.po.residual(x.u, x.p, self.pv(p))

    def jacobian(self, x: BorderedArray, p: float) -> PoTrapJacobian:
        return self.po.jacobian(x.u, x.p, self.pv(p))

    def residual_dparam(self, x: BorderedArray, p: float, eps=None) -> BorderedArray:
        return BorderedArray(self.po.dparam(x.u, x.p, self.pv(p), self.ipar), 0.0)


class _PoLinearSolver:
    """ls(J, rhs) -> (x, ok, it) on the preconditioned solve; ``counts`` keeps the GMRES count of every call."""

    def __init__(self, ls: _GMRES, pl: PoTrapPreconditioner):
        self.ls, self.pl, self.counts = ls, pl, []

    def __call__(self, J, rhs, a0=0.0, a1=1.0):
        x, cv, it = po_solve(J, self.pl, rhs, self.ls)
        self.counts.append(it)
        return x, cv, it


class _PoBordering:
    """BorderingBLS (src/LinearBorderSolver.jl:88-166, no precision check) on the orbit Jacobian: two preconditioned solves."""

    def __init__(self, solver: _PoLinearSolver):
        self.solver = solver

    def __call__(self, J, dR, dzu, dzp, R, n, xiu=1.0, xip=1.0, *, shift=None, dotp=None, dotscale=None):
        x1, c1, i1 = self.solver(J, R)
        x2, c2, i2 = self.solver(J, dR)
        dl = (n - xiu * dotp(dzu, x1)) / (dzp * xip - xiu * dotp(dzu, x2))
        x1.add_(x2, -dl)
        return x1, dl, c1 and c2, (i1, i2)


def _precond_for(po, ls, params):
    pl = getattr(ls, "Pl", None)
    return pl if pl is not None else PoTrapPreconditioner(po, params=params)


def newton_po_trap(po: PeriodicOrbitTrap, orbit_guess: HipVec, T_guess: float, params, ls: _GMRES, tol=1e-10, max_iterations=10,
                   norm_inf=True, verbose=False):
    """newton(poTrapMF, orbitguess_f, opt_po; normN = norminf) (cGL2d.jl:213-219): ``_newton`` on the functional with the
    preconditioned matrix-free solve.  ``ls``: a GMRES solver object (its options; ``ls.Pl`` a PoTrapPreconditioner, or None for
    the default a = r, b = nu); the preconditioner's period is set to ``T_guess``.  Returns dict(u, T, residuals, itlinear (per
    Newton step), converged, itnewton)."""
    params = [float(x) for x in params]
    pl = _precond_for(po, ls, params).set_period(T_guess)
    lin = _PoLinearSolver(ls, pl)
    F = _PoFunctional(po, params, 0)
    opt = Cn.NewtonPar(tol=tol, max_iterations=max_iterations, verbose=verbose, linsolver=lin)
    s = Cn.newton(F, BorderedArray(orbit_guess, float(T_guess)), params[0], opt, _norminf if norm_inf else Cn.norm2)
    return dict(u=s.u.u, T=s.u.p, residuals=s.residuals, itlinear=list(lin.counts), converged=s.converged, itnewton=s.itnewton)


def po_guess_from_hopf(pred: dict, M: int, prob=None, p: float | None = None):
    """The guess of cGL2d.jl:172-174 from ``predictor(hopf, ds)``: the orbit's slices at t_m = 2 pi m / M and ``pred["period"]`` as
    the T entry.  With ``prob`` also the section of :177-181 at the parameter ``p`` (default: the predictor's): phi = F(slice 1) /
    |F(slice 1)| in the first slice, xpi = 0.  Returns dict(orbit, T, phi, xpi, p)."""
    sl = pred["orbit"].slices(M)
    ctx = sl[0].ctx
    orbit = HipVec(ctx, torch.cat([s.t for s in sl]).contiguous())
    out = dict(orbit=orbit, T=float(pred["period"]), phi=None, xpi=None, p=float(pred["p"] if p is None else p))
    if prob is not None:
        f = prob.residual(sl[0], out["p"])
        f.scale_(1.0 / f.norm())
        phi = orbit.zerovector()
        phi.t[:f.n].copy_(f.t)
        out["phi"], out["xpi"] = phi, orbit.zerovector()
    return out


def amplitude(u: HipVec) -> float:
    """max |u| over all slices and both fields: what continuation_po_trap records."""
    return u.norminf()


def continuation_po_trap(po: PeriodicOrbitTrap, orbit: HipVec, T: float, params, lens, cp: Cn.ContinuationPar, ls: _GMRES,
                         theta=0.5, update_section_every_step=1, verbosity=0, nev=0, detect_bifurcation=0, tol_stability=1e-10,
                         eig=None, save_sol=False):
    """PALC on the (N M + 1) + 1 system (continuation(poTrapMF, ..., PALC()) of cGL2d.jl:221-260): two Newton solves and the secant
    tangent, then per step newton_palc with BorderingBLS -- two preconditioned solves per Newton step, d_p G analytic --, the
    step-size control of continuation.py and updatesection! after every accepted step (the reference's default).  ``lens``: the
    name or index of the continuation parameter.  Returns dict(p, T, amplitude, itnewton, itlinear, ds, orbit, converged).

    ``nev > 0``: at every recorded point the ``nev`` leading Floquet multipliers (``floquet_multipliers`` with the orbit
    preconditioner's (a, b), ``eig``), recorded as ``floquet`` (the exponents), ``n_unstable`` (Re sigma > tol_stability), ``n_imag``
    (the unstable ones with |Im sigma| > tol_stability) and ``stable``; ``detect_bifurcation >= 2`` adds ``specialpoints``: one
    dict(step, interval, type, delta, ind_ev) whenever n_unstable changes between two points (``classify_po_bifurcation``; no
    bisection).  With the defaults nothing of this runs.  ``save_sol``: every special point also carries ``x`` (a copy of the orbit
    and T at the point after the crossing, a BorderedArray), ``tau`` (the secant tangent there, BorderedArray(BorderedArray(u, T),
    p)) and ``param`` -- what ``po_fold_point`` starts from; the records and the library calls are otherwise those of the default."""
    params = [float(x) for x in params]
    ipar = po.prob.param_names.index(lens) if isinstance(lens, str) else int(lens)
    pl = _precond_for(po, ls, params).set_period(T)
    lin = _PoLinearSolver(ls, pl)
    bls = _PoBordering(lin)
    F = _PoFunctional(po, params, ipar)
    nopt = Cn.NewtonPar(tol=cp.newton_options.tol, max_iterations=cp.newton_options.max_iterations,
                        verbose=cp.newton_options.verbose, linsolver=lin)
    p0 = params[ipar]
    s0 = Cn.newton(F, BorderedArray(orbit, float(T)), p0, nopt, _norminf)
    if not s0.converged:
        raise RuntimeError("Newton failed to converge for the initial guess on the branch")
    p1 = p0 + cp.ds / cp.eta
    s1 = Cn.newton(F, s0.u, p1, nopt, _norminf)
    if not s1.converged:
        raise RuntimeError("Newton failed to converge. Required for the computation of the initial tangent")
    z0, z1 = BorderedArray(s0.u, p0), BorderedArray(s1.u, p1)
    br = dict(p=[], T=[], amplitude=[], itnewton=[], itlinear=[], ds=[], converged=[])

    def record(z, sol, ds, it):
        br["p"].append(z.p); br["T"].append(z.u.p); br["amplitude"].append(amplitude(z.u.u))
        br["itnewton"].append(sol.itnewton); br["itlinear"].append(it); br["ds"].append(ds); br["converged"].append(sol.converged)

    if nev > 0:
        br.update(floquet=[], n_unstable=[], n_imag=[], stable=[], eig_converged=[])
        if detect_bifurcation >= 2:
            br["specialpoints"] = []

    def record_stability(z, step):
        fl = floquet_multipliers(po, z.u.u, z.u.p, F.pv(z.p), nev, ls, eig=eig, a=pl.a, b=pl.b)
        nu, ni = stability_counts(fl["exponents"], tol_stability)
        if detect_bifurcation >= 2 and br["n_unstable"] and nu != br["n_unstable"][-1]:
            tp = classify_po_bifurcation(nu, br["n_unstable"][-1], ni, br["n_imag"][-1])
            if tp is not None:
                sp = dict(step=step, interval=(br["p"][-2], br["p"][-1]), **tp)
                if save_sol:
                    sp.update(x=z.u.copy(), tau=Cn.secant_tangent(z, z_old, ds, theta), param=z.p)
                br["specialpoints"].append(sp)
        br["floquet"].append(fl["exponents"]); br["n_unstable"].append(nu); br["n_imag"].append(ni); br["stable"].append(nu == 0)
        br["eig_converged"].append(fl["converged"])

    ds = cp.ds
    tau = Cn.secant_tangent(z1, z0, ds, theta)
    z, z_old = z0.copy(), z0.copy()
    z_pred = z.copy().add_(tau, ds)
    record(z, s0, ds, list(lin.counts))
    if nev > 0:
        record_stability(z, 0)
    step = 0
    while step < cp.max_steps and (cp.p_min < z.p < cp.p_max or step == 0):
        before = len(lin.counts)
        if update_section_every_step and step % update_section_every_step == 0:
            po.update_section(z.u.u, z.u.p, F.pv(z.p))
            pl.set_period(z.u.p)
        sol = Cn.newton_palc(F, z, tau, z_pred, ds, theta, bls, nopt, cp.p_min, cp.p_max, _norminf)
        if verbosity:
            print(f"step {step:3d} ds={ds:+.3e} p={z.p:+.6f} -> {sol.u.p:+.6f} conv={sol.converged} itnewton={sol.itnewton}")
        if sol.converged:
            z_old.copyto_(z)
            z.copyto_(sol.u)
            step += 1
            record(z, sol, ds, lin.counts[before:])
            if nev > 0:
                record_stability(z, step)
        ds, stop = Cn.step_size_control(ds, sol.converged, sol.itnewton, cp)
        if stop:
            break
        if sol.converged:
            tau = Cn.secant_tangent(z, z_old, ds, theta)
        z_pred = z.copy().add_(tau, ds)
    br["orbit"] = z.u
    return br


def po_fold_point(br: dict, ind: int = 0, po: PeriodicOrbitTrap | None = None, params=None, lens=None):
    """The guess of newton_fold(br_po, indfold) from special point ``ind`` of a ``continuation_po_trap(..., save_sol=True)`` branch
    (fold_point, cGL2d.jl:354; newton_fold :244-247): dict(orbit, T, p, a, b) with a = b = the (u, T) part of the saved tangent,
    normalised in the 2-norm.  With ``po``, ``params`` and ``lens`` also updatesection! at the guess (cGL2d.jl:365), the section
    the fold system then keeps frozen."""
    sp = br["specialpoints"][ind]
    if "x" not in sp:
        raise ValueError("po_fold_point needs a branch of continuation_po_trap(..., save_sol=True)")
    x, tau = sp["x"], sp["tau"].u.copy()
    nrm = math.sqrt(tau.u.norm() ** 2 + tau.p ** 2)
    tau.u.scale_(1.0 / nrm)
    tau.p /= nrm
    if po is not None:
        pv = [float(v) for v in params]
        pv[po.prob.param_names.index(lens) if isinstance(lens, str) else int(lens)] = float(sp["param"])
        po.update_section(x.u, x.p, pv)
    return dict(orbit=x.u.copy(), T=float(x.p), p=float(sp["param"]), a=tau, b=tau)


def get_periodic_orbit(po: PeriodicOrbitTrap, u: HipVec, T: float):
    """get_periodic_orbit (:651-657): (times, slices) with times = cumsum(T * [1 / M] * M) and slices of shape (M, N)."""
    times = np.cumsum(np.full(po.M, float(T) * (1.0 / po.M)))
    return times, u.numpy().reshape(po.M, po.N)


# ------------------------------------------------------------------------------------------ Floquet multipliers
class PoTrapMonodromy:
    """dx -> MonodromyQaD_matrix_free(trap, u, par, dx) (src/periodicorbit/Floquet.jl:285-315) as an operator handle
    (bk_potrap_monodromy_create): one space-time GMRES on the K = M - 1 slices of the initial-value system per application, in
    the place of K slice solves one after another.  ``ls``: the GMRES options; ``(a, b)``: the preconditioner's constant-coefficient
    operator, default a = r, b = nu.  Keeps ``u`` alive."""

    def __init__(self, po: PeriodicOrbitTrap, u: HipVec, T: float, params, ls: _GMRES, a: float | None = None,
                 b: float | None = None):
        self.po, self.ctx, self.u, self.T, self.params = po, po.ctx, u, float(T), [float(x) for x in params]
        self.a = self.params[0] if a is None else float(a)
        self.b = self.params[2] if b is None else float(b)
        o = ls._opts()
        h = C.c_void_p()
        self.ctx.check(self.ctx.lib.bk_potrap_monodromy_create(po.h, _ptr(u.t), self.T, _parr(self.params), len(self.params),
                                                               self.a, self.b, C.byref(o), C.byref(h)), "bk_potrap_monodromy_create")
        self.h = h

    def _x(self, x: HipVec):
        if x.n != self.po.N:
            raise ValueError(f"the monodromy acts on one slice of N = {self.po.N} doubles")
        return x

    def __call__(self, x: HipVec, a0=0.0, a1=1.0) -> HipVec:
        out = self._x(x).similar()
        self.ctx.check(self.ctx.lib.bk_op_apply(self.h, _ptr(x.t), float(a0), float(a1), _ptr(out.t)), "bk_op_apply")
        return out

    def solve(self, x: HipVec):
        """One application that returns all K slices -> (y_all (K N doubles), converged, niter); the monodromy applied to x is the
        last slice."""
        y = HipVec(self.ctx, self.ctx.empty(self.po.N * (self.po.M - 1)))
        cv, it = C.c_int(), C.c_int()
        self.ctx.check(self.ctx.lib.bk_potrap_monodromy_solve(self.h, _ptr(self._x(x).t), _ptr(y.t), C.byref(cv), C.byref(it)),
                       "bk_potrap_monodromy_solve")
        return y, bool(cv.value), it.value

    def stats(self):
        """dict(solves, failed, inner_its, paths) since creation; paths: the transform kernels of the last preconditioner
        application per axis (PoTrapPreconditioner.transform_paths)."""
        s, f, it, p = C.c_int(), C.c_int(), C.c_int(), (C.c_int * 2)()
        self.ctx.check(self.ctx.lib.bk_potrap_monodromy_stats(self.h, C.byref(s), C.byref(f), C.byref(it), p),
                       "bk_potrap_monodromy_stats")
        return dict(solves=s.value, failed=f.value, inner_its=it.value, paths=(p[0], p[1]))

    def __del__(self):
        try:
            if self.h.value:
                self.ctx.lib.bk_op_destroy(self.h)
        except Exception:
            pass


def ivp_march(po: PeriodicOrbitTrap, u: HipVec, T: float, params, y: HipVec, out: HipVec | None = None) -> HipVec:
    """The initial-value operator of the monodromy on K slices (bk_potrap_ivp_march)."""
    out = y.similar() if out is None else out
    po.ctx.check(po.ctx.lib.bk_potrap_ivp_march(po.h, _ptr(u.t), float(T), _parr(params), len(params), _ptr(y.t), _ptr(out.t)),
                 "bk_potrap_ivp_march")
    return out


class PoTrapIvpPreconditioner:
    """A0^-1 of the initial-value system on K N doubles (bk_precond_potrap_ivp_create); the period is fixed at creation."""

    def __init__(self, po: PeriodicOrbitTrap, a: float, b: float, T: float):
        self.po, self.ctx = po, po.ctx
        h = C.c_void_p()
        self.ctx.check(self.ctx.lib.bk_precond_potrap_ivp_create(po.h, float(a), float(b), float(T), C.byref(h)),
                       "bk_precond_potrap_ivp_create")
        self.h = h

    ldiv = PoTrapPreconditioner.ldiv
    __del__ = PoTrapPreconditioner.__del__

    def transform_paths(self):
        p = (C.c_int * 2)()
        self.ctx.check(self.ctx.lib.bk_precond_potrap_ivp_transform_paths(self.h, p), "bk_precond_potrap_ivp_transform_paths")
        return p[0], p[1]


def monodromy_sequential(po: PeriodicOrbitTrap, u: HipVec, T: float, params, x: HipVec, ls: _GMRES, a: float | None = None,
                         b: float | None = None):
    """The call-by-call mirror of MonodromyQaD_matrix_free(::Trapeze) (Floquet.jl:285-315): per step out <- out + (h / 2) J_prev out
    (bk_jacobian, bk_op_apply with (1, h / 2)), then the slice solve (I - (h / 2) J_i) res = out (bk_gmres with a0 = 1, a1 = -h / 2,
    the options of ``ls``).  Left preconditioner bk_precond_cgl_create(a - 2 / h, b): (L0 - 2 / h)^-1 = -(h / 2) (I - (h / 2) L0)^-1,
    the slice preconditioner up to the factor -2 / h on the right-hand side, which the library applies to both sides of the solve.
    The parity yardstick and the timing baseline of PoTrapMonodromy, not a product path.  Returns (out, inner iterations summed,
    all converged)."""
    from .hip import CGLBlockPreconditioner, HipJacobian
    params = [float(v) for v in params]
    prob, N, K = po.prob, po.N, po.M - 1
    h = float(T) * (1.0 / po.M)
    a = params[0] if a is None else a
    b = params[2] if b is None else b
    sl = [HipVec(po.ctx, u.t[i * N:(i + 1) * N], prob.nglobal) for i in range(K)]
    o = ls._opts()
    pl = CGLBlockPreconditioner(prob, a - 2.0 / h, b)
    out, its, ok = x, 0, True
    lib, ctx = po.ctx.lib, po.ctx
    for i in range(K):
        out = HipJacobian(prob, sl[K - 1 if i == 0 else i - 1], params)(out, 1.0, h / 2.0)
        Ji = HipJacobian(prob, sl[i], params)
        res = out.similar()
        cv, it, rn = C.c_int(), C.c_int(), C.c_double()
        ctx.check(lib.bk_gmres(ctx.h, Ji.h, _ptr(out.t), _ptr(res.t), 1.0, -h / 2.0, C.byref(o), pl.h, C.byref(cv), C.byref(it),
                               C.byref(rn)), "bk_gmres")
        its += it.value
        ok = ok and bool(cv.value)
        out = res
    return out, its, ok


def floquet_multipliers(po: PeriodicOrbitTrap, u: HipVec, T: float, params, nev: int, ls: _GMRES, eig=None, a: float | None = None,
                        b: float | None = None, mono: PoTrapMonodromy | None = None):
    """compute_eigenvalues(::FloquetQaD, ...) (Floquet.jl:59-85) on the matrix-free monodromy: Krylov-Schur with which = :LM
    (bk_eig_krylovkit_lm; ``eig``: an EigKrylovKit whose tol, maxiter, krylovdim, seed and x0 are used; default tol 1e-8, krylovdim
    20).  Returns dict(multipliers, exponents, vectors, converged, numops, inner_its): exponents = log(complex(mu)) sorted by
    decreasing real part (:74-79), multipliers and vectors ((re, im) pairs) in the same order; a value that did not converge is
    NaN.  Warns where a multiplier is infinite or NaN."""
    import warnings

    from .hip import EigKrylovKit
    mono = PoTrapMonodromy(po, u, T, params, ls, a, b) if mono is None else mono
    eig = EigKrylovKit(tol=1e-8, maxiter=20, krylovdim=20) if eig is None else eig
    ctx, n = po.ctx, po.N
    if eig.x0 is not None:
        ctx.check(ctx.lib.bk_eig_set_start_vector(ctx.h, _ptr(eig.x0.t)), "bk_eig_set_start_vector")
    kd = min(eig.krylovdim, 63, n - 1)
    nev = min(int(nev), kd)
    eo = L.EigOpts(0.0, int(kd), int(eig.maxiter), float(eig.tol), 0, int(eig.seed))
    re, im = (C.c_double * (nev + 1))(), (C.c_double * (nev + 1))()
    ld = (n + 31) // 32 * 32
    vr, vi = ctx.empty(ld * (nev + 1)), ctx.empty(ld * (nev + 1))
    nvals, nconv, nops = C.c_int(), C.c_int(), C.c_int()
    before = mono.stats()["inner_its"]
    ctx.check(ctx.lib.bk_eig_krylovkit_lm(ctx.h, mono.h, nev, C.byref(eo), re, im, _ptr(vr), _ptr(vi), ld, C.byref(nvals),
                                          C.byref(nconv), C.byref(nops)), "bk_eig_krylovkit_lm")
    m = nvals.value
    vals = np.array([complex(re[i], im[i]) for i in range(m)])
    if not np.all(np.isfinite(vals)):
        warnings.warn("Detecting infinite or NaN eigenvalue during the computation of Floquet coefficients.")
    sigma = floquet_exponents(vals)
    order = _exponent_order(sigma)
    vecs = [(HipVec(ctx, vr[i * ld:i * ld + n]), HipVec(ctx, vi[i * ld:i * ld + n])) for i in order]
    return dict(multipliers=vals[order], exponents=sigma[order], vectors=vecs, converged=nconv.value >= nev, numops=nops.value,
                inner_its=mono.stats()["inner_its"] - before, monodromy=mono)


def floquet_exponents(mults):
    """log.(complex.(vals)) (Floquet.jl:75), unsorted; log(0) = -inf."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.log(np.asarray(mults, dtype=complex))


def _exponent_order(sigma):
    """sortperm(logvals, by = real, rev = true) (Floquet.jl:76), NaN last."""
    key = np.where(np.isnan(sigma.real), -np.inf, sigma.real)
    return [int(i) for i in np.argsort(-key, kind="stable")]


def floquet_eigenfunction(mono: PoTrapMonodromy, zeta):
    """The space-time eigenfunction of a Floquet eigenvector (Val(:ExtractEigenVector), Floquet.jl:319-355): the K slices of the
    solve that applies the monodromy to ``zeta``; a ``(re, im)`` pair gives a pair.  Slices are numbered as the reference numbers
    them: the last one is mu zeta."""
    if isinstance(zeta, (tuple, list)):
        return tuple(mono.solve(z)[0] if z is not None else None for z in zeta)
    return mono.solve(zeta)[0]


def stability_counts(exponents, tol_stability):
    """(n_unstable, n_imag): the exponents with Re sigma > tol_stability, and those of them with |Im sigma| > tol_stability
    (NaN entries are ignored, as is_stable ignores them)."""
    s = np.asarray(exponents, dtype=complex)
    s = s[~np.isnan(s.real)]
    un = s[s.real > tol_stability]
    return int(un.size), int(np.sum(np.abs(un.imag) > tol_stability))


def classify_po_bifurcation(n_unstable, n_unstable_prev, n_imag, n_imag_prev):
    """_get_bifurcation_type (src/Bifurcations.jl:80-151) for a Floquet solver, from the stability counts of two consecutive points:
    None when n_unstable did not change, else dict(type, delta, ind_ev) with type "bp" (one real exponent crosses), "pd" (one, with
    a nonzero imaginary part: the multiplier crosses at -1), "ns" (a pair) or "nd" (anything else, a missing conjugate -- fewer
    crossings than new imaginary parts --, or counts not yet populated, < 0).  Pure: needs no device."""
    du, di = abs(n_unstable - n_unstable_prev), abs(n_imag - n_imag_prev)
    if du == 0 and not du < di:
        return None
    if du == 1:
        tp = "bp" if di == 0 else ("pd" if di == 1 else "nd")
    elif du == 2:
        tp = "ns" if di == 2 else "nd"
    else:
        tp = "nd"
    if du < di or n_unstable * n_unstable_prev < 0 or n_imag * n_imag_prev < 0:
        tp = "nd"
    return dict(type=tp, delta=(n_unstable - n_unstable_prev, n_imag - n_imag_prev),
                ind_ev=n_unstable_prev if n_unstable < n_unstable_prev else n_unstable)
