"""Periodic orbits of the cGL problem by the trapezoid rule: the second half of examples/cGL2d.jl (:166-260) on the device.

  PeriodicOrbitTrap          Trapeze(prob, phi, xpi, M, 2n; jacobian = FullMatrixFree())   src/periodicorbit/PeriodicOrbitTrapeze.jl
  PoTrapPreconditioner       the space-time spectral preconditioner diag(A0, 1) in the place of the example's ILU (:209-213)
  po_guess_from_hopf         the guess of :172-174 and the section of :177-181 from predictor(hopf, ds)
  newton_po_trap             newton(poTrapMF, orbitguess_f, opt_po; normN = norminf)        :213-219
  continuation_po_trap       continuation(poTrapMF, outpo_f.u, PALC(), ...), secant tangent, BorderingBLS, updatesection every step
  get_periodic_orbit         :651-657

An orbit is ``BorderedArray(u, T)``: ``u`` the M slices [u1; u2] on the device, ``T`` the period entry on the host.  The time step
is h = T / M on each of the M - 1 intervals (src/TimeMesh.jl:21), so ``T`` is M / (M - 1) times the orbit's period -- the
reference's convention, kept.  Newton and PALC are the ones of ``continuation.py`` (``newton``, ``newton_palc``, ``secant_tangent``,
``step_size_control``), run on this functional.  The hot path -- functional, Jacobian-vector product, preconditioner, GMRES -- is
``csrc/potrap.hip``.
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
    """dG(u, T) as an operator handle (bk_potrap_op_create); keeps ``u`` alive."""

    def __init__(self, po: PeriodicOrbitTrap, u: HipVec, T: float, params):
        self.po, self.ctx, self.u, self.T, self.params = po, po.ctx, u, float(T), list(params)
        h = C.c_void_p()
        self.ctx.check(self.ctx.lib.bk_potrap_op_create(po.h, _ptr(u.t), self.T, _parr(params), len(params), C.byref(h)),
                       "bk_potrap_op_create")
        self.h = h

    def __call__(self, dx: BorderedArray) -> BorderedArray:
        return self.po.jvp(self.u, self.T, self.params, dx.u, dx.p)

    def __del__(self):
        try:
            if self.h.value:
                self.ctx.lib.bk_op_destroy(self.h)
        except Exception:
            pass


class PoTrapPreconditioner:
    """P = diag(A0, 1), A0 the orbit Jacobian with every J_i replaced by Lap (x) I_2 + [[a, -b], [b, a]]; the default
    a = r, b = nu is the linearisation at the trivial state.  ``set_period`` refuses a Hopf-critical (a, b)."""

    def __init__(self, po: PeriodicOrbitTrap, a: float | None = None, b: float | None = None, params=None):
        self.po, self.ctx = po, po.ctx
        pv = po.prob._pvec(po.prob.params[po.prob.lens]) if params is None else list(params)
        a = pv[0] if a is None else a
        b = pv[2] if b is None else b
        h = C.c_void_p()
        self.ctx.check(self.ctx.lib.bk_precond_potrap_create(po.h, float(a), float(b), C.byref(h)), "bk_precond_potrap_create")
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
    preconditioner handle ``.h``; the library refuses one that is not a PoTrapPreconditioner of this orbit's size."""
    ctx = J.ctx
    x, xt = rhs.u.similar(), C.c_double()
    o = ls._opts()
    res = L.SolveResult()
    ctx.check(ctx.lib.bk_potrap_solve(ctx.h, J.h, pl.h if pl is not None else None, _ptr(rhs.u.t), float(rhs.p), _ptr(x.t),
                                      C.byref(xt), C.byref(o), C.byref(res)), "bk_potrap_solve")
    return BorderedArray(x, xt.value), bool(res.converged), int(res.niter)


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
                         theta=0.5, update_section_every_step=1, verbosity=0):
    """PALC on the (N M + 1) + 1 system (continuation(poTrapMF, ..., PALC()) of cGL2d.jl:221-260): two Newton solves and the secant
    tangent, then per step newton_palc with BorderingBLS -- two preconditioned solves per Newton step, d_p G analytic --, the
    step-size control of continuation.py and updatesection! after every accepted step (the reference's default).  ``lens``: the
    name or index of the continuation parameter.  Returns dict(p, T, amplitude, itnewton, itlinear, ds, orbit, converged)."""
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

    ds = cp.ds
    tau = Cn.secant_tangent(z1, z0, ds, theta)
    z, z_old = z0.copy(), z0.copy()
    z_pred = z.copy().add_(tau, ds)
    record(z, s0, ds, list(lin.counts))
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
        ds, stop = Cn.step_size_control(ds, sol.converged, sol.itnewton, cp)
        if stop:
            break
        if sol.converged:
            tau = Cn.secant_tangent(z, z_old, ds, theta)
        z_pred = z.copy().add_(tau, ds)
    br["orbit"] = z.u
    return br


def get_periodic_orbit(po: PeriodicOrbitTrap, u: HipVec, T: float):
    """get_periodic_orbit (:651-657): (times, slices) with times = cumsum(T * [1 / M] * M) and slices of shape (M, N)."""
    times = np.cumsum(np.full(po.M, float(T) * (1.0 / po.M)))
    return times, u.numpy().reshape(po.M, po.N)
