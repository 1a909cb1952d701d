"""Periodic orbits of the cGL problem by standard shooting on a spectral ETDRK2 flow: examples/cGL2d-shooting.jl on the device.

  Flow                          the flow of SplitODEProblem(Lap, NL) + ETDRK2 (:108-113): evolve, jvp          csrc/flow.hip
  ShootingProblem               Shooting(prob_sp, ETDRK2(), ...) with SectionSS (:123-128)                     csrc/shooting.hip
  ShootingJacobian              dG(x, T) as an operator handle (stored or recomputed base trajectory)
  shooting_solve                the unpreconditioned GMRES of :135
  shooting_guess_from_flow      the guess of :110-113, :130: integrate, then M states T_guess / M apart
  shooting_guess_from_hopf      the guess and section of continuation(br, 1, ..., Shooting(Mt, ...)) (:160-174; re_make,
                                src/periodicorbit/StandardShooting.jl:369-385) from the Hopf predictor
  newton_po_shooting            newton(probSh, initpo, optn; normN = norminf) (:136-137)
  continuation_po_shooting      continuation(probSh, outpo.u, PALC(), ...) (:142-150), secant tangent, bordering on two solves
  ShootingMonodromy, floquet_multipliers_shooting    MonodromyQaD_matrix_free(::Shooting) + Krylov-Schur (Floquet.jl:59-108)
  get_periodic_orbit_shooting   the orbit by evolve

An orbit is ``BorderedArray(x, T)``: ``x`` the M states [u1; u2] on the device, ``T`` the period on the host (the true period: the
segments are T / M long).  Newton, PALC and the step control are the ones of ``continuation.py``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib as L
from . import continuation as Cn
from .hip import BorderedArray, HipVec, _GMRES, _ptr
from .periodic_orbit import (_exponent_order, _norminf, _parr, amplitude, classify_po_bifurcation, floquet_exponents,
                             stability_counts)


class Flow:
    """B trajectories of the spectral ETDRK2 flow in lock-step (bk_flow_create); trajectory i is [u1; u2] at i N."""

    def __init__(self, prob, B: int = 1):
        self.prob, self.ctx, self.B, self.N = prob, prob.ctx, int(B), prob.nlocal
        h = C.c_void_p()
        self.ctx.check(self.ctx.lib.bk_flow_create(prob.h, self.B, C.byref(h)), "bk_flow_create")
        self.h = h

    def evolve(self, x: HipVec, tau: float, nsteps: int, params, out: HipVec | None = None) -> HipVec:
        out = x.similar() if out is None else out
        self.ctx.check(self.ctx.lib.bk_flow_evolve(self.h, _ptr(x.t), float(tau), int(nsteps), _parr(params), len(params),
                                                   _ptr(out.t)), "bk_flow_evolve")
        return out

    def jvp(self, x: HipVec, dx: HipVec, tau: float, nsteps: int, params):
        """(Phi(x, tau), dPhi(x, tau) dx) from one march."""
        out, dout = x.similar(), x.similar()
        self.ctx.check(self.ctx.lib.bk_flow_jvp(self.h, _ptr(x.t), _ptr(dx.t), float(tau), int(nsteps), _parr(params), len(params),
                                                _ptr(out.t), _ptr(dout.t)), "bk_flow_jvp")
        return out, dout

    def coefficients(self, h: float):
        """(E, h phi1, h phi2) of the step h, one entry per sine mode in natural order."""
        n = self.N // 2
        E, P1, P2 = (np.empty(n) for _ in range(3))
        dp = lambda a: a.ctypes.data_as(L.c_double_p)
        self.ctx.check(self.ctx.lib.bk_flow_coefficients(self.h, float(h), dp(E), dp(P1), dp(P2)), "bk_flow_coefficients")
        return E, P1, P2

    def transform_paths(self):
        p = (C.c_int * 2)()
        self.ctx.check(self.ctx.lib.bk_flow_transform_paths(self.h, p), "bk_flow_transform_paths")
        return p[0], p[1]

    def stats(self):
        b, l = C.c_longlong(), C.c_longlong()
        self.ctx.check(self.ctx.lib.bk_flow_stats(self.h, C.byref(b), C.byref(l)), "bk_flow_stats")
        return dict(base_marches=b.value, launches=l.value)

    def __del__(self):
        try:
            if self.h.value:
                self.ctx.lib.bk_flow_destroy(self.h)
        except Exception:
            pass


class ShootingProblem:
    """The handle of the functional (bk_shooting_create): M segments of nsteps ETDRK2 steps each."""

    def __init__(self, prob, M: int, nsteps: int):
        self.prob, self.ctx, self.M, self.nsteps = prob, prob.ctx, int(M), int(nsteps)
        self.N = prob.nlocal
        h = C.c_void_p()
        self.ctx.check(self.ctx.lib.bk_shooting_create(prob.h, self.M, self.nsteps, C.byref(h)), "bk_shooting_create")
        self.h = h
        self._flow1 = None

    @property
    def n(self):
        return self.N * self.M

    def vec(self, a) -> HipVec:
        return HipVec.from_numpy(self.ctx, np.asarray(a, dtype=np.float64).reshape(-1))

    @property
    def section(self):
        """(normal, center), copies of the section in force."""
        nrm, cen = (HipVec(self.ctx, self.ctx.empty(self.N)) for _ in range(2))
        self.ctx.check(self.ctx.lib.bk_shooting_get_section(self.h, _ptr(nrm.t), _ptr(cen.t)), "bk_shooting_get_section")
        return nrm, cen

    @section.setter
    def section(self, nc):
        normal, center = nc
        if normal.n != self.N or center.n != self.N:
            raise ValueError(f"section vectors must hold N = {self.N} doubles")
        self.ctx.check(self.ctx.lib.bk_shooting_set_section(self.h, _ptr(normal.t), _ptr(center.t)), "bk_shooting_set_section")

    def update_section(self, x: HipVec, T: float, params):
        """updatesection! (StandardShooting.jl:116-122)."""
        self.ctx.check(self.ctx.lib.bk_shooting_update_section(self.h, _ptr(x.t), float(T), _parr(params), len(params)),
                       "bk_shooting_update_section")

    def residual(self, x: HipVec, T: float, params) -> BorderedArray:
        out, tail = x.similar(), C.c_double()
        self.ctx.check(self.ctx.lib.bk_shooting_residual(self.h, _ptr(x.t), float(T), _parr(params), len(params), _ptr(out.t),
                                                         C.byref(tail)), "bk_shooting_residual")
        return BorderedArray(out, tail.value)

    def jvp(self, x: HipVec, T: float, params, dx: HipVec, dT: float) -> BorderedArray:
        out, tail = x.similar(), C.c_double()
        self.ctx.check(self.ctx.lib.bk_shooting_jvp(self.h, _ptr(x.t), float(T), _parr(params), len(params), _ptr(dx.t), float(dT),
                                                    _ptr(out.t), C.byref(tail)), "bk_shooting_jvp")
        return BorderedArray(out, tail.value)

    def jacobian(self, x: HipVec, T: float, params) -> "ShootingJacobian":
        return ShootingJacobian(self, x, T, params)

    def transform_paths(self):
        p = (C.c_int * 2)()
        self.ctx.check(self.ctx.lib.bk_shooting_transform_paths(self.h, p), "bk_shooting_transform_paths")
        return p[0], p[1]

    def _one(self) -> Flow:
        if self._flow1 is None:
            self._flow1 = Flow(self.prob, 1)
        return self._flow1

    def evolve(self, x: HipVec, tau: float, params, nsteps: int | None = None) -> HipVec:
        """evolve(flow, x, par, tau).u for one state; ``nsteps`` defaults to the functional's."""
        return self._one().evolve(x, tau, self.nsteps if nsteps is None else nsteps, params)

    def flow_jvp(self, x: HipVec, dx: HipVec, tau: float, params, nsteps: int | None = None):
        return self._one().jvp(x, dx, tau, self.nsteps if nsteps is None else nsteps, params)

    def __del__(self):
        try:
            if self.h.value:
                self.ctx.lib.bk_shooting_destroy(self.h)
        except Exception:
            pass


class ShootingJacobian:
    """dG(x, T) as an operator handle (bk_shooting_op_create); keeps ``x`` alive.  With context option ``shooting_store`` = 1 (the
    default) the base trajectory is marched once, here, and every application marches the tangent alone."""

    def __init__(self, sh: ShootingProblem, x: HipVec, T: float, params):
        self.sh, self.ctx, self.x, self.T, self.params = sh, sh.ctx, x, float(T), [float(v) for v in params]
        h = C.c_void_p()
        self.ctx.check(self.ctx.lib.bk_shooting_op_create(sh.h, _ptr(x.t), self.T, _parr(self.params), len(self.params), C.byref(h)),
                       "bk_shooting_op_create")
        self.h = h

    def __call__(self, dx: BorderedArray) -> BorderedArray:
        out, tail = dx.u.similar(), C.c_double()
        self.ctx.check(self.ctx.lib.bk_shooting_op_apply(self.h, _ptr(dx.u.t), float(dx.p), _ptr(out.t), C.byref(tail)),
                       "bk_shooting_op_apply")
        return BorderedArray(out, tail.value)

    def stats(self):
        return _op_stats(self.ctx, self.h)

    def __del__(self):
        try:
            if self.h.value:
                self.ctx.lib.bk_op_destroy(self.h)
        except Exception:
            pass


def _op_stats(ctx, h):
    s, b, a = C.c_int(), C.c_longlong(), C.c_longlong()
    ctx.check(ctx.lib.bk_shooting_op_stats(h, C.byref(s), C.byref(b), C.byref(a)), "bk_shooting_op_stats")
    return dict(stored=bool(s.value), base_marches=b.value, applications=a.value)


def shooting_solve(J: ShootingJacobian, rhs: BorderedArray, ls: _GMRES):
    """One unpreconditioned GMRES on dG x = rhs (bk_shooting_solve) -> (x, converged, niter)."""
    ctx = J.ctx
    x, xt = rhs.u.similar(), C.c_double()
    o = ls._opts()
    res = L.SolveResult()
    ctx.check(ctx.lib.bk_shooting_solve(ctx.h, J.h, _ptr(rhs.u.t), float(rhs.p), _ptr(x.t), C.byref(xt), C.byref(o), C.byref(res)),
              "bk_shooting_solve")
    return BorderedArray(x, xt.value), bool(res.converged), int(res.niter)


def _slices_to_orbit(ctx, sl):
    return HipVec(ctx, torch.cat([s.t for s in sl]).contiguous())


def shooting_guess_from_flow(prob, x0: HipVec, t_end: float, nsteps: int, T_guess: float, M: int, params, sh: ShootingProblem | None = None):
    """The guess of cGL2d-shooting.jl:110-113, :130: integrate ``x0`` over ``t_end`` in ``nsteps`` steps, then take M states
    ``T_guess / M`` apart (each segment in ``sh.nsteps`` steps when ``sh`` is given, which also gets the section normal =
    F(x_1) / |F(x_1)|, center = x_1).  Returns dict(orbit, T)."""
    fl = Flow(prob, 1)
    sl = [fl.evolve(x0, t_end, nsteps, params)]
    seg = sh.nsteps if sh is not None else max(1, int(nsteps * T_guess / M / t_end))
    for _ in range(1, int(M)):
        sl.append(fl.evolve(sl[-1], (1.0 / M) * T_guess, seg, params))
    orbit = _slices_to_orbit(prob.ctx, sl)
    if sh is not None:
        sh.update_section(orbit, T_guess, params)
    return dict(orbit=orbit, T=float(T_guess))


def shooting_guess_from_hopf(pred: dict, M: int, prob=None, p: float | None = None, sh: ShootingProblem | None = None, params=None):
    """The guess of continuation(br, 1, ..., Shooting(Mt, ...)) (:160-174) from ``predictor(hopf, ds)``: the predictor's states at
    t_i = 2 pi i / M and its period.  With ``sh`` and ``params`` also the section of re_make (StandardShooting.jl:369-385):
    normal = F(x_1) / |F(x_1)|, center = x_1, at the parameter ``p`` (default: the predictor's).  Returns dict(orbit, T, p)."""
    sl = pred["orbit"].slices(M)
    orbit = _slices_to_orbit(sl[0].ctx, sl)
    out = dict(orbit=orbit, T=float(pred["period"]), p=float(pred["p"] if p is None else p))
    if sh is not None:
        pv = [float(v) for v in params]
        sh.update_section(orbit, out["T"], pv)
    return out


class _ShFunctional:
    """The functional as the ``prob`` of continuation.newton / newton_palc; d_p G by the reference's forward difference
    (Palc.jl:239-240, step ``prob.delta``)."""

    def __init__(self, sh: ShootingProblem, params, ipar: int):
        self.sh, self.params, self.ipar = sh, [float(x) for x in params], int(ipar)
        self.delta = sh.prob.delta

    def pv(self, p):
        pv = list(self.params)
        pv[self.ipar] = float(p)
        return pv

    def residual(self, x: BorderedArray, p: float) -> BorderedArray:
        return self.sh.residual(x.u, x.p, self.pv(p))

    def jacobian(self, x: BorderedArray, p: float) -> ShootingJacobian:
        return self.sh.jacobian(x.u, x.p, self.pv(p))


class _ShLinearSolver:
    """ls(J, rhs) -> (x, ok, it) on the unpreconditioned solve; ``counts`` keeps the GMRES count of every call."""

    def __init__(self, ls: _GMRES):
        self.ls, self.counts = ls, []

    def __call__(self, J, rhs, a0=0.0, a1=1.0):
        x, cv, it = shooting_solve(J, rhs, self.ls)
        self.counts.append(it)
        return x, cv, it


class _ShBordering:
    """BorderingBLS (src/LinearBorderSolver.jl:88-166, no precision check) on the shooting Jacobian: two solves."""

    def __init__(self, solver: _ShLinearSolver):
        self.solver = solver

    def __call__(self, J, dR, dzu, dzp, R, n, xiu=1.0, xip=1.0, *, shift=None, dotp=None, dotscale=None):
        x1, c1, i1 = self.solver(J, R)
        x2, c2, i2 = self.solver(J, dR)
        dl = (n - xiu * dotp(dzu, x1)) / (dzp * xip - xiu * dotp(dzu, x2))
        x1.add_(x2, -dl)
        return x1, dl, c1 and c2, (i1, i2)


def newton_po_shooting(sh: ShootingProblem, x: HipVec, T: float, params, ls: _GMRES, tol=1e-9, max_iterations=25, norm_inf=True,
                       verbose=False):
    """newton(probSh, initpo, optn; normN = norminf) (cGL2d-shooting.jl:135-137): ``_newton`` on the functional with the
    unpreconditioned matrix-free solve.  Returns dict(u, T, residuals, itlinear (per Newton step), converged, itnewton), the keys
    of ``newton_po_trap``."""
    params = [float(v) for v in params]
    lin = _ShLinearSolver(ls)
    F = _ShFunctional(sh, params, 0)
    opt = Cn.NewtonPar(tol=tol, max_iterations=max_iterations, verbose=verbose, linsolver=lin)
    s = Cn.newton(F, BorderedArray(x, float(T)), params[0], opt, _norminf if norm_inf else Cn.norm2)
    return dict(u=s.u.u, T=s.u.p, residuals=s.residuals, itlinear=list(lin.counts), converged=s.converged, itnewton=s.itnewton)


class ShootingMonodromy:
    """dx -> MonodromyQaD_matrix_free(sh, x, par, dx) (Floquet.jl:89-108) as an operator handle (bk_shooting_monodromy_create): the
    M segment tangents in sequence on the base trajectory kept at creation."""

    def __init__(self, sh: ShootingProblem, x: HipVec, T: float, params):
        self.sh, self.ctx, self.T, self.params = sh, sh.ctx, float(T), [float(v) for v in params]
        h = C.c_void_p()
        self.ctx.check(self.ctx.lib.bk_shooting_monodromy_create(sh.h, _ptr(x.t), self.T, _parr(self.params), len(self.params),
                                                                 C.byref(h)), "bk_shooting_monodromy_create")
        self.h = h

    def __call__(self, x: HipVec, a0=0.0, a1=1.0) -> HipVec:
        if x.n != self.sh.N:
            raise ValueError(f"the monodromy acts on one state of N = {self.sh.N} doubles")
        out = x.similar()
        self.ctx.check(self.ctx.lib.bk_op_apply(self.h, _ptr(x.t), float(a0), float(a1), _ptr(out.t)), "bk_op_apply")
        return out

    def stats(self):
        return _op_stats(self.ctx, self.h)

    __del__ = ShootingJacobian.__del__


def floquet_multipliers_shooting(sh: ShootingProblem, x: HipVec, T: float, params, nev: int, eig=None, mono: ShootingMonodromy | None = None):
    """compute_eigenvalues(::FloquetQaD, ...) (Floquet.jl:59-85) on the shooting monodromy: Krylov-Schur with which = :LM
    (bk_eig_krylovkit_lm; ``eig``: an EigKrylovKit whose tol, maxiter, krylovdim, seed and x0 are used; default tol 1e-8, krylovdim
    20).  Returns dict(multipliers, exponents, converged, numops, monodromy): exponents = log(complex(mu)) by decreasing real part."""
    from .hip import EigKrylovKit
    mono = ShootingMonodromy(sh, x, T, params) if mono is None else mono
    eig = EigKrylovKit(tol=1e-8, maxiter=20, krylovdim=20) if eig is None else eig
    ctx, n = sh.ctx, sh.N
    if eig.x0 is not None:
        ctx.check(ctx.lib.bk_eig_set_start_vector(ctx.h, _ptr(eig.x0.t)), "bk_eig_set_start_vector")
    kd = min(eig.krylovdim, 63, n - 1)
    nev = min(int(nev), kd)
    eo = L.EigOpts(0.0, int(kd), int(eig.maxiter), float(eig.tol), 0, int(eig.seed))
    re, im = (C.c_double * (nev + 1))(), (C.c_double * (nev + 1))()
    ld = (n + 31) // 32 * 32
    vr, vi = ctx.empty(ld * (nev + 1)), ctx.empty(ld * (nev + 1))
    nvals, nconv, nops = C.c_int(), C.c_int(), C.c_int()
    ctx.check(ctx.lib.bk_eig_krylovkit_lm(ctx.h, mono.h, nev, C.byref(eo), re, im, _ptr(vr), _ptr(vi), ld, C.byref(nvals),
                                          C.byref(nconv), C.byref(nops)), "bk_eig_krylovkit_lm")
    vals = np.array([complex(re[i], im[i]) for i in range(nvals.value)])
    sigma = floquet_exponents(vals)
    order = _exponent_order(sigma)
    return dict(multipliers=vals[order], exponents=sigma[order], converged=nconv.value >= nev, numops=nops.value, monodromy=mono)


def get_periodic_orbit_shooting(sh: ShootingProblem, x: HipVec, T: float, params, nout: int = 32):
    """(times, states): ``nout`` states of shape (nout, N) at times i T / nout, i < nout, by ``evolve`` from x_1 in steps of the
    functional's size (at least one per interval)."""
    N, tau = sh.N, float(T) / nout
    steps = max(1, -(-sh.nsteps * sh.M // nout))
    cur = HipVec(sh.ctx, x.t[:N].clone())
    states = [cur.numpy()]
    for _ in range(1, nout):
        cur = sh.evolve(cur, tau, params, steps)
        states.append(cur.numpy())
    return np.arange(nout) * tau, np.stack(states)


def continuation_po_shooting(sh: ShootingProblem, x: HipVec, T: float, params, lens, cp: Cn.ContinuationPar, ls: _GMRES, theta=0.5,
                             update_section_every_step=1, verbosity=0, nev=0, detect_bifurcation=0, tol_stability=1e-10, eig=None):
    """PALC on the (M N + 1) + 1 system (continuation(probSh, outpo.u, PALC(), ...), cGL2d-shooting.jl:142-150): two Newton solves
    and the secant tangent, then per step newton_palc with bordering on two unpreconditioned solves, d_p G by the forward
    difference of Palc.jl:239-240, the step control of continuation.py and updatesection! after every accepted step.  Returns
    dict(p, T, amplitude, itnewton, itlinear, ds, orbit, converged); ``nev``, ``detect_bifurcation`` and ``tol_stability`` as in
    ``continuation_po_trap`` (``floquet``, ``n_unstable``, ``n_imag``, ``stable``, ``specialpoints``)."""
    params = [float(v) for v in params]
    ipar = sh.prob.param_names.index(lens) if isinstance(lens, str) else int(lens)
    lin = _ShLinearSolver(ls)
    bls = _ShBordering(lin)
    F = _ShFunctional(sh, params, ipar)
    nopt = Cn.NewtonPar(tol=cp.newton_options.tol, max_iterations=cp.newton_options.max_iterations,
                        verbose=cp.newton_options.verbose, linsolver=lin)
    p0 = params[ipar]
    s0 = Cn.newton(F, BorderedArray(x, float(T)), p0, nopt, _norminf)
    if not s0.converged:
        raise RuntimeError("Newton failed to converge for the initial guess on the branch")
    p1 = p0 + cp.ds / cp.eta
    s1 = Cn.newton(F, s0.u, p1, nopt, _norminf)
    if not s1.converged:
        raise RuntimeError("Newton failed to converge. Required for the computation of the initial tangent")
    z0, z1 = BorderedArray(s0.u, p0), BorderedArray(s1.u, p1)
    br = dict(p=[], T=[], amplitude=[], itnewton=[], itlinear=[], ds=[], converged=[])
    if nev > 0:
        br.update(floquet=[], n_unstable=[], n_imag=[], stable=[], eig_converged=[])
        if detect_bifurcation >= 2:
            br["specialpoints"] = []

    def record(z, sol, ds, it, step):
        br["p"].append(z.p); br["T"].append(z.u.p); br["amplitude"].append(amplitude(z.u.u))
        br["itnewton"].append(sol.itnewton); br["itlinear"].append(it); br["ds"].append(ds); br["converged"].append(sol.converged)
        if nev > 0:
            fl = floquet_multipliers_shooting(sh, z.u.u, z.u.p, F.pv(z.p), nev, eig=eig)
            nu, ni = stability_counts(fl["exponents"], tol_stability)
            if detect_bifurcation >= 2 and br["n_unstable"] and nu != br["n_unstable"][-1]:
                tp = classify_po_bifurcation(nu, br["n_unstable"][-1], ni, br["n_imag"][-1])
                if tp is not None:
                    br["specialpoints"].append(dict(step=step, interval=(br["p"][-2], br["p"][-1]), **tp))
            br["floquet"].append(fl["exponents"]); br["n_unstable"].append(nu); br["n_imag"].append(ni); br["stable"].append(nu == 0)
            br["eig_converged"].append(fl["converged"])

    ds = cp.ds
    tau = Cn.secant_tangent(z1, z0, ds, theta)
    z, z_old = z0.copy(), z0.copy()
    z_pred = z.copy().add_(tau, ds)
    record(z, s0, ds, list(lin.counts), 0)
    step = 0
    while step < cp.max_steps and (cp.p_min < z.p < cp.p_max or step == 0):
        before = len(lin.counts)
        if update_section_every_step and step % update_section_every_step == 0:
            sh.update_section(z.u.u, z.u.p, F.pv(z.p))
        sol = Cn.newton_palc(F, z, tau, z_pred, ds, theta, bls, nopt, cp.p_min, cp.p_max, _norminf)
        if verbosity:
            print(f"step {step:3d} ds={ds:+.3e} p={z.p:+.6f} -> {sol.u.p:+.6f} conv={sol.converged} itnewton={sol.itnewton}")
        if sol.converged:
            z_old.copyto_(z)
            z.copyto_(sol.u)
            step += 1
            record(z, sol, ds, lin.counts[before:], step)
        ds, stop = Cn.step_size_control(ds, sol.converged, sol.itnewton, cp)
        if stop:
            break
        if sol.converged:
            tau = Cn.secant_tangent(z, z_old, ds, theta)
        z_pred = z.copy().add_(tau, ds)
    br["orbit"] = z.u
    return br
