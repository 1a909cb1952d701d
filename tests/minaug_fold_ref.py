"""CPU restatement of the minimally augmented fold formulation of src/codim2/MinAugFold.jl for the tests (test side only).

Generic: a model supplies F, J (dense or scipy.sparse), optionally J' (default: the transpose, so non-symmetric models work),
d2F and the parameter derivatives dF/dp and dJ/dp v (default: the reference's central differences, :88-95).  Every linear
solve is direct (dense LU / sparse LU), so the restatement carries no Krylov tolerance.

  bordered_vectors   _compute_bordered_vectors (:54-69): [J a; b' 0][v; sigma] = [0; 1], [J' b; a' 0][w; sigma2] = [0; 1]
  fold_linsolve      foldMALinearSolver, usehessian branch (:146-164)
  newton_fold        newton_fold (:211-233) under _newton (src/Newton.jl:66-114)
  continuation_fold  continuation_fold (:369-453): PALC on G(X, p2), X = (x, p1), BorderingBLS(check_precision = false) with the
                     fold linear solver, Secant tangent, update! of a / b after every converged step (:280-313), BT and CP of
                     test_bt_cusp (:551-576) -- the loop of bk_amd.codim2.continuation_fold
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle import palc

DELTA = 1e-8


def solve(J, rhs):
    if sp.issparse(J):
        return spla.spsolve(J.tocsc(), rhs)
    return np.linalg.solve(np.asarray(J), rhs)


class FoldModel:
    """F(x, pars), J(x, pars), d2F(x, pars, dx1, dx2) with ``pars`` a dict; lens1 = the fold parameter, lens2 = the second one.
    dFdp(x, pars, lens) and dJvdp(x, pars, lens, v) are optional (None: central differences of step DELTA, as the reference)."""

    def __init__(self, F, J, d2F, pars, lens1, lens2=None, Jt=None, dFdp=None, dJvdp=None):
        self.F, self.J, self.d2F = F, J, d2F
        self.pars = dict(pars)
        self.lens1, self.lens2 = lens1, lens2
        self.Jt = Jt if Jt is not None else (lambda x, q: J(x, q).T)
        self._dFdp, self._dJvdp = dFdp, dJvdp

    def at(self, p1, p2=None):
        q = dict(self.pars)
        q[self.lens1] = p1
        if p2 is not None:
            q[self.lens2] = p2
        return q

    def _pm(self, q, lens):
        qp, qm = dict(q), dict(q)
        qp[lens] += DELTA
        qm[lens] -= DELTA
        return qp, qm

    def dFdp(self, x, q, lens):
        if self._dFdp is not None:
            return self._dFdp(x, q, lens)
        qp, qm = self._pm(q, lens)
        return (self.F(x, qp) - self.F(x, qm)) / (2 * DELTA)

    def dJvdp(self, x, q, lens, v):
        if self._dJvdp is not None:
            return self._dJvdp(x, q, lens, v)
        qp, qm = self._pm(q, lens)
        return (self.J(x, qp) @ v - self.J(x, qm) @ v) / (2 * DELTA)


def bordered_solve(J, a, b):
    """[J a; b' 0][v; sigma] = [0; 1] as MatrixBLS solves it (the reference's default bdlinsolver): the (n+1) matrix, direct.
    Unlike J \\ a it stays regular at the fold itself."""
    n = a.shape[0]
    if sp.issparse(J):
        M = sp.bmat([[J, sp.csr_matrix(a.reshape(-1, 1))], [sp.csr_matrix(b.reshape(1, -1)), None]], format="csc")
    else:
        M = np.block([[np.asarray(J), a.reshape(-1, 1)], [b.reshape(1, -1), np.zeros((1, 1))]])
    rhs = np.zeros(n + 1)
    rhs[n] = 1.0
    y = solve(M, rhs)
    return y[:n], y[n]


def bordered_vectors(model, x, q, a, b):
    """(v, w, sigma) of _compute_bordered_vectors: [J a; b' 0][v; sigma] = [0; 1], [J' b; a' 0][w; sigma2] = [0; 1]."""
    v, sigma = bordered_solve(model.J(x, q), a, b)
    w, _ = bordered_solve(model.Jt(x, q), b, a)
    return v, w, sigma


def fold_linsolve(model, x, q, v, w, rhsu, rhsp):
    """Jfold [dX; dsig] = [rhsu; rhsp] with Jfold = [J dpF; sigma_x sigma_p] (usehessian branch)."""
    J = model.J(x, q)
    x1 = solve(J, rhsu)
    x2 = solve(J, model.dFdp(x, q, model.lens1))
    sx1 = -np.dot(w, model.d2F(x, q, x1, v))
    sx2 = -np.dot(w, model.d2F(x, q, x2, v))
    sp_ = -np.dot(w, model.dJvdp(x, q, model.lens1, v))
    dsig = (rhsp - sx1) / (sp_ - sx2)
    return x1 - dsig * x2, dsig


def _G(model, X, p2, a, b):
    x, p1 = X[:-1], X[-1]
    q = model.at(p1, p2)
    v, w, sigma = bordered_vectors(model, x, q, a, b)
    return np.append(model.F(x, q), sigma), v, w


def newton_fold(model, x0, p0, a, b, p2=None, tol=1e-12, max_iterations=25, normN=palc.norm2):
    """newton_fold with FoldLinearSolverMinAug under _newton: dict(u, p, residuals, converged, itnewton, v, w, sigma)."""
    X = np.append(np.asarray(x0, dtype=float), float(p0))
    G, v, w = _G(model, X, p2, a, b)
    res = [normN(G)]
    step = 0
    while step < max_iterations and res[-1] > tol:
        q = model.at(X[-1], p2)
        dX, dsig = fold_linsolve(model, X[:-1], q, v, w, G[:-1], G[-1])
        X = X - np.append(dX, dsig)
        G, v, w = _G(model, X, p2, a, b)
        res.append(normN(G))
        step += 1
    return dict(u=X[:-1], p=X[-1], residuals=res, converged=res[-1] < tol, itnewton=step, v=v, w=w, sigma=G[-1])


def continuation_fold(model, x0, p1, p2, a, b, *, ds, dsmin=1e-4, dsmax=0.1, a_ctrl=0.5, theta=0.5, p_min=-np.inf,
                      p_max=np.inf, max_steps=100, eta=150.0, tol=1e-12, max_iterations=25, normC=palc.norminf, ds_sequence=None):
    """PALC on G(X, p2) (continuation_fold with FoldLinearSolverMinAug wired through BorderingBLS, :445-453).
    Returns dict(p1, p2, BT, CP, ds, itnewton, X) with one entry per point (the starting point first)."""
    st = dict(a=np.asarray(a, dtype=float).copy(), b=np.asarray(b, dtype=float).copy())

    def G(X, p):
        return _G(model, X, p, st["a"], st["b"])

    def linsolve(X, p, v, w, R):
        dX, dsig = fold_linsolve(model, X[:-1], model.at(X[-1], p), v, w, R[:-1], R[-1])
        return np.append(dX, dsig)

    def dGdp2(X, p, v, w):
        x, q = X[:-1], model.at(X[-1], p)
        return np.append(model.dFdp(x, q, model.lens2), -np.dot(w, model.dJvdp(x, q, model.lens2, v)))

    def newton(X, p):
        R, v, w = G(X, p)
        res = [normC(R)]
        while len(res) <= max_iterations and res[-1] > tol:
            X = X - linsolve(X, p, v, w, R)
            R, v, w = G(X, p)
            res.append(normC(R))
        return X, res[-1] < tol, len(res) - 1

    def newton_palc(z0, tau, zp, ds_):
        N = lambda X, p: palc.arc_length_eq(X, z0[0], p - z0[1], tau[0], tau[1], theta, ds_)
        X, p = zp[0].copy(), float(zp[1])
        R, v, w = G(X, p)
        rn = N(X, p)
        res = [max(normC(R), abs(rn))]
        n_ = X.shape[0]
        while len(res) <= max_iterations and res[-1] > tol:
            x1, dx = linsolve(X, p, v, w, R), linsolve(X, p, v, w, dGdp2(X, p, v, w))      # BEC, check_precision = false
            dl = (rn - np.dot(tau[0], x1) / n_ * theta) / (tau[1] * (1 - theta) - np.dot(tau[0], dx) / n_ * theta)
            X = X - (x1 - dl * dx)
            p = float(np.clip(p - dl, p_min, p_max))
            R, v, w = G(X, p)
            rn = N(X, p)
            res.append(max(normC(R), abs(rn)))
        return (X, p), res[-1] < tol, len(res) - 1

    def update(X, p):
        _, v, w = G(X, p)
        zs, z = w / np.linalg.norm(w), v / np.linalg.norm(v)
        st["a"], st["b"] = zs, z
        return float(np.dot(zs, z))

    out = dict(p1=[], p2=[], BT=[], CP=[], ds=[], itnewton=[], X=[])

    def record(z, bt, cp, ds_, itn):
        out["p1"].append(float(z[0][-1])); out["p2"].append(float(z[1])); out["BT"].append(bt); out["CP"].append(float(cp))
        out["ds"].append(ds_); out["itnewton"].append(itn); out["X"].append(z[0].copy())

    ds_ = ds if ds_sequence is None else ds_sequence[0]
    X0, c0, it0 = newton(np.append(np.asarray(x0, dtype=float), p1), p2)
    assert c0, "Newton failed on the initial fold guess"
    X1, c1, _ = newton(X0, p2 + ds_ / eta)
    assert c1, "Newton failed for the initial tangent"
    z, z1 = (X0, p2), (X1, p2 + ds_ / eta)
    tau = palc.secant_tangent(z1, z, ds_, theta)
    record(z, update(*z), tau[1], ds_, it0)
    zp = palc.add_tangent(z, tau, ds_)
    step = 0
    while step < max_steps and (p_min < z[1] < p_max or step == 0):
        sol, conv, itn = newton_palc(z, tau, zp, ds_)
        if conv:
            z_old, z = z, sol
            step += 1
        if ds_sequence is not None:
            assert conv, f"fold continuation step {step} did not converge with the prescribed ds"
            stop = step >= len(ds_sequence)
            ds_next = ds_ if stop else ds_sequence[step]
        else:
            ds_next, stop = palc.step_size_control(ds_, conv, itn, a=a_ctrl, Nmax=max_iterations, dsmin=dsmin, dsmax=dsmax)
        if conv:
            tau = palc.secant_tangent(z, z_old, ds_next, theta)
            record(z, update(*z), tau[1], ds_, itn)
        ds_ = ds_next
        if stop:
            break
        zp = palc.add_tangent(z, tau, ds_)
    return out


# ---------------------------------------------------------------------------------------------- Swift-Hohenberg pieces
def sh_polys(kind, nu, ipar):
    """Coefficients (c0, c1, c2, c3) of h(u) (d2F = h(u) dx1 dx2) and g(u) (dJ/dp = diag(g(u)), p = params[ipar]):
    "sh"   F = -L1 u + l u + nu u^2 - u^3        h = 2 nu - 6 u           g_l = 1, g_nu = 2 u      (examples/SH2d-fronts.jl:40)
    "sh1d" F = L1 u + lam u + nu u^3 - u^5       h = 6 nu u - 20 u^3      g_lam = 1, g_nu = 3 u^2  (examples/SHpde_snaking.jl:26)"""
    if kind == "sh":
        return np.array([2.0 * nu, -6.0, 0.0, 0.0]), (np.array([1.0, 0, 0, 0]) if ipar == 0 else np.array([0, 2.0, 0, 0]))
    return np.array([0.0, 6.0 * nu, 0.0, -20.0]), (np.array([1.0, 0, 0, 0]) if ipar == 0 else np.array([0, 0, 3.0, 0]))


def horner(c, u):
    """c0 + u (c1 + u (c2 + u c3)), the evaluation order of the device kernels."""
    return c[0] + u * (c[1] + u * (c[2] + u * c[3]))


def sh_model(op, kind, pars, lens1, lens2=None):
    """FoldModel of an oracle SwiftHohenberg / SwiftHohenberg1D operator with analytic derivatives; pars = {name: value} in
    the order (l | lam, nu)."""
    names = list(pars)

    def args(q):
        return [q[k] for k in names]

    def d2F(x, q, dx1, dx2):
        h, _ = sh_polys(kind, q[names[1]], 0)
        return horner(h, x) * dx1 * dx2

    def dFdp(x, q, lens):
        i = names.index(lens)
        return x if i == 0 else (x * x if kind == "sh" else x ** 3)

    def dJvdp(x, q, lens, v):
        _, g = sh_polys(kind, q[names[1]], names.index(lens))
        return horner(g, x) * v

    return FoldModel(lambda x, q: op.F(x, *args(q)), lambda x, q: op.J(x, *args(q)), d2F, pars, lens1, lens2,
                     Jt=lambda x, q: op.J(x, *args(q)), dFdp=dFdp, dJvdp=dJvdp)
