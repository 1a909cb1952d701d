"""CPU restatement of the minimally augmented Hopf formulation of src/codim2/MinAugHopf.jl for the tests (test side only).

Generic: a model supplies F, J (dense or scipy.sparse, real), d2F (bilinear, accepting complex arguments), dF/dp and dJ/dp v.
Every linear solve is direct (dense LU / sparse LU, complex where shifted), so the restatement carries no Krylov tolerance.

  bordered_vectors   _compute_bordered_vectors: [J - i om, a; b^H, 0][v; sigma] = [0; 1], [J' + i om, b; a^H, 0][w; s2] = [0; 1]
  hopf_linsolve      _hopf_MA_linear_solver, usehessian branch, written with S(y) = w^H d2F[v, y], sigma_p = -w^H dJ/dp v,
                     sigma_om = i w^H v:  (sigma_p + S(x2)) dp + sigma_om dom = (rp + i rw) + S(x1),  dX = x1 - dp x2
  newton_hopf        newton_hopf under _newton (src/Newton.jl:66-114)
  continuation_hopf  PALC on G(X, p2), X = (x, p1, om), BorderingBLS(check_precision = false) with the Hopf linear solver, Secant
                     tangent, update! of a / b after every converged step, stop at |om| < 100 tol -- the loop of
                     bk_amd.codim2.continuation_hopf
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

from minaug_fold_ref import solve
from oracle import palc


class HopfModel:
    """F(x, q), J(x, q), d2F(x, q, a, b), dFdp(x, q, lens), dJvdp(x, q, lens, v) with ``q`` a dict of parameters."""

    def __init__(self, F, J, d2F, dFdp, dJvdp, pars, lens1, lens2=None):
        self.F, self.J, self.d2F, self.dFdp, self.dJvdp = F, J, d2F, dFdp, dJvdp
        self.pars = dict(pars)
        self.lens1, self.lens2 = lens1, lens2

    def at(self, p1, p2=None):
        q = dict(self.pars)
        q[self.lens1] = p1
        if p2 is not None:
            q[self.lens2] = p2
        return q


def _shift(J, s):
    n = J.shape[0]
    return (J.astype(complex) + s * sp.identity(n, format="csr")) if sp.issparse(J) else np.asarray(J) + s * np.eye(n)


def bordered_solve_c(A, a, b):
    """[A a; b^H 0][v; sigma] = [0; 1] for complex A, a, b (MatrixBLS, direct)."""
    n = a.shape[0]
    a, b = np.asarray(a, dtype=complex), np.asarray(b, dtype=complex)
    if sp.issparse(A):
        M = sp.bmat([[A, sp.csr_matrix(a.reshape(-1, 1))], [sp.csr_matrix(b.conj().reshape(1, -1)), None]], format="csc")
    else:
        M = np.block([[A, a.reshape(-1, 1)], [b.conj().reshape(1, -1), np.zeros((1, 1))]])
    rhs = np.zeros(n + 1, dtype=complex)
    rhs[n] = 1.0
    y = solve(M, rhs)
    return y[:n], y[n]


def bordered_vectors(model, x, q, om, a, b):
    J = model.J(x, q)
    v, sigma = bordered_solve_c(_shift(J, -1j * om), a, b)
    w, _ = bordered_solve_c(_shift(J.T, 1j * om), b, a)
    return v, w, sigma


def sigma_terms(model, x, q, lens, v, w):
    """(sigma_p, sigma_om) = (-w^H dJ/dp v, i w^H v)."""
    return -np.vdot(w, model.dJvdp(x, q, lens, v)), 1j * np.vdot(w, v)


def hopf_linsolve(model, x, q, om, v, w, rhsu, rp, rw):
    J = model.J(x, q)
    x1 = solve(J, rhsu)
    x2 = solve(J, model.dFdp(x, q, model.lens1))
    S1 = np.vdot(w, model.d2F(x, q, v, x1))
    S2 = np.vdot(w, model.d2F(x, q, v, x2))
    sp_, sw = sigma_terms(model, x, q, model.lens1, v, w)
    A = np.array([[(sp_ + S2).real, sw.real], [(sp_ + S2).imag, sw.imag]])
    rhs = np.array([rp + S1.real, rw + S1.imag])
    dp, dw = np.linalg.solve(A, rhs)
    return x1 - dp * x2, dp, dw


def _G(model, X, p2, a, b):
    x, p1, om = X[:-2], X[-2], X[-1]
    v, w, sigma = bordered_vectors(model, x, model.at(p1, p2), om, a, b)
    return np.concatenate([model.F(x, model.at(p1, p2)), [sigma.real, sigma.imag]]), v, w


def newton_hopf(model, x0, p0, om0, a, b, p2=None, tol=1e-12, max_iterations=25, normN=palc.norm2):
    """dict(u, p, omega, residuals, converged, itnewton, v, w)."""
    X = np.concatenate([np.asarray(x0, dtype=float), [p0, om0]])
    G, v, w = _G(model, X, p2, a, b)
    res = [normN(G)]
    step = 0
    while step < max_iterations and res[-1] > tol:
        dX, dp, dw = hopf_linsolve(model, X[:-2], model.at(X[-2], p2), X[-1], v, w, G[:-2], G[-2], G[-1])
        X = X - np.concatenate([dX, [dp, dw]])
        G, v, w = _G(model, X, p2, a, b)
        res.append(normN(G))
        step += 1
    return dict(u=X[:-2], p=X[-2], omega=X[-1], residuals=res, converged=res[-1] < tol, itnewton=step, v=v, w=w)


def start_vectors(model, x, q, om, seed=0):
    """The reference's default: random complex a, b, then a = w/|w|, b = v/|v| of the bordered vectors."""
    rng = np.random.default_rng(seed)
    n = len(x)
    a = rng.random(n) + 1j * rng.random(n)
    b = rng.random(n) + 1j * rng.random(n)
    v, w, _ = bordered_vectors(model, x, q, om, a, b)
    return w / np.linalg.norm(w), v / np.linalg.norm(v)


def continuation_hopf(model, x0, p1, om, p2, a, b, *, ds, dsmin=1e-4, dsmax=0.1, a_ctrl=0.5, theta=0.5, p_min=-np.inf,
                      p_max=np.inf, max_steps=100, eta=150.0, tol=1e-12, max_iterations=25, normC=palc.norminf, ds_sequence=None):
    """PALC on G(X, p2).  Returns dict(p1, p2, omega, ds, itnewton, X, stopped_at_bt), one entry per point (the start first)."""
    st = dict(a=np.asarray(a, dtype=complex).copy(), b=np.asarray(b, dtype=complex).copy())

    def G(X, p):
        return _G(model, X, p, st["a"], st["b"])

    def linsolve(X, p, v, w, R):
        dX, dp, dw = hopf_linsolve(model, X[:-2], model.at(X[-2], p), X[-1], v, w, R[:-2], R[-2], R[-1])
        return np.concatenate([dX, [dp, dw]])

    def dGdp2(X, p, v, w):
        x, q = X[:-2], model.at(X[-2], p)
        s = -np.vdot(w, model.dJvdp(x, q, model.lens2, v))
        return np.concatenate([model.dFdp(x, q, model.lens2), [s.real, s.imag]])

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
        st["a"], st["b"] = w / np.linalg.norm(w), v / np.linalg.norm(v)
        return float(X[-1])

    out = dict(p1=[], p2=[], omega=[], ds=[], itnewton=[], X=[], stopped_at_bt=False)

    def record(z, ds_, itn):
        out["p1"].append(float(z[0][-2])); out["p2"].append(float(z[1])); out["omega"].append(float(z[0][-1]))
        out["ds"].append(ds_); out["itnewton"].append(itn); out["X"].append(z[0].copy())

    ds_ = ds if ds_sequence is None else ds_sequence[0]
    X0, c0, it0 = newton(np.concatenate([np.asarray(x0, dtype=float), [p1, om]]), p2)
    assert c0, "Newton failed on the initial Hopf guess"
    X1, c1, _ = newton(X0, p2 + ds_ / eta)
    assert c1, "Newton failed for the initial tangent"
    z, z1 = (X0, p2), (X1, p2 + ds_ / eta)
    tau = palc.secant_tangent(z1, z, ds_, theta)
    update(*z)
    record(z, ds_, it0)
    zp = palc.add_tangent(z, tau, ds_)
    step = 0
    while step < max_steps and (p_min < z[1] < p_max or step == 0):
        sol, conv, itn = newton_palc(z, tau, zp, ds_)
        if conv:
            z_old, z = z, sol
            step += 1
        if ds_sequence is not None:
            assert conv, f"Hopf continuation step {step} did not converge with the prescribed ds"
            stop = step >= len(ds_sequence)
            ds_next = ds_ if stop else ds_sequence[step]
        else:
            ds_next, stop = palc.step_size_control(ds_, conv, itn, a=a_ctrl, Nmax=max_iterations, dsmin=dsmin, dsmax=dsmax)
        if conv:
            tau = palc.secant_tangent(z, z_old, ds_next, theta)
            om_ = update(*z)
            record(z, ds_, itn)
            if abs(om_) < 100 * tol:
                out["stopped_at_bt"] = True
                break
        ds_ = ds_next
        if stop:
            break
        zp = palc.add_tangent(z, tau, ds_)
    return out


# ---------------------------------------------------------------------------------------------- cGL pieces
CGL_PARAMS = ("r", "mu", "nu", "c3", "c5", "gamma")


def cgl_hessians(u1, u2, mu, c3, c5):
    """(H1, H2) entries per point: H1 = [[h0, h1], [h1, h2]], H2 = [[h3, h4], [h4, h5]] (the order of hopf.hip:cgl_hess)."""
    ua = u1 * u1 + u2 * u2
    q1, q2 = u1 * (8.0 * u1 * u1 + 12.0 * ua), u2 * (8.0 * u1 * u1 + 4.0 * ua)
    q3, q4 = u1 * (8.0 * u2 * u2 + 4.0 * ua), u2 * (8.0 * u2 * u2 + 12.0 * ua)
    return (-6.0 * c3 * u1 + 2.0 * mu * u2 - c5 * q1, -2.0 * c3 * u2 + 2.0 * mu * u1 - c5 * q2,
            -2.0 * c3 * u1 + 6.0 * mu * u2 - c5 * q3, -2.0 * c3 * u2 - 6.0 * mu * u1 - c5 * q2,
            -2.0 * c3 * u1 - 2.0 * mu * u2 - c5 * q3, -6.0 * c3 * u2 - 2.0 * mu * u1 - c5 * q4)


def cgl_djdp(ipar, u1, u2):
    """dJ/dp per point as (d0, d1, d2, d3) = [[d0, d1], [d2, d3]] for params[ipar] = (r, mu, nu, c3, c5, gamma)."""
    ua = u1 * u1 + u2 * u2
    o, z = np.ones_like(u1), np.zeros_like(u1)
    if ipar == 0:
        return o, z, z, o
    if ipar == 1:
        return 2 * u1 * u2, 2 * u2 * u2 + ua, -(2 * u1 * u1 + ua), -2 * u1 * u2
    if ipar == 2:
        return z, -o, o, z
    if ipar == 3:
        return -(2 * u1 * u1 + ua), -2 * u1 * u2, -2 * u1 * u2, -(2 * u2 * u2 + ua)
    if ipar == 4:
        return -(4 * ua * u1 * u1 + ua * ua), -4 * ua * u1 * u2, -4 * ua * u1 * u2, -(4 * ua * u2 * u2 + ua * ua)
    return z, z, z, z


def cgl_d2F(u, q, a, b):
    n = len(u) // 2
    h = cgl_hessians(u[:n], u[n:], q["mu"], q["c3"], q["c5"])
    a1, a2, b1, b2 = a[:n], a[n:], b[:n], b[n:]
    return np.concatenate([a1 * (h[0] * b1 + h[1] * b2) + a2 * (h[1] * b1 + h[2] * b2),
                           a1 * (h[3] * b1 + h[4] * b2) + a2 * (h[4] * b1 + h[5] * b2)])


def cgl_dJvdp(u, q, lens, v):
    n = len(u) // 2
    d = cgl_djdp(CGL_PARAMS.index(lens), u[:n], u[n:])
    return np.concatenate([d[0] * v[:n] + d[1] * v[n:], d[2] * v[:n] + d[3] * v[n:]])


def cgl_dFdp(u, q, lens):
    n = len(u) // 2
    u1, u2 = u[:n], u[n:]
    ua = u1 * u1 + u2 * u2
    i = CGL_PARAMS.index(lens)
    o = [(u1, u2), (ua * u2, -ua * u1), (-u2, u1), (-ua * u1, -ua * u2), (-ua * ua * u1, -ua * ua * u2),
         (np.ones(n), np.zeros(n))][i]
    return np.concatenate(o)


def cgl_model(op, pars, lens1, lens2=None):
    """HopfModel of an oracle CGL2d operator with the analytic derivatives the device kernels evaluate."""
    return HopfModel(lambda x, q: op.F(x, **q), lambda x, q: op.J(x, **q), cgl_d2F, cgl_dFdp, cgl_dJvdp, pars, lens1, lens2)
