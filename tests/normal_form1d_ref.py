"""CPU restatement of the normal form at a simple branch point or fold, get_normal_form1d (src/NormalForms.jl:189-353), of its
predictors (:389-531) and of the two-point start of branch switching (src/bifdiagram/BranchSwitching.jl:8-44) for the tests
(test side only).

Generic over minaug_fold_ref.FoldModel plus a trilinear ``d3F(x, q, a, b, c)`` and, optionally, ``d2Fdp2(x, q, lens)`` (default
0).  The bordered system [J zeta*; zeta' 0][Psi; s] = [E(R); 0] is solved directly as the (n + 1) matrix (MatrixBLS, the
reference's default), so the restatement carries no Krylov tolerance; ``solver="bordering"`` solves it by BorderingBLS with
SciPy GMRES at ``reltol`` instead -- the yardstick of the solver-dependent tolerances of the GPU tests.  With
E(r) = r - <r, zeta*> zeta:

    a01 = <dpF, zeta*>                                      Psi01: E(-dpF)
    b11 = <dJ/dp zeta + d2F[zeta, Psi01], zeta*>
    a02 = <d2F/dp2 + 2 dJ/dp Psi01 + d2F[Psi01, Psi01], zeta*>
    b20 = <d2F[zeta, zeta], zeta*>                          Psi20: E(-d2F[zeta, zeta])
    b30 = <d3F[zeta, zeta, zeta] + 3 d2F[zeta, Psi20], zeta*>
"""
from __future__ import annotations

import math

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from minaug_fold_ref import horner, sh_polys, solve
from oracle import palc

TOL_FOLD = 1e-3


def classify(a01, a02, b11, b20, b30, tol_fold=TOL_FOLD):
    """:339-350"""
    if max(abs(a01), abs(b11)) > 1e-10:
        if abs(a01) < tol_fold:
            return "Pitchfork" if 100 * abs(b20 / 2) < abs(b30 / 6) else "Transcritical"
        return "Fold"
    return "NonQuadraticParameter" if abs(a02) < tol_fold else "BranchPoint"


def bordered_direct(J, zs, z, R):
    """Psi of [J zs; z' 0][Psi; s] = [R; 0], the (n + 1) matrix solved directly: regular at the singular point itself."""
    n = z.shape[0]
    if sp.issparse(J):
        M = sp.bmat([[J, sp.csr_matrix(zs.reshape(-1, 1))], [sp.csr_matrix(z.reshape(1, -1)), None]], format="csc")
    else:
        M = np.block([[np.asarray(J), zs.reshape(-1, 1)], [z.reshape(1, -1), np.zeros((1, 1))]])
    return solve(M, np.append(R, 0.0))[:n]


def bordered_bordering(J, zs, z, Rs, reltol, Pl=None, restart=40, maxiter=5):
    """BorderingBLS (src/LinearBorderSolver.jl:125-144, one BEC pass) for several right-hand sides with one shared J \\ zs, every
    solve by SciPy GMRES at ``reltol`` (left-preconditioned by ``Pl(v)`` when given; ``maxiter`` cycles of ``restart`` steps,
    converged or not): Psi_k = x1_k - (<z, x1_k> / <z, x2>) x2."""
    n = z.shape[0]
    A = J if Pl is None else spla.LinearOperator((n, n), matvec=lambda v: Pl(J @ v))

    def gm(b):
        x, info = spla.gmres(A, b if Pl is None else Pl(b), rtol=reltol, atol=0.0, restart=restart, maxiter=maxiter)
        return x
    x2 = gm(zs)
    out = []
    for R in Rs:
        x1 = gm(R)
        out.append(x1 - (np.dot(z, x1) / np.dot(z, x2)) * x2)
    return out


def normal_form1d(model, d3F, x, q, lens, zeta, zeta_star, d2Fdp2=None, solver="direct", reltol=None, Pl=None, tol_fold=TOL_FOLD,
                  **gmres_kw):
    """dict(a01, a02, b11, b20, b30, Psi01, Psi20, type, rhs = (r1, r2)) at (x, q) for the parameter ``lens``; ``gmres_kw``
    (restart, maxiter) for solver = "bordering"."""
    nrm = float(np.dot(zeta, zeta_star))
    if not abs(nrm - 1) <= 1e-8:
        raise ValueError(f"Error of precision in normalization: <zeta, zeta*> = {nrm}")
    J = model.J(x, q)
    E = lambda r: r - np.dot(r, zeta_star) * zeta
    R01 = np.asarray(model.dFdp(x, q, lens), dtype=float)
    R02 = np.zeros_like(R01) if d2Fdp2 is None else d2Fdp2(x, q, lens)
    b2v = model.d2F(x, q, zeta, zeta)
    a01 = float(np.dot(R01, zeta_star))
    b20 = float(np.dot(b2v, zeta_star))
    r1, r2 = E(-R01), E(-b2v)
    if solver == "direct":
        Psi01, Psi20 = bordered_direct(J, zeta_star, zeta, r1), bordered_direct(J, zeta_star, zeta, r2)
    else:
        Psi01, Psi20 = bordered_bordering(J, zeta_star, zeta, (r1, r2), reltol, Pl, **gmres_kw)
    b11 = float(np.dot(model.dJvdp(x, q, lens, zeta) + model.d2F(x, q, zeta, Psi01), zeta_star))
    a02 = float(np.dot(R02 + 2 * model.dJvdp(x, q, lens, Psi01) + model.d2F(x, q, Psi01, Psi01), zeta_star))
    b30 = float(np.dot(d3F(x, q, zeta, zeta, zeta) + 3 * model.d2F(x, q, zeta, Psi20), zeta_star))
    return dict(a01=a01, a02=a02, b11=b11, b20=b20, b30=b30, Psi01=Psi01, Psi20=Psi20, rhs=(r1, r2),
                type=classify(a01, a02, b11, b20, b30, tol_fold))


# ---------------------------------------------------------------------------------------------- predictors
def circle_zeros(g, r, samples=4096):
    """Zeros of theta -> g(r cos theta, r sin theta): sign changes over ``samples`` equidistant angles, each bracket bisected."""
    f = lambda t: g(r * math.cos(t), r * math.sin(t))
    th = np.linspace(0.0, 2 * math.pi, samples + 1)
    out = []
    for a, b in zip(th[:-1], th[1:]):
        fa, fb = f(a), f(b)
        if fa * fb < 0:
            for _ in range(80):
                m = 0.5 * (a + b)
                if fa * f(m) <= 0:
                    b = m
                else:
                    a, fa = m, f(m)
            out.append((r * math.cos(a), r * math.sin(a), a))
    return out


def predictor(nf, x0, p0, zeta, tau, ds, ampfactor=1.0):
    """predictor(bp, ds; ampfactor) (:389-531) on NumPy vectors; ``nf`` the dict of normal_form1d, tau = (tau_u, tau_p)."""
    kind = nf["type"]
    if kind == "Fold":
        return None
    if kind == "Transcritical":
        amp = -2 * ds * nf["b11"] / nf["b20"] * ampfactor
        tu, tp = tau
        if np.linalg.norm(tu) > 0 and abs(np.dot(zeta, tu)) >= 0.9 * np.linalg.norm(tu):
            x1, xm1, x0n = x0 + ds * nf["Psi01"], x0.copy(), x0 + ds / tp * tu
        else:
            x0n, x1, xm1 = x0, x0 + amp * zeta - ds * nf["Psi01"], x0 - amp * zeta + ds * nf["Psi01"]
        return dict(x0=x0n, x1=x1, xm1=xm1, p=p0 + ds, pm1=p0 - ds, dsfactor=1.0, amp=amp if amp != 0 else abs(ds), p0=p0)
    if kind == "Pitchfork":
        dsfactor = 1.0 if nf["b11"] * nf["b30"] < 0 else -1.0
        amp = ampfactor * math.sqrt(-6 * abs(ds) * dsfactor * nf["b11"] / nf["b30"])
        pnew = p0 + abs(ds) * dsfactor
        return dict(x0=x0, x1=x0 + amp * zeta, p=pnew, dsfactor=dsfactor, amp=amp, dp=pnew - p0)
    g = lambda x, p: (nf["a01"] + nf["a02"] * p / 2) * p + (nf["b11"] * p + nf["b20"] * x / 2 + nf["b30"] * x * x / 6) * x
    sols = circle_zeros(g, abs(ds))
    assert len(sols) == 4, sols
    tu, tp = tau
    k = int(np.argmin([abs(np.dot(tu, zeta) * s[0] + s[1] * tp) for s in sols]))
    return dict(x0=x0, x1=x0 + sols[k][0] * zeta, p=p0 + sols[k][1], dsfactor=1.0, amp=1.0, dp=sols[k][1], solutions=sols)


# ---------------------------------------------------------------------------------------------- the switched branch
def continuation_two_points(prob, x0, p0, x1, p1, *, ls, bls, ds, dsmin=1e-4, dsmax=1e-1, theta=0.5, a=0.5, p_min=-1.0, p_max=1.0,
                            max_steps=10, tol=1e-12, max_iterations=25, normC=palc.norm2):
    """continuation(prob, x0, par0, x1, p1, ...) (src/bifdiagram/BranchSwitching.jl:8-44, iterate_from_two_points): the PALC
    loop of oracle.palc.continuation started from two given points instead of two Newton solves, ds signed by p1 - p0.  The
    first point is recorded as it is given."""
    ds = abs(ds) * float(np.sign(p1 - p0))
    z, z1 = (np.asarray(x0, dtype=float).copy(), float(p0)), (np.asarray(x1, dtype=float), float(p1))
    tau = palc.secant_tangent(z1, z, ds, theta)
    br = palc.Branch()
    br.param.append(z[1]); br.itnewton.append(0); br.ds.append(ds); br.sol.append(z[0].copy()); br.residuals.append([])
    z_pred = palc.add_tangent(z, tau, ds)
    step = 0
    while step < max_steps and (p_min < z[1] < p_max or step == 0):
        if z_pred[1] <= p_min or z_pred[1] >= p_max:
            z_pred = (z_pred[0], float(np.clip(z_pred[1], p_min, p_max)))
            sol = palc.natural_corrector(prob, z_pred, ls, p_min=p_min, p_max=p_max, tol=tol, max_iterations=max_iterations,
                                         normN=normC)
        else:
            sol = palc.newton_palc(prob, z, tau, z_pred, ds, theta, bls, tol=tol, max_iterations=max_iterations, p_min=p_min,
                                   p_max=p_max, normN=normC)
        conv = sol["converged"]
        if conv:
            z_old, z = (z[0].copy(), z[1]), (sol["u"], sol["p"])
            step += 1
            br.param.append(z[1]); br.itnewton.append(sol["itnewton"]); br.ds.append(ds); br.sol.append(z[0].copy())
            br.residuals.append(sol["residuals"])
        ds, stop = palc.step_size_control(ds, conv, sol["itnewton"], a=a, Nmax=max_iterations, dsmin=dsmin, dsmax=dsmax)
        if stop:
            break
        if conv:
            tau = palc.secant_tangent(z, z_old, ds, theta)
        z_pred = palc.add_tangent(z, tau, ds)
    return br


# ---------------------------------------------------------------------------------------------- Swift-Hohenberg pieces
def sh_d3_poly(kind, nu):
    """Coefficients of t(u) = h'(u), d3F = t(u) dx1 dx2 dx3: "sh" -6, "sh1d" 6 nu - 60 u^2."""
    return np.array([-6.0, 0, 0, 0]) if kind == "sh" else np.array([6.0 * nu, 0.0, -60.0, 0.0])


def sh_dp_poly(kind, ipar):
    """Coefficients of f(u) = dF/dp: l | lam: u; nu: u^2 ("sh"), u^3 ("sh1d")."""
    c = np.zeros(4)
    c[1 if ipar == 0 else (2 if kind == "sh" else 3)] = 1.0
    return c


def sh_d3F(kind, names):
    """d3F(x, q, a, b, c) of a Swift-Hohenberg model whose parameters are ``names`` = (l | lam, nu)."""
    return lambda x, q, a, b, c: horner(sh_d3_poly(kind, q[names[1]]), x) * a * b * c


def sh_trivial_mode(dims, ls, jk):
    """(l*, zeta, mu) of the symmetry-breaking point of u = 0 of 2-D SH for the discrete cosine mode jk = (j, k) of the
    Neumann-ghost grid dims = (Nx, Ny) on the box (2 lx) x (2 ly) (oracle.operators.SwiftHohenberg: h = 2 l / N): the eigenvalues
    of the 1-D Laplacians are mu = -(2 / h)^2 sin^2(pi m / (2 N)), J = -L1 + l = l - (1 + mu_j + mu_k)^2 on that mode (x fastest)."""
    mu = [-(2 * n / (2 * L)) ** 2 * np.sin(np.pi * np.arange(2 * n) / (2 * n)) ** 2 for n, L in zip(dims, ls)]
    j, k = jk
    cx = np.cos(np.pi * j * (np.arange(dims[0]) + 0.5) / dims[0])
    cy = np.cos(np.pi * k * (np.arange(dims[1]) + 0.5) / dims[1])
    z = np.outer(cy, cx).reshape(-1)
    return float((1 + mu[0][j] + mu[1][k]) ** 2), z / np.linalg.norm(z), mu


def sh_trivial_closed_form(dims, ls, jk, nu):
    """The normal form at that point in closed form (j, k >= 1, 2j < Nx, 2k < Ny): a01 = a02 = b20 = 0, b11 = 1 and, because
    zeta^2 = c^2 (1 + cos 2j)(1 + cos 2k) / 4 is a sum of the four cosine modes (0,0), (2j,0), (0,2k), (2j,2k), each an
    eigenvector of J with eigenvalue lam_ab = l* - (1 + mu_a + mu_b)^2 and orthogonal to zeta,

        Psi20 = -2 nu sum_ab w_ab phi_ab / lam_ab,     b30 = -6 sum zeta^4 - 12 nu^2 sum_ab w_ab^2 |phi_ab|^2 / lam_ab

    with w_ab the coefficient of the unnormalised mode phi_ab in zeta^2 and sum zeta^4 = 9 / (4 Nx Ny)."""
    nx, ny = dims
    j, k = jk
    assert 1 <= j and 1 <= k and 2 * j < nx and 2 * k < ny
    lstar, z, mu = sh_trivial_mode(dims, ls, jk)
    c2 = 4.0 / (nx * ny)                                                   # c^2: |cos_j x cos_k|^2 = Nx Ny / 4
    xs, ys = (np.arange(nx) + 0.5) / nx, (np.arange(ny) + 0.5) / ny
    psi = np.zeros(nx * ny)
    s = 0.0
    for a, b in ((0, 0), (2 * j, 0), (0, 2 * k), (2 * j, 2 * k)):
        phi = np.outer(np.cos(np.pi * b * ys), np.cos(np.pi * a * xs)).reshape(-1)
        w = c2 / 4.0
        lam = lstar - (1 + mu[0][a] + mu[1][b]) ** 2
        psi += -2 * nu * w * phi / lam
        s += w * w * float(np.dot(phi, phi)) / lam
    b30 = -6.0 * 9.0 / (4.0 * nx * ny) - 12.0 * nu * nu * s
    return dict(a01=0.0, a02=0.0, b11=1.0, b20=0.0, b30=b30, Psi20=psi, lstar=lstar, zeta=z)
