"""CPU restatement of the trapezoid periodic-orbit functional of cGL (src/periodicorbit/PeriodicOrbitTrapeze.jl: po_residual!
:249-269, po_jvp! :294-330, updatesection! :665-681) in NumPy / SciPy -- long double where it is the yardstick -- with the
assembled sparse Jacobian, the matrix A0 of the space-time preconditioner by sparse LU and by the modal recurrence, Newton with LU
and with preconditioned SciPy GMRES, and the PALC steps of bk_amd.periodic_orbit.continuation_po_trap.

Orbit: U of shape (M, N), N = 2 n, slice i = [u1; u2]; T the period entry; h = T (1 / M) on each of the K = M - 1 intervals
(src/TimeMesh.jl:21).  prev(0) = K - 1, prev(i) = i - 1.  Not a product path: tests only."""
import math

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

LD = np.longdouble
PNAMES = ("r", "mu", "nu", "c3", "c5", "gamma")
PIVOT = 1e-8


class Model:
    def __init__(self, dims, ls):
        self.nx, self.ny = int(dims[0]), int(dims[1])
        self.n = self.nx * self.ny
        self.N = 2 * self.n
        self.ax = 1.0 / (2.0 * ls[0] / self.nx) ** 2
        self.ay = 1.0 / (2.0 * ls[1] / self.ny) ** 2
        d1 = lambda m: sp.diags([np.ones(m - 1), -2.0 * np.ones(m), np.ones(m - 1)], [-1, 0, 1])
        self.lap = (self.ax * sp.kron(sp.identity(self.ny), d1(self.nx)) + self.ay * sp.kron(d1(self.ny), sp.identity(self.nx))).tocsr()
        self.Delta = sp.block_diag([self.lap, self.lap], format="csr")
        kx, ky = np.arange(1, self.nx + 1), np.arange(1, self.ny + 1)
        self.lx = -4.0 * self.ax * np.sin(np.pi * kx / (2.0 * (self.nx + 1))) ** 2
        self.ly = -4.0 * self.ay * np.sin(np.pi * ky / (2.0 * (self.ny + 1))) ** 2
        self.Sx = math.sqrt(2.0 / (self.nx + 1)) * np.sin(np.pi * np.outer(kx, kx) / (self.nx + 1))
        self.Sy = math.sqrt(2.0 / (self.ny + 1)) * np.sin(np.pi * np.outer(ky, ky) / (self.ny + 1))
        self.lam = (self.ly[:, None] + self.lx[None, :]).reshape(-1)        # x fastest

    # ---- the vector field, any float dtype (the Laplacian by shifts, Dirichlet)
    def _lap(self, f, mod=False):
        a = f.reshape(self.ny, self.nx)
        z = np.zeros_like(a)
        w, e, s, nn = z.copy(), z.copy(), z.copy(), z.copy()
        w[:, 1:], e[:, :-1], s[1:, :], nn[:-1, :] = a[:, :-1], a[:, 1:], a[:-1, :], a[1:, :]
        if mod:
            return (self.ax * ((np.abs(w) + np.abs(e)) + 2 * np.abs(a)) + self.ay * ((np.abs(s) + np.abs(nn)) + 2 * np.abs(a))).reshape(-1)
        return (self.ax * ((w + e) - 2 * a) + self.ay * ((s + nn) - 2 * a)).reshape(-1)

    def F(self, u, pars):
        r, mu, nu, c3, c5, g = (pars[k] for k in PNAMES)
        n = self.n
        u1, u2 = u[:n], u[n:]
        ua = u1 * u1 + u2 * u2
        return np.concatenate([self._lap(u1) + (r * u1 - nu * u2 - ua * (c3 * u1 - mu * u2) - c5 * ua * ua * u1 + g),
                               self._lap(u2) + (r * u2 + nu * u1 - ua * (c3 * u2 + mu * u1) - c5 * ua * ua * u2)])

    def F_abs(self, u, pars):
        """The sum of the moduli of the terms of F."""
        r, mu, nu, c3, c5, g = (abs(pars[k]) for k in PNAMES)
        n = self.n
        a1, a2 = np.abs(u[:n]), np.abs(u[n:])
        ua = a1 * a1 + a2 * a2
        return np.concatenate([self._lap(u[:n], True) + (r * a1 + nu * a2 + ua * (c3 * a1 + mu * a2) + c5 * ua * ua * a1 + g),
                               self._lap(u[n:], True) + (r * a2 + nu * a1 + ua * (c3 * a2 + mu * a1) + c5 * ua * ua * a2)])

    def _jac(self, u, pars, mod=False):
        r, mu, nu, c3, c5, _ = ((abs(pars[k]) if mod else pars[k]) for k in PNAMES)
        n = self.n
        u1, u2 = (np.abs(u[:n]), np.abs(u[n:])) if mod else (u[:n], u[n:])
        ua = u1 * u1 + u2 * u2
        s = 1 if mod else -1
        f1u = r + s * 2 * u1 * (c3 * u1 + s * mu * u2) + s * c3 * ua + s * 4 * c5 * ua * u1 * u1 + s * c5 * ua * ua
        f1v = s * nu + s * 2 * u2 * (c3 * u1 + s * mu * u2) + mu * ua + s * 4 * c5 * ua * u1 * u2
        f2u = nu + s * 2 * u1 * (c3 * u2 + mu * u1) + s * mu * ua + s * 4 * c5 * ua * u1 * u2
        f2v = r + s * 2 * u2 * (c3 * u2 + mu * u1) + s * c3 * ua + s * 4 * c5 * ua * u2 * u2 + s * c5 * ua * ua
        return f1u, f1v, f2u, f2v

    def Jv(self, u, pars, du):
        n = self.n
        f1u, f1v, f2u, f2v = self._jac(u, pars)
        return np.concatenate([self._lap(du[:n]) + f1u * du[:n] + f1v * du[n:], self._lap(du[n:]) + f2u * du[:n] + f2v * du[n:]])

    def Jv_abs(self, u, pars, du):
        n = self.n
        f1u, f1v, f2u, f2v = self._jac(u, pars, True)
        d1, d2 = np.abs(du[:n]), np.abs(du[n:])
        return np.concatenate([self._lap(du[:n], True) + f1u * d1 + f1v * d2, self._lap(du[n:], True) + f2u * d1 + f2v * d2])

    def J(self, u, pars):
        n = self.n
        f1u, f1v, f2u, f2v = self._jac(u, pars)
        return (self.Delta + sp.diags([np.concatenate([f1u, f2v]), f1v, f2u], [0, n, -n])).tocsr()

    def dFdp(self, u, pars, name):
        n = self.n
        u1, u2 = u[:n], u[n:]
        ua = u1 * u1 + u2 * u2
        z = np.zeros_like(u1)
        return {"r": np.concatenate([u1, u2]), "mu": np.concatenate([ua * u2, -ua * u1]), "nu": np.concatenate([-u2, u1]),
                "c3": np.concatenate([-ua * u1, -ua * u2]), "c5": np.concatenate([-ua * ua * u1, -ua * ua * u2]),
                "gamma": np.concatenate([z + 1, z])}[name]


def _prev(i, K):
    return K - 1 if i == 0 else i - 1


def _hh(T, M, dtype):
    return dtype(T) * (dtype(1) / dtype(M)) / dtype(2)


# ------------------------------------------------------------------------------------------ functional and JVP
def residual(m, U, T, pars, phi, xpi, mod=False):
    """(G[0 .. M), tail); mod: the sum of the moduli of the terms of every entry instead (the unit of the rounding bounds)."""
    M, K = U.shape[0], U.shape[0] - 1
    dt = U.dtype.type
    hh = abs(_hh(T, M, dt)) if mod else _hh(T, M, dt)
    Fs = [(m.F_abs if mod else m.F)(U[i], pars) for i in range(K)]
    out = np.empty_like(U)
    for i in range(K):
        j = _prev(i, K)
        out[i] = (np.abs(U[i]) + np.abs(U[j])) + hh * (Fs[i] + Fs[j]) if mod else (U[i] - U[j]) - hh * (Fs[i] + Fs[j])
    out[K] = np.abs(U[K]) + np.abs(U[0]) if mod else U[K] - U[0]
    tail = np.sum(np.abs(U * phi)) + np.sum(np.abs(xpi * phi)) if mod else np.sum(U * phi) - np.sum(xpi * phi)
    return out, tail


def jvp(m, U, T, pars, dU, dT, phi, mod=False):
    M, K = U.shape[0], U.shape[0] - 1
    dt = U.dtype.type
    hh, dh = _hh(T, M, dt), dt(dT) / dt(M) / dt(2)
    if mod:
        hh, dh = abs(hh), abs(dh)
    Fs = [(m.F_abs if mod else m.F)(U[i], pars) for i in range(K)]
    Js = [(m.Jv_abs if mod else m.Jv)(U[i], pars, dU[i]) for i in range(K)]
    out = np.empty_like(U)
    for i in range(K):
        j = _prev(i, K)
        if mod:
            out[i] = (np.abs(dU[i]) + np.abs(dU[j])) + hh * (Js[i] + Js[j]) + dh * (Fs[i] + Fs[j])
        else:
            out[i] = ((dU[i] - dU[j]) - hh * (Js[i] + Js[j])) - dh * (Fs[i] + Fs[j])
    out[K] = np.abs(dU[K]) + np.abs(dU[0]) if mod else dU[K] - dU[0]
    return out, (np.sum(np.abs(dU * phi)) if mod else np.sum(dU * phi))


def dparam(m, U, T, pars, name):
    M, K = U.shape[0], U.shape[0] - 1
    hh = _hh(T, M, U.dtype.type)
    D = [m.dFdp(U[i], pars, name) for i in range(K)]
    out = np.zeros_like(U)
    for i in range(K):
        out[i] = -hh * (D[i] + D[_prev(i, K)])
    return out


def update_section(m, U, pars):
    """updatesection!: (phi, xpi) = (F(u_i) / M per slice, U)."""
    M = U.shape[0]
    return np.stack([m.F(U[i], pars) / M for i in range(M)]), U.copy()


def section_from_guess(m, U, pars):
    """cGL2d.jl:177-181: phi = normalize(F(slice 1)) in the first slice, xpi = 0."""
    f = m.F(U[0], pars)
    phi = np.zeros_like(U)
    phi[0] = f / np.linalg.norm(f)
    return phi, np.zeros_like(U)


# ------------------------------------------------------------------------------------------ assembled matrices
def _cyclic(m, M, T, blocks, with_tail=None):
    """The (M N [+ 1]) matrix with the N x N blocks L_i in the place of J_i; with_tail = (Tcol (M, N), phi (M, N)) adds the border."""
    N, K, hh = m.N, M - 1, _hh(T, M, float)
    I = sp.identity(N, format="csr")
    rows = [[None] * (M + (1 if with_tail else 0)) for _ in range(M + (1 if with_tail else 0))]
    for i in range(K):
        j = _prev(i, K)
        rows[i][i] = I - hh * blocks[i]
        rows[i][j] = -I - hh * blocks[j]
    rows[K][K], rows[K][0] = I, -I
    if with_tail:
        tcol, phi = with_tail
        for i in range(M):
            rows[i][M] = sp.csr_matrix(tcol[i].reshape(-1, 1))
            rows[M][i] = sp.csr_matrix(phi[i].reshape(1, -1))
        rows[M][M] = sp.csr_matrix((1, 1))
    return sp.bmat(rows, format="csc")


def jacobian_sparse(m, U, T, pars, phi):
    M, K = U.shape[0], U.shape[0] - 1
    Fs = [m.F(U[i], pars) for i in range(K)]
    tcol = np.zeros_like(U)
    for i in range(K):
        tcol[i] = -(1.0 / M / 2.0) * (Fs[i] + Fs[_prev(i, K)])
    return _cyclic(m, M, T, [m.J(U[i], pars) for i in range(K)], (tcol, phi))


def L0(m, a, b):
    n = m.n
    return (m.Delta + sp.diags([np.full(2 * n, a), np.full(n, -b), np.full(n, b)], [0, n, -n])).tocsr()


def A0_sparse(m, M, T, a, b):
    return _cyclic(m, M, T, [L0(m, a, b)] * (M - 1))


# ------------------------------------------------------------------------------------------ the modal solve
def modal_guards(m, M, T, a, b):
    """(min |alpha|, min |1 - rho^K|) over the sine modes, rho^K by repeated multiplication."""
    hh, K = _hh(T, M, float), M - 1
    mu = a + m.lam + 1j * b
    alpha, beta = 1 - hh * mu, 1 + hh * mu
    rho = beta / alpha
    rk = np.ones_like(rho)
    for _ in range(K):
        rk = rk * rho
    return float(np.abs(alpha).min()), float(np.abs(1 - rk).min())


def modal_solve(m, M, T, a, b, f):
    """A0^-1 f for f of shape (M, N): DST-I of every field, the recurrence of the time solve per mode, DST-I back."""
    n, K, hh = m.n, M - 1, _hh(T, M, float)
    dst = lambda x: (m.Sy @ x.reshape(m.ny, m.nx) @ m.Sx).reshape(-1)
    fh = np.array([dst(f[i, :n]) + 1j * dst(f[i, n:]) for i in range(M)])
    mu = a + m.lam + 1j * b
    alpha, beta = 1 - hh * mu, 1 + hh * mu
    rho = beta / alpha
    acc, rk = np.zeros(n, complex), np.ones(n, complex)
    for i in range(K):
        acc = rho * acc + fh[i] / alpha
        rk = rk * rho
    w = acc / (1 - rk)
    wh = np.empty_like(fh)
    for i in range(K):
        w = rho * w + fh[i] / alpha
        wh[i] = w
    wh[K] = fh[K] + wh[0]
    out = np.empty_like(f)
    for i in range(M):
        out[i, :n], out[i, n:] = dst(wh[i].real), dst(wh[i].imag)
    return out


# ------------------------------------------------------------------------------------------ solves, Newton, PALC
def pack(U, T):
    return np.concatenate([U.reshape(-1), [T]])


def unpack(m, x):
    return x[:-1].reshape(-1, m.N), float(x[-1])


def lu_solver(m, pars_of):
    """solve(U, T, p, rhs) by sparse LU of the assembled Jacobian -> (x, iterations = 0)."""
    def solve(U, T, p, phi, rhs):
        return spla.splu(jacobian_sparse(m, U, T, pars_of(p), phi)).solve(rhs), 0
    return solve


def gmres_solve(m, U, T, pars, phi, rhs, a, b, Tp, rtol, restart=60, maxiter=200, atol=0.0):
    """Left-preconditioned GMRES on diag(A0^-1, 1) dG x = diag(A0^-1, 1) rhs, x0 = 0, matrix-free; stops at
    |r| <= max(rtol |r0|, atol) in the 2-norm of the preconditioned residual (the IterativeSolvers rule).  Returns (x, iterations)."""
    M = U.shape[0]

    def P(v):
        return np.concatenate([modal_solve(m, M, Tp, a, b, v[:-1].reshape(M, -1)).reshape(-1), v[-1:]])

    def B(v):
        o, t = jvp(m, U, T, pars, v[:-1].reshape(M, -1), v[-1], phi)
        return P(np.concatenate([o.reshape(-1), [t]]))

    its = [0]

    def cb(_):
        its[0] += 1

    n = rhs.size
    x, info = spla.gmres(spla.LinearOperator((n, n), matvec=B, dtype=float), P(rhs), rtol=rtol, atol=atol, restart=restart,
                         maxiter=maxiter, callback=cb, callback_type="pr_norm")
    assert info == 0, info
    return x, its[0]


def gmres_solver(m, pars_of, a, b, Tp, rtol, **kw):
    def solve(U, T, p, phi, rhs):
        return gmres_solve(m, U, T, pars_of(p), phi, rhs, a, b, Tp() if callable(Tp) else Tp, rtol, **kw)
    return solve


def _norminf(x):
    return float(np.abs(x).max())


def newton(m, U0, T0, p, pars_of, phi, xpi, solve, tol=1e-10, max_iterations=10):
    """_newton (src/Newton.jl:66-114) on the functional in the sup norm -> dict(U, T, residuals, itlinear, converged)."""
    x = pack(U0, T0)
    G = lambda x: pack(*residual(m, *unpack(m, x), pars_of(p), phi, xpi))
    fx = G(x)
    res, its = [_norminf(fx)], []
    while len(res) - 1 < max_iterations and res[-1] > tol:
        U, T = unpack(m, x)
        dx, it = solve(U, T, p, phi, fx)
        its.append(it)
        x = x - dx
        fx = G(x)
        res.append(_norminf(fx))
    U, T = unpack(m, x)
    return dict(U=U, T=T, residuals=res, itlinear=its, converged=res[-1] < tol)


def _dot_theta(u1, u2, p1, p2, theta):
    return float(u1 @ u2) / u1.size * theta + p1 * p2 * (1.0 - theta)


def _secant(z1, z0, ds, theta):
    du, dp = z1[0] - z0[0], z1[1] - z0[1]
    a = math.copysign(1.0, ds) / math.sqrt(_dot_theta(du, du, dp, dp, theta))
    return du * a, dp * a


def _step_size(ds, converged, itnewton, cp):
    if not converged:
        return math.copysign(max(abs(ds) / 2.0, cp["dsmin"]), ds)
    dsnew = ds * (1.0 + cp["a"] * ((cp["max_iterations"] - itnewton) / cp["max_iterations"]) ** 2)
    return math.copysign(min(max(abs(dsnew), cp["dsmin"]), cp["dsmax"]), dsnew)


def palc(m, U0, T0, pars, lens, phi, xpi, solve, cp, steps, theta=0.5, Tp_box=None):
    """The steps of continuation_po_trap: two Newton solves, the secant tangent, then per step updatesection!, newton_palc with
    BorderingBLS (two solves per Newton step, analytic d_p G) and the step-size control.  cp: dict(ds, dsmin, dsmax, a, eta, tol,
    max_iterations).  Tp_box: a one-element list that receives the period the preconditioner is rebuilt at every step."""
    pars_of = lambda p: dict(pars, **{lens: p})
    p0 = pars[lens]
    if Tp_box is not None:
        Tp_box[0] = T0
    s0 = newton(m, U0, T0, p0, pars_of, phi, xpi, solve, cp["tol"], cp["max_iterations"])
    assert s0["converged"], s0["residuals"]
    p1 = p0 + cp["ds"] / cp["eta"]
    s1 = newton(m, s0["U"], s0["T"], p1, pars_of, phi, xpi, solve, cp["tol"], cp["max_iterations"])
    assert s1["converged"], s1["residuals"]
    z0, z1 = (pack(s0["U"], s0["T"]), p0), (pack(s1["U"], s1["T"]), p1)
    ds = cp["ds"]
    tau = _secant(z1, z0, ds, theta)
    z, z_old = z0, z0
    out = dict(p=[p0], T=[s0["T"]], amplitude=[_norminf(s0["U"])], itnewton=[len(s0["residuals"]) - 1])
    for _ in range(steps):
        zp = (z[0] + ds * tau[0], z[1] + ds * tau[1])
        U, T = unpack(m, z[0])
        phi, xpi = update_section(m, U, pars_of(z[1]))
        if Tp_box is not None:
            Tp_box[0] = T
        G = lambda x, p: pack(*residual(m, *unpack(m, x), pars_of(p), phi, xpi))
        Nf = lambda x, p: (_dot_theta(x, tau[0], p - z[1], tau[1], theta) - ds) - _dot_theta(z[0], tau[0], p - z[1], 0.0, theta)
        x, p = zp
        rf, rn = G(x, p), Nf(x, p)
        res = [max(_norminf(rf), abs(rn))]
        while len(res) - 1 < cp["max_iterations"] and res[-1] > cp["tol"]:
            Ux, Tx = unpack(m, x)
            dR = pack(dparam(m, Ux, Tx, pars_of(p), lens), 0.0)
            x1, _ = solve(Ux, Tx, p, phi, rf)
            x2, _ = solve(Ux, Tx, p, phi, dR)
            xiu, xip, N = theta, 1.0 - theta, x.size
            dl = (rn - xiu * float(tau[0] @ x1) / N) / (tau[1] * xip - xiu * float(tau[0] @ x2) / N)
            x = x - (x1 - dl * x2)
            p = p - dl
            rf, rn = G(x, p), Nf(x, p)
            res.append(max(_norminf(rf), abs(rn)))
        conv = res[-1] < cp["tol"]
        assert conv, res
        z_old, z = z, (x, p)
        Uz, Tz = unpack(m, x)
        out["p"].append(p); out["T"].append(Tz); out["amplitude"].append(_norminf(Uz)); out["itnewton"].append(len(res) - 1)
        ds = _step_size(ds, conv, len(res) - 1, cp)
        tau = _secant(z, z_old, ds, theta)
    out["U"], out["Tlast"] = unpack(m, z[0])
    return out


# ------------------------------------------------------------------------------------------ closed forms
def stuart_landau_orbit(r_eff, pars, M):
    """1 x 1 grid: u_i = R e^{i theta i}, theta = 2 pi / (M - 1), r_eff - c3 R^2 - c5 R^4 = 0, omega = nu + mu R^2 ...  with the
    sign conventions of NL: z' = (r_eff + i nu) z - (c3 + i mu) |z|^2 z - c5 |z|^4 z, so omega = nu - mu R^2, and
    T = (2 M / omega) tan(pi / (M - 1))."""
    c3, c5, mu, nu = pars["c3"], pars["c5"], pars["mu"], pars["nu"]
    R2 = (-c3 + math.sqrt(c3 * c3 + 4 * c5 * r_eff)) / (2 * c5)
    om = nu - mu * R2
    th = 2 * math.pi / (M - 1)
    z = math.sqrt(R2) * np.exp(1j * th * np.arange(M))
    return np.stack([z.real, z.imag], axis=1), (2 * M / om) * math.tan(math.pi / (M - 1)), om
