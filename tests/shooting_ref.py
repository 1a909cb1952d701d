"""CPU restatement of the standard-shooting periodic orbits of cGL on a spectral ETDRK2 flow (examples/cGL2d-shooting.jl;
src/periodicorbit/StandardShooting.jl :138-257, Sections.jl :6-58, Floquet.jl :89-108) in NumPy -- long double where it is the
yardstick: the DST-I as a dense symmetric matrix, the three coefficient tables, one ETDRK2 step and its tangent, the functional,
its JVP, the section, the dense monodromy matrix, and Newton with a dense Jacobian and with SciPy GMRES.

State: X of shape (M, N), N = 2 n, state i = [u1; u2] (x fastest); T the period; the M segments are T / M long and take nsteps
steps each.  Every routine accepts leading batch axes.  Not a product path: tests only."""
import json
import math
import os

import numpy as np
import scipy.sparse.linalg as spla

import potrap_ref as P

LD = np.longdouble
PNAMES = P.PNAMES
LS = (np.pi, np.pi / 2)
PARS = dict(r=1.2, mu=0.1, nu=1.0, c3=-1.0, c5=1.0, gamma=0.0)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shooting_cgl.json")
# the cases of the fixture: the limit cycle at r = 1.2 from a time integration, and the small unstable orbit next to the Hopf point
CYCLE_CASES = [((8, 6), 2, 32), ((12, 9), 3, 48), ((16, 12), 1, 64), ((41, 21), 1, 64)]
HOPF_CASES = [((12, 9), 1, 64, 0.01), ((16, 12), 1, 64, 0.1)]
POLISH_TOL = 1e-11              # the residual the orbits are converged to before their multipliers are taken


def phi_tables(z):
    """(e^z, phi1(z), phi2(z)) in long double: phi1 = expm1(z) / z, phi2 by its series for |z| < 1 and (expm1(z) - z) / z^2 beyond."""
    z = np.asarray(z, dtype=LD)
    em1 = np.expm1(z)
    safe = np.where(z == 0, LD(1), z)
    p1 = np.where(z == 0, LD(1), em1 / safe)
    s = np.zeros_like(z)
    zs = np.where(np.abs(z) < 1, z, LD(0))
    for k in range(27, -1, -1):
        s = s * zs + LD(1) / LD(math.factorial(k + 2))
    p2 = np.where(np.abs(z) < 1, s, (em1 - z) / (safe * safe))
    return np.exp(z), p1, p2


class Flow:
    """The ETDRK2 flow of a potrap_ref.Model in the float type ``dtype``."""

    def __init__(self, m, dtype=LD):
        self.m, self.dt = m, dtype
        pi = LD(4) * np.arctan(LD(1))

        def S(N):
            k = np.arange(1, N + 1).astype(LD)
            return (np.sqrt(LD(2) / LD(N + 1)) * np.sin(pi * np.outer(k, k) / LD(N + 1))).astype(dtype)
        self.Sx, self.Sy = S(m.nx), S(m.ny)
        self.lam = m.ly[:, None] + m.lx[None, :]               # (ny, nx), the doubles the device tables hold

    def tables(self, h):
        """(E, h phi1, h phi2), each (ny, nx), for z = h lam with the product taken in double as the device takes it."""
        z = (float(h) * self.lam).astype(LD)
        E, p1, p2 = phi_tables(z)
        return E.astype(self.dt), (LD(h) * p1).astype(self.dt), (LD(h) * p2).astype(self.dt)

    def tr(self, f):
        return self.Sy @ f @ self.Sx

    def fields(self, x):
        return np.asarray(x, dtype=self.dt).reshape(x.shape[:-1] + (2, self.m.ny, self.m.nx))

    def nl(self, u, pars):
        r, mu, nu, c3, c5, g = (self.dt(pars[k]) for k in PNAMES)
        u1, u2 = u[..., 0, :, :], u[..., 1, :, :]
        ua = u1 * u1 + u2 * u2
        return np.stack([r * u1 - nu * u2 - ua * (c3 * u1 - mu * u2) - c5 * ua * ua * u1 + g,
                         r * u2 + nu * u1 - ua * (c3 * u2 + mu * u1) - c5 * ua * ua * u2], axis=-3)

    def jn(self, u, du, pars):
        r, mu, nu, c3, c5, _ = (self.dt(pars[k]) for k in PNAMES)
        u1, u2 = u[..., 0, :, :], u[..., 1, :, :]
        d1, d2 = du[..., 0, :, :], du[..., 1, :, :]
        ua = u1 * u1 + u2 * u2
        f1u = r - 2 * u1 * (c3 * u1 - mu * u2) - c3 * ua - 4 * c5 * ua * u1 * u1 - c5 * ua * ua
        f1v = -nu - 2 * u2 * (c3 * u1 - mu * u2) + mu * ua - 4 * c5 * ua * u1 * u2
        f2u = nu - 2 * u1 * (c3 * u2 + mu * u1) - mu * ua - 4 * c5 * ua * u1 * u2
        f2v = r - 2 * u2 * (c3 * u2 + mu * u1) - c3 * ua - 4 * c5 * ua * u2 * u2 - c5 * ua * ua
        return np.stack([f1u * d1 + f1v * d2, f2u * d1 + f2v * d2], axis=-3)

    def step(self, u, uh, tab, pars, du=None, duh=None):
        """One step from (u, u^) [and the tangent (du, du^)] -> the same at the next time."""
        E, P1, P2 = tab
        nh = self.tr(self.nl(u, pars))
        ah = E * uh + P1 * nh
        a = self.tr(ah)
        nah = self.tr(self.nl(a, pars))
        uh1 = ah + P2 * (nah - nh)
        if du is None:
            return self.tr(uh1), uh1, None, None
        jh = self.tr(self.jn(u, du, pars))
        bh = E * duh + P1 * jh
        b = self.tr(bh)
        jbh = self.tr(self.jn(a, b, pars))
        duh1 = bh + P2 * (jbh - jh)
        return self.tr(uh1), uh1, self.tr(duh1), duh1

    def march(self, x, tau, nsteps, pars, dx=None):
        """Phi(x, tau) [and dPhi(x, tau) dx] in nsteps steps -> dict(u, du, umax, dumax): the flat results and the largest moduli
        of state and tangent over the steps (the unit of the rounding bounds)."""
        tab = self.tables(float(tau) / nsteps)                 # the step in double, as the device forms it
        u = self.fields(x)
        uh = self.tr(u)
        du = duh = None
        if dx is not None:
            du = self.fields(dx)
            duh = self.tr(du)
        umax, dumax = float(np.abs(u).max()), 0.0 if du is None else float(np.abs(du).max())
        for _ in range(int(nsteps)):
            u, uh, du, duh = self.step(u, uh, tab, pars, du, duh)
            umax = max(umax, float(np.abs(u).max()))
            if du is not None:
                dumax = max(dumax, float(np.abs(du).max()))
        flat = lambda a: a.reshape(a.shape[:-3] + (-1,))
        return dict(u=flat(u), du=None if du is None else flat(du), umax=umax, dumax=dumax)

    def F(self, x, pars):
        """The cGL vector field of every state of x (..., N)."""
        x = np.asarray(x, dtype=self.dt)
        return np.stack([self.m.F(v, pars) for v in x.reshape(-1, x.shape[-1])]).reshape(x.shape)


def seg_tau(dt, M, T):
    return (dt(1) / dt(M)) * dt(T)                       # sh.ds[i] * T


def residual(fl, X, T, pars, nsteps, normal, center):
    """(G[0 .. M), G_T) of StandardShooting.jl:138-165 with the section of Sections.jl:13."""
    dt = fl.dt
    X = np.asarray(X, dtype=dt)
    Phi = fl.march(X, seg_tau(dt, X.shape[0], T), nsteps, pars)["u"]
    return Phi - np.roll(X, -1, axis=0), (np.sum(X[0] * normal) - np.sum(center * normal)) * dt(T)


def jvp(fl, X, T, pars, nsteps, dX, dT, normal, center, parts=False):
    """dG(X, T)(dX, dT) (:190-228, Sections.jl:43-45); parts: also dict(Phi, dPhi, FPhi, umax, dumax)."""
    dt = fl.dt
    X, dX = np.asarray(X, dtype=dt), np.asarray(dX, dtype=dt)
    M = X.shape[0]
    r = fl.march(X, seg_tau(dt, M, T), nsteps, pars, dX)
    FPhi = fl.F(r["u"], pars)
    out = (r["du"] + FPhi * ((dt(1) / dt(M)) * dt(dT))) - np.roll(dX, -1, axis=0)
    tail = (np.sum(X[0] * normal) - np.sum(center * normal)) * dt(dT) + np.sum(dX[0] * normal) * dt(T)
    if parts:
        return out, tail, dict(Phi=r["u"], dPhi=r["du"], FPhi=FPhi, umax=r["umax"], dumax=r["dumax"])
    return out, tail


def update_section(fl, X, pars):
    """updatesection! (:116-122) -> (normal, center)."""
    f = fl.F(np.asarray(X, dtype=fl.dt)[0], pars)
    return f / np.sqrt(np.sum(f * f)), np.array(X[0], dtype=fl.dt)


def monodromy_matrix(fl, X, T, pars, nsteps):
    """The N x N matrix of MonodromyQaD_matrix_free(::Shooting) (Floquet.jl:89-108): dPhi(x_{M-1}) .. dPhi(x_0)."""
    X = np.asarray(X, dtype=fl.dt)
    M, N = X.shape
    D = np.eye(N, dtype=fl.dt)                               # row j: the image of e_j
    for i in range(M):
        D = fl.march(X[i][None, :], seg_tau(fl.dt, M, T), nsteps, pars, D)["du"]
    return D.T


def pack(X, T):
    return np.concatenate([np.asarray(X, dtype=float).reshape(-1), [float(T)]])


def jacobian_dense(fl, X, T, pars, nsteps, normal, center):
    M, N = X.shape
    n = M * N + 1
    J = np.empty((n, n))
    I = np.eye(M * N)
    Xb = np.broadcast_to(X, (M * N,) + X.shape)
    # the M N unit directions as one batch: the march broadcasts over the leading axis
    dt = fl.dt
    r = fl.march(Xb, seg_tau(dt, M, T), nsteps, pars, I.reshape(M * N, M, N))
    J[:-1, :-1] = (r["du"] - np.roll(I.reshape(M * N, M, N), -1, axis=1)).reshape(M * N, M * N).T
    Phi = r["u"][0]
    J[:-1, -1] = (fl.F(Phi, pars) * (dt(1) / dt(M))).reshape(-1)
    J[-1, :-1] = 0.0
    J[-1, :N] = np.asarray(normal, dtype=float) * float(T)
    J[-1, -1] = float(np.sum(X[0] * normal) - np.sum(center * normal))
    return J


def gmres_solve(fl, X, T, pars, nsteps, normal, center, rhs, rtol, restart=50, maxiter=50):
    """Unpreconditioned SciPy GMRES on dG x = rhs, x0 = 0, |r| <= rtol |rhs| -> (x, operator applications inside the iteration)."""
    M, N = X.shape
    its = [0]

    def A(v):
        o, t = jvp(fl, X, T, pars, nsteps, v[:-1].reshape(M, N), v[-1], normal, center)
        return pack(o, t)

    def cb(_):
        its[0] += 1
    n = M * N + 1
    x, info = spla.gmres(spla.LinearOperator((n, n), matvec=A, dtype=float), rhs, rtol=rtol, atol=0.0, restart=restart, maxiter=maxiter,
                         callback=cb, callback_type="pr_norm")
    assert info == 0, info
    return x, its[0]


def newton(fl, X0, T0, pars, nsteps, normal, center, rtol=1e-4, tol=1e-9, max_iterations=25, dense=False):
    """_newton (src/Newton.jl:66-114) on the functional in the sup norm, the linear solves by SciPy GMRES (rtol, restart 50) or by
    LU of the dense Jacobian -> dict(X, T, residuals, itlinear, converged, itnewton)."""
    X, T = np.array(X0, dtype=float), float(T0)
    M, N = X.shape
    G = lambda: pack(*residual(fl, X, T, pars, nsteps, normal, center))
    fx = G()
    res, its = [float(np.abs(fx).max())], []
    while len(res) - 1 < max_iterations and res[-1] > tol:
        if dense:
            dx, it = np.linalg.solve(jacobian_dense(fl, X, T, pars, nsteps, normal, center), fx), 0
        else:
            dx, it = gmres_solve(fl, X, T, pars, nsteps, normal, center, fx, rtol)
        X = X - dx[:-1].reshape(M, N)
        T = T - dx[-1]
        fx = G()
        res.append(float(np.abs(fx).max()))
        its.append(it)
    return dict(X=X, T=T, residuals=res, itlinear=its, converged=res[-1] < tol, itnewton=len(res) - 1)


# ------------------------------------------------------------------------------------------ PALC on the engine of continuation.py
class NpVec:
    """A NumPy vector with the VectorInterface methods continuation.py calls."""

    def __init__(self, a):
        self.a = np.array(a, dtype=float).reshape(-1)

    def copy(self):
        return NpVec(self.a)

    def zerovector(self):
        return NpVec(np.zeros_like(self.a))

    def copyto_(self, src):
        self.a[:] = src.a
        return self

    def scale_(self, c):
        self.a *= c
        return self

    def add_(self, x, a=1.0, b=1.0):
        self.a = b * self.a + a * x.a
        return self

    def inner(self, y):
        return float(self.a @ y.a)

    def norm(self):
        return float(np.linalg.norm(self.a))

    def norminf(self):
        return float(np.abs(self.a).max())

    def __len__(self):
        return self.a.size


def palc(fl, X0, T0, pars, lens, nsteps, normal, center, cp, steps, rtol=1e-4, theta=0.5):
    """The steps of bk_amd.shooting.continuation_po_shooting driven by the same engine (bk_amd.continuation: newton, newton_palc,
    secant_tangent, step_size_control) on NumPy vectors: two Newton solves, the secant tangent, then per step updatesection!,
    newton_palc with bordering on two SciPy-GMRES solves and the forward difference d_p G.  cp: a ContinuationPar.  Returns
    dict(p, T, ds, itnewton, itlinear)."""
    from bk_amd import continuation as Cn
    from bk_amd.hip import BorderedArray
    M, N = X0.shape
    sec = [np.array(normal, dtype=float), np.array(center, dtype=float)]
    counts = []

    class Prob:
        delta = math.sqrt(np.finfo(float).eps)

        def pv(self, p):
            return dict(pars, **{lens: float(p)})

        def residual(self, x, p):
            o, t = residual(fl, x.u.a.reshape(M, N), x.p, self.pv(p), nsteps, *sec)
            return BorderedArray(NpVec(o), float(t))

        def jacobian(self, x, p):
            return (x.u.a.reshape(M, N).copy(), float(x.p), self.pv(p))

    def lin(J, rhs, a0=0.0, a1=1.0):
        x, it = gmres_solve(fl, J[0], J[1], J[2], nsteps, sec[0], sec[1], pack(rhs.u.a, rhs.p), rtol)
        counts.append(it)
        return BorderedArray(NpVec(x[:-1]), float(x[-1])), True, it

    def bls(J, dR, dzu, dzp, R, n, xiu=1.0, xip=1.0, *, shift=None, dotp=None, dotscale=None):
        x1, _, i1 = lin(J, R)
        x2, _, i2 = lin(J, dR)
        dl = (n - xiu * dotp(dzu, x1)) / (dzp * xip - xiu * dotp(dzu, x2))
        x1.add_(x2, -dl)
        return x1, dl, True, (i1, i2)

    def ninf(x):
        return max(x.u.norminf(), abs(x.p))

    F = Prob()
    nopt = Cn.NewtonPar(tol=cp.newton_options.tol, max_iterations=cp.newton_options.max_iterations, linsolver=lin)
    p0 = pars[lens]
    s0 = Cn.newton(F, BorderedArray(NpVec(X0), float(T0)), p0, nopt, ninf)
    assert s0.converged, s0.residuals
    p1 = p0 + cp.ds / cp.eta
    s1 = Cn.newton(F, s0.u, p1, nopt, ninf)
    assert s1.converged, s1.residuals
    z0, z1 = BorderedArray(s0.u, p0), BorderedArray(s1.u, p1)
    br = dict(p=[p0], T=[s0.u.p], ds=[cp.ds], itnewton=[s0.itnewton], itlinear=[list(counts)])
    ds = cp.ds
    tau = Cn.secant_tangent(z1, z0, ds, theta)
    z, z_old = z0.copy(), z0.copy()
    z_pred = z.copy().add_(tau, ds)
    step = 0
    while step < steps:
        before = len(counts)
        sec[0], sec[1] = update_section(fl, z.u.u.a.reshape(M, N), F.pv(z.p))
        sol = Cn.newton_palc(F, z, tau, z_pred, ds, theta, bls, nopt, cp.p_min, cp.p_max, ninf)
        if sol.converged:
            z_old.copyto_(z)
            z.copyto_(sol.u)
            step += 1
            br["p"].append(z.p); br["T"].append(z.u.p); br["ds"].append(ds); br["itnewton"].append(sol.itnewton)
            br["itlinear"].append(counts[before:])
        ds, stop = Cn.step_size_control(ds, sol.converged, sol.itnewton, cp)
        if stop:
            break
        if sol.converged:
            tau = Cn.secant_tangent(z, z_old, ds, theta)
        z_pred = z.copy().add_(tau, ds)
    return br


# ------------------------------------------------------------------------------------------ the guesses
def guess_from_flow(fl, x0, t_end, nsteps, T_guess, M, seg_steps, pars):
    """cGL2d-shooting.jl:110-113, :130: the state after t_end, then M states T_guess / M apart -> X (M, N)."""
    sl = [fl.march(np.asarray(x0, dtype=fl.dt), t_end, nsteps, pars)["u"]]
    for _ in range(1, M):
        sl.append(fl.march(sl[-1], seg_tau(fl.dt, M, T_guess), seg_steps, pars)["u"])
    return np.stack(sl)


def cycle_start(m, seed=0):
    """0.1 rand (cGL2d-shooting.jl:95), reproducible."""
    return 0.1 * np.random.default_rng(seed).random(m.N)


def hopf_guess(m, dr, M, amp_factor=1.0):
    """A normal-form-sized guess next to the Hopf point r_H = -lam_11: with the critical mode phi (unit 2-norm of (phi, 0)) and the
    cubic coefficient, |A|^2 = dr / (-c3 kappa), kappa = sum phi^4 / sum phi^2 -- the projection of |u|^2 u on the mode; the orbit
    z = A phi e^{i nu t} sampled at t_i = 2 pi i / M; the period 2 pi / nu.  Returns (X, T, r)."""
    x = np.sin(np.pi * np.arange(1, m.nx + 1) / (m.nx + 1))
    y = np.sin(np.pi * np.arange(1, m.ny + 1) / (m.ny + 1))
    phi = np.outer(y, x).reshape(-1)
    kappa = np.sum(phi ** 4) / np.sum(phi ** 2)
    rH = -m.lam.max()
    A = amp_factor * math.sqrt(dr / (-PARS["c3"] * kappa))
    T = 2 * math.pi / PARS["nu"]
    X = np.stack([np.concatenate([A * phi * math.cos(2 * math.pi * i / M), A * phi * math.sin(2 * math.pi * i / M)]) for i in range(M)])
    return X, T, rH - dr


# ------------------------------------------------------------------------------------------ the fixture
def _mults(fl, s, pars, nsteps, normal, center, k=5):
    """The k leading eigenvalues of the dense monodromy matrix.  The orbit is first converged on to 1e-11, past the 1e-9 of the
    recorded Newton run: next to the Hopf point |(I - M)^-1| on the section is 1 / (mu - 1) ~ 12, and an orbit known to 1e-9 would
    leave 1e-8 in the multipliers, the size of the bound they are compared under."""
    ev0 = np.linalg.eigvals(monodromy_matrix(fl, s["X"], s["T"], pars, nsteps))
    p = newton(fl, s["X"], s["T"], pars, nsteps, normal, center, tol=POLISH_TOL, max_iterations=6)
    assert p["converged"], p["residuals"]
    ev = np.linalg.eigvals(monodromy_matrix(fl, p["X"], p["T"], pars, nsteps))
    ev = ev[np.argsort(-np.abs(ev), kind="stable")][:k]
    # trivial_distance: how far the trivial multiplier of the RECORDED Newton run (stopped at 1e-9) is from 1 -- the tangent is the
    # exact derivative of the discrete map, so that distance is set by how far Newton went, not by the time step
    return [[float(v.real), float(v.imag)] for v in ev], float(np.min(np.abs(ev0 - 1.0)))


def cycle_case(dims, M, nsteps, with_multipliers=True):
    m = P.Model(dims, LS)
    fl = Flow(m, float)
    X0 = guess_from_flow(fl, cycle_start(m), 120.0, 1200, 6.3, M, nsteps, PARS)
    normal, center = update_section(fl, X0, PARS)
    s = newton(fl, X0, 6.3, PARS, nsteps, normal, center)
    rec = dict(dims=list(dims), M=M, nsteps=nsteps, r=PARS["r"], T=s["T"], amplitude=float(np.abs(s["X"]).max()),
               residuals=s["residuals"], itlinear=s["itlinear"], converged=bool(s["converged"]))
    if with_multipliers:
        rec["multipliers"], rec["trivial_distance"] = _mults(fl, s, PARS, nsteps, normal, center)
    return rec, s, (m, fl, X0, normal, center)


def hopf_case(dims, M, nsteps, dr, with_multipliers=True):
    m = P.Model(dims, LS)
    fl = Flow(m, float)
    X0, T0, r = hopf_guess(m, dr, M)
    pars = dict(PARS, r=r)
    normal, center = update_section(fl, X0, pars)
    s = newton(fl, X0, T0, pars, nsteps, normal, center)
    rec = dict(dims=list(dims), M=M, nsteps=nsteps, dr=dr, r=r, T=s["T"], amplitude=float(np.abs(s["X"]).max()),
               residuals=s["residuals"], itlinear=s["itlinear"], converged=bool(s["converged"]))
    if with_multipliers:
        rec["multipliers"], rec["trivial_distance"] = _mults(fl, s, pars, nsteps, normal, center)
    return rec, s, (m, fl, X0, normal, center, pars, T0)


def build_fixture():
    return dict(cycle=[cycle_case(*c)[0] for c in CYCLE_CASES], hopf=[hopf_case(*c)[0] for c in HOPF_CASES])


def load_fixture():
    with open(GOLDEN) as f:
        return json.load(f)


if __name__ == "__main__":
    fx = build_fixture()
    with open(GOLDEN, "w") as f:
        json.dump(fx, f, indent=1)
    for k in ("cycle", "hopf"):
        for c in fx[k]:
            print(k, c["dims"], c["M"], c["nsteps"], f"T = {c['T']:.6f}", c["itnewton"] if "itnewton" in c else len(c["itlinear"]),
                  c["itlinear"], c["multipliers"][:2])
