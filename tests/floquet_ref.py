"""CPU restatement of the Floquet multipliers of the trapezoid periodic orbits of cGL (src/periodicorbit/Floquet.jl: FloquetQaD
:48-85, MonodromyQaD_matrix_free(::Trapeze) :285-315, the eigenfunction :319-355, the dense MonodromyQaD :358-381) in NumPy / SciPy
on top of tests/potrap_ref.py -- long double where it is the yardstick: the dense monodromy, the initial-value operator whose last
solution slice is the monodromy applied to x, its preconditioner matrix A0 by sparse LU and by the modal recurrence, the space-time
GMRES, the stability counts and the classification of src/Bifurcations.jl:80-151 for a Floquet solver.

Orbit U of shape (M, N), K = M - 1, hh = T (1 / M) / 2, prev(0) = K - 1.  With A_i = I - hh J_i, B_i = I + hh J_i:

    monodromy = prod_{i = K-1 .. 0} A_i^-1 B_prev(i)
    A_i y_i - B_{i-1} y_{i-1} = 0 (i >= 1),   A_0 y_0 = B_{K-1} x,   monodromy x = y_{K-1}

Not a product path: tests only."""
import cmath
import math

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import potrap_ref as R


def hopf_guess(m, M, dr, pars):
    """The one-mode guess of the Hopf predictor at the trivial state in closed form (test_potrap_reference._hopf_guess): a = 1,
    b = 2 (-c3 + i mu) 9 / (4 (Nx + 1) (Ny + 1)), amp = sqrt(dr / Re b), slices 2 Re(zeta amp e^{i t_m}), T entry 2 pi / omega."""
    b = 2 * (-pars["c3"] + 1j * pars["mu"]) * 9 / (4 * (m.nx + 1) * (m.ny + 1))
    amp = math.sqrt(dr / b.real)
    om = pars["nu"] - b.imag / b.real * dr
    phi = np.outer(np.sin(np.pi * np.arange(1, m.ny + 1) / (m.ny + 1)), np.sin(np.pi * np.arange(1, m.nx + 1) / (m.nx + 1))).reshape(-1)
    phi /= np.linalg.norm(phi) * math.sqrt(2)
    t = 2 * np.pi * np.arange(M) / M
    return np.stack([np.concatenate([2 * amp * np.cos(tm) * phi, 2 * amp * np.sin(tm) * phi]) for tm in t]), abs(2 * np.pi / om)


def converged_orbit(m, M, dr, pars0, max_iterations=10):
    """Newton with sparse LU from the guess at r = r_hopf - dr -> (newton record, pars, phi, xpi)."""
    r = -m.lam.max() - dr
    pars = dict(pars0, r=r)
    pars_of = lambda p: dict(pars, r=p)
    U0, T0 = hopf_guess(m, M, dr, pars)
    phi, xpi = R.section_from_guess(m, U0, pars)
    s = R.newton(m, U0, T0, r, pars_of, phi, xpi, R.lu_solver(m, pars_of), tol=1e-10, max_iterations=max_iterations)
    return s, pars, phi, xpi, (U0, T0)


# ------------------------------------------------------------------------------------------ the dense monodromy (:358-381)
def dense_monodromy(m, U, T, pars):
    M, K = U.shape[0], U.shape[0] - 1
    hh = R._hh(T, M, float)
    I = np.eye(m.N)
    Js = [m.J(U[i], pars).toarray() for i in range(K)]
    mono = np.linalg.solve(I - hh * Js[0], I + hh * Js[K - 1])
    for i in range(1, K):
        mono = np.linalg.solve(I - hh * Js[i], I + hh * Js[i - 1]) @ mono
    return mono


def monodromy_sequential(m, U, T, pars, x, rtol=None, a=None, b=None):
    """:285-315: K steps, one slice at a time -> all K slices (the last is the monodromy applied to x).  rtol = None: dense solves;
    else every slice solve by SciPy GMRES at rtol, left-preconditioned by (I - hh L0)^-1 in modal form, counted by the pr_norm
    callback -- then the return value is (slices, iterations summed)."""
    M, K = U.shape[0], U.shape[0] - 1
    hh = R._hh(T, M, float)
    I = np.eye(m.N)
    out, ys, its = np.array(x, dtype=float), [], [0]
    if rtol is not None:
        n = m.n
        dst = lambda v: (m.Sy @ v.reshape(m.ny, m.nx) @ m.Sx).reshape(-1)
        alpha = 1 - hh * ((pars["r"] if a is None else a) + m.lam + 1j * (pars["nu"] if b is None else b))

        def P(v):
            w = (dst(v[:n]) + 1j * dst(v[n:])) / alpha
            return np.concatenate([dst(w.real), dst(w.imag)])

        def cb(_):
            its[0] += 1
    for i in range(K):
        out = out + hh * m.Jv(U[R._prev(i, K)], pars, out)
        if rtol is None:
            out = np.linalg.solve(I - hh * m.J(U[i], pars).toarray(), out)
        else:
            B = lambda v, i=i: P(v - hh * m.Jv(U[i], pars, v))
            out, info = spla.gmres(spla.LinearOperator((m.N, m.N), matvec=B, dtype=float), P(out), rtol=rtol, atol=0.0, restart=60,
                                   maxiter=200, callback=cb, callback_type="pr_norm")
            assert info == 0, info
        ys.append(out)
    return np.array(ys) if rtol is None else (np.array(ys), its[0])


# ------------------------------------------------------------------------------------------ the initial-value operator
def ivp_apply(m, U, T, pars, Y, mod=False):
    """out_0 = y_0 - hh J_0 y_0, out_i = (y_i - hh J_i y_i) - (y_{i-1} + hh J_{i-1} y_{i-1}) for Y of shape (K, N), any float
    dtype; mod: the sum of the moduli of the terms of every entry instead (the unit of the rounding bounds)."""
    M, K = U.shape[0], U.shape[0] - 1
    dt = Y.dtype.type
    hh = abs(R._hh(T, M, dt)) if mod else R._hh(T, M, dt)
    Js = [(m.Jv_abs if mod else m.Jv)(U[i], pars, Y[i]) for i in range(K)]
    out = np.empty_like(Y)
    for i in range(K):
        if mod:
            out[i] = np.abs(Y[i]) + hh * Js[i] + ((np.abs(Y[i - 1]) + hh * Js[i - 1]) if i else 0)
        else:
            out[i] = (Y[i] - hh * Js[i]) - ((Y[i - 1] + hh * Js[i - 1]) if i else 0)
    return out


def ivp_rhs(m, U, T, pars, x):
    """f of shape (K, N): f_0 = x + hh J_{K-1} x, the other rows zero."""
    M, K = U.shape[0], U.shape[0] - 1
    f = np.zeros((K, m.N))
    f[0] = x + R._hh(T, M, float) * m.Jv(U[K - 1], pars, x)
    return f


def _ivp_matrix(m, M, T, blocks):
    N, K, hh = m.N, M - 1, R._hh(T, M, float)
    I = sp.identity(N, format="csr")
    rows = [[None] * K for _ in range(K)]
    for i in range(K):
        rows[i][i] = I - hh * blocks[i]
        if i:
            rows[i][i - 1] = -I - hh * blocks[i - 1]
    return sp.bmat(rows, format="csc")


def ivp_sparse(m, U, T, pars):
    return _ivp_matrix(m, U.shape[0], T, [m.J(U[i], pars) for i in range(U.shape[0] - 1)])


def A0_ivp_sparse(m, M, T, a, b):
    """The matrix of the preconditioner: every J_i replaced by L0 = Lap (x) I_2 + [[a, -b], [b, a]]."""
    return _ivp_matrix(m, M, T, [R.L0(m, a, b)] * (M - 1))


def modal_min_alpha(m, M, T, a, b):
    hh = R._hh(T, M, float)
    return float(np.abs(1 - hh * (a + m.lam + 1j * b)).min())


def modal_solve_ivp(m, M, T, a, b, f):
    """A0^-1 f for f of shape (K, N): DST-I of every field, w_i = rho w_{i-1} + f_i / alpha from w_{-1} = 0 per mode, DST-I back."""
    n, K, hh = m.n, M - 1, R._hh(T, M, float)
    dst = lambda x: (m.Sy @ x.reshape(-1, m.ny, m.nx) @ m.Sx).reshape(x.shape[0], -1)      # all slices of one field at once
    mu = a + m.lam + 1j * b
    alpha, beta = 1 - hh * mu, 1 + hh * mu
    rho = beta / alpha
    fh = (dst(f[:, :n]) + 1j * dst(f[:, n:])) / alpha
    w = np.zeros(n, complex)
    for i in range(K):
        w = rho * w + fh[i]
        fh[i] = w
    return np.concatenate([dst(fh.real), dst(fh.imag)], axis=1)


# ------------------------------------------------------------------------------------------ the space-time solve
def spacetime_solve(m, U, T, pars, x, a, b, rtol, restart=60, maxiter=200, atol=0.0):
    """Left-preconditioned GMRES on A0^-1 A y = A0^-1 f, y0 = 0, matrix-free, stopping at |r| <= max(rtol |r0|, atol) in the 2-norm
    of the preconditioned residual, counted by the pr_norm callback as potrap_ref.gmres_solve counts -> (Y (K, N), iterations)."""
    M, K = U.shape[0], U.shape[0] - 1
    P = lambda v: modal_solve_ivp(m, M, T, a, b, v.reshape(K, -1)).reshape(-1)
    B = lambda v: P(ivp_apply(m, U, T, pars, v.reshape(K, -1)).reshape(-1))
    its = [0]

    def cb(_):
        its[0] += 1

    n = K * m.N
    y, info = spla.gmres(spla.LinearOperator((n, n), matvec=B, dtype=float), P(ivp_rhs(m, U, T, pars, x).reshape(-1)), rtol=rtol,
                         atol=atol, restart=restart, maxiter=maxiter, callback=cb, callback_type="pr_norm")
    assert info == 0, info
    return y.reshape(K, -1), its[0]


# delta = |M_gmres - M_dense|_2 at rtol 1e-9 on the restatement's own LU-Newton orbits, keyed (dims, M, dr): the assembly takes 4 s
# and 8 s of CPU, so it runs once per CPU suite (test_floquet_reference pins these within a factor 2) and the GPU tests read the
# figures from here; the GPU's orbit differs from the restatement's by ~1e-13, far below delta
DELTA = {((16, 12), 12, 0.1): 2.89e-9, ((16, 12), 30, 0.01): 3.55e-9}


def monodromy_by_gmres(m, U, T, pars, a, b, rtol):
    """The monodromy assembled column by column by the space-time GMRES at rtol -> (matrix, iteration counts)."""
    cols, its = [], []
    for k in range(m.N):
        e = np.zeros(m.N)
        e[k] = 1.0
        Y, it = spacetime_solve(m, U, T, pars, e, a, b, rtol)
        cols.append(Y[-1])
        its.append(it)
    return np.array(cols).T, its


# ------------------------------------------------------------------------------------------ multipliers, stability, classification
def leading_multipliers(mono, nev):
    """(multipliers by decreasing modulus, right eigenvectors, kappa = 1 / |y^H x| with unit left and right eigenvectors)."""
    w, vl, vr = _eig_lr(mono)
    order = np.argsort(-np.abs(w), kind="stable")[:nev]
    kappa = [1.0 / abs(np.vdot(vl[:, k], vr[:, k])) for k in order]
    return w[order], vr[:, order], np.array(kappa)


def _eig_lr(A):
    import scipy.linalg as sla
    w, vl, vr = sla.eig(A, left=True, right=True)
    vl = vl / np.linalg.norm(vl, axis=0)
    vr = vr / np.linalg.norm(vr, axis=0)
    return w, vl, vr


def floquet_exponents(mults):
    """log.(complex.(vals)) sorted by decreasing real part (:74-79)."""
    s = np.array([cmath.log(complex(v)) if v != 0 else complex(-math.inf, 0.0) for v in mults])
    return s[np.argsort(-s.real, kind="stable")]


def stability_counts(sigma, tol):
    """(n_unstable, n_imag): Re sigma > tol, and of those the ones with |Im sigma| > tol."""
    s = np.asarray(sigma)
    s = s[~np.isnan(s.real)]
    un = s[s.real > tol]
    return int(un.size), int(np.sum(np.abs(un.imag) > tol))


def branch_stability(m, U0, T0, pars, lens, phi, xpi, solve, cp, steps, nev, tol):
    """The restatement's PALC branch (potrap_ref.palc) with the dense multipliers at every point -> palc's dict plus multipliers,
    exponents, n_unstable, n_imag per point.  palc keeps the last orbit only; it hands every accepted point to update_section at
    the start of the next step, which is where the orbits are picked up."""
    orbits, keep = [], R.update_section

    def tap(m_, U, pars_):
        orbits.append(U.copy())
        return keep(m_, U, pars_)

    R.update_section = tap
    try:
        br = R.palc(m, U0, T0, pars, lens, phi, xpi, solve, cp, steps)
    finally:
        R.update_section = keep
    orbits.append(br["U"])
    assert len(orbits) == steps + 1 == len(br["p"])
    br.update(multipliers=[], exponents=[], n_unstable=[], n_imag=[], orbits=orbits)
    for k in range(steps + 1):
        w, _, _ = leading_multipliers(dense_monodromy(m, orbits[k], br["T"][k], dict(pars, **{lens: br["p"][k]})), nev)
        s = floquet_exponents(w)
        nu, ni = stability_counts(s, tol)
        br["multipliers"].append(w); br["exponents"].append(s); br["n_unstable"].append(nu); br["n_imag"].append(ni)
    return br


# rows of src/Bifurcations.jl:103-131 for a Floquet solver: (|d n_unstable|, |d n_imag|) -> type
def classify(n_unstable, n_unstable_prev, n_imag, n_imag_prev):
    du, di = abs(n_unstable - n_unstable_prev), abs(n_imag - n_imag_prev)
    if n_unstable * n_unstable_prev < 0 or n_imag * n_imag_prev < 0 or du < di:
        return "nd"
    if du == 0:
        return None
    return {(1, 0): "bp", (1, 1): "pd", (2, 2): "ns"}.get((du, di), "nd")
