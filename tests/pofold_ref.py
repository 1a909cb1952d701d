"""CPU restatement of the adjoint layer of the trapezoid periodic-orbit functional of cGL (csrc/pofold.hip), on potrap_ref.py: the
application of dG(u, T)^T -- long double where it is the yardstick --, the time solve of A0^-T per sine mode, and the
left-preconditioned SciPy GMRES on dG^T; the analytic second derivatives and the border row of the fold system; doubly bordered
solves by sparse LU and by SciPy GMRES; Newton on the fold system and PALC along the fold curve in a second parameter with either
(src/codim2/MinAugFold.jl on the Trapeze functional, examples/cGL2d.jl:347-392).

Notation of potrap_ref.py; next(j) = j + 1, next(K - 1) = 0; s_j = w_j + w_next(j), q_j = J_j^T s_j.  Not a product path: tests
only."""
import numpy as np
import scipy.sparse.linalg as spla

import potrap_ref as R


def _next(j, K):
    return 0 if j == K - 1 else j + 1


def JTv(m, u, pars, s):
    """J(u)^T s: the Laplacian is symmetric, the pointwise block is transposed."""
    n = m.n
    f1u, f1v, f2u, f2v = m._jac(u, pars)
    return np.concatenate([m._lap(s[:n]) + f1u * s[:n] + f2u * s[n:], m._lap(s[n:]) + f1v * s[:n] + f2v * s[n:]])


def JTv_abs(m, u, pars, a, b):
    """The sum of the moduli of the terms of J(u)^T (a + b), the Laplacians of a and b taken one by one as the device takes them."""
    n = m.n
    f1u, f1v, f2u, f2v = m._jac(u, pars, True)
    s1, s2 = np.abs(a[:n]) + np.abs(b[:n]), np.abs(a[n:]) + np.abs(b[n:])
    return np.concatenate([m._lap(a[:n], True) + m._lap(b[:n], True) + f1u * s1 + f2u * s2,
                           m._lap(a[n:], True) + m._lap(b[n:], True) + f1v * s1 + f2v * s2])


def jvp_adjoint(m, U, T, pars, W, tau, phi, mod=False):
    """dG(U, T)^T (W, tau) -> (out (M, N), tail); mod: the sum of the moduli of the terms of every entry instead."""
    M, K = U.shape[0], U.shape[0] - 1
    dt = U.dtype.type
    hh = R._hh(T, M, dt)
    out = np.empty_like(U)
    tail = dt(0)
    for j in range(K):
        nx = _next(j, K)
        if mod:
            out[j] = (np.abs(W[j]) + np.abs(W[nx])) + abs(hh) * JTv_abs(m, U[j], pars, W[j], W[nx]) + abs(dt(tau)) * np.abs(phi[j])
            tail += np.sum(m.F_abs(U[j], pars) * (np.abs(W[j]) + np.abs(W[nx])))
        else:
            s = W[j] + W[nx]
            out[j] = ((W[j] - W[nx]) - hh * JTv(m, U[j], pars, s)) + dt(tau) * phi[j]
            tail += np.sum(m.F(U[j], pars) * s)
    if mod:
        out[0] = out[0] + np.abs(W[K])
        out[K] = np.abs(W[K]) + abs(dt(tau)) * np.abs(phi[K])
        return out, tail / dt(M) / dt(2)
    out[0] = out[0] - W[K]
    out[K] = W[K] + dt(tau) * phi[K]
    return out, -(tail / dt(M) / dt(2))


def modal_solve_adjoint(m, M, T, a, b, f):
    """A0^-T f for f of shape (M, N): DST-I of every field (symmetric), per mode w_K = f_K, f_0 <- f_0 + f_K and the recurrence
    backwards in time with conj(rho), conj(alpha), closed with 1 - conj(rho)^K, DST-I back."""
    n, K, hh = m.n, M - 1, R._hh(T, M, float)
    dst = lambda x: (m.Sy @ x.reshape(m.ny, m.nx) @ m.Sx).reshape(-1)
    fh = np.array([dst(f[i, :n]) + 1j * dst(f[i, n:]) for i in range(M)])
    mu = a + m.lam - 1j * b
    alpha, beta = 1 - hh * mu, 1 + hh * mu
    rho = beta / alpha
    g = fh[:K].copy()
    g[0] = g[0] + fh[K]
    acc, rk = np.zeros(n, complex), np.ones(n, complex)
    for j in range(K - 1, -1, -1):
        acc = rho * acc + g[j] / alpha
        rk = rk * rho
    w = acc / (1 - rk)
    wh = np.empty_like(fh)
    for j in range(K - 1, -1, -1):
        w = rho * w + g[j] / alpha
        wh[j] = w
    wh[K] = fh[K]
    out = np.empty_like(f)
    for i in range(M):
        out[i, :n], out[i, n:] = dst(wh[i].real), dst(wh[i].imag)
    return out


def gmres_solve_adjoint(m, U, T, pars, phi, rhs, a, b, Tp, rtol, restart=60, maxiter=200, atol=0.0):
    """potrap_ref.gmres_solve on the transposed system: diag(A0^-T, 1) dG^T x = diag(A0^-T, 1) rhs.  Returns (x, iterations)."""
    M = U.shape[0]

    def P(v):
        return np.concatenate([modal_solve_adjoint(m, M, Tp, a, b, v[:-1].reshape(M, -1)).reshape(-1), v[-1:]])

    def B(v):
        o, t = jvp_adjoint(m, U, T, pars, v[:-1].reshape(M, -1), v[-1], phi)
        return P(np.concatenate([o.reshape(-1), [t]]))

    its = [0]

    def cb(_):
        its[0] += 1

    n = rhs.size
    x, info = spla.gmres(spla.LinearOperator((n, n), matvec=B, dtype=float), P(rhs), rtol=rtol, atol=atol, restart=restart,
                         maxiter=maxiter, callback=cb, callback_type="pr_norm")
    assert info == 0, info
    return x, its[0]


# ------------------------------------------------------------------------------------------ second derivatives
def hess(m, u, pars, mod=False):
    """The pointwise Hessian of NL at u: (h0 .. h5), H1 = [[h0, h1], [h1, h2]] (field 1), H2 = [[h3, h4], [h4, h5]] (field 2)."""
    n = m.n
    c3, mu, c5 = ((abs(pars[k]) if mod else pars[k]) for k in ("c3", "mu", "c5"))
    u1, u2 = (np.abs(u[:n]), np.abs(u[n:])) if mod else (u[:n], u[n:])
    ua = u1 * u1 + u2 * u2
    q1, q2 = u1 * (8 * u1 * u1 + 12 * ua), u2 * (8 * u1 * u1 + 4 * ua)
    q3, q4 = u1 * (8 * u2 * u2 + 4 * ua), u2 * (8 * u2 * u2 + 12 * ua)
    if mod:
        return (6 * c3 * u1 + 2 * mu * u2 + c5 * q1, 2 * c3 * u2 + 2 * mu * u1 + c5 * q2, 2 * c3 * u1 + 6 * mu * u2 + c5 * q3,
                2 * c3 * u2 + 6 * mu * u1 + c5 * q2, 2 * c3 * u1 + 2 * mu * u2 + c5 * q3, 6 * c3 * u2 + 2 * mu * u1 + c5 * q4)
    return (-6 * c3 * u1 + 2 * mu * u2 - c5 * q1, -2 * c3 * u2 + 2 * mu * u1 - c5 * q2, -2 * c3 * u1 + 6 * mu * u2 - c5 * q3,
            -2 * c3 * u2 - 6 * mu * u1 - c5 * q2, -2 * c3 * u1 - 2 * mu * u2 - c5 * q3, -6 * c3 * u2 - 2 * mu * u1 - c5 * q4)


def hess_vT(m, u, pars, v, s, mod=False):
    """(B(u)[v, .])^T s, B the Hessian of the vector field (the Laplacian is linear: B is pointwise)."""
    n = m.n
    h = hess(m, u, pars, mod)
    f = np.abs if mod else (lambda x: x)
    v1, v2, s1, s2 = f(v[:n]), f(v[n:]), f(s[:n]), f(s[n:])
    return np.concatenate([s1 * (h[0] * v1 + h[1] * v2) + s2 * (h[3] * v1 + h[4] * v2),
                           s1 * (h[1] * v1 + h[2] * v2) + s2 * (h[4] * v1 + h[5] * v2)])


def hess_apply(m, u, pars, v, x):
    """B(u)[v, x]."""
    n = m.n
    h = hess(m, u, pars)
    v1, v2, x1, x2 = v[:n], v[n:], x[:n], x[n:]
    return np.concatenate([x1 * (h[0] * v1 + h[1] * v2) + x2 * (h[1] * v1 + h[2] * v2),
                           x1 * (h[3] * v1 + h[4] * v2) + x2 * (h[4] * v1 + h[5] * v2)])


def djdp_v(m, u, name, v, mod=False):
    """D_p(u) v, D_p = dJ/dp for the parameter `name` (pointwise)."""
    n = m.n
    f = np.abs if mod else (lambda x: x)
    u1, u2, v1, v2 = f(u[:n]), f(u[n:]), f(v[:n]), f(v[n:])
    ua = u1 * u1 + u2 * u2
    z = np.zeros_like(u1)
    sg = 1 if mod else -1
    d = {"r": (z + 1, z, z, z + 1), "nu": (z, sg * (z + 1), z + 1, z),
         "mu": (2 * u1 * u2, 2 * u2 * u2 + ua, sg * (2 * u1 * u1 + ua), sg * 2 * u1 * u2),
         "c3": (sg * (2 * u1 * u1 + ua), sg * 2 * u1 * u2, sg * 2 * u1 * u2, sg * (2 * u2 * u2 + ua)),
         "c5": (sg * (4 * ua * u1 * u1 + ua * ua), sg * 4 * ua * u1 * u2, sg * 4 * ua * u1 * u2, sg * (4 * ua * u2 * u2 + ua * ua)),
         "gamma": (z, z, z, z)}[name]
    return np.concatenate([d[0] * v1 + d[1] * v2, d[2] * v1 + d[3] * v2])


def fold_border(m, U, T, pars, name, V, vT, W, mod=False):
    """(sigma_x (M, N), (sigma_x)_T, sigma_p) of the fold of the orbit functional for the parameter `name`:
        <sigma_x, X> = -<w, d2G[v, X]>,  sigma_p = -<w, d_p(dG) v>     (MinAugFold.jl:90-97, 131; w carries no T entry here)
    through s_j = w_j + w_next(j), q_j = J_j^T s_j; mod: the sums of the moduli of the terms instead."""
    M, K = U.shape[0], U.shape[0] - 1
    dt = U.dtype.type
    hh, dv = R._hh(T, M, dt), dt(vT) / dt(M) / dt(2)
    if mod:
        hh, dv = abs(hh), abs(dv)
    out = np.zeros_like(U)
    sT, sp = dt(0), dt(0)
    for j in range(K):
        nx = _next(j, K)
        if mod:
            s = np.abs(W[j]) + np.abs(W[nx])
            q = JTv_abs(m, U[j], pars, W[j], W[nx])
            out[j] = hh * hess_vT(m, U[j], pars, V[j], s, True) + dv * q
            sT += np.sum(q * np.abs(V[j]))
            sp += np.sum(s * (hh * djdp_v(m, U[j], name, V[j], True) + dv * np.abs(m.dFdp(np.abs(U[j]), pars, name))))
        else:
            s = W[j] + W[nx]
            q = JTv(m, U[j], pars, s)
            out[j] = hh * hess_vT(m, U[j], pars, V[j], s) + dv * q
            sT += np.sum(q * V[j])
            sp += np.sum(s * (hh * djdp_v(m, U[j], name, V[j]) + dv * m.dFdp(U[j], pars, name)))
    return out, sT / dt(M) / dt(2), sp


# ------------------------------------------------------------------------------------------ doubly bordered systems
def bordered_matrix(A, a, b, c):
    """[A a; b^T c] for the assembled (M N + 1) matrix A and vectors a, b of its size."""
    import scipy.sparse as sp
    return sp.bmat([[A, sp.csr_matrix(a.reshape(-1, 1))], [sp.csr_matrix(b.reshape(1, -1)), sp.csr_matrix([[c]])]], format="csc")


def bordered_solve_lu(m, U, T, pars, phi, a, b, c, rhs, adjoint=False):
    """[dG a; b^T c] \\ rhs (dG^T with adjoint) by sparse LU -> (x, 0); a, b, rhs carry the T entry, rhs also the border scalar."""
    A = R.jacobian_sparse(m, U, T, pars, phi)
    return spla.splu(bordered_matrix(A.T.tocsc() if adjoint else A, a, b, c)).solve(rhs), 0


def bordered_solve_gmres(m, U, T, pars, phi, a, b, c, rhs, pa, pb, Tp, rtol, adjoint=False, restart=60, maxiter=200):
    """The same system as ONE GMRES left-preconditioned by diag(A0^-1, 1, 1) (A0^-T with adjoint), x0 = 0, stopping at
    |r| <= rtol |r0| in the 2-norm of the preconditioned residual -> (x, iterations)."""
    M = U.shape[0]
    ms = modal_solve_adjoint if adjoint else R.modal_solve

    def P(v):
        return np.concatenate([ms(m, M, Tp, pa, pb, v[:-2].reshape(M, -1)).reshape(-1), v[-2:]])

    def B(v):
        if adjoint:
            o, t = jvp_adjoint(m, U, T, pars, v[:-2].reshape(M, -1), v[-2], phi)
        else:
            o, t = R.jvp(m, U, T, pars, v[:-2].reshape(M, -1), v[-2], phi)
        top = np.concatenate([o.reshape(-1), [t]]) + v[-1] * a
        return P(np.concatenate([top, [b @ v[:-1] + c * v[-1]]]))

    its = [0]

    def cb(_):
        its[0] += 1

    n = rhs.size
    x, info = spla.gmres(spla.LinearOperator((n, n), matvec=B, dtype=float), P(rhs), rtol=rtol, atol=0.0, restart=restart,
                         maxiter=maxiter, callback=cb, callback_type="pr_norm")
    assert info == 0, info
    return x, its[0]


# ------------------------------------------------------------------------------------------ the fold system
def fold_terms(m, U, T, pars, phi, a, b, bsolve):
    """[dG a; b^T 0][v; sigma] = [0; 1], [dG^T b; a^T 0][w; sigma2] = [0; 1] (MinAugFold.jl:15-69) -> (v, w, sigma, (it_v, it_w));
    v, w of length M N + 1.  bsolve(U, T, pars, phi, a, b, c, rhs, adjoint) -> (x, iterations)."""
    e = np.zeros(a.size + 1)
    e[-1] = 1.0
    xv, iv = bsolve(U, T, pars, phi, a, b, 0.0, e, False)
    xw, iw = bsolve(U, T, pars, phi, b, a, 0.0, e, True)
    return xv[:-1], xw[:-1], float(xv[-1]), (iv, iw)


def newton_fold(m, U0, T0, pars, name, phi, xpi, a, b, bsolve, tol=1e-10, max_iterations=10):
    """Newton on G_fold(X, p) = (G(X, p), sigma(X, p)) in the sup norm (src/Newton.jl:66-114), every linear system a doubly
    bordered one: per point the two of fold_terms, per step [dG d_pG; sigma_x^T sigma_p][dX; dp] = [G; sigma] (the branch
    MinAugFold.jl:136-145).  The section (phi, xpi) and (a, b) are frozen.  Returns dict(U, T, p, residuals, itlinear (a triple per
    Newton step: v, w, step), v, w, sigma, converged)."""
    U, T, p = U0.copy(), float(T0), float(pars[name])
    res, its = [], []

    def point():
        pp = dict(pars, **{name: p})
        G = R.pack(*R.residual(m, U, T, pp, phi, xpi))
        v, w, sig, it = fold_terms(m, U, T, pp, phi, a, b, bsolve)
        return pp, G, v, w, sig, it

    pp, G, v, w, sig, it = point()
    res.append(max(R._norminf(G), abs(sig)))
    while len(res) - 1 < max_iterations and res[-1] > tol:
        M = U.shape[0]
        sx, sxT, sp_ = fold_border(m, U, T, pp, name, v[:-1].reshape(M, -1), v[-1], w[:-1].reshape(M, -1))
        dpG = R.pack(R.dparam(m, U, T, pp, name), 0.0)
        dx, its_ = bsolve(U, T, pp, phi, dpG, R.pack(sx, sxT), sp_, np.concatenate([G, [sig]]), False)
        dU, dT = R.unpack(m, dx[:-1])
        U, T, p = U - dU, T - dT, p - float(dx[-1])
        pp, G, v, w, sig, it2 = point()
        its.append((it[0], it[1], its_))
        it = it2
        res.append(max(R._norminf(G), abs(sig)))
    return dict(U=U, T=T, p=p, residuals=res, itlinear=its, last_terms_its=it, v=v, w=w, sigma=sig, converged=res[-1] < tol)


def lu_bsolver(m):
    return lambda U, T, pars, phi, a, b, c, rhs, adjoint: bordered_solve_lu(m, U, T, pars, phi, a, b, c, rhs, adjoint)


def gmres_bsolver(m, pa, pb, Tp, rtol):
    return lambda U, T, pars, phi, a, b, c, rhs, adjoint: bordered_solve_gmres(m, U, T, pars, phi, a, b, c, rhs, pa, pb, Tp, rtol,
                                                                               adjoint)


# ------------------------------------------------------------------------------------------ the recorded fold run
def hopf_guess(m, M, dr, PARS):
    """The one-mode guess of the Hopf predictor at the trivial state in closed form (test_potrap_reference._hopf_guess)."""
    import math
    b = 2 * (-PARS["c3"] + 1j * PARS["mu"]) * 9 / (4 * (m.nx + 1) * (m.ny + 1))
    amp = math.sqrt(dr / b.real)
    om = PARS["nu"] + (0.0 - b.imag * 1.0 / b.real) * dr
    phi = np.outer(np.sin(np.pi * np.arange(1, m.ny + 1) / (m.ny + 1)), np.sin(np.pi * np.arange(1, m.nx + 1) / (m.nx + 1))).reshape(-1)
    phi /= np.linalg.norm(phi) * math.sqrt(2)
    t = 2 * np.pi * np.arange(M) / M
    U = np.stack([np.concatenate([2 * amp * np.cos(tm) * phi, 2 * amp * np.sin(tm) * phi]) for tm in t])
    return U, abs(2 * np.pi / om)


def fold_start(m, U0, T0, pars, lens, phi, xpi, solve, cp, steps):
    """What po_fold_point hands over after `steps` PALC steps of potrap_ref.palc: the last point (U, T, p), a = b = the secant
    tangent of the last step in (U, T), normalised in the 2-norm with the sign of ds, and the section of updatesection! there."""
    import math
    orbits, keep = [], R.update_section

    def tap(m_, U, pars_):                      # palc hands every accepted point to update_section at the start of the next step
        orbits.append(U.copy())
        return keep(m_, U, pars_)

    R.update_section = tap
    try:
        z1 = R.palc(m, U0, T0, pars, lens, phi, xpi, solve, cp, steps)
    finally:
        R.update_section = keep
    z0 = dict(U=orbits[-1], Tlast=z1["T"][-2])
    U, T, p = z1["U"], z1["Tlast"], z1["p"][-1]
    tau = math.copysign(1.0, cp["ds"]) * (R.pack(U, T) - R.pack(z0["U"], z0["Tlast"]))
    tau /= np.linalg.norm(tau)
    sphi, sxpi = R.update_section(m, U, dict(pars, **{lens: p}))
    return dict(U=U, T=T, p=p, tau=tau, phi=sphi, xpi=sxpi, branch=z1)


# ------------------------------------------------------------------------------------------ the fold curve
def _fold_point_terms(m, U, T, pp, name1, phi, xpi, a, b, bsolve):
    """(G_fold residual packed (M N + 2), v, w, iterations) at a point."""
    G = R.pack(*R.residual(m, U, T, pp, phi, xpi))
    v, w, sig, it = fold_terms(m, U, T, pp, phi, a, b, bsolve)
    return np.concatenate([G, [sig]]), v, w, it


def palc_fold(m, U0, T0, pars, name1, name2, phi, xpi, a, b, bsolve, cp, steps, theta=0.5):
    """The steps of continuation_fold_po (codim2._continuation_minaug on the orbit functional): Newton on G_fold at p2 and at
    p2 + ds / eta, the secant tangent in X = (U, T, p1), then per step newton_palc with BorderingBLS over the fold linear solver
    (two solves with the full fold Jacobian [dG d_p1 G; sigma_x^T sigma_p1] per Newton step, d_p2 G_fold analytic), the step-size
    control, and a <- w / |w|, b <- v / |v| after every accepted point (the first included).  The section is frozen.
    Returns dict(p1, p2, T, amplitude, itnewton, itlinear (GMRES counts summed per step))."""
    M = U0.shape[0]
    p2 = float(pars[name2])
    its_total = [0]

    def count(it):
        its_total[0] += int(np.sum(it))

    def G_at(x, q2, a_, b_):
        U, T = R.unpack(m, x[:-1])
        pp = dict(pars, **{name1: float(x[-1]), name2: q2})
        g, v, w, it = _fold_point_terms(m, U, T, pp, name1, phi, xpi, a_, b_, bsolve)
        count(it)
        return g, v, w, (U, T, pp)

    def Jsolve(pt, v, w, rhss):
        U, T, pp = pt
        sx, sxT, sp_ = fold_border(m, U, T, pp, name1, v[:-1].reshape(M, -1), v[-1], w[:-1].reshape(M, -1))
        dpG = R.pack(R.dparam(m, U, T, pp, name1), 0.0)
        out = []
        for r in rhss:
            x, it = bsolve(U, T, pp, phi, dpG, R.pack(sx, sxT), sp_, r, False)
            count(it)
            out.append(x)
        return out

    def newton(x, q2, a_, b_, tol, maxit):
        g, v, w, pt = G_at(x, q2, a_, b_)
        res = [R._norminf(g)]
        while len(res) - 1 < maxit and res[-1] > tol:
            (dx,) = Jsolve(pt, v, w, [g])
            x = x - dx
            g, v, w, pt = G_at(x, q2, a_, b_)
            res.append(R._norminf(g))
        assert res[-1] < tol, res
        return x, v, w, len(res) - 1

    x0 = np.concatenate([R.pack(U0, T0), [float(pars[name1])]])
    z0x, v0, w0, n0 = newton(x0, p2, a, b, cp["tol"], cp["max_iterations"])
    it_first = its_total[0]
    ds = cp["ds"]
    p2b = p2 + ds / cp["eta"]
    z1x, _, _, _ = newton(z0x, p2b, a, b, cp["tol"], cp["max_iterations"])
    tau = R._secant((z1x, p2b), (z0x, p2), ds, theta)
    z, z_old = (z0x, p2), (z0x, p2)
    a, b = w0 / np.linalg.norm(w0), v0 / np.linalg.norm(v0)
    amp = lambda x: R._norminf(x[:-2])
    out = dict(p1=[z0x[-1]], p2=[p2], T=[z0x[-2]], amplitude=[amp(z0x)], itnewton=[n0], itlinear=[it_first])
    for _ in range(steps):
        its_total[0] = 0
        zp = (z[0] + ds * tau[0], z[1] + ds * tau[1])
        Nf = lambda x, p: (R._dot_theta(x, tau[0], p - z[1], tau[1], theta) - ds) - R._dot_theta(z[0], tau[0], p - z[1], 0.0, theta)
        x, p = zp
        g, v, w, pt = G_at(x, p, a, b)
        rn = Nf(x, p)
        res = [max(R._norminf(g), abs(rn))]
        while len(res) - 1 < cp["max_iterations"] and res[-1] > cp["tol"]:
            U, T, pp = pt
            _, _, sp2 = fold_border(m, U, T, pp, name2, v[:-1].reshape(M, -1), v[-1], w[:-1].reshape(M, -1))
            dR = np.concatenate([R.pack(R.dparam(m, U, T, pp, name2), 0.0), [sp2]])
            x1, x2 = Jsolve(pt, v, w, [g, dR])
            xiu, xip, N = theta, 1.0 - theta, x.size
            dl = (rn - xiu * float(tau[0] @ x1) / N) / (tau[1] * xip - xiu * float(tau[0] @ x2) / N)
            x = x - (x1 - dl * x2)
            p = p - dl
            g, v, w, pt = G_at(x, p, a, b)
            rn = Nf(x, p)
            res.append(max(R._norminf(g), abs(rn)))
        conv = res[-1] < cp["tol"]
        assert conv, res
        z_old, z = z, (x, p)
        ds_used = ds
        ds = R._step_size(ds, conv, len(res) - 1, cp)
        tau = R._secant(z, z_old, ds, theta)
        a, b = w / np.linalg.norm(w), v / np.linalg.norm(v)
        out["p1"].append(x[-1]); out["p2"].append(p); out["T"].append(x[-2]); out["amplitude"].append(amp(x))
        out["itnewton"].append(len(res) - 1); out["itlinear"].append(its_total[0])
    return out
