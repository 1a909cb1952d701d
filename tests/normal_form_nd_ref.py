"""CPU restatement of the normal form at a branch point with an N-dimensional kernel, get_normal_formNd
(src/NormalForms.jl:648-896), of the record's reduced equation (:541-574) and of predictor(::NdBranchPoint) (:916-985) for the
tests (test side only).

Generic over minaug_fold_ref.FoldModel (F, J, d2F, dFdp, dJvdp) plus a trilinear ``d3F(x, q, a, b, c)`` and separate adjoint
kernel vectors zeta*: with Z = (zeta_0 ... zeta_{N-1}), Z* alike, <zeta_i, zeta*_j> = delta_ij and E(r) = r - Z (Z*' r), the
bordered system [J Z*; Z' 0][Psi; s] = [E(R); 0] (:759-763, with all N columns) is solved directly as the (n + N) matrix, so the
restatement carries no Krylov tolerance; ``solver="gmres"`` solves the same system by SciPy GMRES left-preconditioned by
diag(Pl, I) and stopped on the preconditioned residual at ``reltol`` -- the yardstick of the solver-dependent tolerances of the
GPU tests.

    a01[i]       = <dpF, zeta*_i>                                         Psi01: E(-dpF)
    b20[i,j,k]   = <d2F[zeta_j, zeta_k], zeta*_i>                         Psijk: E(-d2F[zeta_j, zeta_k])
    b11[i,j]     = <dJ/dp zeta_j + d2F[zeta_j, Psi01], zeta*_i>
    a02[i]       = <2 dJ/dp Psi01 + d2F[Psi01, Psi01], zeta*_i>           (d2F/dp2 = 0 for every model here)
    b30[i,j,k,l] = <d3F[zeta_j, zeta_k, zeta_l] + d2F[zeta_j, Psikl] + d2F[zeta_k, Psijl] + d2F[zeta_l, Psijk], zeta*_i>
"""
from __future__ import annotations

import itertools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from minaug_fold_ref import FoldModel, horner, sh_polys, solve
from normal_form1d_ref import sh_d3_poly, sh_dp_poly

TOL_FOLD = 1e-3


def pairs(N):
    return [(j, k) for j in range(N) for k in range(j, N)]


def triples(N):
    return [(j, k, l) for j in range(N) for k in range(j, N) for l in range(k, N)]


def bordered_matrix(J, Zs, Z):
    """[J Z*; Z' 0], dense or sparse as J is."""
    N = Z.shape[1]
    if sp.issparse(J):
        return sp.bmat([[J, sp.csr_matrix(Zs)], [sp.csr_matrix(Z.T), sp.csr_matrix((N, N))]], format="csc")
    return np.block([[np.asarray(J), Zs], [Z.T, np.zeros((N, N))]])


def bordered_direct(B, R, N):
    n = R.shape[0]
    return solve(B, np.concatenate([R, np.zeros(N)]))[:n]


def bordered_gmres(B, R, N, reltol, Pl, restart=40, maxiter=50):
    """The same system by SciPy GMRES on diag(Pl, I) B, stopped on the preconditioned residual at ``reltol``."""
    n = R.shape[0]
    pre = lambda v: np.concatenate([Pl(v[:n]), v[n:]])
    A = spla.LinearOperator((n + N, n + N), matvec=lambda v: pre(B @ v))
    x, _ = spla.gmres(A, pre(np.concatenate([R, np.zeros(N)])), rtol=reltol, atol=0.0, restart=restart, maxiter=maxiter)
    return x[:n]


def normal_form_nd(model, d3F, x, q, lens, zetas, zeta_stars=None, solver="direct", reltol=None, Pl=None, tol_fold=TOL_FOLD,
                   **gmres_kw):
    """dict(a01[N], a02[N], b11[N,N], b20[N,N,N], b30[N,N,N,N], Psi01, Psi2 = {(j,k): Psijk}, rhs, type, B) at (x, q) for the
    parameter ``lens``.  ``zeta_stars`` None: zeta* = zeta (symmetric J)."""
    Z = np.stack([np.asarray(z, dtype=float) for z in zetas], axis=1)
    Zs = Z if zeta_stars is None else np.stack([np.asarray(z, dtype=float) for z in zeta_stars], axis=1)
    n, N = Z.shape
    gram = Zs.T @ Z
    if not np.abs(gram - np.eye(N)).max() <= 1e-8:
        raise ValueError(f"the kernel bases are not biorthonormal: {gram}")
    J = model.J(x, q)
    B = bordered_matrix(J, Zs, Z)
    E = lambda r: r - Z @ (Zs.T @ r)
    if solver == "direct":
        bls = lambda R: bordered_direct(B, R, N)
    else:
        bls = lambda R: bordered_gmres(B, R, N, reltol, Pl, **gmres_kw)
    z = [Z[:, i] for i in range(N)]
    R01 = np.asarray(model.dFdp(x, q, lens), dtype=float)
    a01 = Zs.T @ R01
    r01 = E(-R01)
    Psi01 = bls(r01)
    b11 = np.zeros((N, N))
    for j in range(N):
        b11[:, j] = Zs.T @ (model.dJvdp(x, q, lens, z[j]) + model.d2F(x, q, z[j], Psi01))
    a02 = Zs.T @ (2 * model.dJvdp(x, q, lens, Psi01) + model.d2F(x, q, Psi01, Psi01))
    b20 = np.zeros((N, N, N))
    Psi2, rhs = {}, [r01]
    for j, k in pairs(N):
        b2v = model.d2F(x, q, z[j], z[k])
        b20[:, j, k] = b20[:, k, j] = Zs.T @ b2v
        rhs.append(E(-b2v))
        Psi2[(j, k)] = bls(rhs[-1])
    P2 = lambda j, k: Psi2[(min(j, k), max(j, k))]
    b30 = np.zeros((N, N, N, N))
    for j, k, l in triples(N):
        b3v = (d3F(x, q, z[j], z[k], z[l]) + model.d2F(x, q, z[j], P2(k, l)) + model.d2F(x, q, z[k], P2(j, l))
               + model.d2F(x, q, z[l], P2(j, k)))
        c = Zs.T @ b3v
        for I in set(itertools.permutations((j, k, l))):
            b30[(slice(None),) + I] = c
    kind = "NonQuadraticParameter" if max(np.abs(a01).max(), np.abs(a02).max(), np.abs(b11).max()) < tol_fold else f"{N}-d"
    return dict(a01=a01, a02=a02, b11=b11, b20=b20, b30=b30, Psi01=Psi01, Psi2=Psi2, rhs=rhs, type=kind, B=B, N=N)


def pack(nf):
    """The device's packed layouts: (a01[N], a02[N], b11[N, N], b20[N, P], b30[N, T])."""
    N = nf["N"]
    return (nf["a01"], nf["a02"], nf["b11"], np.stack([nf["b20"][:, j, k] for j, k in pairs(N)], axis=1),
            np.stack([nf["b30"][:, j, k, l] for j, k, l in triples(N)], axis=1))


def rotate(nf, Rm):
    """The coefficient arrays in the basis zeta'_i = sum_a Rm[i, a] zeta_a (Rm orthogonal, zeta* = zeta), index by index."""
    return dict(a01=Rm @ nf["a01"], a02=Rm @ nf["a02"], b11=np.einsum("ia,jb,ab->ij", Rm, Rm, nf["b11"]),
                b20=np.einsum("ia,jb,kc,abc->ijk", Rm, Rm, Rm, nf["b20"]),
                b30=np.einsum("ia,jb,kc,ld,abcd->ijkl", Rm, Rm, Rm, Rm, nf["b30"]))


# ---------------------------------------------------------------------------------------------- reduced equation, predictor
def reduced_form(nf, x, dp):
    """(bp::NdBranchPoint)(Val(:reducedForm), x, p) (:541-574), loops as the reference writes them (its a02 term carries a
    factor 0 p, :554; the term is kept here, as the reduced equation states it)."""
    N = len(nf["a01"])
    out = np.zeros(N)
    for i in range(N):
        out[i] = dp * (nf["a01"][i] + dp * nf["a02"][i] / 2)
        for j in range(N):
            out[i] += dp * nf["b11"][i, j] * x[j]
            for k in range(N):
                out[i] += nf["b20"][i, j, k] * x[j] * x[k] / 2
                for l in range(N):
                    out[i] += nf["b30"][i, j, k, l] * x[j] * x[k] * x[l] / 6
    return out


def reduced_jacobian(nf, x, dp):
    return dp * nf["b11"] + np.einsum("imk,k->im", nf["b20"], x) + np.einsum("imkl,k,l->im", nf["b30"], x, x) / 2


def deflation(x, roots, power=2, shift=0.1):
    """M(x) = prod_r (<x - r, x - r>^-power + shift) and grad M (DeflationOperator(2, 0.1, [0]), :920)."""
    M, g = 1.0, np.zeros_like(x)
    for r in roots:
        d = x - r
        dd = float(d @ d)
        if dd < 1e-100:                                  # on a deflated zero: M is infinite, the iteration stops unconverged
            return np.inf, g
        m = dd ** -power + shift
        g = g * m + M * (-2.0 * power * dd ** (-power - 1)) * d
        M *= m
    return M, g


def polish(F, J, x, steps=3):
    """The deflated residual M F < tol leaves F itself only as small as tol / M: a few plain Newton steps on the reduced equation
    from the zero the deflated iteration found, kept when they stay at that zero (moved by less than 1e-3 (1 + |x|))."""
    y = x.copy()
    for _ in range(steps):
        try:
            y = y - np.linalg.solve(J(y), F(y))
        except np.linalg.LinAlgError:
            return x
    return y if np.all(np.isfinite(y)) and np.abs(y - x).max() <= 1e-3 * (1 + np.abs(x).max()) else x


def default_igs(N):
    """The vertices of {-1, 0, 1}^N in the order of Iterators.product (:938), then the same vertices at twice the size: a second,
    deterministic shell of starts in place of the random restarts."""
    v = [c[::-1] for c in itertools.product((-1, 0, 1), repeat=N)]
    return [tuple(a * x for x in c) for a in (1.0, 2.0) for c in v]


def predictor(nf, dp, ampfactor=1.0, igs=None, amp_igs=1.0, maxiter=100, tol=1e-10, scale=None):
    """predictor(bp::NdBranchPoint, dp) (:916-985) without the random restarts of :966-976: deflated Newton (exact Jacobian,
    infinity norm, tolerance 1e-10 of NewtonPar) from the vertices of {-1, 0, 1}^N and of {-2, 0, 2}^N (default_igs).  A zero
    counts when the deflated and the plain residual are both below ``tol`` and is then polished on the plain reduced equation.
    The iteration runs on y = x / scale with the residual in units of scale |dp| (deflation distances of order one); the
    default scale is sqrt |dp|, scale = 1 the reference's iteration."""
    N = len(nf["a01"])
    if scale is None:
        scale = np.sqrt(abs(dp)) if dp != 0 else 1.0
    if igs is None:
        igs = default_igs(N)

    def side(d):
        unit = 1.0 if scale == 1.0 else scale * abs(d)
        F = lambda y: reduced_form(nf, scale * y, d) / unit
        J = lambda y: reduced_jacobian(nf, scale * y, d) * (scale / unit)
        roots = [np.zeros(N)]
        for ci in igs:
            x = np.asarray(ci, dtype=float) * amp_igs
            if not np.linalg.norm(x) > 0:
                continue
            ok = False
            for it in range(maxiter + 1):
                M, g = deflation(x, roots)
                if not np.isfinite(M):
                    break
                f = F(x)
                G = M * f
                res = np.abs(G).max()
                if not np.isfinite(res) or res > 1e100:
                    break
                if res < tol and np.abs(f).max() < tol:          # far from every zero M is as small as shift^roots: F itself too
                    ok = True
                    break
                if it == maxiter:
                    break
                try:
                    x = x - np.linalg.solve(M * J(x) + np.outer(f, g), G)
                except np.linalg.LinAlgError:
                    break
            if ok:
                roots.append(polish(F, J, x))
        return [ampfactor * scale * r for r in roots]

    return dict(before=side(-abs(dp)), after=side(abs(dp)))


# ---------------------------------------------------------------------------------------------- polynomial models
def cubic_model(F, pars, lens):
    """FoldModel and d3F of a vector field F(x, pars) that is a polynomial of degree <= 3 in x and affine in pars[lens], by exact
    polarisation (no step size): with G(v) = F(x + v), the odd part o(v) = (G(v) - G(-v)) / 2 = J v + C(v) / 6 and the even part
    (G(v) + G(-v)) / 2 - G(0) = Q(v) / 2 give C(v) = o(2 v) - 2 o(v), d2F[a, b] = (Q(a + b) - Q(a - b)) / 4 and
    d3F[a, b, c] = (C(a + b + c) - C(a + b - c) - C(a - b + c) - C(-a + b + c)) / 24."""
    odd = lambda x, q, v: (F(x + v, q) - F(x - v, q)) / 2
    Q = lambda x, q, v: (F(x + v, q) + F(x - v, q)) - 2 * F(x, q)
    Cc = lambda x, q, v: odd(x, q, 2 * v) - 2 * odd(x, q, v)

    def Jv(x, q, v):
        return odd(x, q, v) - Cc(x, q, v) / 6

    def J(x, q):
        n = x.shape[0]
        return np.stack([Jv(x, q, e) for e in np.eye(n)], axis=1)

    def up(q):
        q1 = dict(q)
        q1[lens] += 1.0
        return q1

    d2F = lambda x, q, a, b: (Q(x, q, a + b) - Q(x, q, a - b)) / 4
    d3F = lambda x, q, a, b, c: (Cc(x, q, a + b + c) - Cc(x, q, a + b - c) - Cc(x, q, a - b + c) - Cc(x, q, -a + b + c)) / 24
    model = FoldModel(F, J, d2F, pars, lens, dFdp=lambda x, q, l: F(x, up(q)) - F(x, q),
                      dJvdp=lambda x, q, l, v: Jv(x, up(q), v) - Jv(x, q, v))
    return model, d3F


def Fbp2d(x, p):
    """test/normal_forms/testNF.jl:224-229"""
    return np.array([p["alpha"] * x[0] * (3.23 * p["mu"] + p["A"] * x[0] ** 2 + p["B"] * x[1] ** 2) + x[2],
                     p["alpha"] * x[1] * (3.23 * p["mu"] + p["C"] * x[0] ** 2 + p["A"] * x[1] ** 2),
                     -x[2] + p["gamma"] * (x[0] ** 3 + x[1] ** 2)])


def FbpD6(x, p):
    """test/normal_forms/testNF.jl:327-331"""
    mu, a, b, c = p["mu"], p["a"], p["b"], p["c"]
    return np.array([mu * x[0] + (a * x[1] * x[2] - b * x[0] ** 3 - c * (x[1] ** 2 + x[2] ** 2) * x[0]),
                     mu * x[1] + (a * x[0] * x[2] - b * x[1] ** 3 - c * (x[2] ** 2 + x[0] ** 2) * x[1]),
                     mu * x[2] + (a * x[0] * x[1] - b * x[2] ** 3 - c * (x[1] ** 2 + x[0] ** 2) * x[2])])


# ---------------------------------------------------------------------------------------------- Swift-Hohenberg pieces
def sh_mu(dims, ls):
    """Eigenvalues of the 1-D Neumann-ghost second differences per axis (oracle.operators.second_difference, h = 2 l / N)."""
    return [-(2 * n / (2 * L)) ** 2 * np.sin(np.pi * np.arange(n) / (2 * n)) ** 2 for n, L in zip(dims, ls)]


def sh_cos_mode(dims, ls, m):
    """(l*, zeta) of the cosine mode m = (m_x, m_y[, m_z]) of u = 0 of 2-D / 3-D SH on the grid ``dims`` (x fastest):
    J = -L1 + l has the eigenvalue l - (1 + sum_a mu_a[m_a])^2 on it."""
    mu = sh_mu(dims, ls)
    z = np.ones(1)
    for n, ma in zip(dims, m):                                   # x fastest: later axes are the outer factors
        z = np.kron(np.cos(np.pi * ma * (np.arange(n) + 0.5) / n), z)
    return float((1 + sum(mu[a][ma] for a, ma in enumerate(m))) ** 2), z / np.linalg.norm(z)


def sh_cos_closed_form_diag(dims, ls, m, nu):
    """b30[i, i, i, i] at the point of sh_cos_mode for the mode m alone, in closed form (2 m_a < n_a on every axis): with k active
    axes (m_a > 0), zeta^2 = c^2 2^-k sum over the subsets S of the active axes of phi_S = prod_{a in S} cos(2 m_a theta_a), each
    an eigenvector of J with eigenvalue lam_S = l* - (1 + sum_{a in S} mu_a[2 m_a])^2 and orthogonal to the kernel, so
    Psi_ii = -2 nu sum_S w phi_S / lam_S and b30 = -6 sum zeta^4 - 12 nu^2 sum_S w^2 |phi_S|^2 / lam_S, w = c^2 2^-k."""
    mu = sh_mu(dims, ls)
    lstar, _ = sh_cos_mode(dims, ls, m)
    act = [a for a, ma in enumerate(m) if ma > 0]
    assert all(2 * m[a] < dims[a] for a in act)
    ntot = float(np.prod(dims))
    c2 = 2.0 ** len(act) / ntot
    w = c2 / 2.0 ** len(act)
    z4 = c2 * c2 * ntot * (3.0 / 8.0) ** len(act)
    s = 0.0
    for r in range(len(act) + 1):
        for S in itertools.combinations(act, r):
            lam = lstar - (1 + sum(mu[a][2 * m[a]] for a in S)) ** 2
            s += w * w * ntot / 2.0 ** len(S) / lam
    return -6.0 * z4 - 12.0 * nu * nu * s


def sh_symbol(dims, ls):
    """(1 + sum_a mu_a)^2 on every cosine mode, flat."""
    mu = sh_mu(dims, ls)
    s = np.zeros(1)
    for m_ in mu:
        s = (m_[:, None] + s[None, :]).reshape(-1)
    return (1 + s) ** 2


def dots_terms(kind, nu, ip, u, zs):
    """The per-point terms of bk_nfnd_dots in the kernel's operation order: (a01[N], b20[N, P], Gram[N, N]) as lists of arrays."""
    N = len(zs)
    h, _ = sh_polys(kind, nu, ip)
    f = sh_dp_poly(kind, ip)
    H, Fv = horner(h, u), horner(f, u)
    a01 = [Fv * zs[i] for i in range(N)]
    b20 = [[((H * zs[j]) * zs[k]) * zs[i] for j, k in pairs(N)] for i in range(N)]
    gram = [[zs[i] * zs[j] for j in range(N)] for i in range(N)]
    return a01, b20, gram


def rhs_exact(kind, nu, ip, u, zs, a01, b20p):
    """bk_nfnd_rhs in the kernel's operation order (bit for bit in IEEE double without contraction)."""
    N = len(zs)
    h, _ = sh_polys(kind, nu, ip)
    f = sh_dp_poly(kind, ip)
    H, Fv = horner(h, u), horner(f, u)
    s = a01[0] * zs[0]
    for i in range(1, N):
        s = s + a01[i] * zs[i]
    out = [s - Fv]
    for q, (j, k) in enumerate(pairs(N)):
        r = b20p[0][q] * zs[0]
        for i in range(1, N):
            r = r + b20p[i][q] * zs[i]
        out.append(r - (H * zs[j]) * zs[k])
    return out


def contract_terms(kind, nu, ip, u, zs, p, qs):
    """... of bk_nfnd_contract: (b11[N, N], a02[N], b30[N, T]); ``qs`` the P vectors Psijk in pair order."""
    N = len(zs)
    h, g = sh_polys(kind, nu, ip)
    t = sh_d3_poly(kind, nu)
    H, G, T = horner(h, u), horner(g, u), horner(t, u)
    hz = [H * z for z in zs]
    pi = {jk: n_ for n_, jk in enumerate(pairs(N))}
    b11 = [[(G * zs[j] + hz[j] * p) * zs[i] for j in range(N)] for i in range(N)]
    a = 2.0 * (G * p) + (H * p) * p
    a02 = [a * zs[i] for i in range(N)]
    br = [((T * zs[j]) * zs[k]) * zs[l] + ((hz[j] * qs[pi[(k, l)]] + hz[k] * qs[pi[(j, l)]]) + hz[l] * qs[pi[(j, k)]])
          for j, k, l in triples(N)]
    b30 = [[b * zs[i] for b in br] for i in range(N)]
    return b11, a02, b30
