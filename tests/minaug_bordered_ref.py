"""CPU restatement of the fold formulation on the bordered systems that stay regular at the fold (src/codim2/MinAugFold.jl:54-69
and :136-145, the branch without `usehessian`, handed to MatrixFreeBLS with the left preconditioner diag(Pl, 1)) for the tests
(test side only).  It extends tests/minaug_fold_ref.py, whose models (FoldModel, sh_model) it takes.

  border_row            sigma_x as a vector: -w h(x) v, so that <sigma_x, X> = -<w, d2F[v, X]>
  fold_matrix           the full fold Jacobian [J dpF; sigma_x' sigma_p], dense
  fold_linsolve_full    its direct solve (next to minaug_fold_ref.fold_linsolve, the elimination path)
  PlBordered            diag(Pl^-1, 1) [J + shift, a; kappa b', c] and its right-hand side as SciPy sees them
  bordered_gmres        SciPy GMRES(restart) on that operator: (u, p, info, inner iterations)
  singular_gmres        SciPy GMRES on Pl^-1 J x = Pl^-1 a, the solve of the elimination path
  newton_fold           newton_fold on the bordered path, every solve direct or through bordered_gmres
  trivial_case          the symmetry-breaking point of u = 0 of tests/test_gpu_fold.py::_trivial_singular_case, without a device
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import minaug_fold_ref as R
from oracle import operators, palc


def trivial_case(dims=(64, 64), ls=(np.pi, 1.3 * np.pi), seed=7):
    """(op, l*, a) on a box with unequal sides (a simple eigenvalue): J(0, l) = -L1 + l is singular exactly at l* = the smallest
    eigenvalue of L1 = (I + Lap)^2, diagonal in the DCT-II basis; a = mode + 0.05 noise, normalised."""
    op = operators.SwiftHohenberg(dims, ls)
    lam = [-(2 * n / (2 * L)) ** 2 * np.sin(np.pi * np.arange(n) / (2 * n)) ** 2 for n, L in zip(dims, ls)]
    L1 = (1 + lam[0][:, None] + lam[1][None, :]) ** 2
    i, j = np.unravel_index(np.argmin(L1), L1.shape)
    x = np.cos(np.pi * i * (np.arange(dims[0]) + 0.5) / dims[0])
    y = np.cos(np.pi * j * (np.arange(dims[1]) + 0.5) / dims[1])
    mode = np.outer(y, x).reshape(-1)
    mode /= np.linalg.norm(mode)
    a = mode + 0.05 * np.random.default_rng(seed).standard_normal(mode.size)
    return op, float(L1[i, j]), a / np.linalg.norm(a)


def border_row(kind, nu, x, v, w):
    h, _ = R.sh_polys(kind, nu, 0)
    return -((w * R.horner(h, x)) * v)


def _terms(model, x, q, v, w, kind):
    names = list(model.pars)
    sigx = border_row(kind, q[names[1]], x, v, w)
    sigp = -np.dot(w, model.dJvdp(x, q, model.lens1, v))
    return sigx, sigp, model.dFdp(x, q, model.lens1)


def fold_matrix(model, x, q, v, w, kind):
    sigx, sigp, dpF = _terms(model, x, q, v, w, kind)
    J = model.J(x, q)
    J = J.toarray() if sp.issparse(J) else np.asarray(J)
    return np.block([[J, dpF.reshape(-1, 1)], [sigx.reshape(1, -1), np.array([[sigp]])]])


def fold_linsolve_full(model, x, q, v, w, rhsu, rhsp, kind):
    y = np.linalg.solve(fold_matrix(model, x, q, v, w, kind), np.append(rhsu, rhsp))
    return y[:-1], y[-1]


def direct_bordered(J, a, b, c, rhst, rhsb, kappa=1.0, shift=0.0):
    """[J + shift, a; kappa b', c][u; p] = [rhst; rhsb], sparse direct."""
    n = a.shape[0]
    Js = sp.csr_matrix(J) + shift * sp.identity(n, format="csr")
    M = sp.bmat([[Js, sp.csr_matrix(a.reshape(-1, 1))], [sp.csr_matrix(kappa * b.reshape(1, -1)), sp.csr_matrix([[c]])]], format="csc")
    y = spla.spsolve(M, np.append(rhst, rhsb))
    return y[:n], y[n]


class PlBordered:
    """diag(Pl^-1, 1) [J + shift, a; kappa b', c] with atil = Pl^-1 a formed once; rhs(rhst, rhsb) = (Pl^-1 rhst, rhsb)."""

    def __init__(self, J, a, b, c, pl, kappa=1.0, shift=0.0):
        self.J, self.b, self.c, self.pl, self.kappa, self.shift = J, b, float(c), pl, kappa, shift
        self.a = a
        self.atil = pl(a)
        self.n = a.shape[0]

    def __call__(self, z):
        u, p = z[:-1], z[-1]
        top = self.pl(self.J @ u + self.shift * u) + p * self.atil
        return np.append(top, self.kappa * np.dot(self.b, u) + self.c * p)

    def rhs(self, rhst, rhsb):
        return np.append(self.pl(rhst), rhsb)

    def unpreconditioned(self, z):
        u, p = z[:-1], z[-1]
        return np.append(self.J @ u + self.shift * u + p * self.a, self.kappa * np.dot(self.b, u) + self.c * p)


def _gmres(matvec, n, b, restart, maxiter, rtol, atol):
    count = [0]

    def cb(_):
        count[0] += 1
    x, info = spla.gmres(spla.LinearOperator((n, n), matvec=matvec, dtype=float), b, rtol=rtol, atol=atol, restart=restart,
                         maxiter=maxiter, callback=cb, callback_type="pr_norm")
    return x, info, count[0]


def bordered_gmres(J, a, b, c, rhst, rhsb, pl, *, kappa=1.0, shift=0.0, restart=40, maxiter=50, rtol=1e-10, atol=0.0):
    """(u, p, info, inner iterations) of SciPy GMRES(restart) x maxiter cycles on the left-preconditioned bordered system."""
    M = PlBordered(J, a, b, c, pl, kappa, shift)
    z, info, it = _gmres(M, M.n + 1, M.rhs(rhst, rhsb), restart, maxiter, rtol, atol)
    return z[:-1], z[-1], info, it


def singular_gmres(J, a, pl, *, restart=40, maxiter=50, rtol=1e-10):
    """(x, info, inner iterations, true relative residual |a - J x| / |a|) of SciPy GMRES on Pl^-1 J x = Pl^-1 a."""
    x, info, it = _gmres(lambda u: pl(J @ u), a.shape[0], pl(a), restart, maxiter, rtol, 0.0)
    return x, info, it, np.linalg.norm(a - J @ x) / np.linalg.norm(a)


def newton_fold(model, x0, p0, a, b, kind, *, pl=None, tol=1e-12, max_iterations=25, normN=palc.norm2, gm=None):
    """newton_fold on the bordered path.  pl = None: every bordered solve direct; else SciPy GMRES with the keywords ``gm`` on the
    left-preconditioned systems.  dict(u, p, residuals, converged, itnewton, v, w, sigma, itlinear, flags)."""
    gm = gm or {}
    its, flags = [], []

    def bsolve(J, col, row, c, rhst, rhsb):
        if pl is None:
            return direct_bordered(J, col, row, c, rhst, rhsb)
        u, p, info, it = bordered_gmres(J, col, row, c, rhst, rhsb, pl, **gm)
        its.append(it)
        flags.append(info == 0)
        return u, p

    def G(x, p):
        q = model.at(p)
        J = model.J(x, q)
        zero = np.zeros_like(x)
        v, sigma = bsolve(J, a, b, 0.0, zero, 1.0)
        w = v if a is b else bsolve(model.Jt(x, q), b, a, 0.0, zero, 1.0)[0]
        return model.F(x, q), sigma, v, w

    x, p = np.asarray(x0, dtype=float).copy(), float(p0)
    F, sigma, v, w = G(x, p)
    res = [normN(np.append(F, sigma))]
    step = 0
    while step < max_iterations and res[-1] > tol:
        q = model.at(p)
        sigx, sigp, dpF = _terms(model, x, q, v, w, kind)
        dX, dsig = bsolve(model.J(x, q), dpF, sigx, sigp, F, sigma)
        x, p = x - dX, p - dsig
        F, sigma, v, w = G(x, p)
        res.append(normN(np.append(F, sigma)))
        step += 1
    return dict(u=x, p=p, residuals=res, converged=res[-1] < tol, itnewton=step, v=v, w=w, sigma=sigma, itlinear=sum(its),
                flags=flags)


def tmode_matrices(T, Jd, Pinv, a, b, c, kappa, alpha0, alpha1):
    """Dense (alpha0 I + alpha1 M', diag(Pl^-1, 1) [J a; kappa b' c]) for a stencil-free T with Pl^-1 J = alpha0 I + alpha1 T, the
    border of M' handed over as the device code does: columns atil / alpha1, rows kappa b / alpha1, block (c - alpha0) / alpha1."""
    n = Jd.shape[0]
    atil = Pinv @ a
    Mp = np.block([[T, (atil / alpha1).reshape(-1, 1)], [(kappa * b / alpha1).reshape(1, -1), np.array([[(c - alpha0) / alpha1]])]])
    lhs = alpha0 * np.eye(n + 1) + alpha1 * Mp
    full = np.block([[Jd, a.reshape(-1, 1)], [kappa * b.reshape(1, -1), np.array([[c]])]])
    D = np.block([[Pinv, np.zeros((n, 1))], [np.zeros((1, n)), np.ones((1, 1))]])
    return lhs, D @ full


NU_HEX = 1.2
_HEX = {}


def hex_fold_case():
    """The hexagon fold of tests/test_gpu_fold.py::hex_branch, rebuilt the same way (without its fine-step branch): the z-invariant
    hexagons of tests/golden/bench_cell_states.npz reflected once in y, 64 x 64, continued in l by the CPU oracle past the first
    fold.  dict(op, dims, ls, br, k); computed once per process."""
    if _HEX:
        return _HEX
    import os
    from oracle import bordered
    d = np.load(os.path.join(os.path.dirname(__file__), "golden", "bench_cell_states.npz"))
    cx, cy, cz = (int(c) for c in d["cell"])
    u2 = d["u0"].reshape(cz, cy, cx)[0]
    u = np.concatenate([u2, u2[::-1]], axis=0).reshape(-1)
    dims, ls = (cx, 2 * cy), (float(d["cell_l"][0]), 2 * float(d["cell_l"][1]))
    op = operators.SwiftHohenberg(dims, ls)
    prob = palc.Problem(lambda x, p: op.F(x, p, NU_HEX), lambda x, p: op.J(x, p, NU_HEX), dparam_factor=lambda x, p: x)
    bls = lambda *a, **k: bordered.bordering_bls(bordered.default_ls, *a, check_precision=False, **k)
    br = palc.continuation(prob, u, float(d["p0"]), ds=-0.01, dsmax=0.02, max_steps=20, ls=bordered.default_ls, bls=bls, dsmin=1e-5,
                           p_min=-1.0, p_max=1.0, keep_solutions=True, normC=palc.norminf, tol=1e-11)
    dp = np.diff(br.param)
    k = [i for i in range(len(dp) - 1) if dp[i] * dp[i + 1] < 0][0] + 1
    _HEX.update(op=op, dims=dims, ls=ls, br=br, k=k)
    return _HEX


def hex_fold_guess(hb):
    """(x, p, zeta) as codim2.fold_point gives them on that branch: the middle point of the turn, zeta = the normalised difference
    of its neighbours."""
    k = hb["k"]
    tau = hb["br"].sol[k + 1] - hb["br"].sol[k - 1]
    return hb["br"].sol[k], float(hb["br"].param[k]), tau / np.linalg.norm(tau)


# ---------------------------------------------------------------------------------------------- m-column border
def direct_block(J, A, Bm, Cm, rhst, rhsb, kappa=1.0, shift=0.0):
    """[J + shift, A; kappa B', C][u1; u2] = [rhst; rhsb] with A, B n x m and C m x m, sparse direct."""
    n, m = A.shape
    Js = sp.csr_matrix(J) + shift * sp.identity(n, format="csr")
    M = sp.bmat([[Js, sp.csr_matrix(A)], [sp.csr_matrix(kappa * Bm.T), sp.csr_matrix(Cm)]], format="csc")
    y = spla.spsolve(M, np.concatenate([rhst, rhsb]))
    return y[:n], y[n:]


def block_gmres(J, A, Bm, Cm, rhst, rhsb, pl, *, kappa=1.0, shift=0.0, restart=40, maxiter=50, rtol=1e-10, atol=0.0):
    """(u1, u2, info, inner iterations) of SciPy GMRES on diag(Pl^-1, I_m) [J + shift, A; kappa B', C], Atil = Pl^-1 A formed once."""
    n, m = A.shape
    At = np.column_stack([pl(A[:, j]) for j in range(m)])

    def mv(z):
        u, p = z[:n], z[n:]
        return np.concatenate([pl(J @ u + shift * u) + At @ p, kappa * (Bm.T @ u) + Cm @ p])
    z, info, it = _gmres(mv, n + m, np.concatenate([pl(rhst), rhsb]), restart, maxiter, rtol, atol)
    return z[:n], z[n:], info, it


def block_residual(J, A, Bm, Cm, rhst, rhsb, u1, u2, kappa=1.0, shift=0.0):
    """2-norm of the residual of the UNpreconditioned bordered system at (u1, u2)."""
    u2 = np.atleast_1d(u2)
    rt = rhst - (J @ u1 + shift * u1 + A @ u2)
    rb = np.atleast_1d(rhsb) - (kappa * (Bm.T @ u1) + np.atleast_2d(Cm) @ u2)
    return float(np.sqrt(np.dot(rt, rt) + np.dot(rb, rb)))


# ---------------------------------------------------------------------------------------------- the trivial state in the DCT basis
def spectral_block(dims, ls, l, A, Bm, Cm, rhst, rhsb, kappa=1.0, shift=0.0):
    """[J + shift, A; kappa B', C][u1; u2] = [rhst; rhsb] at x = 0 WITHOUT the assembled matrix: J(0, l) = -L1 + l is
    diag(l - symbol) in the orthonormal DCT-II basis (oracle.operators.dct_symbol), so the system is an arrowhead matrix with an
    exact diagonal, solved with pivoting (no division by l - symbol, which vanishes at the singular point).  The second yardstick of
    the solver comparisons on the trivial state: the sparse direct solve works on L1 = A A rounded entry by entry, and at a
    near-singular J that rounding moves the border scalars by more than two Krylov solves of the SAME matrix differ."""
    import scipy.fft as sfft
    shape = tuple(int(d) for d in dims)[::-1]
    f = lambda v: sfft.dctn(np.asarray(v, dtype=float).reshape(shape), type=2, norm="ortho").reshape(-1)
    A, Bm, Cm = np.atleast_2d(A.T).T, np.atleast_2d(Bm.T).T, np.atleast_2d(Cm)
    n, m = A.shape
    D = sp.diags((l + shift) - operators.dct_symbol(dims, ls, 0.0).reshape(-1))
    Ah = np.column_stack([f(A[:, j]) for j in range(m)])
    Bh = np.column_stack([f(Bm[:, j]) for j in range(m)])
    M = sp.bmat([[D, sp.csr_matrix(Ah)], [sp.csr_matrix(kappa * Bh.T), sp.csr_matrix(Cm)]], format="csc")
    y = spla.spsolve(M, np.concatenate([f(rhst), np.atleast_1d(rhsb)]))
    return sfft.idctn(y[:n].reshape(shape), type=2, norm="ortho").reshape(-1), y[n:]
