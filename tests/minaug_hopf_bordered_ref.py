"""CPU restatement of the complex bordered solve that stays regular at a Hopf point (src/codim2/MinAugHopf.jl:17, 72-76 handed to
MatrixFreeBLS with the left preconditioner diag(Pl, 1)) for the tests (test side only).  It extends tests/minaug_hopf_ref.py, whose
models and Newton loop -- direct solves of the same bordered systems -- it takes.

Complex vectors are numpy complex arrays here; the real-equivalent form the device iterates on stacks them as [re; im] with the
border scalar as the last two entries (re, im).

  trivial_case          the first Hopf point of u = 0 of tests/test_gpu_hopf.py (r* = -lam_11, omega = nu), a, b = mode + noise
  complex_matrix        [shift + J, a; kappa b^H, c], complex (N + 1), sparse
  direct_cbordered      its sparse direct solve
  PlCBordered           diag(Pl^-1, Pl^-1, 1, 1) on the real-equivalent (2N + 2) operator, and its right-hand side, as SciPy sees them
  cbordered_gmres       SciPy GMRES(restart) on that operator: (u, p, info, inner iterations, operator applications)
  elimination_gmres     SciPy GMRES on the real-equivalent Pl^-1 (shift + J) x = Pl^-1 a, a solve of the elimination path
  cresidual             2-norm of the residual of the UNpreconditioned complex system
  spectral_cbordered    the system at u = 0 in the DST-I basis, where J(0) is exactly block-diagonal
  krylov_solves         inside the block minaug_hopf_ref takes every solve from SciPy GMRES at the device's tolerance
"""
from __future__ import annotations

import contextlib

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import minaug_hopf_ref as R
from oracle import operators

PARS = dict(r=0.5, mu=0.1, nu=1.0, c3=-1.0, c5=1.0, gamma=0.0)


def dirichlet_eigenvalues(dims, ls):
    """lam_x[k] + lam_y[j] of the Dirichlet Laplacian, array axes (y, x): the symbol of oracle.operators.dst_block_preconditioner_cgl."""
    lam = []
    for n, l in zip(dims, ls):
        h = 2.0 * l / n
        lam.append(-(4.0 / h ** 2) * np.sin(np.pi * (np.arange(n) + 1) / (2.0 * (n + 1))) ** 2)
    return lam[1][:, None] + lam[0][None, :]


def hopf_mode(dims):
    """The eigenvector (phi, -i phi) of J(0) for lam_11 + r + i nu, phi the first sine mode, unit norm (complex, stacked fields)."""
    x = np.sin(np.pi * np.arange(1, dims[0] + 1) / (dims[0] + 1))
    y = np.sin(np.pi * np.arange(1, dims[1] + 1) / (dims[1] + 1))
    phi = np.outer(y, x).reshape(-1)
    phi = phi / (np.linalg.norm(phi) * np.sqrt(2.0))
    return np.concatenate([phi, -1j * phi])


def trivial_case(dims=(41, 21), ls=(np.pi, np.pi / 2), seed=7):
    """(op, r*, a, b): J(0, r) - i nu is singular exactly at r* = -lam_11; a, b = Hopf mode + 0.05 complex noise, normalised."""
    op = operators.CGL2d(dims, ls)
    rstar = float(-dirichlet_eigenvalues(dims, ls).max())
    z = hopf_mode(dims)
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(2):
        v = z + 0.05 * (rng.standard_normal(z.size) + 1j * rng.standard_normal(z.size)) / np.sqrt(2.0)
        out.append(v / np.linalg.norm(v))
    return op, rstar, out[0], out[1]


def stack(z):
    z = np.asarray(z, dtype=complex)
    return np.concatenate([z.real, z.imag])


def unstack(x):
    n = x.shape[0] // 2
    return x[:n] + 1j * x[n:]


def complex_matrix(J, a, b, c, kappa=1.0, shift=0.0):
    n = a.shape[0]
    Js = sp.csr_matrix(J).astype(complex) + complex(shift) * sp.identity(n, format="csr")
    return sp.bmat([[Js, sp.csr_matrix(np.asarray(a, dtype=complex).reshape(-1, 1))],
                    [sp.csr_matrix(kappa * np.conj(b).reshape(1, -1)), sp.csr_matrix(np.array([[complex(c)]]))]], format="csc")


def direct_cbordered(J, a, b, c, rhst, rhsb, kappa=1.0, shift=0.0):
    """[shift + J, a; kappa b^H, c][u; p] = [rhst; rhsb], complex sparse direct."""
    n = a.shape[0]
    y = spla.spsolve(complex_matrix(J, a, b, c, kappa, shift), np.append(np.asarray(rhst, dtype=complex), complex(rhsb)))
    return y[:n], complex(y[n])


def cresidual(J, a, b, c, rhst, rhsb, u, p, kappa=1.0, shift=0.0):
    r = np.append(np.asarray(rhst, dtype=complex), complex(rhsb)) - complex_matrix(J, a, b, c, kappa, shift) @ np.append(u, p)
    return float(np.linalg.norm(r))


class PlCBordered:
    """The real-equivalent operator on z = [xr; xi; pr; pi]:  top = Pl^-1 ((shift + J) x) + p atil with Pl^-1 on each half and
    atil = Pl^-1 a formed once, tail = kappa b^H x + c p;  rhs(rhst, rhsb) = (Pl^-1 rhst, rhsb)."""

    def __init__(self, J, a, b, c, pl, kappa=1.0, shift=0.0):
        self.J, self.b, self.c, self.pl, self.kappa, self.shift = J, np.asarray(b, dtype=complex), complex(c), pl, kappa, complex(shift)
        self.n = a.shape[0]
        self.atil = self.cpl(a)
        self.napply = 0

    def cpl(self, v):
        v = np.asarray(v, dtype=complex)
        return self.pl(v.real) + 1j * self.pl(v.imag)

    def __call__(self, z):
        self.napply += 1
        n = self.n
        x, p = z[:n] + 1j * z[n:2 * n], complex(z[2 * n], z[2 * n + 1])
        top = self.cpl(self.J @ x + self.shift * x) + p * self.atil
        t = self.kappa * np.vdot(self.b, x) + self.c * p
        return np.concatenate([top.real, top.imag, [t.real, t.imag]])

    def rhs(self, rhst, rhsb):
        t = self.cpl(rhst)
        return np.concatenate([t.real, t.imag, [complex(rhsb).real, complex(rhsb).imag]])

    def dense(self):
        """The (2N + 2) matrix, column by column (small grids)."""
        m = 2 * self.n + 2
        return np.column_stack([self(e) for e in np.eye(m)])


def _gmres(matvec, n, b, restart, maxiter, rtol, atol):
    count = [0]

    def cb(_):
        count[0] += 1
    x, info = spla.gmres(spla.LinearOperator((n, n), matvec=matvec, dtype=float), b, rtol=rtol, atol=atol, restart=restart,
                         maxiter=maxiter, callback=cb, callback_type="pr_norm")
    return x, info, count[0]


def cbordered_gmres(J, a, b, c, rhst, rhsb, pl, *, kappa=1.0, shift=0.0, restart=60, maxiter=10, rtol=1e-13, atol=0.0):
    """(u, p, info, inner iterations, operator applications) of SciPy GMRES(restart) x maxiter cycles on the real-equivalent
    left-preconditioned bordered system."""
    M = PlCBordered(J, a, b, c, pl, kappa, shift)
    z, info, it = _gmres(M, 2 * M.n + 2, M.rhs(rhst, rhsb), restart, maxiter, rtol, atol)
    n = M.n
    return z[:n] + 1j * z[n:2 * n], complex(z[2 * n], z[2 * n + 1]), info, it, M.napply


def elimination_gmres(J, a, pl, *, shift=0.0, restart=60, maxiter=10, rtol=1e-13):
    """(x, info, inner iterations, operator applications, true relative residual) of SciPy GMRES on the real-equivalent
    Pl^-1 (shift + J) x = Pl^-1 a: one of the two solves of a block elimination pass."""
    n = a.shape[0]
    cpl = lambda v: pl(v.real) + 1j * pl(v.imag)
    napply = [0]

    def mv(z):
        napply[0] += 1
        x = z[:n] + 1j * z[n:]
        return stack(cpl(J @ x + shift * x))
    z, info, it = _gmres(mv, 2 * n, stack(cpl(np.asarray(a, dtype=complex))), restart, maxiter, rtol, 0.0)
    x = unstack(z)
    return x, info, it, napply[0], float(np.linalg.norm(a - (J @ x + shift * x)) / np.linalg.norm(a))


def spectral_cbordered(dims, ls, r, nu, a, b, c, rhst, rhsb, kappa=1.0, shift=0.0, adjoint=False):
    """[shift + J(0), a; kappa b^H, c][u; p] = [rhst; rhsb] at u = 0 WITHOUT the assembled Laplacian: in the orthonormal DST-I basis
    J(0) = Lap (x) I_2 + [[r, -nu], [nu, r]] is the exact 2 x 2 block diag [[lam_k + r, -nu], [nu, lam_k + r]] (adjoint: nu -> -nu),
    so the system is an arrowhead matrix, solved with pivoting.  The second yardstick of the solver comparisons on the trivial
    state: the sparse direct solve works on a Laplacian rounded entry by entry."""
    import scipy.fft as sfft
    shape = tuple(int(d) for d in dims)[::-1]
    npts = int(np.prod(shape))

    def f(v, inv=False):
        v = np.asarray(v, dtype=complex)
        t = sfft.idstn if inv else sfft.dstn
        g = lambda q: t(q.reshape(shape), type=1, norm="ortho").reshape(-1)
        return np.concatenate([g(v[:npts].real) + 1j * g(v[:npts].imag), g(v[npts:].real) + 1j * g(v[npts:].imag)])
    m = (dirichlet_eigenvalues(dims, ls).reshape(-1) + r).astype(complex) + complex(shift)
    s = -nu if adjoint else nu
    D = sp.bmat([[sp.diags(m), -s * sp.identity(npts)], [s * sp.identity(npts), sp.diags(m)]], format="csr")
    y = spla.spsolve(complex_matrix(D, f(a), f(b), c, kappa, 0.0), np.append(f(rhst), complex(rhsb)))
    return f(y[:-1], inv=True), complex(y[-1])


@contextlib.contextmanager
def krylov_solves(pl, **gm):
    """Inside the block the restatement tests/minaug_hopf_ref.py (newton_hopf, continuation_hopf) takes its bordered vectors from
    cbordered_gmres and its real solves J \\ rhs from SciPy GMRES on Pl^-1 J x = Pl^-1 rhs, keywords ``gm`` (restart, maxiter, rtol):
    the device's path with hopf_bordered = 1, against which the direct restatement gives the yardstick's spread.  Yields the list
    of (info, inner iterations) of the solves."""
    log = []

    def bordered(A, a, b):
        n = a.shape[0]
        u, p, info, it, _ = cbordered_gmres(A, a, b, 0.0, np.zeros(n), 1.0, pl, **gm)
        log.append((info, it))
        return u, p

    def real(J, rhs):
        n = rhs.shape[0]
        x, info, it = _gmres(lambda v: pl(J @ v), n, pl(np.asarray(rhs, dtype=float)), gm.get("restart", 60), gm.get("maxiter", 10),
                             gm.get("rtol", 1e-13), 0.0)
        log.append((info, it))
        return x
    keep = R.bordered_solve_c, R.solve
    R.bordered_solve_c, R.solve = bordered, real
    try:
        yield log
    finally:
        R.bordered_solve_c, R.solve = keep
