"""Normal forms at branch points whose kernel has dimension N = 2 or 3, and their predictor, for the Swift-Hohenberg problems
(SwiftHohenberg 2-D / 3-D, SwiftHohenberg1D): get_normal_formNd (src/NormalForms.jl:648-896), the NdBranchPoint record
(:541-582) and predictor(::NdBranchPoint) (:916-985), matrix-free on the preconditioned bordered GMRES solve.

  nfnd_dots, nfnd_rhs, nfnd_contract   the device passes (bk_nfnd_dots, bk_nfnd_rhs, bk_nfnd_contract)
  normal_form_nd           the computation call by call on the plugin surface: the three passes and 1 + P block solves of
                           MatrixFreeBLS(ls, use_pl=True)
  normal_form_nd_native    the same as one library call (bk_normal_form_nd)
  get_normal_form_nd       for a point of type "nd" of a native branch
  predictor                the zeros of the reduced equation on both sides of the point, deflated Newton on the host
  predicted_states         x0 + sum_i x_i zeta_i for a list of zeros (bk_nf1d_predict)
  get_first_points_on_branch   the predicted zeros turned into zeros of F on both sides, deflated Newton with the exact dM
  multicontinuation        normal form -> predictor -> first points -> one branch per state found

J' = J, the reference's is_symmetric branch: zeta*_i = zeta_i, and biorthogonalise reduces to orthonormalising the kernel basis
zeta_0 .. zeta_{N-1}.  With E(r) = r - sum_i <r, zeta_i> zeta_i and B = [J Z; Z' 0], Z = (zeta_0 ... zeta_{N-1}):

  a01[i]       = <dpF, zeta_i>                                          Psi01: B [Psi01; s] = [E(-dpF); 0]
  b20[i,j,k]   = <d2F[zeta_j, zeta_k], zeta_i>                          Psijk: B [Psijk; s] = [E(-d2F[zeta_j, zeta_k]); 0]
  b11[i,j]     = <dJ/dp zeta_j + d2F[zeta_j, Psi01], zeta_i>
  a02[i]       = <2 dJ/dp Psi01 + d2F[Psi01, Psi01], zeta_i>            (d2F/dp2 = 0 for these problems)
  b30[i,j,k,l] = <d3F[zeta_j, zeta_k, zeta_l] + d2F[zeta_j, Psikl] + d2F[zeta_k, Psijl] + d2F[zeta_l, Psijk], zeta_i>

in the reduced equation  a01 dp + a02 dp^2 / 2 + b11 x dp + b20 x x / 2 + b30 x x x / 6.  The device works on the P = N (N + 1) / 2
pairs j <= k and the T = N (N + 1) (N + 2) / 6 triples j <= k <= l in lexicographic order; the record holds the full symmetric
arrays of the reference's NdBPNormalForm.

Deviations from the reference, stated once: every tensor is pointwise and analytic (the reference: ForwardDiff or central
differences); the border has all N kernel vectors (the reference hard-codes the first two, :759-760); each Psijk is solved once
and reused (the reference re-solves three systems per triple); a02 is computed once per i; the predictor leaves out the random
restarts of :966-976, so its result is reproducible (a second shell of start points at twice the size stands in for them), counts
a zero only when the plain residual is below the tolerance too, polishes every zero on the undeflated reduced equation, and
iterates in units of sqrt |dp| unless told otherwise (scale = 1 is the reference's iteration).
"""
from __future__ import annotations

import ctypes as C
import itertools
import math
import warnings
from dataclasses import dataclass, field, replace

import numpy as np

from . import continuation as Cn
from .codim2 import _carr, _saved, _vptrs
from .hip import DeflationOperator, HipVec, MatrixFreeBLS, _GMRES, _ptr, newton_deflated_native, newton_native
from .normal_form1d import TOL_FOLD, Branch, _tangent, is_sh_problem, nf1d_predict


def pairs(N: int):
    """The pairs j <= k in lexicographic order."""
    return [(j, k) for j in range(N) for k in range(j, N)]


def triples(N: int):
    """The triples j <= k <= l in lexicographic order."""
    return [(j, k, l) for j in range(N) for k in range(j, N) for l in range(k, N)]


def expand_b20(b20p) -> np.ndarray:
    """b20[N, P] on the pairs -> the symmetric b20[N, N, N]."""
    b20p = np.asarray(b20p, dtype=float)
    N = b20p.shape[0]
    out = np.zeros((N, N, N))
    for q, (j, k) in enumerate(pairs(N)):
        out[:, j, k] = out[:, k, j] = b20p[:, q]
    return out


def expand_b30(b30p) -> np.ndarray:
    """b30[N, T] on the triples -> the symmetric b30[N, N, N, N]."""
    b30p = np.asarray(b30p, dtype=float)
    N = b30p.shape[0]
    out = np.zeros((N, N, N, N))
    for q, t in enumerate(triples(N)):
        for I in set(itertools.permutations(t)):
            out[(slice(None),) + I] = b30p[:, q]
    return out


# ------------------------------------------------------------------------------------------ records
@dataclass
class NdBPNormalForm:
    """NdBPNormalForm (:531-539): a01[N], a02[N], b11[N, N], b20[N, N, N], b30[N, N, N, N], plus the vectors of the bordered
    solves: Psi01 and Psi2 = {(j, k): Psijk, j <= k}."""
    a01: np.ndarray
    a02: np.ndarray
    b11: np.ndarray
    b20: np.ndarray
    b30: np.ndarray
    Psi01: object = None
    Psi2: dict = None


@dataclass
class NdBranchPoint:
    """The reference's NdBranchPoint (x0, tau, p, params, lens, zeta, zeta_star, nf, type) plus what the solves reported:
    ``converged`` (their AND), ``itlinear`` (GMRES counts of the Psi01 and the Psijk solves) and, from the native call,
    ``unconverged_solves``.  ``type`` is "NonQuadraticParameter" or "N-d".  ``bp(x, dp)`` is the state x0 + sum_i x_i zeta_i
    (:576-582), ``bp.reduced_form(x, dp)`` the reduced equation (:541-574)."""
    x0: object
    tau: object
    p: float
    params: list
    lens: str
    zeta: list
    zeta_star: list
    nf: NdBPNormalForm
    type: str
    converged: bool | None = None
    itlinear: tuple = ()
    unconverged_solves: int | None = None

    @property
    def N(self) -> int:
        return len(self.zeta)

    def reduced_form(self, x, dp: float) -> np.ndarray:
        x = np.asarray(x, dtype=float)
        if x.shape != (self.N,):
            raise ValueError(f"N = {self.N} and length(x) = {x.size} should match!")
        nf = self.nf
        # the reference multiplies a02 by 0 p (:554): the term is kept here, as the reduced equation above states it
        return (dp * (nf.a01 + dp * nf.a02 / 2) + dp * (nf.b11 @ x) + np.einsum("ijk,j,k->i", nf.b20, x, x) / 2
                + np.einsum("ijkl,j,k,l->i", nf.b30, x, x, x) / 6)

    def reduced_jacobian(self, x, dp: float) -> np.ndarray:
        x = np.asarray(x, dtype=float)
        nf = self.nf
        return dp * nf.b11 + np.einsum("imk,k->im", nf.b20, x) + np.einsum("imkl,k,l->im", nf.b30, x, x) / 2

    def __call__(self, x, dp: float = 0.0) -> HipVec:
        return predicted_states(self, [x])[0]


def classify_nd(a01, a02, b11, N: int, tol_fold=TOL_FOLD) -> str:
    """:882"""
    m = max(np.abs(a01).max(), np.abs(a02).max(), np.abs(b11).max())
    return "NonQuadraticParameter" if m < tol_fold else f"{N}-d"


# ------------------------------------------------------------------------------------------ device passes
def _check_n(N: int):
    if N not in (2, 3):
        raise NotImplementedError(f"kernels of dimension 2 and 3 only (got N = {N})")


def nfnd_dots(prob, x: HipVec, pars, ipar: int, zetas):
    """One pass over x and the N zeta that writes nothing (bk_nfnd_dots): (a01[N], b20[N, P], Gram[N, N])."""
    ctx, N = prob.ctx, len(zetas)
    P = len(pairs(N))
    out = (C.c_double * max(N + N * P + N * N, 1))()
    ctx.check(ctx.lib.bk_nfnd_dots(prob.h, _ptr(x.t), _carr(pars), len(pars), int(ipar), N, _vptrs(zetas), out), "bk_nfnd_dots")
    o = np.array(list(out))
    return o[:N].copy(), o[N:N + N * P].reshape(N, P).copy(), o[N + N * P:].reshape(N, N).copy()


def nfnd_rhs(prob, x: HipVec, pars, ipar: int, zetas, a01, b20p):
    """One pass over x and the N zeta (bk_nfnd_rhs): [E(-dpF)] + [E(-d2F[zeta_j, zeta_k]) for j <= k]."""
    ctx, N = prob.ctx, len(zetas)
    outs = [x.similar() for _ in range(1 + len(pairs(N)))]
    ctx.check(ctx.lib.bk_nfnd_rhs(prob.h, _ptr(x.t), _carr(pars), len(pars), int(ipar), N, _vptrs(zetas),
                                  _carr([float(v) for v in np.ravel(a01)]), _carr([float(v) for v in np.ravel(b20p)]), _vptrs(outs)),
              "bk_nfnd_rhs")
    return outs


def nfnd_contract(prob, x: HipVec, pars, ipar: int, zetas, Psi01: HipVec, Psi2):
    """One pass over x, the N zeta, Psi01 and the P Psijk (bk_nfnd_contract): (b11[N, N], a02[N], b30[N, T])."""
    ctx, N = prob.ctx, len(zetas)
    T = len(triples(N))
    out = (C.c_double * max(N * N + N + N * T, 1))()
    ctx.check(ctx.lib.bk_nfnd_contract(prob.h, _ptr(x.t), _carr(pars), len(pars), int(ipar), N, _vptrs(zetas), _ptr(Psi01.t),
                                       _vptrs(Psi2), out), "bk_nfnd_contract")
    o = np.array(list(out))
    return o[:N * N].reshape(N, N).copy(), o[N * N:N * N + N].copy(), o[N * N + N:].reshape(N, T).copy()


# ------------------------------------------------------------------------------------------ the normal form
def _record(prob, x0, p, tau, zetas, a01, a02, b11, b20p, b30p, Psi01, Psi2, cv, it, bad=None, tol_fold=TOL_FOLD) -> NdBranchPoint:
    N = len(zetas)
    nf = NdBPNormalForm(np.array(a01, dtype=float), np.array(a02, dtype=float), np.array(b11, dtype=float), expand_b20(b20p),
                        expand_b30(b30p), Psi01, dict(zip(pairs(N), Psi2)))
    return NdBranchPoint(x0=x0, tau=tau, p=float(p), params=prob._pvec(p), lens=prob.lens, zeta=list(zetas), zeta_star=list(zetas),
                         nf=nf, type=classify_nd(nf.a01, nf.a02, nf.b11, N, tol_fold), converged=bool(cv),
                         itlinear=tuple(int(i) for i in it), unconverged_solves=bad)


def normal_form_nd(prob, x0: HipVec, p: float, zetas, ls: _GMRES, tau=None, tol_fold=TOL_FOLD) -> NdBranchPoint:
    """The computation of get_normal_formNd (:755-895) call by call on the plugin surface at (x0, p) with the orthonormal kernel
    basis ``zetas``: bk_nfnd_dots, bk_nfnd_rhs, 1 + P block solves bls(J, zetas, zetas, 0, r, 0) of MatrixFreeBLS(ls,
    use_pl=True), bk_nfnd_contract."""
    N = len(zetas)
    _check_n(N)
    pv, ipar = prob._pvec(p), prob.ipar
    a01, b20p, gram = nfnd_dots(prob, x0, pv, ipar, zetas)
    if not np.abs(gram - np.eye(N)).max() <= 1e-8:
        raise ValueError(f"the kernel basis is not orthonormal: Gram matrix {gram.tolist()}")
    rhs = nfnd_rhs(prob, x0, pv, ipar, zetas, a01, b20p)
    J = prob.jacobian(x0, p)
    bls = MatrixFreeBLS(ls, use_pl=True)
    sols, cv, it = [], True, []
    for r in rhs:
        u1, _, c1, i1 = bls.solve_block(J, zetas, zetas, np.zeros((N, N)), r, np.zeros(N))
        sols.append(u1)
        cv = cv and c1
        it.append(i1)
    b11, a02, b30p = nfnd_contract(prob, x0, pv, ipar, zetas, sols[0], sols[1:])
    return _record(prob, x0, p, tau, zetas, a01, a02, b11, b20p, b30p, sols[0], sols[1:], cv, it, tol_fold=tol_fold)


def normal_form_nd_native(prob, x0: HipVec, p: float, zetas, ls: _GMRES, tau=None, tol_fold=TOL_FOLD) -> NdBranchPoint:
    """The same as one library call (bk_normal_form_nd)."""
    ctx, N = prob.ctx, len(zetas)
    P, T = len(pairs(max(N, 0))), len(triples(max(N, 0)))
    pv = prob._pvec(p)
    Psi01, Psi2 = x0.similar(), [x0.similar() for _ in range(P)]
    ncoef = 2 * N + N * N + N * P + N * T
    coef = (C.c_double * max(ncoef, 1))()
    cv = C.c_int()
    it = (C.c_int * (1 + P))()
    lo = ls._opts()
    bad0 = ctx.get_option("nfnd_unconverged_solves")
    ctx.check(ctx.lib.bk_normal_form_nd(ctx.h, prob.h, _ptr(x0.t), _carr(pv), len(pv), prob.ipar, N, _vptrs(zetas), C.byref(lo),
                                        ls._pl(), _ptr(Psi01.t), _vptrs(Psi2), coef, C.byref(cv), it), "bk_normal_form_nd")
    c = np.array(list(coef))
    o = np.cumsum([0, N, N, N * N, N * P, N * T])
    a01, a02, b11, b20p, b30p = (c[o[i]:o[i + 1]] for i in range(5))
    return _record(prob, x0, p, tau, zetas, a01, a02, b11.reshape(N, N), b20p.reshape(N, P), b30p.reshape(N, T), Psi01, Psi2,
                   cv.value, list(it), int(ctx.get_option("nfnd_unconverged_solves") - bad0), tol_fold)


def orthonormalise(zetas):
    """Two Gram-Schmidt sweeps over copies of ``zetas`` (what biorthogonalise, :752, amounts to for zeta* = zeta)."""
    out = []
    for z in zetas:
        z = z.copy()
        for _ in range(2):
            for q in out:
                z.add_(q, -q.inner(z))
        nrm = z.norm()
        if not nrm > 0:
            raise ValueError("orthonormalise: the kernel vectors are linearly dependent")
        out.append(z.scale_(1.0 / nrm))
    return out


def get_normal_form_nd(br, ind: int, prob, ls: _GMRES, eig=None, nev=None, zetas=None, tol_fold=TOL_FOLD,
                       tol_stability=1e-10) -> NdBranchPoint:
    """get_normal_formNd(prob, br, ind) (:656-896) for a point of type "nd" of a branch of continuation.continuation_native(...,
    bisection = True, save_sol = True) in the problem's own lens.  N = |delta n_unstable| of the record, x0 and p the saved
    (bisected) state, tau from the saved neighbours.  The kernel basis: the user's ``zetas`` (the reference's zeta_s =), or the N
    eigenvectors nearest 0 from ``eig`` asked for max(2 N, nev) pairs (:681); either is orthonormalised by two Gram-Schmidt
    sweeps.  An eigenvalue counts as one of the N crossing ones within ``tol_stability`` plus ten times the width of the bisection
    interval of 0: the point is known no better than that.  The branch record does not keep its ContinuationPar, so
    ``tol_stability`` is not read from ``br``: its default is ContinuationPar's; pass the branch's value if it was another."""
    if not is_sh_problem(prob):
        raise TypeError("get_normal_form_nd is available for SwiftHohenberg and SwiftHohenberg1D problems only")
    sp = br.specialpoint[ind]
    kind = sp.get("type")
    if kind != "nd":
        raise ValueError("The provided index does not refer to a Branch Point with a kernel of dimension > 1. The type of the "
                         f"bifurcation is {kind}. The bifurcation point is {sp}.")
    nu = sp["n_unstable"]
    N = abs(int(nu[0]) - int(nu[1]))
    if N > 3:
        raise NotImplementedError(f"get_normal_form_nd: kernels of dimension 2 and 3 only (this point has N = {N})")
    i = sp["idx"] if "idx" in sp else sp["step"]
    x, p = _saved(br, i)
    x, p = x.copy(), float(p)
    tau = _tangent(br, i)
    if zetas is None:
        if eig is None:
            raise ValueError("get_normal_form_nd needs an eigensolver (eig = ...) or the kernel basis (zetas = ...)")
        vals, vecs, _, _ = eig(prob.jacobian(x, p), max(2 * N, nev or 0))
        if vecs is None:
            raise ValueError("get_normal_form_nd needs the eigenvectors (an eigensolver with save_vectors = True)")
        vals = np.asarray(vals)
        iv = sp.get("interval", (p, p))
        tol0 = float(tol_stability) + 10.0 * abs(float(iv[1]) - float(iv[0]))
        near = int(np.sum(np.abs(vals) <= tol0))
        if near < N:
            raise RuntimeError(f"get_normal_form_nd: the eigensolver returned {near} eigenvalues within {tol0:.3e} of 0, the "
                               f"kernel has dimension {N} (eigenvalues {vals.tolist()})")
        order = np.argsort(np.abs(vals), kind="stable")[:N]
        zetas = [vecs[int(k)][0] for k in order]
    elif len(zetas) != N:
        raise ValueError(f"get_normal_form_nd: {len(zetas)} kernel vectors given, the point has N = {N}")
    return normal_form_nd_native(prob, x, p, orthonormalise(zetas), ls, tau=tau, tol_fold=tol_fold)


# ------------------------------------------------------------------------------------------ predictor
def _deflation(x, roots, power=2, shift=0.1):
    """M(x) = prod_r (<x - r, x - r>^-power + shift) and its gradient (DeflationOperator(2, 0.1, roots), :920)."""
    M, g = 1.0, np.zeros_like(x)
    for r in roots:
        d = x - r
        dd = float(d @ d)
        if dd < 1e-100:                                  # on a deflated zero M is infinite (and dd^-3 overflows): not converged
            return math.inf, g
        m = dd ** -power + shift
        g = g * m + M * (-2.0 * power * dd ** (-power - 1)) * d
        M *= m
    return M, g


def _deflated_newton(F, J, roots, x, tol=1e-10, maxiter=100):
    """Newton on M(x) F(x) with the exact Jacobian M J + F grad M' (solve(prob, deflationOp, optn, Val(:autodiff)), :957), the
    infinity norm and the callback cbMaxNorm(1e100) of :940.  Converged when the deflated AND the plain residual are below ``tol``: with
    many zeros deflated M falls to shift^k far from all of them, and M F alone would accept any start."""
    for it in range(maxiter + 1):
        M, g = _deflation(x, roots)
        if not np.isfinite(M):
            return x, False
        f = F(x)
        G = M * f
        res = np.abs(G).max()
        if not np.isfinite(res) or res > 1e100:
            return x, False
        if res < tol and np.abs(f).max() < tol:          # far from every zero M is as small as shift^roots: F itself too
            return x, True
        if it == maxiter:
            break
        A = M * J(x) + np.outer(f, g)
        try:
            x = x - np.linalg.solve(A, G)
        except np.linalg.LinAlgError:
            return x, False
    return x, False


def _polish(F, J, x, steps=3):
    """The deflated residual M F < tol leaves F itself only as small as tol / M: a few plain Newton steps on the reduced equation
    from the zero the deflated iteration found, kept when they stay at that zero (moved by less than 1e-3 (1 + |x|))."""
    y = x.copy()
    for _ in range(steps):
        try:
            y = y - np.linalg.solve(J(y), F(y))
        except np.linalg.LinAlgError:
            return x
    return y if np.all(np.isfinite(y)) and np.abs(y - x).max() <= 1e-3 * (1 + np.abs(x).max()) else x


def predictor(bp: NdBranchPoint, dp: float, ampfactor=1.0, igs=None, amp_igs=1.0, maxiter=100, scale=None):
    """predictor(bp::NdBranchPoint, dp) (:916-985): the zeros of the reduced equation at -|dp| ("before") and +|dp| ("after"),
    the trivial one first.  Deflated Newton on the host in R^N (power 2, shift 0.1, the trivial zero deflated from the start),
    started from the vertices of {-1, 0, 1}^N times ``amp_igs`` in the order of Iterators.product (first index fastest), or from
    ``igs``.  The random restarts of :966-976 are left out: the result is reproducible.  In their place the vertices are visited a
    second time at twice the size: with one start per expected zero a single Newton path that ends at a zero already found loses
    one.  Every zero found is polished by three plain Newton steps on the reduced equation (the deflated residual below the
    tolerance bounds F only by tolerance / M).
    ``scale``: the iteration runs on y = x / scale with the residual in units of scale |dp|; ``igs`` and ``amp_igs`` are in units
    of ``scale``.  The default, sqrt |dp|, is the size of the zeros at a pitchfork (a01 = a02 = b20 = 0): the scaled equation and
    with it the set of zeros found do not depend on |dp|.  scale = 1 is the reference's iteration; its deflation factors are
    powers of the DISTANCE between zeros, so for zeros much closer than 1 (small |dp|) the deflated residual of the later zeros
    cannot reach the tolerance in fp64 and zeros are lost (section 9g of DESIGN.md has the counts).  No finite set of starts
    guarantees every zero: compare the counts of both sides with what the symmetry of the problem predicts."""
    N = bp.N
    scale = float(scale) if scale is not None else (math.sqrt(abs(float(dp))) if dp != 0 else 1.0)
    if igs is None:
        vert = [c[::-1] for c in itertools.product((-1, 0, 1), repeat=N)]
        igs = [tuple(a * x for x in c) for a in (1.0, 2.0) for c in vert]

    def side(d):
        unit = 1.0 if scale == 1.0 else scale * abs(d)
        F = lambda y: bp.reduced_form(scale * y, d) / unit
        J = lambda y: bp.reduced_jacobian(scale * y, d) * (scale / unit)
        roots = [np.zeros(N)]
        for ci in igs:
            ci = np.asarray(ci, dtype=float)
            if np.linalg.norm(ci) > 0:
                x, ok = _deflated_newton(F, J, roots, ci * amp_igs, maxiter=maxiter)
                if ok:
                    roots.append(_polish(F, J, x))
        return [ampfactor * scale * r for r in roots]

    return {"before": side(-abs(float(dp))), "after": side(abs(float(dp)))}


def predicted_states(bp: NdBranchPoint, roots):
    """[x0 + sum_i x_i zeta_i for x in roots] (:576-582) through bk_nf1d_predict with zeta_0, zeta_1, zeta_2 in its (zeta, psi01,
    tau) slots, up to four states per pass."""
    z = list(bp.zeta) + [None] * (3 - bp.N)
    coefs = [tuple(float(v) for v in np.asarray(x, dtype=float)) + (0.0,) * (3 - bp.N) for x in roots]
    out = []
    for k in range(0, len(coefs), 4):
        out.extend(nf1d_predict(bp.x0, z[0], z[1], z[2], coefs[k:k + 4]))
    return out


# ------------------------------------------------------------------------------------------ multicontinuation
@dataclass
class FirstPoints:
    """What get_first_points_on_branch returns (the reference's named tuple, :351, plus the bookkeeping): ``before`` / ``after`` are
    the DeflationOperators of the two sides, roots[0] a copy of bp.x0 and roots[1:] the states found at ``bpm`` = bp.p - |dp| /
    ``bpp`` = bp.p + |dp|; ``records`` has one dict per predicted zero: side, index, zero, status ("found" | "lost" | "trivial" |
    "duplicate"), itnewton, itlinear, residual (final, of the quantity stopped on) and min_dist (smallest distance to the roots held when
    the zero was tried; None for "trivial")."""
    before: DeflationOperator
    after: DeflationOperator
    bpm: float
    bpp: float
    records: list = field(default_factory=list)

    def count(self, side: str, status: str) -> int:
        return sum(1 for r in self.records if r["side"] == side and r["status"] == status)


def get_first_points_on_branch(bp: NdBranchPoint, roots, prob, ls, nopt, delta_p, usedeflation=True, max_iter_deflation=None,
                               perturb_guess=None, normC=Cn.norm2, stop_plain=True, solver=None) -> FirstPoints:
    """get_first_points_on_branch (src/bifdiagram/BranchSwitching.jl:298-352): the zeros ``roots`` = {"before": [...], "after":
    [...]} of the reduced equation (predictor) turned into zeros of F.  Each side has its own DeflationOperator(2, 1, [copy of
    x0], autodiff=True) (:325, :339) and walks its zeros in order: deflated Newton (bk_newton_deflated_exact; plain bk_newton
    with usedeflation = False) from perturb_guess(bp(x, dp)) at bp.p -+ |delta_p| with ``nopt``'s tolerance, ``max_iter_deflation``
    (default min(50, 15 nopt.max_iterations), :304) iterations and the norm ``normC``; what converges is pushed (:335, :348).
    ``solver`` (default hip.newton_deflated_native) is called as solver(prob, defop, x, p, ls, tol=, max_iterations=, norm_inf=,
    stop_plain=) and returns a dict with u, converged, itnewton, residuals, min_dist.

    Deviations from the reference:
      stop_plain = True   Newton stops on |F| < tol, not on |M F| < tol.  With the roots of a multicontinuation 0.2 - 0.4 apart
          M = prod (d_i^-2 + 1) ~ 1e5, and the reference's rule asks |F| < 1e-15, below the rounding floor of F: starts that sit
          on their zero never "converge".  Measured with the dense restatement (tests/multicontinuation_ref.py; 16 x 16 SH,
          half-lengths (pi, pi), modes (1,2), (2,1), nu = 1.3, tol 1e-10): the reference's rule finds 6 of the 8 states at
          dp = 0.008 and 2 of 8 at 0.004, the plain rule 8 of 8 at dp = 0.008 .. 0.001 in 4 - 12 iterations; 8 x 8 x 8,
          half-lengths 2.5, nu = 0.9: 26 of 26 at dp = 1e-4.  |F| < tol follows from |M F| < tol whenever alpha >= 1, so the plain
          rule only accepts more.  stop_plain = False is the reference's rule.
      duplicates          with the plain rule a state may converge onto a root already held (M is finite next to it): a state
          within 1e-6 (1 + |x|_2) of a held root is recorded as "duplicate" and not pushed.
      nothing is printed; the zero at the origin is recorded as "trivial" and not tried (the reference starts Newton on x0 with x0
          deflated, which cannot converge); lost zeros are named by one warning per side."""
    dp = abs(float(delta_p))
    nmax = max_iter_deflation if max_iter_deflation is not None else min(50, 15 * nopt.max_iterations)
    if normC not in (Cn.norm2, Cn.norminf):
        raise TypeError("get_first_points_on_branch: normC must be norm2 or norminf")
    inf = normC is Cn.norminf
    if solver is None:
        solver = newton_deflated_native
    records = []

    def side(name, zeros, sgn):
        defop = DeflationOperator(2, 1.0, [bp.x0.copy()], autodiff=True)
        p = bp.p + sgn * dp
        for k, z in enumerate(zeros):
            z = np.asarray(z, dtype=float)
            rec = dict(side=name, index=k, zero=z, status="trivial", itnewton=0, itlinear=0, residual=None, min_dist=None)
            records.append(rec)
            if not np.abs(z).max() > 0:
                continue
            x = bp(z, sgn * dp)
            if perturb_guess is not None:
                x = perturb_guess(x)
            if usedeflation:
                sol = solver(prob, defop, x, p, ls, tol=nopt.tol, max_iterations=nmax, norm_inf=inf, stop_plain=stop_plain)
                dmin = sol["min_dist"]
            else:
                sol = newton_native(prob, x, p, ls, tol=nopt.tol, max_iterations=nmax, norm_inf=inf)
                dmin = math.sqrt(min(defop.dots(sol["u"])[0]))
            rec.update(itnewton=sol["itnewton"], itlinear=sol.get("itlineartot"), residual=sol["residuals"][-1], min_dist=dmin)
            if not sol["converged"]:
                rec["status"] = "lost"
            elif not dmin > 1e-6 * (1.0 + sol["u"].norm()):
                rec["status"] = "duplicate"
            else:
                rec["status"] = "found"
                defop.push(sol["u"])
        lost = sum(1 for r in records if r["side"] == name and r["status"] == "lost")
        if lost:
            warnings.warn(f"get_first_points_on_branch: {lost} of the {len(zeros)} predicted zeros {name} the bifurcation point "
                          "did not converge (status \"lost\")")
        return defop

    after = side("after", roots["after"], 1.0)              # the reference's order: after, then before
    before = side("before", roots["before"], -1.0)
    return FirstPoints(before=before, after=after, bpm=bp.p - dp, bpp=bp.p + dp, records=records)


def multicontinuation(br, ind, prob, alg: Cn.PALC, cp: Cn.ContinuationPar, delta_p=None, ampfactor=1.0, predictor_kwargs=None,
                      first_points: FirstPoints = None, roots=None, usedeflation=True, max_iter_deflation=None, perturb_guess=None,
                      stop_plain=True, eig=None, nev=None, zetas=None, tol_fold=TOL_FOLD, normC=Cn.norm2, verbosity=0,
                      save_sol=False, bisection=False, finalise_solution=None, callback_newton=None, filename=None):
    """multicontinuation (src/bifdiagram/BranchSwitching.jl:234-291, 355-442) at a point of type "nd" of a native branch: every
    branch that leaves it.  ``ind``: the index of the special point (the normal form is computed: get_normal_form_nd with ``eig``,
    default the eigensolver of cp.newton_options, ``nev`` and ``zetas``) or an NdBranchPoint.  Then predictor(bp, |dp|,
    ampfactor, **predictor_kwargs) unless ``roots`` is given, get_first_points_on_branch unless ``first_points`` is given -- the
    stages are decoupled as the reference advises for large problems (:231-232) -- and one branch per root from the second on
    (the first is the trivial state, :396): from (bp.x0, bp.p) to (root, bp.p -+ |dp|) with ds = -+|cp.ds| (:432-435), every step
    one library call as in continuation_native.  dp = delta_p, default cp.ds (:413).  Returns ([normal_form1d.Branch(branch, bp)
    for the roots before, then after], FirstPoints).

    Deviations from the reference: the first points stop on |F| (``stop_plain`` = True) and drop duplicates, both stated with
    their measurements in get_first_points_on_branch; nothing is printed."""
    if normC not in (Cn.norm2, Cn.norminf):
        raise TypeError("multicontinuation: normC must be norm2 or norminf")
    nopt = cp.newton_options
    ls = nopt.linsolver
    if isinstance(ind, NdBranchPoint):
        bp = ind
    else:
        bp = get_normal_form_nd(br, ind, prob, ls, eig=eig if eig is not None else nopt.eigsolver,
                                nev=nev if nev is not None else cp.nev, zetas=zetas, tol_fold=tol_fold)
    dp = abs(float(cp.ds if delta_p is None else delta_p))
    if first_points is None:
        if roots is None:
            roots = predictor(bp, dp, ampfactor=ampfactor, **(predictor_kwargs or {}))
        first_points = get_first_points_on_branch(bp, roots, prob, ls, nopt, dp, usedeflation=usedeflation,
                                                  max_iter_deflation=max_iter_deflation, perturb_guess=perturb_guess, normC=normC,
                                                  stop_plain=stop_plain)
    inf = normC is Cn.norminf
    dscont = abs(cp.ds)
    first = lambda x: dict(u=x, itnewton=0, itlineartot=0, residuals=[])

    def run(sol, p1, ds):
        cp2 = replace(cp, ds=ds)
        return Cn._continuation_native_from(prob, first(bp.x0), float(bp.p), dict(u=sol), float(p1), alg.update(cp2), cp2, inf,
                                            verbosity, save_sol, bisection, finalise_solution, callback_newton, None, filename)

    branches = [Branch(run(r, first_points.bpm, -dscont), bp) for r in first_points.before.roots[1:]]
    branches += [Branch(run(r, first_points.bpp, dscont), bp) for r in first_points.after.roots[1:]]
    return branches, first_points
