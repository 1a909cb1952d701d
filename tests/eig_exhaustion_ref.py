"""Dense references for the Krylov-Schur eigensolvers of csrc/eig.hip where the Krylov space runs out: NumPy only, no GPU code.

Every case is a dense Jacobian ``J`` from oracle.operators, a shift sigma and a start vector.  For a case this module gives

  * the dense spectrum and eigenvectors and ``kappa``, the condition number of the eigenvector matrix (1 for the symmetric cases);
  * the grade ``d`` of the start vector: the dimension of its Krylov space, the number of eigen-directions it has a component along;
  * the wanted set per mode -- "si" (nearest sigma, what bk_eig_shiftinvert returns), "lr" (rightmost, bk_eig_krylovkit), "lm" (largest
    modulus, bk_eig_krylovkit_lm) -- in the order the library documents, with conjugate pairs kept whole, and the gap behind it;
  * true residuals ``|J v - lambda v| / |v|`` in numpy.longdouble;
  * a float64 restatement of the two-pass Arnoldi step of csrc/solver.hip (``arnoldi``) with the breakdown test on or off, which
    tests/test_eig_exhaustion_reference.py uses to show that each case exhausts where claimed and what a solver that misses the breakdown
    would return.  The restatement is not the kernels: summation order and fma differ on the device.

Groups (tests/test_gpu_eig_exhaustion.py runs the library on them):
  A  the whole space is exhausted (d = n): SH (4,3,2), (6,5), (8,4) at guess() + 0.1 noise; cGL (4,3) at u = 0 and at a small random state.
  B  the start vector lies in an invariant subspace of a larger space: SH (8,8,6), n = 384.
  C  a conjugate pair at the cut: cGL (4,3) at u = 0.
"""
from __future__ import annotations

import functools
import os
import sys
from dataclasses import dataclass

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import operators  # noqa: E402

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
LS = (np.pi, 3.0, 2.5)                   # half lengths of the SH grids (as tests/krylov_dense_ref.py)
CGL_LS = (np.pi, np.pi / 2)
SH_PARAMS = dict(l=0.1, nu=1.2)
CGL_PARAMS = dict(r=1.2, mu=0.1, nu=1.0, c3=-1.0, c5=1.0, gamma=0.0)
SEED = 1234                              # EigOpts.seed of every solve from the library's own random start (its default)
GAP_RATIO = 1.05                         # tests/test_gpu_eigensolve_at_size.py: the wanted set ends at a clear gap
BREAKDOWN = 1e-30                        # csrc/solver.hip: `!(nn > 1e-30 * ww)` declares the breakdown
CANCEL = 1e-8                            # kCancelTol (csrc/common.h): below it the Pythagorean remainder is replaced by the explicit one
KRYLOVDIM_MAX = 63                       # kMaxBasis - 1
TOL_STABILITY = 1e-10                    # ContinuationPar.tol_stability


@dataclass(frozen=True)
class Case:
    cid: str
    kind: str                  # "sh" | "cgl"
    dims: tuple
    state: str                 # "guess+noise" | "zero" | "random"
    sigma: float
    hermitian: bool
    useed: int = 0
    start: str = "random"      # "random": the library's v_fill_random(SEED) | "upload": rng.random(n) | "eigsum6" | "eig1"

    @property
    def n(self):
        return int(np.prod(self.dims)) * (2 if self.kind == "cgl" else 1)

    @property
    def ls(self):
        return CGL_LS if self.kind == "cgl" else LS[:len(self.dims)]


A_CASES = {c.cid: c for c in (
    Case("sh-4x3x2", "sh", (4, 3, 2), "guess+noise", 0.1, True, useed=11),
    Case("sh-6x5", "sh", (6, 5), "guess+noise", 0.1, True, useed=12, start="upload"),
    Case("sh-8x4", "sh", (8, 4), "guess+noise", 0.1, True, useed=13),
    Case("cgl-4x3-zero", "cgl", (4, 3), "zero", 1.0, False),
    Case("cgl-4x3-rand", "cgl", (4, 3), "random", 1.0, False, useed=14, start="upload"),
)}
B_BASE = Case("sh-8x8x6", "sh", (8, 8, 6), "guess+noise", 0.1, True, useed=15)
# (cid, start, nev)
B_CASES = {"sh-8x8x6/eigsum6/nev6": ("eigsum6", 6), "sh-8x8x6/eigsum6/nev10": ("eigsum6", 10), "sh-8x8x6/eig1/nev3": ("eig1", 3)}
B_KRYLOVDIM = 30
C_CASE = "cgl-4x3-zero"
MODES = ("si", "lr", "lm")
NEV_ASKED = lambda n: (1, 6, n - 2)      # noqa: E731  (the grid asked for; nev_grid moves a value that ends inside a cluster)


def krylovdims(n):
    return (n - 1, n, n + 1, 45, 63)


def case(cid) -> Case:
    if cid in A_CASES:
        return A_CASES[cid]
    start, _ = B_CASES[cid]
    return Case(cid, B_BASE.kind, B_BASE.dims, B_BASE.state, B_BASE.sigma, True, useed=B_BASE.useed, start=start)


# ------------------------------------------------------------------------------------------------------------------ dense side
def library_random(n, seed=SEED, goff=0):
    """v_fill_random of csrc/vecops.hip restated: splitmix64 of (seed, global index), uniform in [0, 1)."""
    with np.errstate(over="ignore"):
        i = np.arange(n, dtype=np.uint64) + np.uint64(goff + 1)
        z = np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * i
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


@functools.lru_cache(maxsize=None)
def state(cid):
    """(u, J): the state and the oracle's Jacobian there as a dense float64 matrix (read-only)."""
    c = case(cid)
    if c.kind == "sh":
        op = operators.SwiftHohenberg(c.dims, c.ls)
        u = op.guess() + 0.1 * np.random.default_rng(c.useed).standard_normal(op.N)
        J = op.J(u, SH_PARAMS["l"], SH_PARAMS["nu"])
    else:
        op = operators.CGL2d(c.dims, c.ls)
        u = np.zeros(c.n) if c.state == "zero" else 0.3 * np.random.default_rng(c.useed).standard_normal(c.n)
        J = op.J(u, **CGL_PARAMS)
    J = np.ascontiguousarray(J.toarray())
    for a in (u, J):
        a.setflags(write=False)
    return u, J


@dataclass
class Spectrum:
    lam: np.ndarray            # eigenvalues (real array for the hermitian cases)
    V: np.ndarray              # eigenvectors in the columns, unit 2-norm
    kappa: float               # cond_2 of V
    normJ: float               # |J|_2
    delta: float               # min |lambda - sigma|
    normJs: float              # |J - sigma|_2


@functools.lru_cache(maxsize=None)
def spectrum(cid) -> Spectrum:
    c = case(cid)
    _, J = state(cid)
    if c.hermitian:
        assert np.array_equal(J, J.T)
        lam, V = np.linalg.eigh(J)
        kappa = 1.0
    else:
        lam, V = np.linalg.eig(J)
        V = V / np.linalg.norm(V, axis=0)
        kappa = float(np.linalg.cond(V))
    sv = np.linalg.svd(J, compute_uv=False)
    svs = np.linalg.svd(J - c.sigma * np.eye(c.n), compute_uv=False)
    return Spectrum(lam, V, kappa, float(sv[0]), float(np.abs(lam - c.sigma).min()), float(svs[0]))


@functools.lru_cache(maxsize=None)
def start_vector(cid):
    """The start vector of the case (not normalised; the library normalises it) and whether it must be uploaded."""
    c = case(cid)
    sp = spectrum(cid)
    if c.start == "random":
        x = library_random(c.n)
    elif c.start == "upload":
        x = np.random.default_rng(c.useed + 500).random(c.n)
    else:
        near = np.argsort(np.abs(sp.lam - c.sigma), kind="stable")
        x = sp.V[:, near[:6]].sum(axis=1) if c.start == "eigsum6" else sp.V[:, near[0]].copy()
    x.setflags(write=False)
    return x, c.start != "random"


def components(cid):
    """|coefficients| of the normalised start vector in the eigenvector basis."""
    x, _ = start_vector(cid)
    sp = spectrum(cid)
    return np.abs(np.linalg.solve(sp.V, (x / np.linalg.norm(x)).astype(sp.V.dtype)))


def grade(cid):
    """Dimension of the Krylov space of the start vector: with pairwise distinct eigenvalues, the number of eigen-directions it has a
    component along.  Components below 1e-8 of the largest are rounding (the B cases are sums of float64 eigenvectors)."""
    c = components(cid)
    return int(np.sum(c > 1e-8 * c.max()))


def residual(cid, lam, v):
    """|J v - lam v| / |v| with products and sums in numpy.longdouble; v real or complex."""
    _, J = state(cid)
    Jl = J.astype(LD)
    vr, vi = np.asarray(np.real(v), dtype=LD), np.asarray(np.imag(v), dtype=LD)
    lr, li = LD(np.real(lam)), LD(np.imag(lam))
    rr = Jl @ vr - (lr * vr - li * vi)
    ri = Jl @ vi - (lr * vi + li * vr)
    return float(np.sqrt(np.sum(rr * rr + ri * ri)) / np.sqrt(np.sum(vr * vr + vi * vi)))


# ------------------------------------------------------------------------------------------------------------------ wanted sets
def _key(cid, mode, lam):
    """What the mode orders by, larger = more wanted: si: |1 / (lambda - sigma)|; lr: Re lambda; lm: |lambda|."""
    if mode == "si":
        return 1.0 / np.abs(lam - case(cid).sigma)
    return np.real(lam).astype(float) if mode == "lr" else np.abs(lam)


@dataclass
class Wanted:
    values: np.ndarray         # in the returned order: si, lr by decreasing real part, lm by decreasing modulus (complex array)
    nvals: int                 # nev, or nev + 1 where position nev splits a conjugate pair
    gap: float                 # how clearly the set ends (>= GAP_RATIO: well defined); inf where nothing is excluded
    n_unstable: int            # values of the set with Re > TOL_STABILITY


def wanted(cid, mode, nev) -> Wanted:
    """The nev most wanted eigenvalues of the mode, a conjugate pair at the cut kept whole.  ``gap``: si and lm order by a positive
    quantity (distance to sigma, modulus) and the first excluded value must be GAP_RATIO times as far / as small as the last included
    one.  lr orders by the real part, and the same rule is read on it: both on the stable side, the excluded real part is GAP_RATIO
    times as far from zero as the included one; both on the unstable side, the included one is GAP_RATIO times the excluded one; on
    different sides of zero the set is the unstable part and ends clearly."""
    lam = np.asarray(spectrum(cid).lam, dtype=complex)
    key = _key(cid, mode, lam)
    order = np.argsort(-key, kind="stable")
    m = min(nev, len(lam))
    tiny = 64 * EPS * np.abs(lam).max()
    if m < len(lam) and abs(lam[order[m - 1]].imag) > tiny and abs(lam[order[m - 1]] - np.conj(lam[order[m]])) <= tiny:
        inside = np.sum(np.abs(lam[order[:m]] - np.conj(lam[order[m - 1]])) <= tiny)
        if inside == 0:
            m += 1                                        # position nev splits a pair: both members are returned
    sel = lam[order[:m]]
    if m == len(lam):
        gap = np.inf
    elif mode == "lr":
        a, b = key[order[m - 1]], key[order[m]]
        gap = np.inf if a > 0.0 >= b else (a / b if b > 0.0 else b / a)
    else:
        gap = key[order[m - 1]] / key[order[m]]
    out_key = np.abs(sel) if mode == "lm" else sel.real
    sel = sel[np.argsort(-out_key, kind="stable")]
    return Wanted(sel, m, float(gap), int(np.sum(sel.real > TOL_STABILITY)))


def nev_grid(cid, mode):
    """The nev grid of the A cases: 1, 6 and n - 2, each moved to the nearest value (up first, then down) whose wanted set ends at a clear
    gap -- "where a case fails that, change nev, not the rule"."""
    n = case(cid).n
    out = []
    for nev in NEV_ASKED(n):
        for cand in sorted(range(1, n - 1), key=lambda k: (abs(k - nev), -k)):
            if wanted(cid, mode, cand).gap >= GAP_RATIO and cand not in out:
                out.append(cand)
                break
    return tuple(out)


def pair_split_nev(cid, mode="si"):
    """Group C: the smallest nev > 1 at which position nev splits a conjugate pair and the completed set ends at a clear gap."""
    for nev in range(2, case(cid).n - 2):
        w = wanted(cid, mode, nev)
        if w.nvals == nev + 1 and w.gap >= GAP_RATIO:
            return nev
    raise AssertionError("no nev splits a pair")


def match(values, lam):
    """Injective assignment of returned values to dense eigenvalues minimising the largest distance (sorted greedy on the distance
    matrix would do for well separated spectra; the assignment problem does it always): (index of the dense value per returned one,
    distances)."""
    from scipy.optimize import linear_sum_assignment
    values, lam = np.asarray(values, dtype=complex), np.asarray(lam, dtype=complex)
    D = np.abs(values[:, None] - lam[None, :])
    rows, cols = linear_sum_assignment(D ** 2)
    assert np.array_equal(rows, np.arange(len(values)))
    return cols, D[rows, cols]


# ------------------------------------------------------------------------------------------------------------------ bounds
def lmax_sh(dims, ls):
    """Largest eigenvalue of L1 = (I + Lap)^2, bounded above (tests/test_gpu_eigensolve_at_size.py)."""
    return (1.0 - sum(4.0 / (2.0 * l / n) ** 2 for n, l in zip(dims, ls))) ** 2


def inner_factor(cid, preconditioned):
    """|b - (J - sigma) x| <= factor * eta |b| for the inner solver at hand.  None: GMRES stops on the 2-norm, factor 1.  SH with
    Pl = (L1 + I)^-1 and MINRES (M-norm stop): sqrt(1 + Lmax), as derived in tests/test_gpu_eigensolve_at_size.py.  cGL with the exact
    inverse of the trivial state's shifted Jacobian and left-preconditioned GMRES, which stops on |Pl r| <= eta |Pl b|:
    |r| <= |Pl^-1| |Pl| eta |b|, the condition number of Pl -- here of the normal matrix Lap (x) I + [[r - sigma, -nu], [nu, r - sigma]]."""
    c = case(cid)
    if not preconditioned:
        return 1.0
    if c.kind == "sh":
        return float(np.sqrt(1.0 + lmax_sh(c.dims, c.ls)))
    op = operators.CGL2d(c.dims, c.ls)
    P = op.J(np.zeros(c.n), **{**CGL_PARAMS, "r": CGL_PARAMS["r"] - c.sigma}).toarray()
    return float(np.linalg.cond(P))


def bounds_from(mode, lam_ref, n, sigma, kappa, delta, normJ, normJs, eta=0.0, factor=1.0, tau=0.0):
    """(E, R) per reference value: eigenvalue and residual bounds, every term from the dense reference.
    si: the inexact inverse differs from the exact one by at most f eta / delta per unit vector (f = inner_factor), Bauer-Fike gives
    |dmu| <= kappa (f eta / delta + 64 n eps / delta), and lambda = sigma + 1 / mu turns that into E_i = 2 d_i^2 |dmu|;
    R_i = kappa |J - sigma| E_i / d_i.  lr / lm: E = 64 n eps kappa |J|, R = 64 n eps |J|.
    tau (group B only, where the pairs converge on the eigensolver's tolerance and not by a breakdown): a Ritz pair accepted with
    residual tau is within kappa tau of an eigenvalue of the inexact inverse, so tau joins f eta / delta inside |dmu|."""
    lam_ref = np.asarray(lam_ref, dtype=complex)
    if mode == "si":
        d = np.abs(lam_ref - sigma)
        dmu = kappa * (tau + factor * eta / delta + 64 * n * EPS / delta)
        E = 2.0 * d ** 2 * dmu
        return E, kappa * normJs * E / d
    E = np.full(len(lam_ref), 64 * n * EPS * kappa * normJ)
    return E, np.full(len(lam_ref), 64 * n * EPS * normJ)


def bounds(cid, mode, lam_ref, eta=0.0, preconditioned=False, tau=0.0):
    c, sp = case(cid), spectrum(cid)
    return bounds_from(mode, lam_ref, c.n, c.sigma, sp.kappa, sp.delta, sp.normJ, sp.normJs, eta, inner_factor(cid, preconditioned), tau)


# ------------------------------------------------------------------------------------------------------------------ the restatement
def operator(cid, mode):
    """v -> A v of the mode as a float64 callable: the dense LU solve of J - sigma for si, J itself for lr / lm."""
    c = case(cid)
    _, J = state(cid)
    if mode != "si":
        return lambda v: J @ v
    import scipy.linalg as sla
    lu = sla.lu_factor(J - c.sigma * np.eye(c.n))
    return lambda v: sla.lu_solve(lu, v)


@dataclass
class Arnoldi:
    H: np.ndarray              # (m + 1) x m Hessenberg matrix of the m steps taken
    V: np.ndarray
    first: list                # per step: remainder^2 / |w|^2 after the first pass (explicit where the Pythagorean form cancels)
    second: list               # per step: |v - V V'v|^2 / |v|^2 of the second pass (nan where the step ended before it)
    breakdown: int             # the step (1-based) at which the breakdown test fired, 0: never
    applied: int               # operator applications


def arnoldi(apply, x0, steps, detect=True) -> Arnoldi:
    """The two-pass Arnoldi step of csrc/solver.hip (arnoldi_step with eta = 2, as csrc/eig.hip calls it when the Gram-corrected pass
    does not apply or cancels) in float64 NumPy: projections V'w, the Pythagorean remainder while it is above kCancelTol |w|^2 and the
    explicit one below, then always the second pass; both passes declare a breakdown on `!(nn > 1e-30 * ww)`.  detect = False takes
    the two tests out: what a solver that misses the breakdown computes."""
    n = len(x0)
    V = np.zeros((n, steps + 1))
    H = np.zeros((steps + 1, steps))
    V[:, 0] = x0 / np.linalg.norm(x0)
    first, second, brk, m = [], [], 0, 0
    for j in range(steps):
        k = j + 1
        w = apply(V[:, j])
        m = k
        hh = V[:, :k].T @ w
        ww = float(w @ w)
        b2 = ww - float(hh @ hh)
        if b2 > CANCEL * ww:
            be = np.sqrt(b2)
            v = (w - V[:, :k] @ hh) / be
            first.append(b2 / ww)
        else:
            r = w - V[:, :k] @ hh
            nn = float(r @ r)
            first.append(nn / ww)
            if detect and not nn > BREAKDOWN * ww:
                second.append(np.nan)
                brk = k
                H[:k, j] = hh
                break
            be = np.sqrt(nn)
            v = r / be
        ss = V[:, :k].T @ v
        vv = float(v @ v)
        v2 = v - V[:, :k] @ ss
        nn2 = float(v2 @ v2)
        second.append(nn2 / vv)
        H[:k, j] = hh + be * ss
        if detect and not nn2 > BREAKDOWN * vv:
            brk = k
            break
        cn = np.sqrt(nn2)
        V[:, k] = v2 / cn
        H[k, j] = be * cn
    return Arnoldi(H[:m + 1, :m], V[:, :m + 1], first, second, brk, m)


def ritz_values(cid, mode, H):
    """Eigenvalues of the square part of H mapped back to eigenvalues of J (si: sigma + 1 / mu)."""
    m = H.shape[1]
    mu = np.linalg.eigvals(H[:m, :m])
    return case(cid).sigma + 1.0 / mu if mode == "si" else mu


def off_spectrum(cid, mode, ritz):
    """How many Ritz values cannot be assigned to a dense eigenvalue of their own within the mode's bound E (unpreconditioned, eta =
    1e-12): ghost copies and values off the spectrum both count."""
    lam = np.asarray(spectrum(cid).lam, dtype=complex)
    ritz = np.asarray(ritz, dtype=complex)
    taken, bad = set(), 0
    for z in ritz[np.argsort(np.abs(ritz[:, None] - lam[None, :]).min(axis=1))]:
        for i in np.argsort(np.abs(lam - z)):
            if i not in taken:
                break
        E, _ = bounds(cid, mode, [lam[i]], eta=1e-12)
        if len(taken) == len(lam) or abs(z - lam[i]) > E[0]:
            bad += 1
        else:
            taken.add(int(i))
    return bad


# ------------------------------------------------------------------------------------------------------------------ native branch
BRANCH_DIMS, BRANCH_STEPS, BRANCH_NEV = (8, 4), 3, 6
BRANCH_DS, BRANCH_DSMAX = 0.004, 0.004


def branch_lstar():
    """The first l* of the trivial branch u = 0 of SH (8,4): J(0, l) = l - L1, so the smallest eigenvalue of L1."""
    op = operators.SwiftHohenberg(BRANCH_DIMS, LS[:2])
    return float(np.linalg.eigvalsh(op.L1.toarray()).min())


def branch_spectrum(p):
    """eig(J(0, p)) of SH (8,4), ascending."""
    op = operators.SwiftHohenberg(BRANCH_DIMS, LS[:2])
    return np.linalg.eigvalsh(op.J(np.zeros(op.N), p, SH_PARAMS["nu"]).toarray())


@functools.lru_cache(maxsize=None)
def branch_reference():
    """The oracle's PALC branch along u = 0 of SH (8,4) on dense solves: 3 steps of fixed length (ds = dsmax) from a p0 that puts l* in
    the middle of the second step.  Returns (param list, dense n_unstable per point, the oracle's own record)."""
    from oracle import bifurcations, bordered, palc
    op = operators.SwiftHohenberg(BRANCH_DIMS, LS[:2])
    nu = SH_PARAMS["nu"]
    p0 = branch_lstar() - 1.5 * BRANCH_DS / np.sqrt(0.5)
    n = op.N

    def ls(J, r, a0=0.0, a1=1.0):
        return np.linalg.solve(a0 * np.eye(n) + a1 * J, r), True, 1

    def eig(J, nev):
        ev = np.linalg.eigvalsh(J)
        near = ev[np.argsort(np.abs(ev - 0.1), kind="stable")][:nev]
        return np.sort(near)[::-1], None, True, 0

    prob = palc.Problem(lambda x, p: op.F(x, p, nu), lambda x, p: op.J(x, p, nu).toarray())
    cp = bifurcations.ContPar(ds=BRANCH_DS, dsmin=1e-4, dsmax=BRANCH_DSMAX, theta=0.5, p_min=-0.1, p_max=0.15, max_steps=BRANCH_STEPS,
                              nev=BRANCH_NEV, tol=1e-9, max_iterations=15, tangent="bordered")
    bls = lambda *a, **k: bordered.bordering_bls(ls, *a, check_precision=False, **k)      # noqa: E731
    br = bifurcations.continuation(prob, np.zeros(n), p0, ls=ls, bls=bls, eig=eig, cp=cp, normC=palc.norminf, detect_bifurcation_level=2)
    params = [float(p) for p in br["param"]]
    return params, [int(np.sum(branch_spectrum(p) > TOL_STABILITY)) for p in params], br
