"""Dense references for the Krylov solvers where the Krylov space runs out (n < dim): no GPU code.

Every case is a system of at most 64 unknowns built from oracle.operators.  For a case this module gives

  * the dense matrix ``A = a0 I + a1 J`` (or the left-preconditioned / bordered form a flavor solves) and its right-hand side;
  * the solution of the dense system in extended precision (float64 LU refined with numpy.longdouble residuals until the correction
    stagnates; ``solve_mp`` is the same solve through mpmath at 50 digits, which the reference test holds the first against);
  * ``sigma_min(A)`` and ``||A||_2``;
  * the exact GMRES residual norms per step, from an Arnoldi process in mpmath (60 digits);
  * the oracle's counts per flavor (oracle.krylov, oracle.bordered) and the oracle's true residual ``||b - A x||`` in extended precision.

tests/test_krylov_exhaustion_reference.py certifies on these alone that every case is an exhaustion case;
tests/test_gpu_krylov_exhaustion.py runs the library on the same cases and reads the oracle's numbers from
tests/golden/krylov_exhaustion.json.

Re-record the golden file (CPU only):  python tests/krylov_dense_ref.py --record
"""
from __future__ import annotations

import functools
import json
import os
import sys
from dataclasses import dataclass

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import bordered, krylov, operators  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "krylov_exhaustion.json")

DIM = 63                       # krylovdim / restart of every case: larger than every n but 63
RTOL = 1e-8
SHIFTS = ((0.0, 1.0), (0.3, 0.9))
LS = (np.pi, 3.0, 2.5)         # half lengths of the SH / cGL grids
THETA = 0.5                    # group D: xi_u = theta, xi_p = 1 - theta, dotp = <., .> / n
LD = np.longdouble
EPS64 = float(np.finfo(np.float64).eps)
EPSLD = float(np.finfo(LD).eps)


# ------------------------------------------------------------------------------------------------------------------ systems
@dataclass(frozen=True)
class System:
    """One Jacobian and one right-hand side: problem kind, grid, state seed, right-hand-side seed."""
    kind: str                  # "sh1d" | "sh" | "cgl"
    dims: tuple
    useed: int
    bseed: int
    tag: str = ""              # tells systems on the same grid apart
    uscale: float = 0.0        # amplitude of the state (0: the kind's default, USCALE)

    @property
    def sid(self):
        return self.kind + self.tag + "-" + "x".join(str(d) for d in self.dims)

    @property
    def n(self):
        return int(np.prod(self.dims)) * (2 if self.kind == "cgl" else 1)

    @property
    def ls(self):
        return (6.0,) if self.kind == "sh1d" else LS[:len(self.dims)]


SH1D_PARAMS = dict(lam=-0.7, nu=2.0)
SH_PARAMS = dict(l=0.1, nu=1.2)
CGL_PARAMS = dict(r=1.2, mu=0.1, nu=1.0, c3=-1.0, c5=1.0, gamma=0.0)
USCALE = dict(sh1d=0.7, sh=0.7, cgl=0.5)

_SH1D_N = (2, 3, 5, 9, 17, 32, 33, 36, 40, 62, 63)
_GRIDS = ([("sh1d", (N,)) for N in _SH1D_N] + [("cgl", d) for d in ((2, 2), (3, 3), (4, 4))] +
          [("sh", d) for d in ((3, 3), (7, 5), (4, 3, 3))])
# Seeds: 100 + i for the state, 200 + i for the right-hand side, + 1000 t where the first draw missed a condition of the reference test.
# A case that misses one gets another draw HERE, never a skip.  The three re-drawn sizes missed the same condition: the block
# restatement (oracle.krylov.gmres_block) took n + 3 applications or a second cycle where the step-by-step one took n + 2 -- its true
# residual after the exhausting cycle lands within a factor 2 of the tolerance for about one draw in three at n >= 32 (measured over
# nine to twelve draws per size: 32: 5 of 9, 36: 4 of 9, 62: 6 of 12, 63: 2 of 12 draws with unequal counts in either shift form).
_REDRAW = {"sh1d-32": 2, "sh1d-36": 5, "sh1d-63": 8}
SYSTEMS = {s.sid: s for s in (System(k, d, 100 + i + 1000 * _REDRAW.get(System(k, d, 0, 0).sid, 0),
                                     200 + i + 1000 * _REDRAW.get(System(k, d, 0, 0).sid, 0)) for i, (k, d) in enumerate(_GRIDS))}
# Group C (preconditioned) candidates that the seventeen above do not hold.  The cGL candidates are systems of their own ("cglp"): at the
# amplitude 0.5 of group A the exact preconditioner of the trivial state leaves so little to do that the solve ends before the space does
# (the residual at step n - 1 is 2e2 x the tolerance on (2,2), below it on (3,2) and (3,3); amplitude 1: 2e-3 x on (3,2); amplitude 1.5:
# 8e2 x on (3,2)); a state of amplitude 2 is far enough away on all three grids (>= 3e5 x).
C_CGL_USCALE = 2.0
for _i, (_k, _d) in enumerate([("sh", (2, 2)), ("sh", (3, 2)), ("sh", (2, 2, 2)), ("sh", (3, 2, 2))]):
    SYSTEMS.setdefault(System(_k, _d, 0, 0).sid, System(_k, _d, 300 + _i, 400 + _i))
for _i, _d in enumerate([(2, 2), (3, 2), (3, 3)]):
    _s = System("cgl", _d, 350 + _i, 450 + _i, tag="p", uscale=C_CGL_USCALE)
    SYSTEMS[_s.sid] = _s


def oracle_problem(s: System):
    if s.kind == "sh1d":
        return operators.SwiftHohenberg1D(s.dims[0], 6.0)
    if s.kind == "sh":
        return operators.SwiftHohenberg(s.dims, s.ls)
    return operators.CGL2d(s.dims, s.ls)


@functools.lru_cache(maxsize=None)
def state(sid):
    """(u, b, J): the state the Jacobian is taken at, the right-hand side, the oracle's Jacobian as a dense float64 matrix."""
    s = SYSTEMS[sid]
    u = (s.uscale or USCALE[s.kind]) * np.random.default_rng(s.useed).standard_normal(s.n)
    b = np.random.default_rng(s.bseed).standard_normal(s.n)
    op = oracle_problem(s)
    if s.kind == "sh1d":
        J = op.J(u, SH1D_PARAMS["lam"], SH1D_PARAMS["nu"])
    elif s.kind == "sh":
        J = op.J(u, SH_PARAMS["l"], SH_PARAMS["nu"])
    else:
        J = op.J(u, **CGL_PARAMS)
    J = np.ascontiguousarray(J.toarray())
    for a in (u, b, J):
        a.setflags(write=False)
    return u, b, J


@functools.lru_cache(maxsize=None)
def border(sid):
    """(dR, dzu, dzp, nn) of group D: the border column, row and corner and the last entry of the right-hand side (R is the system's b)."""
    s = SYSTEMS[sid]
    rng = np.random.default_rng(s.bseed + 5000)
    dR, dzu = rng.standard_normal(s.n), rng.standard_normal(s.n)
    dzp, nn = (float(v) for v in rng.standard_normal(2))
    dR.setflags(write=False)
    dzu.setflags(write=False)
    return dR, dzu, dzp, nn


def oracle_preconditioner(sid):
    """The callable v -> Pl^-1 v: (L1 + I)^-1 for SH, the exact inverse of the trivial state's Jacobian for cGL, None for SH1D."""
    s = SYSTEMS[sid]
    if s.kind == "sh":
        return operators.dct_preconditioner(s.dims, s.ls, 1.0)
    if s.kind == "cgl":
        return operators.dst_block_preconditioner_cgl(s.dims, s.ls, CGL_PARAMS["r"], CGL_PARAMS["nu"])
    return None


# ------------------------------------------------------------------------------------------------------------------ cases
@dataclass(frozen=True)
class Case:
    """A linear system as a solver flavor sees it.  ``form``:
      "plain"        (a0 I + a1 J) x = b
      "pl_kk"        (a0 I + a1 Pl^-1 J) x = Pl^-1 b        the KrylovKit branch: shift after the preconditioner
      "pl_is"        Pl^-1 (a0 I + a1 J) x = Pl^-1 b        IterativeSolvers / Krylov.jl
      "bordered"     [J dR; xi_u dzu'/n  xi_p dzp] (x, l) = (b, nn)       MatrixFreeBLS, a0 = 0, a1 = 1
      "bordered_pl"  the same system multiplied by diag(Pl^-1, 1) from the left"""
    sid: str
    a0: float = 0.0
    a1: float = 1.0
    form: str = "plain"
    rtol: float = RTOL

    @property
    def cid(self):
        t = "" if self.rtol == RTOL else f"/rtol{self.rtol:g}"
        return f"{self.sid}/{self.form}/{self.a0:g}_{self.a1:g}{t}"

    @property
    def n(self):
        return SYSTEMS[self.sid].n + (1 if self.form.startswith("bordered") else 0)

    @property
    def flavors(self):
        return {"plain": ("krylovkit", "iterativesolvers", "krylovjl"), "pl_kk": ("krylovkit",), "pl_is": ("iterativesolvers", "krylovjl"),
                "bordered": ("krylovkit", "iterativesolvers", "krylovjl"),
                "bordered_pl": ("krylovkit", "iterativesolvers", "krylovjl")}[self.form]

    @property
    def blocks(self):
        """Whether the library's block Arnoldi serves this form (bordered operators take single steps on the host path)."""
        return not self.form.startswith("bordered")


A_SIDS = tuple(System(k, d, 0, 0).sid for k, d in _GRIDS)
A_CASES = tuple(Case(sid, a0, a1) for sid in A_SIDS for a0, a1 in SHIFTS)
B_SIDS = ("sh1d-5", "sh1d-33", "sh1d-40", "sh1d-63")
B_CASES = tuple(c for c in A_CASES if c.sid in B_SIDS)
F_CASE = Case("sh1d-40", 0.0, 1.0)
G_FOLD_SIDS = ("sh1d-5", "sh1d-9")
G_CHUNK_SIDS = ("sh1d-33", "sh1d-36", "sh1d-40")
# group G, the one case that is NOT an exhaustion case: n = 5 with a tolerance between the residuals at steps 3 and 4 (0.529 and 0.463 of
# ||b||), so that the solve ends at step n - 1 inside a two-step block -- the solution update folds the deferred block in, which a solve
# that exhausts the space never does (its last column always comes from the single-vector path)
G_INSIDE_CASE = Case("sh1d-5", 0.0, 1.0, "plain", 0.495)
# group C: the candidate grids of both problems; C_SIDS = the candidates the reference test certifies (it asserts that these are exactly
# the ones that pass, so a candidate can neither be dropped nor kept by hand)
C_CANDIDATE_SIDS = ("sh-2x2", "sh-3x2", "sh-3x3", "sh-2x2x2", "sh-3x2x2", "sh-4x3x3", "cglp-2x2", "cglp-3x2", "cglp-3x3")
C_SIDS = C_CANDIDATE_SIDS


def c_cases(sid):
    return tuple(Case(sid, a0, a1, form) for form in ("pl_kk", "pl_is") for a0, a1 in SHIFTS)


C_TIGHT_CASE = Case("sh-4x3x3", 0.0, 1.0, "pl_kk", 1e-12)     # the block restatement needs a second cycle here
D_SIDS = ("sh1d-2", "sh1d-3", "sh1d-5", "sh1d-9", "sh1d-33", "sh-3x3")
D_CASES = tuple(Case(sid, form="bordered") for sid in D_SIDS) + (Case("sh-3x3", form="bordered_pl"),)
E_SIDS = ("sh1d-2", "sh1d-3", "sh1d-5")


def lambda_max(sid):
    return float(np.linalg.eigvalsh(state(sid)[2]).max())


def e_cases():
    """Group E: (label, solver kind, Case) -- MINRES on J, MINRES and CG on (lambda_max + 1) I - J."""
    out = []
    for sid in E_SIDS:
        out.append((f"{sid}/minres/J", "minres", Case(sid, 0.0, 1.0)))
        sh = lambda_max(sid) + 1.0
        out.append((f"{sid}/minres/spd", "minres", Case(sid, sh, -1.0)))
        out.append((f"{sid}/cg/spd", "cg", Case(sid, sh, -1.0)))
    return out


def all_gmres_cases():
    """Every GMRES case a GPU test runs (groups B, F and G run cases of A)."""
    out = list(A_CASES)
    for sid in C_SIDS:
        out += c_cases(sid)
    out.append(C_TIGHT_CASE)
    out += D_CASES
    out.append(G_INSIDE_CASE)
    return tuple(out)


# ------------------------------------------------------------------------------------------------------------------ dense algebra
def _bordered_matrix(sid):
    u, b, J = state(sid)
    dR, dzu, dzp, nn = border(sid)
    n = J.shape[0]
    A = np.zeros((n + 1, n + 1))
    A[:n, :n] = J
    A[:n, n] = dR
    A[n, :n] = THETA * dzu / n                 # xi_u * dotp(dzu, .), dotp = <., .> / n
    A[n, n] = (1.0 - THETA) * dzp
    return A, np.concatenate([b, [nn]])


def system(case: Case):
    """(A, rhs) of the case as float64 arrays (the entries of the oracle's operators; extended precision starts from these)."""
    u, b, J = state(case.sid)
    n = J.shape[0]
    if case.form == "plain":
        return case.a0 * np.eye(n) + case.a1 * J, b.copy()
    if case.form == "bordered":
        return _bordered_matrix(case.sid)
    Pl = oracle_preconditioner(case.sid)
    P = np.column_stack([Pl(e) for e in np.eye(n)])
    if case.form == "pl_kk":
        return case.a0 * np.eye(n) + case.a1 * (P @ J), P @ b
    if case.form == "pl_is":
        return P @ (case.a0 * np.eye(n) + case.a1 * J), P @ b
    if case.form == "bordered_pl":
        A, rhs = _bordered_matrix(case.sid)
        Pb = np.eye(n + 1)
        Pb[:n, :n] = P
        return Pb @ A, Pb @ rhs
    raise ValueError(case.form)


def residual_ld(A, rhs, x):
    """||rhs - A x||_2 with products and sums in numpy.longdouble (64-bit mantissa)."""
    r = np.asarray(rhs, dtype=LD) - np.asarray(A, dtype=LD) @ np.asarray(x, dtype=LD)
    return float(np.sqrt(np.sum(r * r)))


def solve_ld(A, rhs):
    """Dense solve in extended precision: float64 LU, refined with longdouble residuals until the correction stops shrinking."""
    import scipy.linalg as sla
    lu = sla.lu_factor(A)
    Al, bl = np.asarray(A, dtype=LD), np.asarray(rhs, dtype=LD)
    x = np.asarray(sla.lu_solve(lu, rhs), dtype=LD)
    last = np.inf
    for _ in range(20):
        d = sla.lu_solve(lu, np.asarray(bl - Al @ x, dtype=np.float64))
        step = float(np.abs(d).max())
        if not step < 0.5 * last:
            break
        x = x + d
        last = step
    return x


def solve_mp(A, rhs, dps=50):
    import mpmath as mp
    with mp.workdps(dps):
        x = mp.lu_solve(mp.matrix(A.tolist()), mp.matrix(rhs.tolist()))
        return np.array([LD(mp.nstr(v, 25)) for v in x], dtype=LD)


def gmres_residuals_mp(A, rhs, dps=60):
    """Exact GMRES residual norms [||r_0||, ||r_1||, .., ||r_n||] of A x = rhs from x0 = 0: Arnoldi (modified Gram-Schmidt) with
    progressive Givens rotations, every operation in mpmath at ``dps`` digits."""
    import mpmath as mp
    with mp.workdps(dps):
        n = len(rhs)
        rows = [[(j, mp.mpf(float(a))) for j, a in enumerate(row) if a != 0.0] for row in A]
        b = [mp.mpf(float(v)) for v in rhs]
        beta = mp.sqrt(mp.fdot(b, b))
        V = [[v / beta for v in b]]
        g = [beta]
        cs, sn = [], []
        res = [float(beta)]
        tiny = mp.mpf(10) ** (-(dps - 8))
        for k in range(n):
            v = V[k]
            w = [mp.fsum(a * v[j] for j, a in row) for row in rows]
            h = []
            for i in range(k + 1):
                hi = mp.fdot(V[i], w)
                Vi = V[i]
                w = [wj - hi * vj for wj, vj in zip(w, Vi)]
                h.append(hi)
            hn = mp.sqrt(mp.fdot(w, w))
            for i in range(k):
                t = cs[i] * h[i] + sn[i] * h[i + 1]
                h[i + 1] = -sn[i] * h[i] + cs[i] * h[i + 1]
                h[i] = t
            r = mp.sqrt(h[k] * h[k] + hn * hn)
            cs.append(h[k] / r)
            sn.append(hn / r)
            g.append(-sn[k] * g[k])
            g[k] = cs[k] * g[k]
            res.append(float(abs(g[k + 1])))
            if hn <= tiny * beta or k + 1 == n:
                res += [res[-1]] * (n - k - 1)
                break
            V.append([wj / hn for wj in w])
        return res


@dataclass
class Ref:
    case: Case
    A: np.ndarray
    rhs: np.ndarray
    x: np.ndarray              # dense solution, longdouble
    sigma_min: float
    norm2: float

    @property
    def bnorm(self):
        return float(np.linalg.norm(self.rhs))

    @property
    def tol(self):
        return self.case.rtol * self.bnorm

    def residual(self, x):
        return residual_ld(self.A, self.rhs, x)

    def error(self, x):
        d = np.asarray(x, dtype=LD) - self.x
        return float(np.sqrt(np.sum(d * d)))

    def error_bound(self, res):
        """||x - x_dense|| <= ||b - A x|| / sigma_min, plus the rounding of the comparison itself: sigma_min comes from a float64 SVD
        (absolute error ~ eps ||A||), x_dense from longdouble refinement (relative error ~ eps_ld cond)."""
        cond = self.norm2 / self.sigma_min
        xn = float(np.sqrt(np.sum(self.x * self.x)))
        n = self.case.n
        return res / self.sigma_min * (1.0 + 4.0 * n * EPS64 * cond) + 4.0 * n * EPSLD * cond * xn


@functools.lru_cache(maxsize=None)
def reference(case: Case) -> Ref:
    A, rhs = system(case)
    sv = np.linalg.svd(A, compute_uv=False)
    x = solve_ld(A, rhs)
    for a in (A, rhs, x):
        a.setflags(write=False)
    return Ref(case, A, rhs, x, float(sv[-1]), float(sv[0]))


# ------------------------------------------------------------------------------------------------------------------ the oracle
def _oracle_solvers(case: Case, Pl, maxcycles, maxiter):
    """flavor -> ls(J, rhs, a0, a1) -> (x, converged, count) on the restatements of oracle.krylov, with the case's settings."""
    rtol = case.rtol
    return {
        "krylovkit": lambda J, r, a0=0.0, a1=1.0: krylov.gmres_krylovkit(J, r, a0, a1, krylovdim=DIM, maxiter=maxcycles, atol=0.0,
                                                                         rtol=rtol, Pl=Pl)[:3],
        "block": lambda J, r, a0=0.0, a1=1.0: krylov.gmres_block(J, r, a0, a1, krylovdim=DIM, maxiter=maxcycles, atol=0.0, rtol=rtol,
                                                                 Pl=Pl, block=4)[:3],
        "iterativesolvers": lambda J, r, a0=0.0, a1=1.0: krylov.gmres_iterativesolvers(J, r, a0, a1, restart=DIM, maxiter=maxiter,
                                                                                       reltol=rtol, abstol=0.0, Pl=Pl),
        "krylovjl": lambda J, r, a0=0.0, a1=1.0: krylov.gmres_krylovjl(J, r, a0, a1, memory=DIM, restart=False, itmax=maxiter, atol=0.0,
                                                                       rtol=rtol, M=Pl),
    }


def oracle_gmres(case: Case, maxcycles=100, maxiter=4000):
    """Counts of the GMRES restatements on the case -- the flavors of the form, and the block restatement next to the KrylovKit one --
    and their true residuals (extended precision, of the system in the case's form)."""
    u, b, J = state(case.sid)
    ref = reference(case)
    Pl = oracle_preconditioner(case.sid) if case.form in ("pl_kk", "pl_is", "bordered_pl") else None
    names = case.flavors + (("block",) if "krylovkit" in case.flavors and case.blocks else ())
    counts, ok, true_res = {}, {}, {}
    if case.form.startswith("bordered"):
        dR, dzu, dzp, nn = border(case.sid)
        n = J.shape[0]
        Pb = (lambda v: np.concatenate([Pl(v[:-1]), v[-1:]])) if Pl is not None else None
        solvers = _oracle_solvers(case, Pb, maxcycles, maxiter)
        for name in names:
            x, l, ok[name], counts[name] = bordered.matrixfree_bls(solvers[name], J, dR, dzu, dzp, b, nn, THETA, 1.0 - THETA,
                                                                   dotp=lambda p, q: float(np.dot(p, q)) / n)
            true_res[name] = ref.residual(np.concatenate([x, [l]]))
    else:
        solvers = _oracle_solvers(case, Pl, maxcycles, maxiter)
        for name in names:
            x, ok[name], counts[name] = solvers[name](J, b, case.a0, case.a1)
            true_res[name] = ref.residual(x)
    return dict(converged={k: bool(v) for k, v in ok.items()}, counts={k: int(v) for k, v in counts.items()}, true_residual=true_res)


def oracle_symmetric(kind, case: Case):
    u, b, J = state(case.sid)
    fn = krylov.minres_krylovjl if kind == "minres" else krylov.cg_krylovjl
    x, ok, it = fn(J, b, case.a0, case.a1, atol=0.0, rtol=case.rtol)
    return dict(converged=bool(ok), count=int(it), true_residual=reference(case).residual(x))


B_RTOL = 1e-17                 # group B: a tolerance no float64 solve can meet


def b_budget(flavor, n):
    """Group B's budgets: 3 restart cycles (KrylovKit counts cycles), 2 n + 5 inner iterations (IterativeSolvers)."""
    return 3 if flavor == "krylovkit" else 2 * n + 5


def b_label(case: Case):
    return case.cid + "/unattainable"


def oracle_unattainable(case: Case):
    """The step-by-step restatements on a case of group B at rtol = 1e-17 within group B's budgets: flavor -> (converged, count), and their
    true residuals relative to ||b||."""
    u, b, J = state(case.sid)
    ref = reference(case)
    n = case.n
    x, ok, nops, _ = krylov.gmres_krylovkit(J, b, case.a0, case.a1, krylovdim=DIM, maxiter=b_budget("krylovkit", n), atol=0.0, rtol=B_RTOL)
    out = dict(outcome={"krylovkit": [bool(ok), int(nops)]}, true_residual={"krylovkit": ref.residual(x) / ref.bnorm})
    x, ok, it = krylov.gmres_iterativesolvers(J, b, case.a0, case.a1, restart=DIM, maxiter=b_budget("iterativesolvers", n), reltol=B_RTOL,
                                              abstol=0.0)
    out["outcome"]["iterativesolvers"] = [bool(ok), int(it)]
    out["true_residual"]["iterativesolvers"] = ref.residual(x) / ref.bnorm
    return out


def certify(case: Case):
    """The conditions that make a case an exhaustion case, on the reference alone: (residual at step n - 1) / tol, (residual at step n)
    / tol, from the extended-precision Arnoldi process.  Certified: the first >= 1e3, the second <= 1e-3."""
    ref = reference(case)
    res = gmres_residuals_mp(ref.A, ref.rhs)
    n = case.n
    return res[n - 1] / ref.tol, res[n] / ref.tol


def record():
    """The numbers the GPU tests take from the oracle: counts per flavor and the oracle's true residuals."""
    out = {}
    for c in all_gmres_cases():
        o = oracle_gmres(c)
        out[c.cid] = dict(n=c.n, counts=o["counts"], true_residual=o["true_residual"])
    for label, kind, c in e_cases():
        o = oracle_symmetric(kind, c)
        out[label] = dict(n=c.n, counts={kind: o["count"]}, true_residual={kind: o["true_residual"]})
    for c in B_CASES:
        out[b_label(c)] = dict(n=c.n, **oracle_unattainable(c))
    return out


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], "usage: python tests/krylov_dense_ref.py --record"
    rec = record()
    with open(GOLDEN, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(rec)} entries -> {GOLDEN}")
