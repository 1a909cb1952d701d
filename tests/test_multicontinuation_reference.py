"""CPU tests of the multicontinuation restatement (tests/multicontinuation_ref.py) and of the host logic of
bk_amd.normal_form_nd.get_first_points_on_branch: the one-solve Newton step against DeflatedProblemCustomLS's two solves, the
analytic dM against an extended-precision difference quotient, the counts and classes of the states found next to the 2-d and 3-d
branch points of Swift-Hohenberg under both stopping rules, the found / lost / duplicate / trivial bookkeeping on a stub problem,
and the C boundary."""
import math
import os
import warnings

import numpy as np
import pytest

import multicontinuation_ref as MC

EPS = np.finfo(float).eps
LD = np.longdouble


def _random_setup(seed, n_roots, dims=(8, 6)):
    from oracle import operators
    op = operators.SwiftHohenberg(dims, (3.0, 2.0))
    rng = np.random.default_rng(seed)
    u = 0.4 * rng.standard_normal(op.N)
    roots = [u + (0.3 + 0.2 * k) * (lambda v: v / np.linalg.norm(v))(rng.standard_normal(op.N)) for k in range(n_roots)]
    return op, rng, u, roots


# ------------------------------------------------------------------------------------------ 1: the one-solve step
@pytest.mark.parametrize("n_roots", [1, 3, 9])
@pytest.mark.parametrize("mean", [False, True], ids=["prod", "mean"])
def test_one_solve_step_equals_the_two_solve_formula(n_roots, mean):
    """h = (h1 - z h2) / M with h1 = J^-1 (M F), h2 = J^-1 F against M / (M + dM.h2) h2 at a random u, random roots 0.3 .. 1.9 away
    and a random F, J the dense SH Jacobian at u.  Both forms are exact rearrangements of each other; they differ by the
    rounding of the solves: each solve carries a forward error of eps kappa(J) |h| at most (times a modest constant: LU with
    partial pivoting on n = 48), the two-solve form uses two of them and a dM of each, the one-solve form one.  Allowed:
    8 eps kappa(J) |h|, kappa computed here."""
    op, rng, u, roots = _random_setup(5 + n_roots, n_roots)
    J = op.J(u, 0.1, 1.2).toarray()
    F = rng.standard_normal(op.N)
    kappa = np.linalg.cond(J)
    solve = lambda b: np.linalg.solve(J, b)
    a = MC.step_two_solves(solve, F, u, roots, mean=mean)
    b = MC.step_one_solve(solve, F, u, roots, mean=mean)
    diff, bound = float(np.linalg.norm(a - b)), 8 * EPS * kappa * float(np.linalg.norm(b))
    print(f"k = {n_roots} mean = {mean}: |two - one| = {diff:.3e}, bound {bound:.3e}, kappa = {kappa:.3e}")
    assert np.linalg.norm(b) > 0 and diff <= bound, (diff, bound)


# ------------------------------------------------------------------------------------------ 2: exact dM
@pytest.mark.parametrize("n_roots", [1, 2, 9, 17])
@pytest.mark.parametrize("mean", [False, True], ids=["prod", "mean"])
def test_analytic_dM_matches_an_extended_precision_difference_quotient(n_roots, mean):
    """dM(u) . h in fp64 against the central quotient (M(u + delta h) - M(u - delta h)) / (2 delta) in np.longdouble at
    delta = 1e-6 |h| = 1.  The quotient's own error is measured by halving delta (truncation falls by 4: the difference of the
    two quotients is 3/4 of it); allowed is 10 x that difference plus the rounding of the fp64 formula, 8 n eps per sum carried
    through d^-3 e: (3 + 1) 8 n eps sum_i |c_i| sum |t_i h| with c_i the coefficient of e_i."""
    op, rng, u, roots = _random_setup(40 + n_roots, n_roots)
    n = op.N
    h = rng.standard_normal(n)
    h /= np.linalg.norm(h)
    kw = dict(mean=mean)
    got = MC.dM_exact(u, h, roots, **kw)

    def quotient(delta):
        Mp = MC.combine(MC.sums(u.astype(LD) + LD(delta) * h.astype(LD), roots, dtype=LD)[0], **kw)[0]
        Mm = MC.combine(MC.sums(u.astype(LD) - LD(delta) * h.astype(LD), roots, dtype=LD)[0], **kw)[0]
        return (Mp - Mm) / (2 * LD(delta))

    q1, q2 = quotient(1e-6), quotient(5e-7)
    d, _ = MC.sums(u, roots, h)
    _, te = MC.sum_terms(u, roots, h)
    coef = [abs(MC.combine(d, [1.0 if j == i else 0.0 for j in range(n_roots)], **kw)[1]) for i in range(n_roots)]
    rounding = 4 * 8 * n * EPS * sum(c * float(np.abs(t).sum()) for c, t in zip(coef, te))
    allowed = 10 * float(abs(q1 - q2)) + rounding
    print(f"k = {n_roots} mean = {mean}: dM = {got:.16e}, |dM - quotient| = {abs(got - float(q2)):.3e}, allowed {allowed:.3e}")
    assert got != 0.0 and abs(got - float(q2)) <= allowed


# ------------------------------------------------------------------------------------------ 3: counts and classes
@pytest.mark.parametrize("theta", [0.0, 0.3, 0.7])
@pytest.mark.parametrize("dp", [0.008, 0.002])
def test_first_points_2d_finds_all_eight_states(theta, dp):
    """16 x 16 SH, modes (1, 2), (2, 1), nu = 1.3, kernel basis rotated by theta: 8 states after the point, none before, none
    lost or duplicate, by the plain rule; 4 rolls and 4 squares by their mode coordinates; all distinct."""
    fp = MC.sh_first_points(2, theta, dp)
    c = MC.sh_case(2, theta)
    print([(r["side"], r["status"], r["itnewton"], r["residual"], r["min_dist"]) for r in fp["records"]])
    assert len(fp["zeros"]["after"]) == 9 and len(fp["zeros"]["before"]) == 1
    assert MC.count(fp, "after", "found") == 8 and MC.count(fp, "before", "found") == 0
    assert all(r["status"] in ("found", "trivial") for r in fp["records"])
    assert len(fp["after"]) == 9 and len(fp["before"]) == 1
    assert MC.class_counts(c["Q"], fp["after"][1:]) == {1: 4, 2: 4}
    assert MC.smallest_pairwise_distance(fp["after"]) > 0.09                        # 0.30 at dp = 0.008 .. 0.096 at 0.001
    for x in fp["after"][1:]:
        assert np.abs(c["F"](x, c["p"] + dp)).max() < 1e-10


def test_first_points_3d_finds_all_twenty_six_states():
    """8 x 8 x 8 SH, half-lengths 2.5, modes (2,0,0), (0,2,0), (0,0,2), nu = 0.9, dp = 1e-4: the 27 zeros lie before the point; 26
    states found, none after; 6 on one mode, 12 on two, 8 on three."""
    fp = MC.sh_first_points(3, 0.0, 1e-4)
    c = MC.sh_case(3, 0.0)
    assert len(fp["zeros"]["before"]) == 27 and len(fp["zeros"]["after"]) == 1
    assert MC.count(fp, "before", "found") == 26 and MC.count(fp, "after", "found") == 0
    assert all(r["status"] in ("found", "trivial") for r in fp["records"])
    assert MC.class_counts(c["Q"], fp["before"][1:]) == {1: 6, 2: 12, 3: 8}
    assert MC.smallest_pairwise_distance(fp["before"]) > 0.1


def test_reference_stopping_rule_loses_zeros_close_to_the_point():
    """The same walk stopping on |M F| < tol at dp = 0.004: fewer than 8 found, the rest recorded as "lost" (they sit on their
    zero with |F| at its rounding floor and |M| |F| above the tolerance), where the plain rule finds 8."""
    ref = MC.sh_first_points(2, 0.0, 0.004, stop_plain=False)
    plain = MC.sh_first_points(2, 0.0, 0.004, stop_plain=True)
    found, lost = MC.count(ref, "after", "found"), MC.count(ref, "after", "lost")
    print("reference rule:", [(r["status"], r["itnewton"], r["residual"]) for r in ref["records"] if r["side"] == "after"])
    assert found < 8 and lost == 8 - found and lost > 0
    assert MC.count(plain, "after", "found") == 8 and MC.count(plain, "after", "lost") == 0
    # |F| < tol follows from |M F| < tol (alpha = 1, M >= 1): whatever the reference's rule found is a zero by the plain rule too
    c = MC.sh_case(2, 0.0)
    for x in ref["after"][1:]:
        assert np.abs(c["F"](x, c["p"] + 0.004)).max() < 1e-10


# ------------------------------------------------------------------------------------------ 4: bookkeeping on a stub
class _Vec:
    """A host vector with the few methods get_first_points_on_branch uses."""

    def __init__(self, a):
        self.a = np.array(a, dtype=float)

    def copy(self):
        return _Vec(self.a)

    def norm(self):
        return float(np.linalg.norm(self.a))


class _StubBP:
    N, p = 2, 0.5
    x0 = _Vec([0.0, 0.0])

    def __call__(self, x, dp=0.0):
        return _Vec(x)


class _NewtonPar:
    tol, max_iterations = 1e-10, 20


def test_first_points_bookkeeping_on_a_stub_problem():
    """get_first_points_on_branch with a stub solver: a start with a negative first coordinate does not converge ("lost"), every
    other start converges to its coordinates rounded to one decimal.  Each side has its own operator starting from a copy of x0;
    the origin is "trivial" and not tried; a state that lands on a held root is "duplicate" and not pushed; the lost ones are
    named by one warning per side; records keep the order of the zeros; the solver sees tol, max_iter_deflation, the norm, the
    rule and the side's parameter."""
    from bk_amd import continuation as Cn
    from bk_amd import normal_form_nd as ND
    calls = []

    def solver(prob, defop, x, p, ls, tol, max_iterations, norm_inf, stop_plain):
        assert defop.autodiff and defop.power == 2 and defop.alpha == 1.0
        calls.append(dict(p=p, tol=tol, nmax=max_iterations, inf=norm_inf, plain=stop_plain, held=len(defop)))
        u = _Vec(np.round(x.a, 1))
        dmin = min(float(np.linalg.norm(u.a - r.a)) for r in defop.roots)
        ok = x.a[0] >= 0
        return dict(u=u, converged=ok, itnewton=3 if ok else max_iterations, residuals=[1.0, 1e-11 if ok else 0.5], min_dist=dmin)

    zeros = dict(after=[np.zeros(2), [0.3, 0.0], [0.31, 0.04], [-0.3, 0.0], [0.0, 0.3], [1e-9, 0.0]],
                 before=[np.zeros(2), [-1.0, 1.0], [0.3, 0.0]])
    bp = _StubBP()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        fp = ND.get_first_points_on_branch(bp, zeros, None, None, _NewtonPar(), -0.01, normC=Cn.norminf, solver=solver)
    assert [r["status"] for r in fp.records] == ["trivial", "found", "duplicate", "lost", "found", "duplicate",
                                                 "trivial", "lost", "found"]
    assert [(r["side"], r["index"]) for r in fp.records] == [("after", k) for k in range(6)] + [("before", k) for k in range(3)]
    assert [len(fp.after), len(fp.before)] == [3, 2] and fp.after.roots[0] is not bp.x0 and fp.before.roots[0] is not fp.after.roots[0]
    assert fp.bpp == 0.51 and fp.bpm == 0.49
    assert fp.count("after", "found") == 2 and fp.count("after", "lost") == 1 and fp.count("before", "lost") == 1
    msgs = [str(x.message) for x in w]
    assert len(msgs) == 2 and "1 of the 6 predicted zeros after" in msgs[0] and "1 of the 3 predicted zeros before" in msgs[1]
    assert [c["held"] for c in calls] == [1, 2, 2, 2, 3, 1, 1]
    assert all(c["tol"] == 1e-10 and c["nmax"] == 50 and c["inf"] and c["plain"] for c in calls)
    assert [c["p"] for c in calls] == [0.51] * 5 + [0.49] * 2
    r = fp.records[2]
    assert r["itnewton"] == 3 and r["residual"] == 1e-11 and r["min_dist"] == 0.0 and fp.records[0]["min_dist"] is None
    # the reference's rule, a perturbed guess and an iteration cap of the caller's travel to the solver
    calls.clear()
    fp = ND.get_first_points_on_branch(bp, dict(before=[], after=[[0.2, 0.0]]), None, None, _NewtonPar(), 0.01, max_iter_deflation=7,
                                       perturb_guess=lambda v: _Vec(v.a + 0.2), stop_plain=False, solver=solver)
    assert calls == [dict(p=0.51, tol=1e-10, nmax=7, inf=False, plain=False, held=1)]
    assert fp.records[0]["status"] == "found" and np.array_equal(fp.after.roots[1].a, [0.4, 0.2])
    with pytest.raises(TypeError, match="normC"):
        ND.get_first_points_on_branch(bp, zeros, None, None, _NewtonPar(), 0.01, normC=max, solver=solver)


def test_deflation_operator_combine_matches_the_restatement():
    """hip.DeflationOperator.combine (the host formula of the autodiff path, the library's order) against the restatement's, for
    both accumulators, k = 1 .. 17, and a root on u: M infinite, no exception."""
    from bk_amd import hip
    rng = np.random.default_rng(9)
    for mean in (False, True):
        for k in (1, 2, 8, 9, 17):
            d = list(rng.uniform(0.05, 2.0, k))
            e = list(rng.standard_normal(k))
            op = hip.DeflationOperator(2, 1.0, [None] * k, accumulator="mean" if mean else "prod", autodiff=True)
            M, dM = op.combine(d, e)
            Mr, dMr = MC.combine([LD(x) for x in d], [LD(x) for x in e], mean=mean)
            assert abs(M - float(Mr)) <= 4 * k * EPS * abs(float(Mr))
            terms = [abs(float(MC.combine([LD(x) for x in d], [LD(e[i]) if j == i else LD(0) for j in range(k)], mean=mean)[1]))
                     for i in range(k)]
            assert abs(dM - float(dMr)) <= 8 * k * EPS * sum(terms)
    op = hip.DeflationOperator(2, 1.0, [None, None], autodiff=True)
    M, dM = op.combine([0.0, 0.5], [0.0, 0.1])
    assert math.isinf(M)
    assert op.combine([], [])[0] == 1.0 and hip.DeflationOperator(2, 1.0).autodiff is False


# ------------------------------------------------------------------------------------------ 5: the C boundary
def test_library_exports_the_deflation_entries():
    """The two entries are declared in the header, bound by ctypes and exported by the built library; the result struct has the
    layout of the header; the ABI version stays."""
    import ctypes
    import re

    from bk_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "bkhip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ["bk_deflation_dots", "bk_newton_deflated_exact"]:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert len(_lib.SIGNATURES["bk_deflation_dots"][1]) == 8 and len(_lib.SIGNATURES["bk_newton_deflated_exact"][1]) == 15
    R = _lib.DeflatedResult
    assert ctypes.sizeof(R) == 16 + 8 * (_lib.BK_MAX_NEWTON_ITER + 1) + 16 and R.M.offset == 16 + 8 * (_lib.BK_MAX_NEWTON_ITER + 1)
    assert ctypes.sizeof(_lib.NewtonResult) == 16 + 8 * (_lib.BK_MAX_NEWTON_ITER + 1)
    assert re.search(r"#define\s+BK_ABI_VERSION\s+6\b", hdr) and _lib.BK_ABI_VERSION == 6
    mk = open(os.path.join(root, "bifurcationkit.jl_amd", "csrc", "Makefile")).read()
    assert "deflate.hip" in mk and "-ffp-contract=off" in mk
