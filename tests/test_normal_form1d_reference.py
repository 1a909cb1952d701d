"""CPU tests of the dense restatement of the normal form at simple branch points and folds (tests/normal_form1d_ref.py): it is
pinned to the answers the reference's own tests hold for the vector field Fbp (test/normal_forms/testNF.jl), to a closed form on
the trivial branch of 2-D Swift-Hohenberg, its predictors to hand values, and its switched branch to the normal form it came
from.  The GPU tests compare the library against this restatement.  Also here: the dispatch of codim2.get_normal_form."""
import json
import math
import os

import numpy as np
import pytest

import minaug_fold_ref as R
import normal_form1d_ref as N
from oracle import bordered, operators, palc

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "normal_form_1d_known_answers.json")))


# ------------------------------------------------------------------------------------------ the reference's own example
def _fbp_model(q):
    """F(x, p) = [x1 (3.23 mu - x2 x1 + x3 x1^2) + x_2, -x_2 + gamma x1^2] with its analytic derivatives."""
    def F(x, q):
        return np.array([x[0] * (3.23 * q["mu"] - q["x2"] * x[0] + q["x3"] * x[0] ** 2) + x[1], -x[1] + q["gamma"] * x[0] ** 2])

    def J(x, q):
        return np.array([[3.23 * q["mu"] - 2 * q["x2"] * x[0] + 3 * q["x3"] * x[0] ** 2, 1.0], [2 * q["gamma"] * x[0], -1.0]])

    d2F = lambda x, q, a, b: np.array([(-2 * q["x2"] + 6 * q["x3"] * x[0]) * a[0] * b[0], 2 * q["gamma"] * a[0] * b[0]])
    d3F = lambda x, q, a, b, c: np.array([6 * q["x3"] * a[0] * b[0] * c[0], 0.0])
    dFdp = lambda x, q, lens: np.array([3.23 * x[0], 0.0])
    dJvdp = lambda x, q, lens, v: np.array([3.23 * v[0], 0.0])
    return R.FoldModel(F, J, d2F, q, "mu", dFdp=dFdp, dJvdp=dJvdp), d3F


@pytest.mark.parametrize("case", GOLD["cases"], ids=lambda c: c["name"])
def test_restatement_reproduces_the_references_known_answers(case):
    q = dict(case["params"])
    model, d3F = _fbp_model(q)
    nf = N.normal_form1d(model, d3F, np.zeros(2), q, "mu", np.array(case["zeta"]), np.array(case["zeta_star"]))
    atol = GOLD["atol"]
    got = dict(a01=nf["a01"], a02=nf["a02"], b11=nf["b11"], b20_half=nf["b20"] / 2, b30_sixth=nf["b30"] / 6, Psi20=nf["Psi20"])
    for k, v in case["expect"].items():
        assert np.abs(np.asarray(got[k]) - np.asarray(v)).max() <= atol, (k, got[k], v)
    if "type" in case:
        assert nf["type"] == case["type"]


def test_normalisation_is_checked():
    q = dict(GOLD["cases"][0]["params"])
    model, d3F = _fbp_model(q)
    with pytest.raises(ValueError, match="normalization"):
        N.normal_form1d(model, d3F, np.zeros(2), q, "mu", np.array([1.0, 0.0]), np.array([0.5, 0.5]))


def test_classification():
    """:339-350"""
    assert N.classify(0.0, 0.0, 3.23, 2 * 3.3, 6 * 0.234) == "Transcritical"
    assert N.classify(0.0, 0.0, 1.0, 1e-4, 6.0) == "Pitchfork"             # 100 |b20 / 2| < |b30 / 6|
    assert N.classify(0.0, 0.0, 1.0, 0.02, 0.9) == "Transcritical"
    assert N.classify(2e-3, 0.0, 1.0, 0.5, 0.9) == "Fold"                  # |a01| >= tol_fold
    assert N.classify(5e-4, 0.0, 1.0, 0.5, 0.9) == "Transcritical"
    assert N.classify(0.0, 0.3, 0.0, 0.5, 0.9) == "BranchPoint"
    assert N.classify(1e-11, 1e-4, 1e-11, 0.5, 0.9) == "NonQuadraticParameter"


# ------------------------------------------------------------------------------------------ Swift-Hohenberg closed form
def _sh_case():
    g = GOLD["sh_closed_form"]
    dims, ls, jk, nu = tuple(g["dims"]), tuple(g["half_lengths"]), tuple(g["mode"]), g["nu"]
    cf = N.sh_trivial_closed_form(dims, ls, jk, nu)
    op = operators.SwiftHohenberg(dims, ls)
    model = R.sh_model(op, "sh", dict(l=cf["lstar"], nu=nu), "l")
    return g, cf, op, model, N.sh_d3F("sh", ["l", "nu"])


def test_sh_trivial_branch_closed_form():
    g, cf, op, model, d3F = _sh_case()
    n = cf["zeta"].shape[0]
    J = op.J(np.zeros(n), cf["lstar"], g["nu"]).toarray()
    e = np.sort(np.abs(np.linalg.eigvalsh(J)))
    assert np.abs(J @ cf["zeta"]).max() <= 1e-13 and e[0] <= 1e-13 and 9e-3 < e[1] < 1e-2      # simple: the next one is 9.5e-3 away
    nf = N.normal_form1d(model, d3F, np.zeros(n), model.at(cf["lstar"]), "l", cf["zeta"], cf["zeta"])
    for k in ("a01", "a02", "b20"):
        assert abs(nf[k]) <= 1e-14, (k, nf[k])
    assert abs(nf["b11"] - 1.0) <= 1e-14
    assert abs(cf["b30"] - g["b30"]) <= g["rtol"] * abs(g["b30"])
    assert abs(nf["b30"] - cf["b30"]) <= g["rtol"] * abs(cf["b30"]), (nf["b30"], cf["b30"])
    assert np.abs(nf["Psi20"] - cf["Psi20"]).max() <= g["rtol"] * np.abs(cf["Psi20"]).max()
    assert np.abs(nf["Psi01"]).max() <= 1e-14
    assert nf["type"] == "Pitchfork" and nf["b11"] * nf["b30"] > 0                              # subcritical
    # in nu: dF/dnu = u^2 = 0 and dJ/dnu = 2 u = 0 on u = 0, so a01 = b11 = 0: not a bifurcation in nu
    m2 = R.sh_model(op, "sh", dict(l=cf["lstar"], nu=g["nu"]), "nu")
    nf2 = N.normal_form1d(m2, d3F, np.zeros(n), m2.at(g["nu"]), "nu", cf["zeta"], cf["zeta"])
    assert nf2["type"] == "NonQuadraticParameter" and abs(nf2["b30"] - cf["b30"]) <= g["rtol"] * abs(cf["b30"])


def test_bordering_with_gmres_agrees_with_the_direct_bordered_solve():
    """The yardstick of the solver-dependent GPU tolerances: BorderingBLS with SciPy GMRES at reltol against the direct solve of
    the (n + 1) matrix, at a point that is singular only up to the bisection accuracy (an exactly singular J has no J \\ zeta*)."""
    g, cf, op, model, d3F = _sh_case()
    n = cf["zeta"].shape[0]
    rng = np.random.default_rng(3)
    x = 1e-3 * rng.standard_normal(n)
    p = cf["lstar"] + 1e-6
    J = op.J(x, p, g["nu"]).toarray()
    w, V = np.linalg.eigh(J)
    z = V[:, np.argmin(np.abs(w))]
    lu = N.normal_form1d(model, d3F, x, model.at(p), "l", z, z)
    reltol = 1e-10
    gm = N.normal_form1d(model, d3F, x, model.at(p), "l", z, z, solver="bordering", reltol=reltol, restart=n, maxiter=2)
    # a relative residual reltol leaves a relative error <= reltol cond(J on the complement of zeta) = reltol |J| / |lambda_2| in
    # each Psi (the component along zeta is removed by the elimination); the coefficients are inner products with them
    a = np.sort(np.abs(w))
    bound = reltol * a[-1] / a[1]
    spread = {k: abs(gm[k] - lu[k]) / max(1.0, abs(lu[k])) for k in ("a01", "a02", "b11", "b20", "b30")}
    spread.update({k: np.abs(gm[k] - lu[k]).max() / max(np.abs(lu[k]).max(), 1.0) for k in ("Psi01", "Psi20")})
    print("bordering + GMRES against the direct bordered solve:", spread, "bound", bound)
    assert max(spread.values()) <= bound, (spread, bound)


# ------------------------------------------------------------------------------------------ predictors
def test_predictor_formulas_against_hand_values():
    z, x0 = np.array([1.0, 0.0]), np.array([0.5, -0.25])
    P01 = np.array([0.0, 2.0])
    # Transcritical, tau not along zeta: amp = -2 ds b11 / b20 (:402), x1 = x0 + amp zeta - ds Psi01 (:417)
    nf = dict(type="Transcritical", a01=0.0, a02=0.0, b11=3.23, b20=-2.24, b30=1.0, Psi01=P01)
    pr = N.predictor(nf, x0, 0.1, z, (np.zeros(2), 1.0), 0.1)
    amp = -2 * 0.1 * 3.23 / -2.24
    assert pr["amp"] == pytest.approx(amp, rel=1e-15) and pr["p"] == pytest.approx(0.2) and pr["pm1"] == pytest.approx(0.0)
    assert np.allclose(pr["x1"], [0.5 + amp, -0.25 - 0.2], rtol=0, atol=1e-15)
    assert np.allclose(pr["xm1"], [0.5 - amp, -0.25 + 0.2], rtol=0, atol=1e-15) and pr["x0"] is x0
    # ... tau along zeta: the computed branch IS the x-axis of the normal form (:410-414)
    pr = N.predictor(nf, x0, 0.1, z, (np.array([2.0, 0.1]), 0.5), 0.1)
    assert np.allclose(pr["x1"], x0 + 0.1 * P01) and np.allclose(pr["xm1"], x0)
    assert np.allclose(pr["x0"], x0 + 0.1 / 0.5 * np.array([2.0, 0.1]))
    # Pitchfork: dsfactor = +1 iff b11 b30 < 0 (:465), amp = sqrt(-6 |ds| dsfactor b11 / b30) (:468)
    for b30, side in ((-6.0, 1.0), (6.0, -1.0)):
        nf = dict(type="Pitchfork", a01=0.0, a02=0.0, b11=2.0, b20=0.0, b30=b30, Psi01=P01)
        for ds in (0.02, -0.02):
            pr = N.predictor(nf, x0, 1.0, z, (np.zeros(2), 1.0), ds, ampfactor=1.5)
            assert pr["dsfactor"] == side and pr["p"] == pytest.approx(1.0 + 0.02 * side)
            assert pr["amp"] == pytest.approx(1.5 * math.sqrt(6 * 0.02 * 2.0 / 6.0), rel=1e-15)
            assert np.allclose(pr["x1"], x0 + pr["amp"] * z, rtol=0, atol=1e-15)
    assert N.predictor(dict(type="Fold"), x0, 0.0, z, None, 0.1) is None
    # BranchPoint: g = p^2 / 2 - x^2 / 2 (a02 = 1, b20 = -1): the four zeros on the circle are at 45, 135, 225, 315 degrees;
    # the one nearest orthogonal to tau = (zeta, 1) / sqrt 2 ... is x = -p: two candidates, the first in angle order is kept
    nf = dict(type="BranchPoint", a01=0.0, a02=1.0, b11=0.0, b20=-1.0, b30=0.0, Psi01=P01)
    pr = N.predictor(nf, x0, 0.0, z, (z, 1.0), 0.1)
    th = sorted(s[2] for s in pr["solutions"])
    assert np.allclose(th, np.pi * np.array([0.25, 0.75, 1.25, 1.75]), rtol=0, atol=1e-12)
    r = 0.1 / math.sqrt(2)
    assert pr["dp"] == pytest.approx(r, abs=1e-14) and np.allclose(pr["x1"], x0 - r * z, rtol=0, atol=1e-14)


# ------------------------------------------------------------------------------------------ the switched branch
def test_switched_branch_leaves_the_trivial_state_on_the_predicted_side():
    """Branch switching on the restatement itself (dense PALC from the two points): the switched branch of the SH pitchfork
    lives on the side dsfactor says, |s| = |<x - x0, zeta>| grows along it, and the defect of b11 dp + b30 s^2 / 6 = 0, being
    O(s^4), grows with |s| even after division by s^2."""
    g, cf, op, model, d3F = _sh_case()
    n = cf["zeta"].shape[0]
    nu, lstar, z = g["nu"], cf["lstar"], cf["zeta"]
    nf = N.normal_form1d(model, d3F, np.zeros(n), model.at(lstar), "l", z, z)
    prob = palc.Problem(lambda x, p: op.F(x, p, nu), lambda x, p: op.J(x, p, nu), dparam_factor=lambda x, p: x)
    bls = lambda *a, **k: bordered.bordering_bls(bordered.default_ls, *a, check_precision=False, **k)
    ds = 2e-3
    pr = N.predictor(nf, np.zeros(n), lstar, z, (np.zeros(n), 1.0), ds)
    assert pr["dsfactor"] == -1.0 and pr["p"] < lstar                      # subcritical: the branch lives below l*
    br = N.continuation_two_points(prob, pr["x0"], lstar, pr["x1"], pr["p"], ls=bordered.default_ls, bls=bls, ds=ds, dsmin=ds,
                                   dsmax=ds, p_min=lstar - 1.0, p_max=lstar + 1.0, max_steps=3, tol=1e-12, normC=palc.norminf)
    assert len(br.param) == 4 and br.ds[0] == -ds                          # ds signed by p1 - p0
    s = np.array([float(np.dot(x, z)) for x in br.sol])
    dp = np.array(br.param) - lstar
    assert s[0] == 0.0 and np.all(np.diff(np.abs(s)) > 0) and np.all(dp[1:] < 0)
    q = np.abs(nf["b11"] * dp[1:] + nf["b30"] * s[1:] ** 2 / 6) / s[1:] ** 2
    print("s", s, "dp", dp, "defect / s^2", q)
    assert np.all(np.diff(q) > 0), q


def test_switched_branch_defect_is_fourth_order():
    """The restatement's own switched branch obeys the normal form: with s = <x - x0, zeta> at the dense-Newton point of the
    branch at p = l* + dp, the defect |b11 dp + b30 s^2 / 6| is fourth order in s ~ sqrt |dp|, so halving ds reduces it by a
    factor >= 3 (4 in the limit)."""
    g, cf, op, model, d3F = _sh_case()
    n = cf["zeta"].shape[0]
    nu, lstar, z = g["nu"], cf["lstar"], cf["zeta"]
    nf = N.normal_form1d(model, d3F, np.zeros(n), model.at(lstar), "l", z, z)
    ls = bordered.default_ls
    defect = []
    for ds in (2e-3, 1e-3):
        pr = N.predictor(nf, np.zeros(n), lstar, z, (np.zeros(n), 1.0), ds)
        prob = palc.Problem(lambda x, p: op.F(x, p, nu), lambda x, p: op.J(x, p, nu))
        sol = palc.newton(prob, pr["x1"], pr["p"], ls, tol=1e-13, max_iterations=20, normN=palc.norminf)
        assert sol["converged"]
        s = float(np.dot(sol["u"], z))
        assert abs(s) > 0.5 * pr["amp"]
        defect.append(abs(nf["b11"] * (pr["p"] - lstar) + nf["b30"] * s * s / 6))
    print("defect of the normal form at ds, ds / 2:", defect)
    assert defect[0] >= 3 * defect[1], defect


# ------------------------------------------------------------------------------------------ dispatch (no GPU needed)
def test_get_normal_form_dispatches_on_the_problem_type(monkeypatch):
    """codim2.get_normal_form sends "bp" / "fold" points of a Swift-Hohenberg problem to normal_form1d.get_normal_form1d and
    keeps its NotImplementedError for "nd" points and for every non-Hopf point of another problem."""
    from bk_amd import codim2, hip
    from bk_amd import normal_form1d as N1
    calls = []
    monkeypatch.setattr(N1, "get_normal_form1d", lambda br, ind, prob, ls, **kw: calls.append((ind, sorted(kw))) or "record")
    sh = hip.SwiftHohenberg.__new__(hip.SwiftHohenberg)
    sh1 = hip.SwiftHohenberg1D.__new__(hip.SwiftHohenberg1D)
    cgl = hip.CGL2d.__new__(hip.CGL2d)
    br = type("B", (), dict(specialpoint=[dict(type="bp"), dict(type="fold"), dict(type="nd")]))()
    assert codim2.get_normal_form(br, 0, sh, None) == "record" and codim2.get_normal_form(br, 1, sh1, None) == "record"
    assert [c[0] for c in calls] == [0, 1] and "bls" in calls[0][1] and "refine" in calls[0][1]
    with pytest.raises(NotImplementedError, match="newton_fold"):
        codim2.get_normal_form(br, 2, sh, None)
    for i in range(3):
        with pytest.raises(NotImplementedError, match="newton_fold"):
            codim2.get_normal_form(br, i, cgl, None)
    assert len(calls) == 2
    with pytest.raises(ValueError, match="cannot branch from a :fold"):
        N1.continuation_from_branch_point(br, 1, sh, None, None)
    assert N1.classify(0.0, 0.0, 1.0, 0.0, 1.0) == "Pitchfork"


def test_library_exports_the_normal_form_entries():
    """The six entries of the 1-D normal form are declared in the header, bound by ctypes and exported by the built library."""
    import ctypes
    import re

    from bk_amd import _lib
    names = ["bk_d3f", "bk_nf1d_dots", "bk_nf1d_rhs", "bk_nf1d_contract", "bk_nf1d_predict", "bk_normal_form_1d"]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "bkhip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in names:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert len(_lib.SIGNATURES["bk_normal_form_1d"][1]) == 16
