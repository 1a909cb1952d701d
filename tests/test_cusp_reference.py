"""The CPU restatement of the cusp on fold curves (tests/cusp_ref.py) against the known answers the reference's own tests hold
(tests/golden/reference_cusp_answers.json), the third-derivative formulas the device passes evaluate against central differences
of the oracle Jacobians, and the Swift-Hohenberg cusp fixture (tests/golden/sh_cusp_128x2.npz) re-derived from its fold point."""
import json
import os

import numpy as np
import pytest

import cusp_ref as Cr
import minaug_fold_ref as R
from oracle import operators, palc
from test_fold_reference import Q, _com_F, _com_J, _comodel, _null_vectors
from test_reference_known_answers import _both_sides

HERE = os.path.dirname(__file__)
GOLD = json.load(open(os.path.join(HERE, "golden", "reference_cusp_answers.json")))


# ---------------------------------------------------------------------------------------------- the scalar cusp
def _scalar_model():
    P = dict(b1=GOLD["scalar_cusp"]["beta1"], b2=GOLD["scalar_cusp"]["beta2"], c=GOLD["scalar_cusp"]["c"])
    F = lambda x, q: np.array([q["b1"] + q["b2"] * x[0] + q["c"] * x[0] ** 3])
    J = lambda x, q: np.array([[q["b2"] + 3 * q["c"] * x[0] ** 2]])
    B = lambda x, q, a, b: np.array([6 * q["c"] * x[0] * a[0] * b[0]])
    C = lambda x, q, a, b, c: np.array([6 * q["c"] * a[0] * b[0] * c[0]])
    return Cr.CuspModel(R.FoldModel(F, J, B, P, "b1", "b2"), C), P


def test_scalar_cusp_has_the_coefficient_of_the_reference_test():
    """testNF.jl:452-471: F = beta1 + beta2 x + c x^3, the fold curve in (beta1, beta2) from beta2 = -0.01 with the options of the
    reference test; the cusp sits at beta1 = beta2 = 0, x = 0, and the normal form returns c itself: q = p = 1, C(q, q, q) = 6 c
    and H2 = 0 in exact arithmetic, so the comparison is ==, as in the reference."""
    m, P = _scalar_model()
    x0 = np.sqrt(-P["b2"] / (3 * P["c"]))
    one = np.ones(1)
    sn = R.newton_fold(m, [x0], -(P["b2"] * x0 + P["c"] * x0 ** 3), one, one, tol=1e-12)
    assert sn["converged"]
    kw = dict(ds=0.01, dsmin=0.001, dsmax=0.02, p_min=-0.3, p_max=0.1, max_steps=40)
    br = Cr.continuation_fold(m, sn["u"], sn["p"], P["b2"], one, one, detect_codim2=2, n_inversion=8, **kw)
    assert [s["type"] for s in br["specialpoint"]] == ["cusp"]
    sp = br["specialpoint"][0]
    i = sp["idx"]
    # CP of a point is the secant over the step that led to it: the sign change of b2 lies within the two steps before point i
    assert br["CP"][i - 1] * br["CP"][i] < 0 and br["b2"][i - 2] * br["b2"][i] < 0, (br["CP"][:i + 1], br["b2"][:i + 1])
    assert sp["n_inversion"] >= 1 and sp["CP_interval"][0] * sp["CP_interval"][1] < 0
    X = sp["X"]
    nf = Cr.cusp_at_fold(m, X[:-1], m.at(X[-1], sp["p2"]))
    assert nf["c"] == P["c"], nf
    # The located point against the cusp x = 0.  A bisection in PALC steps ends within 3 ``reach`` of the crossing along the curve
    # (reach = the ds of the last step that passed it: the secant event sees a crossing one step late, so it lies in that step or
    # in the second half of the twice as long one before).  |tau|_theta = 1 with theta = 1/2 and N = 2 bounds |dx/ds| by 2, and on
    # the fold curve beta2 = -3 c x^2, beta1 = 2 c x^3, b2 = 6 c x.
    print(f"scalar cusp: located beta1 {sp['p1']:.3e} beta2 {sp['p2']:.3e} x {X[0]:.3e} b2 {sp['b2']:.3e} after {sp['bisection_steps']} "
          f"bisection steps, {sp['n_inversion']} inversions, reach {sp['reach']:.3e}")
    xb = 2.0 * 3.0 * sp["reach"]
    assert abs(X[0]) <= xb, (X[0], xb)
    assert abs(sp["p2"]) <= 3 * P["c"] * xb ** 2 and abs(sp["p1"]) <= 2 * P["c"] * xb ** 3 and abs(sp["b2"]) <= 6 * P["c"] * xb
    assert abs(sp["b2"] - 6 * P["c"] * X[0]) <= 1e-12 and abs(X[0]) < min(abs(br["X"][j][0]) for j in (i - 2, i))
    # detection off: the curve of minaug_fold_ref, bit for bit; detection 1: the same points and a guess
    br0 = Cr.continuation_fold(m, sn["u"], sn["p"], P["b2"], one, one, **kw)
    rr = R.continuation_fold(m, sn["u"], sn["p"], P["b2"], one, one, **kw)
    br1 = Cr.continuation_fold(m, sn["u"], sn["p"], P["b2"], one, one, detect_codim2=1, **kw)
    for k in ("p1", "p2", "BT", "CP"):
        assert br0[k] == rr[k] == br1[k] == br[k], k
    assert br0["specialpoint"] == [] and [s["status"] for s in br1["specialpoint"]] == ["guess"]
    assert br1["specialpoint"][0]["idx"] == i


# ---------------------------------------------------------------------------------------------- the CO model
@pytest.fixture(scope="module")
def comodel_cusp():
    """COModel.jl:38-64 with the reference's own options, from the q2 = 1.04205 fold of the q2 branch."""
    sp, _ = _both_sides(palc.Problem(lambda u, p: _com_F(u, {**Q, "q2": p}), lambda u, p: _com_J(u, {**Q, "q2": p})),
                        np.array([0.001137, 0.891483, 0.062345]), 1.0, ds=0.002, dsmax=0.01, p_min=0.5, p_max=2.3, max_steps=100,
                        nev=3, n_inversion=6, max_bisection_steps=25, tangent="secant")
    g = sp[2]
    assert abs(g["param"] - 1.04204851) <= 1e-6
    m = _comodel()
    z, zs = _null_vectors(_com_J(g["x"], m.at(g["param"])))
    sn = R.newton_fold(m, g["x"], g["param"], zs, z, tol=1e-12, max_iterations=10)
    assert sn["converged"]
    m2 = Cr.CuspModel(_comodel("k"), lambda x, q, a, b, c: np.zeros(3))           # quadratic model: d3F = 0
    a, b = sn["w"] / np.linalg.norm(sn["w"]), sn["v"] / np.linalg.norm(sn["v"])
    kw = dict(ds=-0.001, dsmax=0.05, p_min=0.0, p_max=2.2, max_steps=50, max_iterations=10, tol=1e-12, normC=palc.norminf)
    br = Cr.continuation_fold(m2, sn["u"], sn["p"], Q["k"], a, b, detect_codim2=2, n_inversion=8, max_bisection_steps=25,
                              dsmin_bisection=1e-5, **kw)
    return m2, br


def test_comodel_cusp_matches_the_reference_test(comodel_cusp):
    """The unbisected curve changes the sign of CP between k = 0.356519 and k = 0.37197 (and of b2 one step earlier: the secant
    lags).  After the bisection the restatement sits on the extremum of k along the curve, k = 0.3559913 with b2 = -6e-5, where
    c = 0.36275: within the reference's rtol = 1e-2 of its 0.362 (COModel.jl:64).  The reference's k = 0.35665351 (COModel.jl:53,
    rtol = 1e-4) is the output of ITS finite bisection, not the extremum: the curve itself reaches k = 0.3559913 < 0.35665351.
    Measured deviation of the located k from the reference's number: 1.857e-3; asserted at twice that, capped at 2e-3."""
    m2, br = comodel_cusp
    f = GOLD["comodel_cusp"]
    assert [s["type"] for s in br["specialpoint"]] == ["cusp"]
    sp = br["specialpoint"][0]
    i = sp["idx"]
    assert min(br["p2"][i - 1], br["p2"][i]) <= f["k"] <= max(br["p2"][i - 1], br["p2"][i]), (br["p2"][i - 1], br["p2"][i])
    assert br["b2"][i - 2] * br["b2"][i] < 0
    X = sp["X"]
    nf = Cr.cusp_at_fold(m2, X[:-1], m2.at(X[-1], sp["p2"]))
    cs = [Cr.cusp_at_fold(m2, br["X"][j][:-1], m2.at(br["X"][j][-1], br["p2"][j]))["c"] for j in (i - 2, i - 1, i)]
    dk, dc = abs(sp["p2"] - f["k"]) / f["k"], abs(nf["c"] - f["c"]) / f["c"]
    print(f"COModel cusp: k {sp['p2']:.8f} (reference {f['k']}, rel {dk:.3e}), c {nf['c']:.5f} (reference {f['c']}, rel {dc:.3e}), "
          f"b2 {nf['b2']:.2e}, c at the curve points around it {cs}, {sp['bisection_steps']} bisection steps, "
          f"{sp['n_inversion']} inversions, {sp['status']}")
    assert dc <= f["c_rtol"], (nf["c"], f["c"])
    assert abs(nf["b2"]) <= 1e-3 * max(abs(b) for b in br["b2"][:i + 1])
    assert all(k >= sp["p2"] - 1e-9 for k in br["p2"]), "the located point is the extremum of k along the curve"
    assert dk <= min(2 * 1.857e-3, 2e-3), dk
    # every point of the curve, the located one included, is a fold of the q2 problem
    for Xj, kk in list(zip(br["X"], br["p2"])) + [(X, sp["p2"])]:
        q = {**Q, "q2": Xj[-1], "k": kk}
        assert np.abs(_com_F(Xj[:-1], q)).max() <= 1e-10
        assert np.abs(np.linalg.eigvals(_com_J(Xj[:-1], q))).min() <= 1e-8


# ---------------------------------------------------------------------------------------------- the SH tensors
@pytest.mark.parametrize("kind,dims", [("sh", (14, 11)), ("sh", (7, 6, 5)), ("sh1d", (41,))])
def test_third_derivative_formulas_match_central_differences_of_the_oracle_jacobian(kind, dims):
    """h (d2F) and t (d3F) as the cusp passes use them: d2F[a, b] from the first and d3F[a, a, b] from the second central
    difference of the oracle Jacobian in the direction a.  Step 1e-3: the second difference of the pointwise cubic (SH) is exact
    and that of the quintic (SH1D) is off by eps^2 / 12 d5F a^4 b ~ 1e-5 |a|^4 |b|, the stencil part cancels up to
    eps_mach |L1| / eps^2 ~ 1e-6 -- both inside 1e-4 of the largest entry."""
    rng = np.random.default_rng(4)
    if kind == "sh":
        op, pars = operators.SwiftHohenberg(dims, (np.pi,) * len(dims)), dict(l=-0.15, nu=1.3)
    else:
        op, pars = operators.SwiftHohenberg1D(dims[0], 6.0), dict(lam=-0.7, nu=2.0)
    names = list(pars)
    n = int(np.prod(dims))
    u, a, b = 0.5 * rng.standard_normal(n), 0.5 * rng.standard_normal(n), rng.standard_normal(n)
    J = lambda uu: op.J(uu, *[pars[k] for k in names])
    m = Cr.sh_cusp_model(op, kind, pars, names[0])
    eps = 1e-3
    fd2 = (J(u + eps * a) @ b - J(u - eps * a) @ b) / (2 * eps)
    ref2 = m.d2F(u, pars, a, b)
    assert np.abs(fd2 - ref2).max() <= 1e-4 * np.abs(ref2).max()
    fd3 = (J(u + eps * a) @ b - 2.0 * (J(u) @ b) + J(u - eps * a) @ b) / eps ** 2
    ref3 = m.d3F(u, pars, a, a, b)
    assert np.abs(fd3 - ref3).max() <= 1e-4 * np.abs(ref3).max()
    # the passes' element expressions contract to the same numbers as the materialised tensors
    q, p, H2 = a, b, rng.standard_normal(n)
    nu = pars[names[1]]
    d = Cr.cusp_dots(kind, nu, u, q, p)
    assert np.allclose(d, [p @ m.d2F(u, pars, q, q), q @ q, p @ p, q @ p], rtol=1e-12, atol=0)
    assert np.allclose(Cr.cusp_rhs(kind, nu, u, q, 0.7), 0.7 * q - m.d2F(u, pars, q, q), rtol=1e-12, atol=1e-14)
    assert np.allclose(Cr.cusp_contract(kind, nu, u, q, p, H2), [p @ m.d3F(u, pars, q, q, q), p @ m.d2F(u, pars, q, H2)], rtol=1e-11,
                       atol=0)


# ---------------------------------------------------------------------------------------------- the SH cusp fixture
@pytest.fixture(scope="module")
def sh_cusp():
    d = np.load(os.path.join(HERE, "golden", "sh_cusp_128x2.npz"))
    op = operators.SwiftHohenberg(tuple(int(k) for k in d["dims"]), tuple(float(x) for x in d["ls"]))
    return d, op, Cr.sh_cusp_model(op, "sh", dict(l=float(d["fold_l"]), nu=float(d["fold_nu"])), "l", "nu")


def test_sh_cusp_fixture_is_rederived_from_its_fold_point(sh_cusp):
    """scripts/gen_sh_cusp_fixture.py restated on the stored data: the stored fold point is a fold, the stored steps reach the
    sign change of CP, the b2-driven bisection with the stored options lands on the stored cusp, and the normal form there is the
    stored one.  The Newton solves stop at |G|_inf <= 1e-10, which a different BLAS may reach along another path: (l, nu) at
    1e-8, c at 1e-6."""
    d, op, m = sh_cusp
    l0, nu0, v = float(d["fold_l"]), float(d["fold_nu"]), d["fold_v"]
    assert np.abs(op.F(d["fold_u"], l0, nu0)).max() <= 1e-10
    e = np.sort(np.abs(np.linalg.eigvalsh(op.J(d["fold_u"], l0, nu0).toarray())))
    assert e[0] <= 1e-8 and e[1] >= 1e-2, e[:3]
    assert abs(np.linalg.norm(v) - 1) <= 1e-12 and np.abs(op.J(d["fold_u"], l0, nu0) @ v).max() <= 1e-8
    dss = [float(x) for x in d["ds_sequence"]]
    assert 3 <= len(dss) <= 5
    br = Cr.continuation_fold(m, d["fold_u"], l0, nu0, v, v, ds=dss[0], ds_sequence=dss, max_steps=len(dss), p_min=float(d["p_min"]),
                              p_max=float(d["p_max"]), max_iterations=int(d["max_iterations"]), tol=float(d["dense_tol"]),
                              detect_codim2=2, bisect="b2", n_inversion=int(d["dense_n_inversion"]),
                              max_bisection_steps=int(d["dense_max_bisection_steps"]),
                              dsmin_bisection=float(d["dense_dsmin_bisection"]))
    assert [s["idx"] for s in br["specialpoint"]] == [len(dss)]
    sp = br["specialpoint"][0]
    assert np.abs(np.array(br["p1"]) - d["curve_l"]).max() <= 1e-8 and np.abs(np.array(br["p2"]) - d["curve_nu"]).max() <= 1e-8
    X = sp["X"]
    pars = m.at(X[-1], sp["p2"])
    q, p = Cr.null_vectors(m.J(X[:-1], pars))
    if q @ d["cusp_q"] < 0:
        q, p = -q, -p
    nf = Cr.cusp_normal_form(m, X[:-1], pars, q, p)
    print(f"SH cusp: l {sp['p1']:.10f} nu {sp['p2']:.10f} c {nf['c']:.8f} b2 {nf['b2']:.2e} CP {sp['CP']:.2e}; stored "
          f"l {float(d['cusp_l']):.10f} nu {float(d['cusp_nu']):.10f} c {float(d['cusp_c']):.8f}")
    assert abs(sp["p1"] - float(d["cusp_l"])) <= 1e-8 and abs(sp["p2"] - float(d["cusp_nu"])) <= 1e-8
    assert abs(nf["c"] - float(d["cusp_c"])) <= 1e-6
    # a genuine cusp: b2 and the secant's nu component vanish together, small against their values along the curve
    assert abs(nf["b2"]) <= 1e-4 * np.abs(d["curve_b2"]).max() and abs(sp["CP"]) <= 1e-3 * np.abs(d["curve_CP"]).max()
    assert d["curve_b2"][0] * d["curve_b2"][-1] < 0 and d["curve_CP"][-2] * d["curve_CP"][-1] < 0
    # the stored normal form at the stored state, by the dense formulas and by the passes' element expressions
    lc, nuc, u, qs = float(d["cusp_l"]), float(d["cusp_nu"]), d["cusp_u"], d["cusp_q"]
    nfs = Cr.cusp_normal_form(m, u, m.at(lc, nuc), qs, qs)
    assert abs(nfs["c"] - float(d["cusp_c"])) <= 1e-12 and np.abs(nfs["H2"] - d["cusp_H2"]).max() <= 1e-10
    dd = Cr.cusp_dots("sh", nuc, u, qs, qs)
    cc = Cr.cusp_contract("sh", nuc, u, qs, qs, d["cusp_H2"])
    assert abs(dd[0] - float(d["cusp_b2"])) <= 1e-14 and abs((cc[0] + 3 * cc[1]) / 6 - float(d["cusp_c"])) <= 1e-14
    assert np.abs(u.reshape(2, 128)[0] - u.reshape(2, 128)[1]).max() <= 1e-12             # y-uniform
    assert d["cusp_eig"][0] <= 1e-9 and d["cusp_eig"][1] >= 0.04                        # a simple, well separated kernel


def test_cusp_entries_are_bound():
    from bk_amd import _lib
    for name, nargs in (("bk_cusp_dots", 7), ("bk_cusp_rhs", 7), ("bk_cusp_contract", 8), ("bk_cusp_normal_form", 14)):
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
    from bk_amd import codim2
    import inspect
    assert inspect.signature(codim2.continuation_fold).parameters["detect_codim2"].default == 0
    assert {"b2", "specialpoint", "lens2"} <= set(codim2.FoldBranch.__dataclass_fields__)
