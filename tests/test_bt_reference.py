"""CPU tests that pin the Bogdanov-Takens restatement (tests/bt_ref.py) on the reference alone and certify the golden values the
GPU tests of tests/test_gpu_bt.py read (tests/golden/bt_cgl.json, tests/golden/reference_bt_answers.json):

  * the planar normal form of test/normal_forms/testNF.jl:474-522, where a, b, the Jordan basis and the unfolding are known exactly;
  * Lorenz-84 in (F, T) (test/hopf_codim_2/lorenz84.jl:197-229): Newton from a neighbouring fold point of that test, then the
    reference's recorded a, b, gamma, c, K10, K11, K2 and H0001;
  * the analytic Jacobian of the Bogdanov-Takens system against central differences of its functional;
  * cGL at 8 x 6 and 12 x 9: the Bogdanov-Takens point of the example's Hopf curve from two starts, its normal form, the limit
    (p - p_BT) / omega^2 -> K11 b / (2 a) along the computed Hopf curve, and dense LU next to SciPy GMRES under the device's
    preconditioner and tolerance.
"""
import functools
import json
import os

import numpy as np
import pytest

import bt_ref as BT

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = np.finfo(float).eps


def _load(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


# ------------------------------------------------------------------------------------------ the planar normal form
def _planar():
    lenses = ("b1", "b2")
    m = BT.planar_model(dict(b1=0.01, b2=-0.1, a=-1.0, b=1.0))
    x0, p0 = np.array([0.1, 0.0]), np.array([0.01, -0.1])
    a, b = BT.start_vectors(m, x0, BT._at(m, lenses, p0))
    s = BT.newton_bt(m, x0, p0, lenses, a, b, tol=1e-12)
    q = BT._at(m, lenses, s["p"])
    basis = BT.jordan_basis(m, s["u"], q, s["terms"]["v1"], s["terms"]["w1"])
    return m, s, q, basis, BT.normal_form(m, s["u"], q, lenses, *basis)


def test_planar_normal_form_is_reproduced_exactly():
    """x1' = x2, x2' = b1 + b2 x2 + a x1^2 + b x1 x2 with a = -1, b = 1: the point is the origin at (b1, b2) = 0, a sign(sum q0) = -1
    and b sign(sum q0) = 1 to 1e-12 (analytic derivatives; the reference allows 1e-5 for its differences), |q0| = (1, 0),
    |q1| = (0, 1), K2 = 0, and K10, K11 map (b1, b2) to themselves up to the orientation sign of q0."""
    m, s, q, (q0, q1, p0, p1), nf = _planar()
    assert s["converged"] and np.abs(s["u"]).max() <= 1e-12 and np.abs(s["p"]).max() <= 1e-12, (s["u"], s["p"])
    sg = np.sign(q0.sum())
    assert abs(nf["a"] * sg + 1.0) <= 1e-12 and abs(nf["b"] * sg - 1.0) <= 1e-12, (nf["a"], nf["b"])
    assert np.abs(np.abs(q0) - [1, 0]).max() <= 1e-12 and np.abs(np.abs(q1) - [0, 1]).max() <= 1e-12
    assert np.abs(np.abs(p0) - [1, 0]).max() <= 1e-12 and np.abs(np.abs(p1) - [0, 1]).max() <= 1e-12
    assert np.abs(nf["K2"]).max() <= 1e-12
    assert np.abs(nf["K10"] - sg * np.array([1.0, 0.0])).max() <= 1e-12 and np.abs(nf["K11"] - [0.0, 1.0]).max() <= 1e-12
    assert BT.jordan_defect(m, s["u"], q, q0, q1, p0, p1) <= 1e-12


def test_planar_predictors_lie_on_the_curves_of_the_normal_form():
    """On the planar system the predictors are exact: the Hopf curve is b2 = -b x, b1 = -a x^2 with omega^2 = -2 a x, the fold
    curve b1 = 0."""
    m, s, q, (q0, q1, p0, p1), nf = _planar()
    if nf["a"] > 0:
        nf = BT.flipped(nf)
    for ds in (1e-3, 2e-2):
        h = BT.predictor_hopf(nf, s["p"], q0, q1, p0, p1, ds)
        x = h["x"]
        sg = np.sign(q0.sum())
        # in the original coordinates x1 = sg x: a_true = -1, b_true = 1
        x1 = sg * x
        assert abs(h["pars"][0] - x1 ** 2) <= 1e-12 and abs(h["pars"][1] + x1) <= 1e-12, (h["pars"], x1)
        assert abs(h["omega"] ** 2 - 2 * x1) <= 1e-12 and x1 > 0
        J = m.J(h["x0"] + s["u"], BT._at(m, ("b1", "b2"), h["pars"]))
        ev = np.linalg.eigvals(J)
        assert np.abs(ev.real).max() <= 1e-12 and abs(np.abs(ev.imag).max() - h["omega"]) <= 1e-12, ev
        assert np.abs(J @ h["EigenVec"] - 1j * h["omega"] * h["EigenVec"]).max() <= 1e-12
        assert np.abs(J.T @ h["EigenVecAd"] + 1j * h["omega"] * h["EigenVecAd"]).max() <= 1e-12
        f = BT.predictor_fold(nf, s["p"], q0, p1, ds)
        assert abs(f["pars"][0]) <= 1e-12 and abs(f["pars"][1] - ds) <= 1e-12


# ------------------------------------------------------------------------------------------ Lorenz-84
@functools.lru_cache(maxsize=None)
def _lorenz():
    ref = _load("reference_bt_answers.json")
    lenses = tuple(ref["lenses"])
    m = BT.lorenz84_model(ref["params"])
    x, F, res = BT.newton_fold_full(m, ref["fold_point"]["x"], ref["fold_point"]["F"], "F", dict(ref["params"]))
    p = np.array([F, ref["params"]["T"]])
    q = BT._at(m, lenses, p)
    out = []
    for seed in (0, 1):
        a, b = BT.start_vectors(m, x, q, seed)
        s = BT.newton_bt(m, x, p, lenses, a, b, tol=1e-13, max_iterations=30)
        qq = BT._at(m, lenses, s["p"])
        basis = BT.jordan_basis(m, s["u"], qq, s["terms"]["v1"], s["terms"]["w1"])
        out.append((s, qq, basis, BT.normal_form(m, s["u"], qq, lenses, *basis)))
    return ref, m, (x, F, res, q), out


def test_lorenz84_start_is_the_fold_point_of_the_reference_test():
    ref, m, (x, F, res, q), _ = _lorenz()
    lo, hi = 1.546648372620807, 1.5466483727182652          # the interval the reference asserts for this fold (lorenz84.jl:65)
    assert res <= 1e-14 and lo - 1e-9 <= F <= hi + 1e-9, (res, F)
    ev = np.sort(np.abs(np.linalg.eigvals(m.J(x, q))))
    assert ev[0] <= 1e-12 and ev[1] >= 0.05, ev         # a simple fold: the start is NOT a Bogdanov-Takens point


def test_lorenz84_matches_the_answers_the_reference_records():
    """a and b to rtol 1e-6, everything past them to the reference's own rtol 1e-3, after orienting q0 so that a > 0; measured here:
    all of them agree to 1e-9 relative or better (the reference's values come from finite differences at a converged point).  Under q0 -> -q0 the
    coefficients a, b, K10, gamma and c change sign and K11, K2 and H0001 do not, which is asserted on the restatement by running
    the normal form on the negated basis."""
    ref, m, _, runs = _lorenz()
    lenses = tuple(ref["lenses"])
    pts = []
    for s, qq, basis, nf in runs:
        assert s["converged"] and s["itnewton"] <= 8, s["residuals"]
        ev = np.sort(np.abs(np.linalg.eigvals(m.J(s["u"], qq))))
        assert ev[1] <= 1e-7 and ev[2] >= 1.0, ev        # a double zero eigenvalue
        assert BT.jordan_defect(m, s["u"], qq, *basis) <= 1e-12
        neg = BT.normal_form(m, s["u"], qq, lenses, *[-v for v in basis])
        fl = BT.flipped(nf)
        for k in ("a", "b", "gamma", "c", "K10", "K11", "K2", "H0001"):
            assert np.allclose(neg[k], fl[k], rtol=1e-12, atol=1e-13), (k, neg[k], fl[k])
            if k in ("K11", "K2", "H0001"):
                assert np.allclose(neg[k], nf[k], rtol=1e-12, atol=1e-13), k
        o = nf if nf["a"] > 0 else fl
        worst = 0.0
        for k in ("a", "b", "gamma", "c", "K10", "K11", "K2", "H0001"):
            rel = float(np.max(np.abs(np.asarray(o[k]) - np.asarray(ref[k])) / np.abs(np.asarray(ref[k]))))
            worst = max(worst, rel)
            print(f"lorenz84 {k}: {o[k]} reference {ref[k]} relative difference {rel:.2e}")
            assert rel <= (1e-6 if k in ("a", "b") else 1e-3), (k, o[k], ref[k])
        pts.append((s["p"], o["a"], o["b"]))
    # both random starts give the same point and coefficients
    assert np.abs(pts[0][0] - pts[1][0]).max() <= 1e-12 and abs(pts[0][1] - pts[1][1]) <= 1e-12 and abs(pts[0][2] - pts[1][2]) <= 1e-12


def test_bt_jacobian_matches_central_differences_of_the_functional():
    """The analytic [J dpF; sigma_x sigma_p] against (G(z + h e) - G(z - h e)) / 2h on Lorenz-84 near (not at) the point: h = 1e-6
    leaves O(h^2) truncation and eps / h rounding, 1e-8 relative to the largest entry covers both."""
    ref, m, (x, F, res, q), _ = _lorenz()
    lenses = tuple(ref["lenses"])
    a, b = BT.start_vectors(m, x, q)
    p = np.array([F, ref["params"]["T"]])
    _, t, qq = BT.G(m, x, p, lenses, a, b)
    Jbt = BT.bt_jacobian(m, x, qq, lenses, t)
    z, h = np.concatenate([x, p]), 1e-6
    fd = np.zeros_like(Jbt)
    for j in range(len(z)):
        e = np.zeros(len(z)); e[j] = h
        gp = BT.G(m, (z + e)[:-2], (z + e)[-2:], lenses, a, b)[0]
        gm = BT.G(m, (z - e)[:-2], (z - e)[-2:], lenses, a, b)[0]
        fd[:, j] = (gp - gm) / (2 * h)
    assert np.abs(fd - Jbt).max() <= 1e-8 * np.abs(Jbt).max(), np.abs(fd - Jbt).max()


# ------------------------------------------------------------------------------------------ cGL
# an independent dense Newton (analytic derivatives, singular vectors of J as a and b) gave this table: point, |x|_inf, a, b,
# cond(J_BT), the first three residuals from each start, and the second smallest |eigenvalue| of J at the curve's stop point
TABLE = {"8x6": dict(p=(1.87101672, 1.05550621), xinf=0.98479, a=0.43946879469, b=-1.90592842734, steps=49, cond=(121, 123),
                     res=dict(stop=(8.4e-3, 1.5e-4, 1.1e-8), before=(1.3e-2, 7.8e-4, 5.7e-7))),
         "12x9": dict(p=(1.97060156, 1.02402438), xinf=1.01421, a=0.28948669320, b=-1.16579445394, steps=47, cond=(382, 388),
                      res=dict(stop=(2.0e-2, 1.1e-3, 8.9e-7), before=(1.0e-2, 4.9e-4, 2.2e-7)))}


@functools.lru_cache(maxsize=None)
def _cgl(key):
    dims = tuple(int(v) for v in key.split("x"))
    return BT.cgl_yardstick(dims)


@pytest.mark.parametrize("key", ["8x6", "12x9"])
def test_cgl_bt_point_reproduces_the_table(key):
    """The Hopf curve of the example stops with stopped_at_bt after the table's step count at a FOLD point near the
    Bogdanov-Takens point: its second smallest |eigenvalue| is 0.0224 / 0.0470, a simple zero.  (The table came with 0.0201 / 0.0449
    for that figure without saying at which state or by which measure it was taken; those two numbers are NOT reproduced here and
    nothing is asserted against them.)  The table's residuals belong to other start vectors (the singular vectors of J, here the
    reference's default), so only their decades are compared.  newton_bt converges from it and from the Hopf point
    before it in 3 steps to the same point, the table's; a and b agree between the starts; the Jordan identities hold to the
    residual Newton stopped at (the chain is solved at that point, J q0 = -sigma vl), asserted below the Newton tolerance; the two
    smallest |eigenvalues| of the dense Jacobian at the result are of the order sqrt(rounding)."""
    y, T = _cgl(key), TABLE[key]
    assert y["stopped_at_bt"] and y["steps"] == T["steps"]
    st = y["starts"]["stop"]
    assert abs(st["omega"]) < 1e-8 and st["eig2"][0] <= 1e-9 and 0.02 <= st["eig2"][1] <= 0.05, st["eig2"]
    assert 0.1 <= y["starts"]["before"]["omega"] <= 0.2
    for name in ("stop", "before"):
        r = y["lu"][name]
        print(key, name, {k: r[k] for k in ("p", "xinf", "residuals", "cond", "eig2", "defect", "a", "b", "gamma", "c", "K10", "K11", "K2")})
        assert r["itnewton"] == 3 and r["residuals"][-1] <= 1e-10
        assert np.abs(np.array(r["p"]) - T["p"]).max() <= 1e-8 and abs(r["xinf"] - T["xinf"]) <= 1e-5
        assert abs(r["a"] - T["a"]) <= 1e-10 and abs(r["b"] - T["b"]) <= 1e-10
        # the table's residuals were printed to two digits and belong to another start vector draw: the same decades
        for got, want in zip(r["residuals"], T["res"][name]):
            assert 0.1 <= got / want <= 10, (name, r["residuals"], T["res"][name])
        assert r["defect"] <= 1e-10 and max(r["eig2"]) <= 1e-5 and 0.98 * T["cond"][0] <= r["cond"] <= 1.02 * T["cond"][1]
    s, b = y["lu"]["stop"], y["lu"]["before"]
    assert np.abs(np.array(s["p"]) - b["p"]).max() <= 1e-11 and abs(s["xinf"] - b["xinf"]) <= 1e-11
    for k in BT.NF_KEYS:
        assert np.allclose(s[k], b[k], rtol=1e-9, atol=0), (k, s[k], b[k])
    assert abs(s["a"] - b["a"]) <= 1e-11 and abs(s["b"] - b["b"]) <= 1e-11


@pytest.mark.parametrize("key", ["8x6", "12x9"])
def test_cgl_unfolding_matches_the_limit_along_the_hopf_curve(key):
    """The independent check of K11: on the Hopf curve beta2 = b omega^2 / (2 a) and beta1 = O(omega^4), so
    (p - p_BT) / omega^2 -> K11 b / (2 a).  The left side is Richardson-extrapolated in omega^2 over the last three Hopf points of the
    restatement's curve; the extrapolation's own error is measured as |two-point - three-point extrapolant| and given a factor 10.
    Measured (r, gamma): 8 x 6 extrapolant (-0.920581, -0.496803), limit (-0.920777, -0.496867), difference (2.0e-4, 6.3e-5), allowed
    (3.7e-3, 5.2e-3); 12 x 9 extrapolant (-0.970109, -0.496071), limit (-0.970081, -0.496043), difference (2.7e-5, 2.7e-5), allowed
    (7.5e-4, 1.3e-3)."""
    r = _cgl(key)["richardson"]
    two, three, lim = np.array(r["two"]), np.array(r["three"]), np.array(r["limit"])
    allowed = 10 * np.abs(two - three)
    print(key, "extrapolants", two, three, "K11 b / (2 a)", lim, "difference", np.abs(three - lim), "allowed", allowed)
    assert (np.abs(three - lim) <= allowed).all() and (allowed <= 1e-2).all()


@pytest.mark.parametrize("key", ["8x6", "12x9"])
def test_cgl_gmres_stays_next_to_lu(key):
    """SciPy GMRES (restart 60, rtol 1e-13) on the bordered systems left-preconditioned by the cGL block of the stop point's r, the
    solver the GPU tests run: every solve converges, the four bordered vectors agree with sparse LU to 1e-11, Newton takes the same
    three steps and the point, a, b and the unfolding agree with LU to 1e-10 relative -- the margins the GPU tests widen by 10."""
    y = _cgl(key)
    t, g = y["terms"], y["gmres"]
    assert t["bad"] == 0 and g["bad"] == 0 and g["itnewton"] == 3
    assert all(10 <= i <= 30 for i in t["its"] + g["its_all"]), (t["its"], g["its_all"])
    for k in ("v1", "v2", "w1", "w2"):
        assert t[k]["diff"] <= 1e-11 * max(1.0, t[k]["norminf"]), (k, t[k])
    assert g["diff"]["p"] <= 1e-11 and g["diff"]["xinf"] <= 1e-11
    for k in BT.NF_KEYS:
        assert g["diff"][k] <= 1e-10 * np.abs(np.asarray(y["lu"]["stop"][k])).max(), (k, g["diff"][k])
    # the double eigenvalue at the point of the GMRES run: within the factor the GPU tests allow the device
    assert max(g["eig2"]) <= min(10 * max(y["lu"]["stop"]["eig2"]), 1e-5), (g["eig2"], y["lu"]["stop"]["eig2"])


def _close(a, b, rtol, atol):
    if isinstance(a, dict):
        return set(a) == set(b) and all(_close(a[k], b[k], rtol, atol) for k in a)
    return np.allclose(np.asarray(a, dtype=float), np.asarray(b, dtype=float), rtol=rtol, atol=atol)


@pytest.mark.parametrize("key", ["8x6", "12x9"])
def test_golden_file_holds_what_the_restatement_computes(key):
    """tests/golden/bt_cgl.json (python tests/bt_ref.py) against a fresh run: states, points and coefficients to 1e-9 relative (the
    Newton results carry cond(J_BT) <= 400 times rounding), measured differences and eigenvalues at rounding level to a factor,
    GMRES counts to +-1."""
    gold, y = _load("bt_cgl.json")[key], _cgl(key)
    assert gold["dims"] == y["dims"] and gold["steps"] == y["steps"] and gold["precond"] == pytest.approx(y["precond"], rel=1e-12)
    assert _close(gold["curve"], y["curve"], 1e-9, 1e-9)
    for name in ("stop", "before"):
        assert _close(gold["starts"][name]["x"], y["starts"][name]["x"], 1e-9, 1e-9)
        assert _close(gold["starts"][name]["p"], y["starts"][name]["p"], 1e-10, 0)
        for k in ("p", "xinf") + BT.NF_KEYS:
            assert _close(gold["lu"][name][k], y["lu"][name][k], 1e-9, 0), (name, k)
        assert gold["lu"][name]["itnewton"] == y["lu"][name]["itnewton"]
        assert _close(gold["lu"][name]["residuals"][:3], y["lu"][name]["residuals"][:3], 1e-3, 0)
        assert max(gold["lu"][name]["eig2"]) <= 1e-5
    assert _close(gold["terms"]["a"], y["terms"]["a"], 1e-9, 1e-12) and _close(gold["terms"]["b"], y["terms"]["b"], 1e-9, 1e-12)
    assert _close(gold["terms"]["sigma"], y["terms"]["sigma"], 1e-6, 1e-12)
    for a, b in ((gold["terms"]["its"], y["terms"]["its"]), (gold["gmres"]["its_all"], y["gmres"]["its_all"])):
        assert len(a) == len(b) and all(abs(i - j) <= 1 for i, j in zip(a, b)), (a, b)
    for k in ("v1", "v2", "w1", "w2"):
        assert gold["terms"][k]["diff"] <= 1e-11 and gold["terms"][k]["norminf"] == pytest.approx(y["terms"][k]["norminf"], rel=1e-9)
    for k, v in gold["gmres"]["diff"].items():
        assert v <= 1e-10 * max(1.0, np.abs(np.asarray(gold["lu"]["stop"].get(k, 1.0))).max()), (k, v)
    assert _close(gold["richardson"], y["richardson"], 1e-6, 0)
