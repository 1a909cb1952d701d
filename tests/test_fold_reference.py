"""The CPU restatement of the minimally augmented fold formulation (tests/minaug_fold_ref.py) against known answers held by the
reference's own tests, and the Hessian formulas the device kernels evaluate against central differences of the oracle Jacobians."""
import json
import os

import numpy as np
import pytest

import minaug_fold_ref as R
from oracle import operators, palc
from test_reference_known_answers import GOLD, _both_sides

FOLD_GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "reference_fold_answers.json")))

Q = dict(q1=2.5, q2=1.0, q3=10.0, q4=0.0675, q5=1.0, q6=0.1, k=0.4)


def _com_F(u, q):
    x, y, s = u
    z = 1 - x - y - s
    return np.array([2 * q["q1"] * z**2 - 2 * q["q5"] * x**2 - q["q3"] * x * y, q["q2"] * z - q["q6"] * y - q["q3"] * x * y,
                     q["q4"] * (z - q["k"] * s)])


def _com_J(u, q):
    x, y, s = u
    z = 1 - x - y - s
    q1, q2, q3, q4, q5, q6, k = (q[n] for n in ("q1", "q2", "q3", "q4", "q5", "q6", "k"))
    return np.array([[-4 * q1 * z - 4 * q5 * x - q3 * y, -4 * q1 * z - q3 * x, -4 * q1 * z],
                     [-q2 - q3 * y, -q2 - q6 - q3 * x, -q2],
                     [-q4, -q4, -q4 * (1 + k)]])


def _com_d2F(u, q, a, b):
    da, db = -(a[0] + a[1] + a[2]), -(b[0] + b[1] + b[2])
    xy = a[0] * b[1] + a[1] * b[0]
    return np.array([4 * q["q1"] * da * db - 4 * q["q5"] * a[0] * b[0] - q["q3"] * xy, -q["q3"] * xy, 0.0])


def _comodel(lens2=None):
    """COModel of test/fold_codim_2/codim2.jl:9-18 (the reference differentiates it with ForwardDiff; here J and d2F are
    written out, dF/dp and dJ/dp v are the reference's central differences)."""
    return R.FoldModel(_com_F, _com_J, _com_d2F, Q, "q2", lens2)


def _null_vectors(Jm):
    """start_with_eigen: eigenvectors of J and J' for the eigenvalue nearest 0, zeta* scaled to <zeta, zeta*> = 1 (:480-496)."""
    w, V = np.linalg.eig(Jm)
    z = np.real(V[:, np.argmin(np.abs(w))])
    z /= np.linalg.norm(z)
    wt, Vt = np.linalg.eig(Jm.T)
    zs = np.real(Vt[:, np.argmin(np.abs(wt))])
    zs /= np.linalg.norm(zs)
    return z, zs / np.dot(z, zs)


@pytest.fixture(scope="module")
def comodel_fold():
    """newton(br, 3) of codim2.jl:53: the fold of the q2 branch located by the oracle's PALC + bisection, refined."""
    sp, _ = _both_sides(palc.Problem(lambda u, p: _com_F(u, {**Q, "q2": p}), lambda u, p: _com_J(u, {**Q, "q2": p})),
                        np.array([0.001137, 0.891483, 0.062345]), 1.0, ds=0.002, dsmax=0.01, p_min=0.5, p_max=2.3, max_steps=100,
                        nev=3, n_inversion=6, max_bisection_steps=25, tangent="secant")
    guess = sp[1]
    m = _comodel()
    z, zs = _null_vectors(_com_J(guess["x"], m.at(guess["param"])))
    return m, guess, R.newton_fold(m, guess["x"], guess["param"], zs, z, tol=1e-12, max_iterations=10)


def test_comodel_fold_matches_the_reference_test(comodel_fold):
    _, _, sn = comodel_fold
    f = GOLD["comodel_fold"]
    u, p = np.array(f["u"]), f["p"]
    assert sn["converged"] and sn["itnewton"] <= 10, sn["residuals"]
    eu = np.abs(sn["u"] - u).max() / np.abs(u).max()
    ep = abs(sn["p"] - p) / abs(p)
    # codim2.jl:54-55 asserts rtol = 1e-4; the restatement reaches the reference's digits far beyond it
    print(f"COModel fold: relative error u {eu:.2e}, p {ep:.2e} ({-np.log10(max(eu, ep, 1e-17)):.1f} digits)")
    assert eu <= f["rtol"] and ep <= f["rtol"], (eu, ep)
    assert eu <= 1e-8 and ep <= 1e-8, (eu, ep)


def test_comodel_fold_curve_brackets_the_bogdanov_takens_point(comodel_fold):
    """continuation_fold in k (codim2.jl:65): the BT test function <zeta*, zeta> changes sign between two consecutive points
    whose k bracket the reference's BT point (codim2.jl:74)."""
    m, _, sn = comodel_fold
    m2 = _comodel("k")
    a, b = sn["w"] / np.linalg.norm(sn["w"]), sn["v"] / np.linalg.norm(sn["v"])
    br = R.continuation_fold(m2, sn["u"], sn["p"], Q["k"], a, b, ds=0.002, dsmax=0.01, p_min=0.0, p_max=1.0, max_steps=400,
                             max_iterations=10, normC=palc.norm2)
    bt = np.array(br["BT"])
    k = np.array(br["p2"])
    cross = [i for i in range(len(bt) - 1) if bt[i] * bt[i + 1] < 0]
    assert cross, (k[-5:], bt[-5:])
    i = cross[0]
    kbt = FOLD_GOLD["comodel_bt"]["k"]
    assert min(k[i], k[i + 1]) <= kbt <= max(k[i], k[i + 1]), (k[i], k[i + 1], kbt)
    # every point of the curve is a fold of the q2 problem: J(x, q2, k) has an eigenvalue ~ 0
    for X, kk in zip(br["X"], br["p2"]):
        q = {**Q, "q2": X[-1], "k": kk}
        assert np.abs(_com_F(X[:-1], q)).max() <= 1e-10
        assert np.abs(np.linalg.eigvals(_com_J(X[:-1], q))).min() <= 1e-8


@pytest.mark.parametrize("kind,dims", [("sh", (14, 11)), ("sh", (7, 6, 5)), ("sh1d", (41,))])
def test_hessian_formulas_match_central_differences_of_the_oracle_jacobian(kind, dims):
    rng = np.random.default_rng(3)
    if kind == "sh":
        op = operators.SwiftHohenberg(dims, (np.pi,) * len(dims))
        pars = dict(l=-0.15, nu=1.3)
    else:
        op = operators.SwiftHohenberg1D(dims[0], 6.0)
        pars = dict(lam=-0.7, nu=2.0)
    names = list(pars)
    n = int(np.prod(dims))
    u, a, b = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
    J = lambda uu, **q: op.J(uu, *[{**pars, **q}[k] for k in names])
    eps = 1e-5
    h, _ = R.sh_polys(kind, pars["nu"], 0)
    fd = (J(u + eps * a) @ b - J(u - eps * a) @ b) / (2 * eps)
    ref = R.horner(h, u) * a * b
    assert np.abs(fd - ref).max() <= 1e-7 * np.abs(ref).max()
    for ip, name in enumerate(names):
        _, g = R.sh_polys(kind, pars["nu"], ip)
        fdp = (J(u, **{name: pars[name] + eps}) @ b - J(u, **{name: pars[name] - eps}) @ b) / (2 * eps)
        refp = R.horner(g, u) * b
        assert np.abs(fdp - refp).max() <= 1e-7 * np.abs(refp).max(), name
        # dF/dp of the model = phi_p(u), the factor bk_residual_dparam evaluates
        m = R.sh_model(op, kind, pars, names[0])
        Fp = (op.F(u, *[pars[k] + (eps if k == name else 0) for k in names]) -
              op.F(u, *[pars[k] - (eps if k == name else 0) for k in names])) / (2 * eps)
        assert np.abs(Fp - m.dFdp(u, pars, name)).max() <= 1e-7 * np.abs(Fp).max(), name


def test_fold_max_norm_propagates_nan():
    """normN(BorderedArray(F, sigma)) in the max norm is NaN when F or sigma is NaN, whatever its position (norm_fold of
    fold.hip); for finite input it is the plain max."""
    from bk_amd import codim2

    class F:
        def __init__(self, v, p=None):
            self.v, self.u, self.p = v, self, p

        def norminf(self):
            return self.v

        def norm(self):
            return self.v

    nan = float("nan")
    for f, sg in ((1.0, nan), (nan, 2.0), (0.0, nan), (nan, nan)):
        assert codim2._norm_fold(F(f), sg, True) != codim2._norm_fold(F(f), sg, True), (f, sg)
        assert codim2._norm_fold(F(f), sg, False) != codim2._norm_fold(F(f), sg, False), (f, sg)
        assert codim2._norminf_fold(F(f, sg)) != codim2._norminf_fold(F(f, sg)), (f, sg)
    assert codim2._norm_fold(F(1.0), -3.0, True) == 3.0 and codim2._norm_fold(F(4.0), -3.0, True) == 4.0
    assert codim2._norm_fold(F(4.0), -3.0, False) == 5.0
    assert codim2._norminf_fold(F(1.0, -3.0)) == 3.0 and codim2._norminf_fold(F(4.0, -3.0)) == 4.0
