"""The CPU restatement of the minimally augmented Hopf formulation (tests/minaug_hopf_ref.py) against known answers of the
reference's COModel test, its linear solver against a finite-difference Jacobian of G, and the cGL Hessian formulas the device
kernels evaluate against differences of the closed-form Jacobian."""
import json
import os

import numpy as np
import pytest

import minaug_hopf_ref as R
from oracle import operators, palc
from test_fold_reference import Q, _com_F, _com_J, _com_d2F
from test_reference_known_answers import _both_sides

HOPF_GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "reference_hopf_answers.json")))


def _dFdp(x, q, lens, d=1e-7):
    qp, qm = dict(q), dict(q)
    qp[lens] += d
    qm[lens] -= d
    return (_com_F(x, qp) - _com_F(x, qm)) / (2 * d)


def _dJvdp(x, q, lens, v, d=1e-7):
    qp, qm = dict(q), dict(q)
    qp[lens] += d
    qm[lens] -= d
    return (_com_J(x, qp) @ v - _com_J(x, qm) @ v) / (2 * d)


def _comodel(lens2=None):
    """COModel (test/hopf_codim_2/COModel.jl:7-16) with its written-out J and d2F; dF/dp and dJ/dp v by central differences."""
    return R.HopfModel(_com_F, _com_J, _com_d2F, _dFdp, _dJvdp, Q, "q2", lens2)


@pytest.fixture(scope="module")
def comodel_hopf():
    """newton_hopf of the reference's Hopf points 2 and 5, located by the oracle's PALC + bisection (COModel.jl:27-34)."""
    sp, _ = _both_sides(palc.Problem(lambda u, p: _com_F(u, {**Q, "q2": p}), lambda u, p: _com_J(u, {**Q, "q2": p})),
                        np.array([0.001137, 0.891483, 0.062345]), 1.0, ds=0.002, dsmax=0.01, p_min=0.5, p_max=2.3, max_steps=100,
                        nev=3, n_inversion=6, max_bisection_steps=25, tangent="secant")
    assert [s["type"] for s in sp] == ["hopf", "bp", "bp", "hopf"]
    m = _comodel()
    out = []
    for s in (sp[0], sp[3]):
        q = m.at(s["param"])
        ev = np.linalg.eigvals(_com_J(s["x"], q))
        om = abs(ev[np.abs(ev.imag) > 0][np.argmin(np.abs(ev[np.abs(ev.imag) > 0].real))].imag)
        a, b = R.start_vectors(m, s["x"], q, om)
        out.append(R.newton_hopf(m, s["x"], s["param"], om, a, b, tol=1e-12, max_iterations=15))
    return m, out


def test_comodel_hopf_points_satisfy_the_hopf_condition(comodel_hopf):
    m, sols = comodel_hopf
    g = HOPF_GOLD["comodel_hopf"]
    for i, sn in enumerate(sols):
        assert sn["converged"] and sn["itnewton"] <= 15, sn["residuals"]
        q = m.at(sn["p"])
        assert np.abs(_com_F(sn["u"], q)).max() <= 1e-12
        ev = np.linalg.eigvals(_com_J(sn["u"], q))
        om = sn["omega"]
        k = np.argmin(np.abs(ev - 1j * abs(om)))
        assert abs(ev[k].real) <= 1e-10 * abs(om) and abs(abs(ev[k].imag) - abs(om)) <= 1e-10 * abs(om), (ev, om)
        assert abs(sn["p"] - g["q2_hopf_condition"][i]) <= g["atol_q2"], (sn["p"], g)
        assert abs(sn["p"] - g["q2_bisection"][i]) <= g["atol_q2"], (sn["p"], g)
        assert abs(abs(om) - g["omega_hopf_condition"][i]) <= g["atol_omega"], (om, g)


def test_comodel_hopf_curve_ends_at_a_bogdanov_takens_point(comodel_hopf):
    """continuation_hopf in k from Hopf point 2 until omega -> 0: the curve ends where it meets the fold curve, at one of the
    reference's BT points (COModel.jl:56-59)."""
    m, sols = comodel_hopf
    sn = sols[0]
    m2 = _comodel("k")
    q = m2.at(sn["p"], Q["k"])
    a, b = sn["w"] / np.linalg.norm(sn["w"]), sn["v"] / np.linalg.norm(sn["v"])
    ends = []
    for ds in (0.002, -0.002):
        br = R.continuation_hopf(m2, sn["u"], sn["p"], sn["omega"], Q["k"], a, b, ds=ds, dsmin=1e-9, dsmax=0.005, p_min=0.0,
                                 p_max=2.0, max_steps=600, max_iterations=10, tol=1e-11)
        for X, kk in zip(br["X"], br["p2"]):
            assert np.abs(_com_F(X[:-2], m2.at(X[-2], kk))).max() <= 1e-10
        om = np.abs(br["omega"])
        if not br["stopped_at_bt"]:
            continue
        # omega^2 is smooth in k through the BT point (it changes sign there: Hopf -> neutral saddle), so the end of the Hopf
        # curve is the root of a quadratic fit of omega^2(k) through its last three points, and q2 is that fit's companion
        i = int(np.nonzero(om < 1e-6)[0][0])
        kk, q2, w2 = (np.array(br[f][i - 3:i]) for f in ("p2", "p1", "omega"))
        roots = np.roots(np.polyfit(kk, w2 ** 2, 2))
        kb = float(np.real(roots[np.argmin(np.abs(roots - kk[-1]))]))
        ends.append((kb, float(np.polyval(np.polyfit(kk, q2, 2), kb)), float(w2[-1])))
    assert ends, "the Hopf curve never reached omega -> 0"
    bt = np.array(HOPF_GOLD["comodel_bt"]["points"])
    errs = [np.min(np.max(np.abs(bt - [k, q2]) / np.abs(bt), axis=1)) for k, q2, _ in ends]
    k, q2, om = ends[int(np.argmin(errs))]
    err = min(errs)
    print(f"COModel Hopf curve end: k = {k:.7f}, q2 = {q2:.7f} (last omega {om:.2e}), rel. distance to the nearest BT {err:.1e}")
    assert err <= HOPF_GOLD["comodel_bt"]["rtol"], (ends, bt)


def test_hopf_linear_solver_matches_a_finite_difference_jacobian(comodel_hopf):
    """The step of hopf_linsolve solves J_G dX = R, J_G the central-difference Jacobian of G (testHopfMA.jl:104-137)."""
    m, sols = comodel_hopf
    sn = sols[0]
    rng = np.random.default_rng(2)
    x = sn["u"] + 1e-3 * rng.standard_normal(3)
    p, om = sn["p"] + 1e-3, sn["omega"] * 1.01
    a, b = sn["w"] / np.linalg.norm(sn["w"]), sn["v"] / np.linalg.norm(sn["v"])
    X = np.concatenate([x, [p, om]])
    G = lambda Y: R._G(m, Y, None, a, b)[0]
    eps = 1e-6
    JG = np.column_stack([(G(X + eps * e) - G(X - eps * e)) / (2 * eps) for e in np.eye(5)])
    rhs = rng.standard_normal(5)
    _, v, w = R._G(m, X, None, a, b)
    dX, dp, dw = R.hopf_linsolve(m, x, m.at(p), om, v, w, rhs[:3], rhs[3], rhs[4])
    got = np.concatenate([dX, [dp, dw]])
    want = np.linalg.solve(JG, rhs)
    assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max(), (got, want)


def test_cgl_hessian_and_djdp_match_differences_of_the_closed_form_jacobian():
    dims = (9, 7)
    op = operators.CGL2d(dims, (np.pi, np.pi / 2))
    rng = np.random.default_rng(4)
    pars = dict(r=0.3, mu=0.1, nu=1.0, c3=-1.0, c5=1.0, gamma=0.2)
    n = 2 * int(np.prod(dims))
    u, a, b = 0.7 * rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
    eps = 1e-5
    fd = (op.J(u + eps * a, **pars) @ b - op.J(u - eps * a, **pars) @ b) / (2 * eps)
    ref = R.cgl_d2F(u, pars, a, b)
    assert np.abs(fd - ref).max() <= 1e-8 * np.abs(ref).max()
    assert np.abs(R.cgl_d2F(u, pars, a, b) - R.cgl_d2F(u, pars, b, a)).max() <= 1e-13 * np.abs(ref).max()     # symmetric
    for name in R.CGL_PARAMS:
        qp, qm = {**pars, name: pars[name] + eps}, {**pars, name: pars[name] - eps}
        fdp = (op.J(u, **qp) @ b - op.J(u, **qm) @ b) / (2 * eps)
        refp = R.cgl_dJvdp(u, pars, name, b)
        assert np.abs(fdp - refp).max() <= 1e-8 * max(np.abs(fdp).max(), 1.0), name
        Fp = (op.F(u, **qp) - op.F(u, **qm)) / (2 * eps)
        assert np.abs(Fp - R.cgl_dFdp(u, pars, name)).max() <= 1e-8 * np.abs(Fp).max(), name
    assert np.all(R.cgl_dJvdp(u, pars, "gamma", b) == 0)


def test_hopf_max_norm_propagates_nan():
    """normN(BorderedArray(F, [Re sigma, Im sigma])) in the max norm is NaN when any component is NaN, whatever its position."""
    from bk_amd import codim2

    class F:
        def __init__(self, v):
            self.v = v

        def norminf(self):
            return self.v

        def norm(self):
            return self.v

    nan = float("nan")
    for f, sg in ((1.0, complex(nan, 0.5)), (1.0, complex(0.5, nan)), (nan, complex(2.0, 3.0)), (0.0, complex(0.0, nan))):
        assert codim2._norm_hopf(F(f), sg, True) != codim2._norm_hopf(F(f), sg, True), (f, sg)
        assert codim2._norm_hopf(F(f), sg, False) != codim2._norm_hopf(F(f), sg, False), (f, sg)
    assert codim2._norm_hopf(F(1.0), complex(-3.0, 2.0), True) == 3.0
    assert codim2._nanmax(1.0, nan) != codim2._nanmax(1.0, nan) and codim2._nanmax(nan, 1.0) != codim2._nanmax(nan, 1.0)
