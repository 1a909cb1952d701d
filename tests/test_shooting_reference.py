"""CPU tests that certify the restatement of the shooting periodic orbits (tests/shooting_ref.py) on the reference's own terms: the
flow is the cGL flow to second order, its tangent is the derivative of the discrete map, the monodromy of a converged orbit has
the trivial multiplier, the coefficient tables are exact, and the committed fixture tests/golden/shooting_cgl.json is what the
restatement produces.  Loads no library."""
import functools
import math

import numpy as np
import pytest
from scipy.integrate import solve_ivp

import potrap_ref as P
import shooting_ref as S

LD = np.longdouble
EPS = np.finfo(float).eps


@functools.lru_cache(maxsize=None)
def _flow(dims, dtype):
    return S.Flow(P.Model(dims, S.LS), dtype)


@functools.lru_cache(maxsize=None)
def _state(dims):
    """A state near the limit cycle at r = 1.2: 0.1 rand after t = 30."""
    fl = _flow(dims, float)
    x = fl.march(S.cycle_start(fl.m), 30.0, 300, S.PARS)["u"]
    x.setflags(write=False)
    return x


def test_flow_is_second_order_against_dop853():
    """(12, 9), r = 1.2, tau = 2, nsteps = 40, 80, 160 against solve_ivp(DOP853, rtol = atol = 1e-12) on the assembled sparse F:
    the error ratios of consecutive step counts lie in [3.5, 4.5]."""
    dims = (12, 9)
    fl = _flow(dims, float)
    m, x0 = fl.m, _state(dims)
    f = lambda t, u: m.F(u, S.PARS)
    ref = solve_ivp(f, (0.0, 2.0), x0, method="DOP853", rtol=1e-12, atol=1e-12).y[:, -1]
    err = [float(np.abs(fl.march(x0, 2.0, n, S.PARS)["u"] - ref).max()) for n in (40, 80, 160)]
    print("ETDRK2 errors at 40, 80, 160 steps:", err)
    assert 3.5 <= err[0] / err[1] <= 4.5 and 3.5 <= err[1] / err[2] <= 4.5, err
    assert err[2] < 1e-4


def test_tangent_is_the_derivative_of_the_discrete_map():
    """dPhi(x, tau) dx in long double against central differences of the restated flow, step 1e-6: the quotient's own error is
    h^2 |Phi'''| / 6 + eps_LD |Phi| / h ~ 1e-12 |dx|^3; 1e-10 of the tangent's size is asked."""
    dims = (8, 6)
    fl = _flow(dims, LD)
    x0 = _state(dims).astype(LD)
    dx = np.random.default_rng(3).standard_normal(fl.m.N).astype(LD)
    r = fl.march(x0, 1.7, 24, S.PARS, dx)
    h = LD(1e-6)
    fd = (fl.march(x0 + h * dx, 1.7, 24, S.PARS)["u"] - fl.march(x0 - h * dx, 1.7, 24, S.PARS)["u"]) / (2 * h)
    err = float(np.abs(fd - r["du"]).max())
    print("tangent vs central differences:", err, "of", r["dumax"])
    assert err <= 1e-10 * r["dumax"]


def test_functional_jvp_matches_the_dense_jacobian_and_differences():
    dims, M, nsteps = (8, 6), 2, 8
    fl = _flow(dims, float)
    rng = np.random.default_rng(5)
    X = np.stack([_state(dims), fl.march(_state(dims), 3.0, 30, S.PARS)["u"]])
    normal, center = S.update_section(fl, X, S.PARS)
    dX, dT, T = rng.standard_normal(X.shape), 0.3, 6.1
    o, t = S.jvp(fl, X, T, S.PARS, nsteps, dX, dT, normal, center)
    J = S.jacobian_dense(fl, X, T, S.PARS, nsteps, normal, center)
    assert np.abs(J @ S.pack(dX, dT) - S.pack(o, t)).max() <= 1e-11 * np.abs(o).max()
    # dT = 0: the derivative of the residual in X, by central differences
    o0, t0 = S.jvp(fl, X, T, S.PARS, nsteps, dX, 0.0, normal, center)
    h = 1e-6
    gp, gm = (S.residual(fl, X + s * h * dX, T, S.PARS, nsteps, normal, center) for s in (1, -1))
    assert np.abs((gp[0] - gm[0]) / (2 * h) - o0).max() <= 1e-8 * np.abs(o0).max()
    assert abs((gp[1] - gm[1]) / (2 * h) - t0) <= 1e-8 * max(abs(t0), 1.0)


def test_tables_against_mpmath():
    """E, phi1, phi2 at z in {-1e-8, -1e-3, -0.1, -0.99, -1.01, -30, -800}: the long-double tables against mpmath (50 digits) where it
    is installed, else against the two formulas of phi2 evaluated on both sides of the switch at |z| = 1.  Every entry is finite."""
    zs = [-1e-8, -1e-3, -0.1, -0.99, -1.01, -30.0, -800.0]
    E, p1, p2 = S.phi_tables(np.array(zs))
    assert np.all(np.isfinite(E)) and np.all(np.isfinite(p1)) and np.all(np.isfinite(p2))
    try:
        import mpmath
    except ImportError:
        mpmath = None
    epsld = float(np.finfo(LD).eps)
    for i, z in enumerate(zs):
        if mpmath is not None:
            mpmath.mp.dps = 50
            zz = mpmath.mpf(z)
            ref = (mpmath.exp(zz), mpmath.expm1(zz) / zz, (mpmath.expm1(zz) - zz) / zz ** 2)
            for got, want in zip((E[i], p1[i], p2[i]), ref):
                # z = -800: e^z underflows the double range of the device and is compared in absolute terms
                assert abs(mpmath.mpf(float(got)) + mpmath.mpf(float(got - LD(float(got)))) - want) <= 64 * epsld * abs(want) + 1e-300, (z, got, want)
        else:
            series = sum(LD(z) ** k / LD(math.factorial(k + 2)) for k in range(200) if abs(z) < 40) if abs(z) < 40 else None
            if series is not None:
                assert abs(p2[i] - series) <= 1e-15 * abs(series)
    # the double-precision rounding of the tables is what the device is compared with
    assert float(E[-1]) == 0.0 and abs(float(p1[-1]) - 1.0 / 800.0) <= EPS / 800.0


def _close(a, b, rel):
    return abs(a - b) <= rel * max(abs(a), abs(b))


def _check(rec, got):
    assert got["converged"] and rec["converged"]
    assert len(got["residuals"]) == len(rec["residuals"]) and got["residuals"][-1] < 1e-9
    assert _close(got["T"], rec["T"], 1e-9) and _close(got["amplitude"], rec["amplitude"], 1e-8)
    assert max(abs(a - b) for a, b in zip(got["itlinear"], rec["itlinear"])) <= 1
    assert 0.0 <= rec["trivial_distance"] <= 1e-6
    if "multipliers" in got:
        for a, b in zip(got["multipliers"], rec["multipliers"]):
            assert abs(complex(*a) - complex(*b)) <= 1e-7 * max(1.0, abs(complex(*b)))


@pytest.mark.parametrize("k", range(len(S.CYCLE_CASES)))
def test_fixture_holds_the_cycle_cases(k):
    """Newton from the state after t = 120 in 1200 steps from 0.1 rand and T = 6.3, GMRES rtol 1e-4, restart 50: below 1e-9 in at
    most 6 steps; the committed record is what the restatement gives (the dense multipliers of the 41 x 21 case, a 1722 x 1722
    monodromy matrix, are regenerated by `python tests/shooting_ref.py` only)."""
    case = S.CYCLE_CASES[k]
    rec = S.load_fixture()["cycle"][k]
    assert rec["dims"] == list(case[0]) and rec["M"] == case[1] and rec["nsteps"] == case[2]
    got, _, _ = S.cycle_case(*case, with_multipliers=case[0][0] < 32)
    assert len(got["residuals"]) - 1 <= 6
    _check(rec, got)
    # the trivial multiplier: within the time-discretisation error of 1
    mu = [complex(*v) for v in rec["multipliers"]]
    assert min(abs(v - 1.0) for v in mu) <= 1e-6 and max(abs(v) for v in mu) <= 1.0 + 1e-6


@pytest.mark.parametrize("k", range(len(S.HOPF_CASES)))
def test_fixture_holds_the_hopf_side_cases(k):
    """The small orbit at r_H - dr from the normal-form-sized guess: exactly one multiplier outside the unit circle, and the trivial
    one."""
    case = S.HOPF_CASES[k]
    rec = S.load_fixture()["hopf"][k]
    got, s, _ = S.hopf_case(*case)
    _check(rec, got)
    mu = [complex(*v) for v in rec["multipliers"]]
    assert sum(abs(v) > 1.0 + 1e-6 for v in mu) == 1 and min(abs(v - 1.0) for v in mu) <= 1e-6
    assert rec["amplitude"] > 1e-2                       # the orbit, not the trivial state
