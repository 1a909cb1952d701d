"""The CPU restatement of the Bautin normal form (tests/bautin_ref.py) against the known answer of the reference's own test
(Stuart-Landau, l2 = 4 c5), the analytic fourth and fifth derivatives of cGL against differences of the third, the identities the
library call relies on (G21 = 2 conj(b), h22 real, what vanishes on the trivial state), the yardstick of the GPU comparisons, the
binding of the new entries and the host-side pieces of the detection on Hopf curves."""
import itertools
import math
import os
import re

import numpy as np
import pytest

import bautin_ref as BR
import minaug_hopf_ref as R
import normal_form_ref as NF
from conftest import probe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(float).eps
ENTRIES = {"bk_bautin_rhs3": 14, "bk_bautin_rhs4": 17, "bk_bautin_contract": 19, "bk_bautin_normal_form": 26}


def test_binding_declares_the_bautin_entries_with_the_arguments_of_the_header():
    from bk_amd import _lib, codim2
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bkhip.h")).read(), flags=re.S)
    for name, nargs in ENTRIES.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", src)
        assert m, f"{name} is not declared in include/bkhip.h"
        assert len(m.group(1).split(",")) == nargs, (name, m.group(1))
        assert name in _lib.SIGNATURES, f"{name} is not bound in _lib.SIGNATURES"
        assert len(_lib.SIGNATURES[name][1]) == nargs, (name, len(_lib.SIGNATURES[name][1]))
    assert _lib.BK_ABI_VERSION == 6
    for name in ("bautin_rhs3", "bautin_rhs4", "bautin_contract", "bautin_normal_form", "bautin_normal_form_native", "Bautin",
                 "get_normal_form", "continuation_hopf"):
        assert callable(getattr(codim2, name)), name


def test_stuart_landau_second_lyapunov_coefficient_matches_the_reference_test():
    """test/normal_forms/testNF.jl:564-600: Fsl2! with c3 = 0.1, c5 = 0.3, mu = 0, nu = 1; the Hopf curve in (r, c3) of the
    trivial state is r = 0 and its Bautin point c3 = 0, where the reference asserts l2 = 4 c5 at atol 1e-6 (:600; its D and E are
    finite differences).  With the analytic tensors: 1e-12.  At c3 = 0.1 (off the Bautin point) G21 = 2 conj(b) = 4 c3."""
    m, d3, d4, d5 = BR.stuart_landau_reference(r=0.0, mu=0.0, nu=1.0, c3=0.0, c5=0.3)
    x, par = np.zeros(2), m.at(0.0)
    z, zs = NF.eigenpair(m.J(x, par), 1.0)
    nf = BR.bautin_normal_form(m, d3, d4, d5, x, par, 1.0, z, zs)
    assert abs(nf["l2"] - 4 * 0.3) <= 1e-12, nf["l2"]
    assert nf["type"] == "Subcritical" and abs(nf["G21"]) <= 1e-15
    m, d3, d4, d5 = BR.stuart_landau_reference(r=0.0, mu=0.0, nu=1.0, c3=0.1, c5=0.3)
    nf1 = BR.bautin_normal_form(m, d3, d4, d5, x, m.at(0.0), 1.0, z, zs)
    b = NF.hopf_normal_form(m, d3, x, m.at(0.0), "r", 1.0, z, zs)["b"]
    assert abs(nf1["G21"] - 2 * np.conj(b)) <= 1e-15 and abs(nf1["G21"] - 0.4) <= 1e-15, (nf1["G21"], b)
    with pytest.raises(ValueError, match="normalization"):
        BR.bautin_normal_form(m, d3, d4, d5, x, par, 1.0, z, 0.5 * zs)


def test_cgl_d4F_and_d5F_match_central_differences_and_are_symmetric():
    """D is linear in u, so the central difference quotient of cgl_d3F in u is D up to the rounding of the two evaluations over
    the step: 8 eps sum |monomials of d3F| / (2 h) (each evaluation within 4 eps of its monomial sum, as the device test of d3F
    counts); E against the quotient of D in the same way, D being exact in u there too (E is constant)."""
    rng = np.random.default_rng(3)
    pars = dict(r=0.3, mu=0.1, nu=1.0, c3=-1.0, c5=1.0, gamma=0.2)
    n = 2 * 63
    u, a, b, c, d, e = (0.7 * rng.standard_normal(n) if k == 0 else rng.standard_normal(n) for k in range(6))
    h = 1e-3
    fd = (NF.cgl_d3F(u + h * d, pars, a, b, c) - NF.cgl_d3F(u - h * d, pars, a, b, c)) / (2 * h)
    D = BR.cgl_d4F(u, pars, a, b, c, d)
    scale3 = np.maximum(NF.cgl_d3F_abs(u + h * d, pars, a, b, c), NF.cgl_d3F_abs(u - h * d, pars, a, b, c))
    assert np.all(np.abs(fd - D) <= 8 * EPS * scale3 / (2 * h) + 8 * EPS * np.abs(D)), np.abs(fd - D).max()
    fe = (BR.cgl_d4F(u + h * e, pars, a, b, c, d) - BR.cgl_d4F(u - h * e, pars, a, b, c, d)) / (2 * h)
    E = BR.cgl_d5F(u, pars, a, b, c, d, e)
    scale4 = np.maximum(BR.cgl_d4F_abs(u + h * e, pars, a, b, c, d), BR.cgl_d4F_abs(u - h * e, pars, a, b, c, d))
    assert np.all(np.abs(fe - E) <= 8 * EPS * scale4 / (2 * h) + 8 * EPS * np.abs(E)), np.abs(fe - E).max()
    assert np.abs(D).max() > 1 and np.abs(E).max() > 1
    for perm in itertools.permutations((a, b, c, d)):
        assert np.abs(BR.cgl_d4F(u, pars, *perm) - D).max() <= 1e-13 * np.abs(D).max()
    for perm in itertools.islice(itertools.permutations((a, b, c, d, e)), 0, 120, 7):
        assert np.abs(BR.cgl_d5F(u, pars, *perm) - E).max() <= 1e-13 * np.abs(E).max()
    z = a + 1j * b                                                          # complex arguments by linearity
    lin = BR.cgl_d4F(u, pars, a, c, c, d) + 1j * BR.cgl_d4F(u, pars, b, c, c, d)
    assert np.abs(BR.cgl_d4F(u, pars, z, c, c, d) - lin).max() <= 1e-13 * np.abs(lin).max()
    assert np.all(BR.cgl_d4F_abs(u, pars, a, b, c, d) >= np.abs(D)) and np.all(BR.cgl_d5F_abs(u, pars, a, b, c, d, e) >= np.abs(E))


def test_trivial_state_of_cgl_on_the_example_grid():
    """41 x 21, u = 0, gamma = 0, c3 = 0, r* = -lam_11, omega = nu, zeta = zeta* = phi (1, -i) / sqrt 2: B(0) = 0 and D(0) = 0, so
    H20, H11, H31, H22 vanish exactly, H30 to rounding (C(q, q, q) = 0 analytically for this zeta), Re b = 0 and l2 < 0 comes
    from E and the C-H21 terms alone."""
    from oracle import operators
    op = operators.CGL2d(BR.DIMS, BR.LS)
    pars = dict(BR.PARS, c3=0.0, r=BR.first_hopf_r(BR.DIMS, BR.LS))
    m = R.cgl_model(op, pars, "r")
    z = BR._hopf_mode(BR.DIMS)
    x = np.zeros(2 * op.n)
    nf = BR.bautin_normal_form(m, NF.cgl_d3F, BR.cgl_d4F, BR.cgl_d5F, x, dict(pars), pars["nu"], z, z)
    for k in ("H20", "H11", "H31", "H22"):
        assert np.abs(nf[k]).max() == 0.0, k
    assert np.abs(nf["H30"]).max() <= EPS
    b = NF.hopf_normal_form(m, NF.cgl_d3F, x, dict(pars), "r", pars["nu"], z, z)["b"]
    assert abs(b.real) <= 1e-18 and abs(nf["G21"] - 2 * np.conj(b)) <= 1e-18
    assert abs(nf["l2"] - (-2.92996e-5)) <= 1e-10, nf["l2"]
    assert nf["type"] == "Supercritical"


def test_bautin_point_of_the_cgl_hopf_curve_and_the_yardstick_of_the_gpu_tests():
    """gamma = 0.1, 41 x 21: Re b changes sign once between c3 = -0.2 and 0, near c3 = -0.102 (r = 1.1455, omega = 0.99716).  There
    G21 = 2 conj(b), h22 is real, all six H vectors are alive and l2 = -2.99e-5.  The yardstick of the GPU comparisons is logged:
    the restatement's own spread between direct solves and left-preconditioned SciPy GMRES at the device's reltol, and what the GPU
    tests allow, 10 x it plus, for a coefficient, the rounding of its own sum (bautin_ref.cgl_bautin_yardstick)."""
    y = BR.cgl_bautin_yardstick()
    loc, lu = y["loc"], y["lu"]
    reb = [g for _, g in loc["curve"]]
    assert sum(1 for g0, g1 in zip(reb, reb[1:]) if g0 * g1 < 0) == 1 and reb[0] > 0, loc["curve"]
    assert abs(loc["p2"] + 0.1024) <= 1e-3 and abs(loc["p1"] - 1.1455) <= 1e-3 and abs(loc["omega"] - 0.99716) <= 1e-4, loc
    assert abs(loc["b"].real) <= 1e-14, loc["b"]
    b = NF.hopf_normal_form(y["model"], NF.cgl_d3F, loc["u"], y["par"], "r", loc["omega"], y["zeta"], y["zeta_star"])["b"]
    assert abs(lu["G21"] - 2 * np.conj(b)) <= 1e-17, (lu["G21"], b)
    h22 = lu["rhs"][3]
    assert np.abs(h22.imag).max() <= 1e-15 * np.abs(h22.real).max()
    for k in ("H20", "H11", "H30", "H21", "H31", "H22"):
        assert 1e-5 <= np.abs(lu[k]).max() <= 1e-2, (k, np.abs(lu[k]).max())
    assert abs(lu["l2"] + 2.99e-5) <= 1e-7 and lu["type"] == "Supercritical", lu["l2"]
    assert abs(np.vdot(y["zeta_star"], lu["H21"])) <= 1e-14                  # the bordering row: p0^H H21 = 0
    for k, v in y["spread"].items():
        ref = abs(lu[k]) if np.isscalar(lu[k]) else np.abs(lu[k]).max()
        print(f"yardstick {k}: spread {v:.3e} ({v / ref:.1e} relative), summation {y['summation'].get(k, 0.0):.3e}, "
              f"allowed {y['allowed'].get(k, float('nan')):.3e}")
        probe(f"bautin.yardstick_spread.{k}", v / ref, 1e-12)
    for k, v in y["allowed"].items():
        ref = abs(lu[k]) if np.isscalar(lu[k]) else np.abs(lu[k]).max()
        probe(f"bautin.yardstick_allowed.{k}", v / ref, 1e-10)


def test_detection_pieces_on_the_host():
    """The GH test function keeps the previous value when |Re b| >= 1e5 (MinAugHopf.jl:632), a sign change is a strict one, the
    record types follow the sign of l2, and lens2 is restored after a block at another value."""
    from bk_amd import codim2
    assert codim2._gh_value(complex(0.25, 3.0), math.nan) == 0.25
    assert codim2._gh_value(complex(-2e5, 0.0), 0.5) == 0.5
    assert codim2._sign_change(1e-3, -1e-5) and not codim2._sign_change(1e-3, 2e-3) and not codim2._sign_change(0.0, -1.0)
    assert codim2.bautin_type(-3e-5) == "Supercritical" == BR.bautin_type(-3e-5)
    assert codim2.bautin_type(1.2) == "Subcritical" == BR.bautin_type(1.2)
    prob = type("P", (), dict(params=dict(r=0.5, c3=-1.0)))()
    with codim2._lens2_at(prob, "c3", -0.1):
        assert prob.params["c3"] == -0.1
    assert prob.params == dict(r=0.5, c3=-1.0)
    br = codim2.HopfBranch(lens2="c3")
    assert br.l1 == [] and br.GH == [] and br.specialpoint == [] and br.lens2 == "c3"
    hp = codim2.Hopf(x0=None, p=1.0, omega=0.9, zeta=None, zeta_star=None, nf=codim2.HopfNormalForm(b=1e-3 + 2e-3j),
                     params=[1.0, 0.1, 1.0, -0.1, 1.0, 0.1], lens="r")
    rec = codim2._bautin_record(hp, "c3", 2 * np.conj(hp.nf.b), complex(-3.6e-4, 1e-6), None, None, None, None, None, True,
                                (3, 8, 4, 5), 0)
    assert rec.lens == ("r", "c3") and rec.type == "Supercritical" and rec.nf.l2 == -3.6e-4 / 12 and rec.nf.omega == 0.9
    assert rec.nf.G21 == complex(2e-3, -4e-3) and rec.itlinear == (3, 8, 4, 5) and rec.converged is True
