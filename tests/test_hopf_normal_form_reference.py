"""The CPU restatement of the Hopf normal form (tests/normal_form_ref.py) against the known answers of the reference's own tests
(Stuart-Landau, COModel), the cGL third derivative against differences of the Hessian formulas, the invariances of a and b, the
closed form the GPU tests use, and the scalars of bk_amd.codim2.predictor against hand-computed values."""
import json
import math
import os
import re

import numpy as np
import pytest

import minaug_hopf_ref as R
import normal_form_ref as NF
from oracle import operators
from test_fold_reference import _com_J
from test_hopf_reference import comodel_hopf  # noqa: F401  (fixture: the refined Hopf points 2 and 5 of COModel)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "reference_normal_form_answers.json")))
NF_ENTRIES = ("bk_hopf_d3f", "bk_hopf_nf_rhs", "bk_hopf_nf_contract", "bk_hopf_normal_form", "bk_hopf_orbit")


def test_binding_declares_the_normal_form_entries():
    from bk_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bkhip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(bk_[a-z0-9_]+)\s*\(", src))
    for name in NF_ENTRIES:
        assert name in declared, f"{name} is not declared in include/bkhip.h"
        assert name in _lib.SIGNATURES, f"{name} is not bound in _lib.SIGNATURES"
    from bk_amd import codim2
    for name in ("hopf_d3F", "hopf_nf_rhs", "hopf_nf_contract", "hopf_orbit", "hopf_normal_form", "hopf_normal_form_native",
                 "hopf_eigenpair", "get_normal_form", "predictor"):
        assert callable(getattr(codim2, name)), name


def test_stuart_landau_matches_the_reference_test():
    """testNF.jl:419,439-440: a = 1 (atol 1e-9), b / 2 = -c3 + i mu (atol 1e-14), at the Hopf point r = 0 of the trivial state,
    for the eigenvalue +i nu; the conjugate eigenvalue gives the conjugate coefficients."""
    g = GOLD["stuart_landau"]
    q = g["params"]
    model, d3F = NF.stuart_landau(**q)
    x, at = np.zeros(2), model.at(0.0)
    z, zs = NF.eigenpair(model.J(x, at), q["nu"])
    nf = NF.hopf_normal_form(model, d3F, x, at, "r", q["nu"], z, zs)
    assert abs(nf["a"] - g["a"]) <= g["atol_a"], nf["a"]
    assert abs(nf["b"] / 2 - complex(-q["c3"], q["mu"])) <= g["atol_half_b"], nf["b"]
    assert nf["type"] == "SuperCritical"
    assert all(np.all(nf[k] == 0) for k in ("Psi001", "Psi110", "Psi200"))
    zc, zsc = NF.eigenpair(model.J(x, at), -q["nu"])
    nfc = NF.hopf_normal_form(model, d3F, x, at, "r", -q["nu"], zc, zsc)
    assert abs(nfc["a"] - np.conj(nf["a"])) <= 1e-14 and abs(nfc["b"] - np.conj(nf["b"])) <= 1e-14, (nfc["a"], nfc["b"])


def _comodel_nf(m, sn, sign=1.0):
    q = m.at(sn["p"])
    om = sign * abs(sn["omega"])
    z, zs = NF.eigenpair(_com_J(sn["u"], q), om)
    zero3 = lambda x, q_, a, b, c: np.zeros(3, dtype=complex)               # COModel is quadratic: d3F = 0
    return NF.hopf_normal_form(m, zero3, sn["u"], q, "q2", om, z, zs)


def test_comodel_normal_forms_match_the_reference_test(comodel_hopf):
    """codim2.jl:38,41: Re b of Hopf points 5 and 2 at the reference's tolerances; codim2.jl:94-95: a and b of point 2.  The
    restatement works at the REFINED Hopf points (q2 = 1.04099157, 1.05155746), the reference at the bisected ones (q2 =
    1.04099606, 1.05158367): the values of :94-95 differ from the refined point's by 2.3e-3 (a) and 1.5e-3 (b) relative, so they
    are asserted at the looser of the reference's own tolerances for this quantity, rtol 1e-2 (:41)."""
    m, sols = comodel_hopf
    nf2, nf5 = _comodel_nf(m, sols[0]), _comodel_nf(m, sols[1])
    g = GOLD["comodel_re_b"]
    print(f"COModel point 2: a = {nf2['a']:.6f}, b = {nf2['b']:.6f}; point 5: a = {nf5['a']:.6f}, b = {nf5['b']:.6f}")
    assert abs(nf5["b"].real - g["point5"]) <= g["rtol5"] * abs(g["point5"]), nf5["b"]
    assert abs(nf2["b"].real - g["point2"]) <= g["rtol2"] * abs(g["point2"]), nf2["b"]
    g2 = GOLD["comodel_point2"]
    a_ref, b_ref = complex(*g2["a"]), complex(*g2["b"])
    assert abs(nf2["a"] - a_ref) <= g2["rtol"] * abs(a_ref), nf2["a"]
    assert abs(nf2["b"] - b_ref) <= g2["rtol"] * abs(b_ref), nf2["b"]
    assert nf2["type"] == nf5["type"] == "SubCritical"
    # the conjugate eigenvalue gives the conjugate coefficients: the signs of Im a, Im b follow the sign of omega
    nf2c = _comodel_nf(m, sols[0], -1.0)
    assert abs(nf2c["a"] - np.conj(nf2["a"])) <= 1e-9 * abs(nf2["a"]) and abs(nf2c["b"] - np.conj(nf2["b"])) <= 1e-9 * abs(nf2["b"])


def _random_cgl(seed, dims=(9, 7)):
    rng = np.random.default_rng(seed)
    pars = dict(r=0.3, mu=0.1, nu=1.0, c3=-1.0, c5=1.0, gamma=0.2)
    n = 2 * int(np.prod(dims))
    return rng, pars, n


def test_cgl_d3F_matches_central_differences_of_the_hessian_formulas():
    rng, pars, n = _random_cgl(6)
    u, a, b, c = 0.7 * rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
    eps = 1e-5
    fd = (R.cgl_d2F(u + eps * c, pars, a, b) - R.cgl_d2F(u - eps * c, pars, a, b)) / (2 * eps)
    ref = NF.cgl_d3F(u, pars, a, b, c)
    assert np.abs(fd - ref).max() <= 1e-8 * np.abs(ref).max()
    for perm in ((b, a, c), (c, b, a), (a, c, b)):                          # symmetric in its three arguments
        assert np.abs(NF.cgl_d3F(u, pars, *perm) - ref).max() <= 1e-13 * np.abs(ref).max()
    z = a + 1j * b                                                          # complex arguments by linearity
    lin = NF.cgl_d3F(u, pars, a, c, c) + 1j * NF.cgl_d3F(u, pars, b, c, c)
    assert np.abs(NF.cgl_d3F(u, pars, z, c, c) - lin).max() <= 1e-13 * np.abs(lin).max()
    assert np.all(NF.cgl_d3F_abs(u, pars, a, b, c) >= np.abs(ref))
    assert np.all(NF.cgl_d2F_abs(u, pars, a, b) >= np.abs(R.cgl_d2F(u, pars, a, b)))


def _nontrivial_cgl_hopf(dims=(9, 7), ls=(np.pi, np.pi / 2)):
    """A refined Hopf point of cGL off the trivial state (gamma = 0.1) on a small grid: (model, solution, zeta, zeta*)."""
    op = operators.CGL2d(dims, ls)
    lam = []
    for nn, l in zip(dims, ls):
        h = 2 * l / nn
        lam.append(-(4 / h ** 2) * np.sin(np.pi / (2 * (nn + 1))) ** 2)
    rstar = -(lam[0] + lam[1])
    pars = dict(r=rstar, mu=0.1, nu=1.0, c3=-1.0, c5=1.0, gamma=0.1)
    m = R.cgl_model(op, pars, "r")
    zr, zi = _hopf_mode(dims)
    s = R.newton_hopf(m, np.zeros(2 * dims[0] * dims[1]), rstar, 1.0, zr + 1j * zi, zr + 1j * zi, tol=1e-12, max_iterations=20)
    assert s["converged"] and np.abs(s["u"]).max() > 0.05, s["residuals"]
    z, zs = NF.normalise(s["v"], s["w"])
    return m, s, z, zs


def _hopf_mode(dims):
    x = np.sin(np.pi * np.arange(1, dims[0] + 1) / (dims[0] + 1))
    y = np.sin(np.pi * np.arange(1, dims[1] + 1) / (dims[1] + 1))
    phi = np.outer(y, x).reshape(-1)
    phi /= np.linalg.norm(phi) * math.sqrt(2)
    z = np.zeros_like(phi)
    return np.concatenate([phi, z]), np.concatenate([z, -phi])


def test_coefficients_are_invariant_under_the_phase_and_scale_as_the_square_of_the_modulus():
    """a and b do not depend on the phase of zeta (zeta* turns with it); under zeta -> c zeta with zeta* renormalised to
    <zeta, zeta*> = 1, a stays and b -> |c|^2 b (b is cubic in (zeta, conj zeta, zeta*), zeta* -> zeta* / conj c)."""
    m, s, z, zs = _nontrivial_cgl_hopf()
    q = m.at(s["p"])
    nf = NF.hopf_normal_form(m, NF.cgl_d3F, s["u"], q, "r", s["omega"], z, zs)
    assert abs(nf["b"]) > 1e-3 and abs(nf["a"]) > 1e-3 and all(np.abs(nf[k]).max() > 1e-6 for k in ("Psi001", "Psi110", "Psi200"))
    ph = np.exp(0.7j)
    nfp = NF.hopf_normal_form(m, NF.cgl_d3F, s["u"], q, "r", s["omega"], ph * z, ph * zs)
    assert abs(nfp["a"] - nf["a"]) <= 1e-12 * abs(nf["a"]) and abs(nfp["b"] - nf["b"]) <= 1e-12 * abs(nf["b"]), (nfp, nf)
    c = 1.7 * np.exp(-0.4j)
    z2, zs2 = c * z, zs / np.conj(c)
    assert abs(np.vdot(z2, zs2) - 1) <= 1e-14
    nfc = NF.hopf_normal_form(m, NF.cgl_d3F, s["u"], q, "r", s["omega"], z2, zs2)
    assert abs(nfc["a"] - nf["a"]) <= 1e-12 * abs(nf["a"]), (nfc["a"], nf["a"])
    assert abs(nfc["b"] - abs(c) ** 2 * nf["b"]) <= 1e-12 * abs(nfc["b"]), (nfc["b"], nf["b"])
    with pytest.raises(ValueError, match="normalization"):
        NF.hopf_normal_form(m, NF.cgl_d3F, s["u"], q, "r", s["omega"], z, 0.5 * zs)


@pytest.mark.parametrize("dims", [(7, 5), (6, 4), (12, 9)])
@pytest.mark.parametrize("c3", [-1.0, 0.8])
def test_closed_form_on_the_trivial_state_matches_the_dense_restatement(dims, c3):
    """u = 0, gamma = 0, r* = -lam_11: a = 1, b = 2 (-c3 + i mu) 9 / (4 (Nx + 1)(Ny + 1)) for omega = +nu; conjugates for -nu."""
    ls = (np.pi, np.pi / 2)
    op = operators.CGL2d(dims, ls)
    lam = [-(4 / (2 * l / nn) ** 2) * np.sin(np.pi / (2 * (nn + 1))) ** 2 for nn, l in zip(dims, ls)]
    pars = dict(r=-(lam[0] + lam[1]), mu=0.1, nu=1.0, c3=c3, c5=1.0, gamma=0.0)
    m = R.cgl_model(op, pars, "r")
    zr, zi = _hopf_mode(dims)
    z = zr + 1j * zi
    x = np.zeros(2 * dims[0] * dims[1])
    a0, b0 = NF.cgl_closed_form(dims, pars["mu"], c3)
    nf = NF.hopf_normal_form(m, NF.cgl_d3F, x, dict(pars), "r", pars["nu"], z, z)
    assert abs(nf["a"] - a0) <= 1e-14 and abs(nf["b"] - b0) <= 1e-14 * abs(b0), (nf["a"], nf["b"], b0)
    assert nf["type"] == ("SuperCritical" if c3 > 0 else "SubCritical")
    nfc = NF.hopf_normal_form(m, NF.cgl_d3F, x, dict(pars), "r", -pars["nu"], np.conj(z), np.conj(z))
    assert abs(nfc["a"] - np.conj(a0)) <= 1e-14 and abs(nfc["b"] - np.conj(b0)) <= 1e-14 * abs(b0)


@pytest.mark.parametrize("a, b, ds, want", [
    # Re a Re b < 0: the orbits live at p > p0 (dsfactor +1), whatever the sign of ds
    (2 + 1j, -8 + 3j, 0.02, dict(dsfactor=1, p=0.32, amp_orbit=math.sqrt(0.02 * 2 / 8), omega=1.5 + (1 + 3 * 2 / 8) * 0.02)),
    (2 + 1j, -8 + 3j, -0.02, dict(dsfactor=1, p=0.32, amp_orbit=math.sqrt(0.02 * 2 / 8), omega=1.5 - (1 + 3 * 2 / 8) * 0.02)),
    (-2 + 1j, 8 + 3j, 0.02, dict(dsfactor=1, p=0.32, amp_orbit=math.sqrt(0.02 * 2 / 8), omega=1.5 + (1 + 3 * 2 / 8) * 0.02)),
    # Re a Re b > 0: at p < p0 (dsfactor -1)
    (2 - 1j, 8 + 3j, 0.02, dict(dsfactor=-1, p=0.28, amp_orbit=math.sqrt(0.02 * 2 / 8), omega=1.5 + (-1 - 3 * 2 / 8) * 0.02)),
    (-2 - 1j, -8 - 3j, 0.02, dict(dsfactor=-1, p=0.28, amp_orbit=math.sqrt(0.02 * 2 / 8), omega=1.5 + (-1 + 3 * 2 / 8) * 0.02)),
])
def test_predictor_record_matches_the_formulas(a, b, ds, want):
    """predictor(hp, ds) (NormalForms.jl:1241-1249, 1273-1280) on hand-picked coefficients of each sign pattern, p0 = 0.3,
    omega0 = 1.5: dsfactor, p = p0 + |ds| dsfactor, amp = 2 sqrt(-dp Re a / Re b) in the record, omega = omega0 + (Im a -
    Im b Re a / Re b) ds, period = |2 pi / omega|; the product's predictor and the restatement's give the same record."""
    from bk_amd import codim2
    hp = codim2.Hopf(x0=None, p=0.3, omega=1.5, zeta=None, zeta_star=None, nf=codim2.HopfNormalForm(a=a, b=b))
    for amf in (1.0, 0.5):
        rec, ref = codim2.predictor(hp, ds, ampfactor=amf), NF.predictor(0.3, 1.5, a, b, ds, ampfactor=amf)
        assert rec["dsfactor"] == ref["dsfactor"] == want["dsfactor"]
        assert abs(rec["p"] - want["p"]) <= 1e-15 and abs(ref["p"] - want["p"]) <= 1e-15
        assert abs(rec["amp"] - 2 * amf * want["amp_orbit"]) <= 1e-15 and abs(ref["amp"] - rec["amp"]) <= 1e-15
        assert abs(rec["orbit"].amp - amf * want["amp_orbit"]) <= 1e-15 and rec["orbit"].ds == ds
        assert abs(rec["omega"] - want["omega"]) <= 1e-15 and abs(ref["omega"] - rec["omega"]) <= 1e-15
        assert abs(rec["period"] - 2 * math.pi / want["omega"]) <= 1e-14
        assert set(rec) == {"orbit", "Psi001", "amp", "omega", "period", "p", "dsfactor"}
    assert codim2.hopf_type(b) == NF.hopf_type(b) == ("SuperCritical" if b.real < 0 else "SubCritical")


def test_predictor_without_coefficients_and_singular_point():
    from bk_amd import codim2
    hp = codim2.Hopf(x0=None, p=0.3, omega=-1.5, zeta=None, zeta_star=None)
    rec = codim2.predictor(hp, -0.1, ampfactor=0.25)                         # :1253-1260
    assert (rec["p"], rec["amp"], rec["omega"], rec["dsfactor"]) == (0.3 - 0.1, 0.5, -1.5, 1)
    assert abs(rec["period"] - 2 * math.pi / 1.5) <= 1e-15
    hp = codim2.Hopf(x0=None, p=0.3, omega=1.5, zeta=None, zeta_star=None, nf=codim2.HopfNormalForm(a=1 + 0j, b=2j))
    assert codim2.hopf_type(hp.nf.b) == "Singular"
    with pytest.raises(ValueError, match="singular"):
        codim2.predictor(hp, 0.1)


def test_orbit_restatement_is_two_pi_periodic_and_real():
    rng = np.random.default_rng(8)
    n = 10
    x0, P001, P110 = (rng.standard_normal(n) for _ in range(3))
    z, P200 = rng.standard_normal(n) + 1j * rng.standard_normal(n), rng.standard_normal(n) + 1j * rng.standard_normal(n)
    o = lambda t: NF.orbit(x0, z, P001, P110, P200, 0.03, 0.2, t)
    assert np.abs(o(0.4) - o(0.4 + 2 * np.pi)).max() <= 1e-14
    assert np.abs(o(0.0) - (x0 + 0.4 * z.real + 0.03 * P001 + 0.04 * P110 + 0.08 * P200.real)).max() <= 1e-15
