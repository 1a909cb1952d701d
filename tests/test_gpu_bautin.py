"""GPU tests of the Bautin normal form and of the detection of generalised Hopf points on Hopf curves of cGL (bk_bautin_rhs3,
bk_bautin_rhs4, bk_bautin_contract, bk_bautin_normal_form; bk_amd.codim2): the two writing passes against the restatement
(tests/bautin_ref.py) in extended precision, the reducing pass against an exact sum, and the normal form -- native, call-by-call
mirror and dense restatement -- on the trivial state and at the Bautin point of the Hopf curve in (r, c3) at gamma = 0.1, then
continuation_hopf(detect_codim2 = 2) -> get_normal_form end to end.  The bounds of the comparisons with the restatement are
bautin_ref.cgl_bautin_yardstick()["allowed"]: 10 x the restatement's own spread between direct solves and SciPy GMRES with the
device's left preconditioning and reltol; a coefficient is also allowed the rounding of its own sum."""
import math

import numpy as np
import pytest

import bautin_ref as BR
import minaug_hopf_ref as R
import normal_form_ref as NF
from conftest import probe
from test_gpu_hopf import _pair, _solver, _vec_at

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
LD, CLD = np.longdouble, np.clongdouble
DIMS, LS, PARS = BR.DIMS, BR.LS, BR.PARS
HVECS = ("H30", "H21", "H31", "H22")


def _lib():
    from bk_amd import codim2, hip
    return codim2, hip


def _pv(pars):
    return [pars[k] for k in R.CGL_PARAMS]


def _model(pars):
    return R.HopfModel(None, None, R.cgl_d2F, None, None, pars, "r")


def _cplx(rng, n, s=1.0):
    return s * (rng.standard_normal(n) + 1j * rng.standard_normal(n))


def _dev_c(dev, z):
    return dev(np.ascontiguousarray(z.real)), dev(np.ascontiguousarray(z.imag))


def _num(pair):
    return pair[0].numpy() + 1j * pair[1].numpy()


# ------------------------------------------------------------------------------------------ 1: the writing passes
def _rhs3_abs(u, pars, q, H20, H11, G21):
    B = lambda a, b: NF.cgl_d2F_abs(u, pars, a, b)
    C = lambda a, b, c: NF.cgl_d3F_abs(u, pars, a, b, c)
    a, A, Bv, g = BR.cabs(q), BR.cabs(H20), np.abs(H11), BR.cabs(G21)
    return C(a, a, a) + 3 * B(a, A), g * a + C(a, a, a) + B(a, A) + 2 * B(a, Bv)


def _rhs4_abs(u, pars, q, H20, H11, H30, H21, G21):
    B = lambda a, b: NF.cgl_d2F_abs(u, pars, a, b)
    C = lambda a, b, c: NF.cgl_d3F_abs(u, pars, a, b, c)
    D = lambda a, b, c, d: BR.cgl_d4F_abs(u, pars, a, b, c, d)
    a, A, Bv, c30, c21, g = BR.cabs(q), BR.cabs(H20), np.abs(H11), BR.cabs(H30), BR.cabs(H21), BR.cabs(G21)
    h31 = D(a, a, a, a) + 3 * C(a, a, Bv) + 3 * C(a, a, A) + 3 * B(A, Bv) + B(a, c30) + 3 * B(a, c21) + 3 * g * A
    h22 = D(a, a, a, a) + 4 * C(a, a, Bv) + 2 * C(a, a, A) + 2 * B(Bv, Bv) + 4 * B(a, c21) + B(A, A) + 4 * g * Bv
    return h31, h22


def _sub(v, idx, N):
    """The entries of both stacked fields of v at the grid points idx."""
    return np.concatenate([v[idx], v[N + idx]])


@pytest.mark.parametrize("dims, offset", [((24, 16), 0), ((24, 16), 1), ((23, 17), 0), ((2048, 1024), 0)])
def test_bautin_rhs_passes_match_the_restatement(ctx, dims, offset):
    """bk_bautin_rhs3 and bk_bautin_rhs4 on random inputs against BR.rhs3 / BR.rhs4 in extended precision, in units of
    eps * (sum of the moduli of the monomials).  Roundings on the longest path of the device expressions (csrc/bautin.hip,
    -ffp-contract=off; a tensor entry of cgl_hess carries at most 8, of cgl_d3 5, of cgl_d4 3; lowering a real tensor by a complex
    vector adds 2, a complex one 3, the last dot 3, or 2 against a real vector):
      h30: B(q, H20) 8 + 2 + 3, times 3, plus the C term: 15;   h21: 15 for the three-term sum, G21 q - (.) : 16
      h31: 3 ((((C + C) + B) + B(q, H21)) - G21 H20): 13, 14, 15, 16, 17, times 3: 18, plus (D(q, q, q, conj q) + B(conj q, H30)): 19
      h22: ((r0 + 2 r2) + 4 r4) with r0 = D.. (3 + 2 + 3 + 3 + 3 = 14) + B(H20, conj H20) (13): 15, then 16 and 17
    i.e. at most 8 / 9.5 units; the bounds are the counts, 16 for the first pass and 19 for the second.  Aligned, misaligned and
    odd-point-count layouts, and n = 2^22 (non-temporal instantiation; the restatement on 12288 of its points)."""
    codim2, hip = _lib()
    rng = np.random.default_rng(41 + offset + dims[0])
    pars = dict(PARS, r=0.3, gamma=0.2)
    prob = hip.CGL2d(ctx, dims, LS, **pars)
    n, N = prob.nlocal, prob.nlocal // 2
    assert dims[0] < 2048 or n >= 1 << 22
    u, H11 = 0.6 * rng.standard_normal(n), rng.standard_normal(n)
    q, H20, H30, H21 = (_cplx(rng, n) for _ in range(4))
    G21 = complex(0.7, -1.3)
    dev = lambda x: _vec_at(ctx, hip, x, offset)
    U, Q, A, B_, C30, C21 = dev(u), _dev_c(dev, q), _dev_c(dev, H20), dev(H11), _dev_c(dev, H30), _dev_c(dev, H21)
    h30, h21 = codim2.bautin_rhs3(prob, U, _pv(pars), Q, A, B_, G21)
    h31, h22 = codim2.bautin_rhs4(prob, U, _pv(pars), Q, A, B_, C30, C21, G21)
    idx = np.arange(N) if N <= 1 << 16 else np.unique(np.concatenate([np.arange(4096), N - 1 - np.arange(4096),
                                                                     rng.integers(0, N, 4096)]))
    s = lambda v: _sub(v, idx, N)
    us, qs, As, Bs, C30s, C21s = s(u), s(q), s(H20), s(H11), s(H30), s(H21)
    m = _model(pars)
    xl = lambda v: v.astype(CLD if np.iscomplexobj(v) else LD)
    r30, r21 = BR.rhs3(m, NF.cgl_d3F, xl(us), pars, xl(qs), xl(As), xl(Bs), CLD(G21))
    r31, r22 = BR.rhs4(m, NF.cgl_d3F, BR.cgl_d4F, xl(us), pars, xl(qs), xl(As), xl(Bs), xl(C30s), xl(C21s), CLD(G21))
    a30, a21 = _rhs3_abs(us, pars, qs, As, Bs, G21)
    a31, a22 = _rhs4_abs(us, pars, qs, As, Bs, C30s, C21s, G21)
    tag = f"{dims[0]}x{dims[1]}+{offset}"
    for name, got, ref, unit, bound in (("h30", s(_num(h30)), r30, a30, 16.0), ("h21", s(_num(h21)), r21, a21, 16.0),
                                        ("h31", s(_num(h31)), r31, a31, 19.0)):
        probe(f"bautin.rhs_{name}_re_ulps.{tag}", float((np.abs(got.real - ref.real) / (EPS * unit)).max()), bound, tight=4.0)
        probe(f"bautin.rhs_{name}_im_ulps.{tag}", float((np.abs(got.imag - ref.imag) / (EPS * unit)).max()), bound, tight=4.0)
    probe(f"bautin.rhs_h22_ulps.{tag}", float((np.abs(s(h22.numpy()) - r22.real) / (EPS * a22)).max()), 19.0, tight=4.0)
    assert float(np.abs(r22.imag).max()) <= 1e-16 * float(np.abs(r22.real).max())     # h22 is real: rounding of the extended format


# ------------------------------------------------------------------------------------------ 2: the reducing pass
def _contract_case(ctx, dims, offset, seed):
    codim2, hip = _lib()
    rng = np.random.default_rng(seed)
    pars = dict(PARS)
    prob = hip.CGL2d(ctx, dims, (1.0, 1.0), **pars)
    n = prob.nlocal
    u, H11, H22 = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
    q, p0, H20, H30, H21, H31 = (_cplx(rng, n) for _ in range(6))
    dev = (lambda x: _vec_at(ctx, hip, x, offset)) if offset else prob.vec
    got = codim2.bautin_contract(prob, dev(u), _pv(pars), _dev_c(dev, q), _dev_c(dev, p0), _dev_c(dev, H20), dev(H11),
                                 _dev_c(dev, H30), _dev_c(dev, H21), _dev_c(dev, H31), dev(H22))
    terms = np.conj(p0) * BR.g32_vector(_model(pars), NF.cgl_d3F, BR.cgl_d4F, BR.cgl_d5F, u, pars, q, H20, H11, H30, H21, H31, H22)
    for part in ("real", "imag"):
        t = getattr(terms, part)
        bound = 4 * n * EPS * np.abs(t).sum() + 1e-300
        probe(f"bautin.contract_{part}.N{n // 2}+{offset}", abs(getattr(got, part) - math.fsum(t)) / bound, 1.0)


@pytest.mark.parametrize("Nx", [2, 3, 127, 128, 4099, 65537])
@pytest.mark.parametrize("offset", [0, 1])
def test_bautin_contract_matches_an_exact_sum(ctx, Nx, offset):
    """G32 within the summation-rounding bound of the fp64 sum, 4 n eps sum |terms| per component, against math.fsum of the
    restatement's per-point terms conj(p0) g32 on fifteen random vectors: the grid / alignment matrix of
    test_hopf_nf_contract_matches_an_exact_sum (Ny = 2 for even Nx, 3 for odd Nx: an odd point count misaligns the second field)."""
    _contract_case(ctx, (Nx, 2 if Nx % 2 == 0 else 3), offset, 200 + Nx + offset)


def test_bautin_contract_non_temporal_path_at_2048_squared(ctx):
    """n = 2 * 2048^2 = 2^23 >= 2^22 selects the non-temporal 16-B instantiation: the exact sum as for the small lengths."""
    _contract_case(ctx, (2048, 2048), 0, 13)


# ------------------------------------------------------------------------------------------ 3: the trivial state
def _check_ulps(name, a, b, ulps):
    a, b = np.asarray(a), np.asarray(b)
    scale = np.maximum(np.abs(a), np.abs(b)).max()
    assert np.abs(a - b).max() <= ulps * EPS * scale, (name, np.abs(a - b).max(), scale)


def _compare_native_and_mirror(na, mi, ulps=8):
    """Native and mirror issue the same solves on fresh contexts: equal GMRES counts and flags, the results to ``ulps``."""
    assert na.itlinear == mi.itlinear and na.converged == mi.converged and na.type == mi.type, (na.itlinear, mi.itlinear)
    for k in ("G21", "G32", "l2"):
        _check_ulps(k, [complex(getattr(na.nf, k)).real, complex(getattr(na.nf, k)).imag],
                    [complex(getattr(mi.nf, k)).real, complex(getattr(mi.nf, k)).imag], ulps)
    for k in HVECS:
        a, b = getattr(na.nf, k), getattr(mi.nf, k)
        _check_ulps(k, _num(a) if isinstance(a, tuple) else a.numpy(), _num(b) if isinstance(b, tuple) else b.numpy(), ulps)


def test_bautin_normal_form_on_the_trivial_state_native_and_mirror():
    """41 x 21, u = 0, gamma = 0, c3 = 0, r* = -lam_11, omega = nu, zeta = zeta* = phi (1, -i) / sqrt 2: B(0) = D(0) = 0, so
    H20, H11, H31 and H22 are exactly zero (zero right-hand sides), H30 is below eps (C(q, q, q) vanishes analytically), and l2 -- the E term and the C-H21 terms -- equals the restatement's within the yardstick.  Native against mirror: 8 ulp."""
    codim2, hip = _lib()
    from oracle import operators
    allowed = BR.cgl_bautin_yardstick()["allowed"]
    rstar = BR.first_hopf_r(DIMS, LS)
    pars = dict(PARS, c3=0.0, r=rstar)
    op = operators.CGL2d(DIMS, LS)
    z = BR._hopf_mode(DIMS)
    n = 2 * op.n
    ref = BR.bautin_normal_form(R.cgl_model(op, pars, "r"), NF.cgl_d3F, BR.cgl_d4F, BR.cgl_d5F, np.zeros(n), dict(pars), pars["nu"],
                                z, z)
    out = {}
    for kind in ("native", "mirror"):
        ctx = hip.Context(0)
        prob = hip.CGL2d(ctx, DIMS, LS, **pars)
        ls = _solver(hip, prob, rstar)
        X = codim2.HopfVec(prob.vec(np.zeros(n)), [rstar, pars["nu"]])
        Z = _pair(prob, z.real, z.imag)
        hp = codim2.hopf_normal_form_native(prob, X, Z, Z, ls)
        f = codim2.bautin_normal_form_native if kind == "native" else codim2.bautin_normal_form
        out[kind] = bt = f(prob, hp, ls, lens2="c3")
        print(f"{kind}: G21 = {bt.nf.G21:.12g}, G32 = {bt.nf.G32:.12g}, l2 = {bt.nf.l2:.12g} (restatement {ref['l2']:.12g}), "
              f"converged {bt.converged}, itlinear {bt.itlinear}, unconverged {bt.unconverged_solves}")
        for v in (*bt.nf.H20, bt.nf.H11, *bt.nf.H31, bt.nf.H22):
            assert np.abs(v.numpy()).max() == 0.0, kind
        assert np.abs(_num(bt.nf.H30)).max() <= EPS, kind
        probe(f"bautin.trivial_l2.{kind}", abs(bt.nf.l2 - ref["l2"]), allowed["l2"], relative=abs(bt.nf.l2 - ref["l2"]) / abs(ref["l2"]))
        assert bt.type == "Supercritical" and bt.lens == ("r", "c3") and bt.params == _pv(pars) and bt.nf.omega == pars["nu"]
        assert bt.nf.G21 == 2 * np.conj(hp.nf.b)
    _compare_native_and_mirror(out["native"], out["mirror"])


# ------------------------------------------------------------------------------------------ 4: off the trivial state
def _device_hopf_record(codim2, hip, prob, ls, y):
    loc = y["loc"]
    X = codim2.HopfVec(prob.vec(loc["u"]), [loc["p1"], loc["omega"]])
    z, zs = y["zeta"], y["zeta_star"]
    return codim2.hopf_normal_form_native(prob, X, _pair(prob, z.real, z.imag), _pair(prob, zs.real, zs.imag), ls)


def test_bautin_normal_form_at_the_bautin_point_native_mirror_and_restatement():
    """gamma = 0.1, 41 x 21: the restatement's Bautin point of the Hopf curve in (r, c3) (c3 = -0.1024, r = 1.1455, omega = 0.99716)
    handed over as the state, zeta, zeta* from its null vectors; all six H vectors are alive there, so every term of G32 acts.
    G21, G32, l2 and H30, H21, H31, H22 of native and mirror against the dense restatement within the yardstick's ``allowed``
    (10 x the restatement's own spread between direct solves and left-preconditioned SciPy GMRES at the device's reltol; for the
    three coefficients also the rounding of their own sums).  Native against mirror: equal GMRES counts, results to 8 ulp.  The
    bordered solve runs on the singular J - i omega: whether it reports convergence is recorded, not required; the counter of
    unconverged solves agrees with the flag."""
    codim2, hip = _lib()
    y = BR.cgl_bautin_yardstick()
    lu, allowed, loc = y["lu"], y["allowed"], y["loc"]
    pars = dict(y["par"])
    out = {}
    for kind in ("native", "mirror"):
        ctx = hip.Context(0)
        prob = hip.CGL2d(ctx, DIMS, LS, **pars)
        ls = _solver(hip, prob, loc["p1"], reltol=BR.RELTOL)
        hp = _device_hopf_record(codim2, hip, prob, ls, y)
        assert hp.converged, hp.itlinear
        f = codim2.bautin_normal_form_native if kind == "native" else codim2.bautin_normal_form
        out[kind] = bt = f(prob, hp, ls, lens2="c3")
        print(f"{kind}: G21 = {bt.nf.G21:.12g}, G32 = {bt.nf.G32:.12g}, l2 = {bt.nf.l2:.12g} (restatement {lu['l2']:.12g}), type "
              f"{bt.type}, converged {bt.converged}, itlinear {bt.itlinear}, unconverged {bt.unconverged_solves}")
        assert bt.type == lu["type"] == "Supercritical"
        assert len(bt.itlinear) == 4 and all(i >= 1 for i in bt.itlinear), bt.itlinear
        for k in ("G21", "G32", "l2"):
            d = abs(complex(getattr(bt.nf, k)) - lu[k])
            probe(f"bautin.point_{k}.{kind}", d, allowed[k], relative=d / abs(lu[k]))
        for k in HVECS:
            v = getattr(bt.nf, k)
            d = np.abs((_num(v) if isinstance(v, tuple) else v.numpy()) - lu[k]).max()
            probe(f"bautin.point_{k}.{kind}", d, allowed[k], relative=d / np.abs(lu[k]).max())
    na, mi = out["native"], out["mirror"]
    assert na.converged == (na.unconverged_solves == 0), (na.converged, na.unconverged_solves)
    assert mi.unconverged_solves is None
    _compare_native_and_mirror(na, mi)


# ------------------------------------------------------------------------------------------ 5: end to end
def _curve(codim2, hip, Cn, detect, tol):
    op, pars, s = BR.cgl_curve_start()
    ctx = hip.Context(0)
    prob = hip.CGL2d(ctx, DIMS, LS, **dict(pars, r=s["p"]))
    ls = _solver(hip, prob, s["p"], reltol=BR.RELTOL)
    a, b = s["w"] / np.linalg.norm(s["w"]), s["v"] / np.linalg.norm(s["v"])
    cp = Cn.ContinuationPar(ds=0.05, dsmin=1e-4, dsmax=0.05, p_min=-1.0, p_max=1.0, max_steps=3, n_inversion=8,
                            max_bisection_steps=4, dsmin_bisection=1e-6, newton_options=Cn.NewtonPar(tol=tol, max_iterations=12))
    br = codim2.continuation_hopf(prob, codim2.HopfVec(prob.vec(s["u"]), [s["p"], s["omega"]]), pars["c3"], "c3",
                                  _pair(prob, a.real, a.imag), _pair(prob, b.real, b.imag), ls, cp, detect_codim2=detect)
    return prob, ls, br


def test_hopf_curve_locates_the_bautin_point_and_gives_its_normal_form():
    """continuation_hopf in (r, c3) at gamma = 0.1 from c3 = -0.2 towards 0, three steps of ds = 0.05, detect_codim2 = 2 with
    max_bisection_steps = 4: exactly one "gh" point; every bisection step halves the arclength step, so the bracket's final width is W / 2^4
    of the crossing step's W up to the variation of dp2/ds along that step, which the three recorded steps of equal ds bound (their
    p2 increments differ by less than 1e-3 relative, asserted); 5 % is allowed, where one halving more or fewer is 50 % or 100 %; the restatement's root lies inside the
    bracket widened by (allowed G21 / 2 + Newton tolerance) / |d Re b / d c3| (GH = Re G21 / 2; a point converged to tol is that
    close to the curve); get_normal_form on it gives the restatement's l2 at the located c3 within allowed l2 plus 10 x what the
    restatement's own l2 moves per unit of Hopf residual times the Newton tolerance.  The same curve with detect_codim2 = 0
    records bit-identical p1, p2, omega."""
    codim2, hip = _lib()
    from bk_amd import continuation as Cn
    tol = 1e-11
    y = BR.cgl_bautin_yardstick()
    loc, allowed = y["loc"], y["allowed"]
    prob, ls, br = _curve(codim2, hip, Cn, 2, tol)
    print("curve", list(zip(br.p2, br.GH)), "restatement", loc["curve"], "special points",
          [{k: v for k, v in sp.items() if k not in ("x", "a", "b")} for sp in br.specialpoint])
    assert len(br.p2) == 4 and len(br.GH) == len(br.l1) == 4
    gh = [sp for sp in br.specialpoint if sp["type"] == "gh"]
    assert len(gh) == 1 and len(br.specialpoint) == 1, br.specialpoint
    sp = gh[0]
    i = sp["idx"]
    assert br.GH[i - 1] * br.GH[i] < 0 and sp["status"] == "max_bisection_steps" and sp["bisection_steps"] == 4, sp
    W = abs(br.p2[i] - br.p2[i - 1])
    lo, hi = sp["interval"]
    incs = np.abs(np.diff(br.p2))
    assert all(abs(d - 0.05) <= 1e-12 for d in br.ds[1:]) and len(incs) == 3 and float(incs.max() / incs.min() - 1) <= 1e-3, (br.ds, incs)
    probe("bautin.bracket_shrink", abs((hi - lo) / (W / 2 ** sp["bisection_steps"]) - 1), 0.05)
    assert min(br.p2[i - 1], br.p2[i]) <= lo < hi <= max(br.p2[i - 1], br.p2[i]) and lo <= sp["p2"] <= hi
    (c0, g0), (c1, g1) = loc["curve"][i - 1], loc["curve"][i]
    slope = abs((g1 - g0) / (c1 - c0))
    widen = (allowed["G21"] / 2 + tol) / slope
    assert lo - widen <= loc["p2"] <= hi + widen, (lo, loc["p2"], hi, widen)
    assert len(loc["curve"]) == i + 1                      # the restatement's curve ends with the point after the crossing
    for k in range(i + 1):
        assert abs(br.p2[k] - loc["curve"][k][0]) <= 1e-8 and abs(br.GH[k] - loc["curve"][k][1]) <= 1e-8 * max(1.0, abs(br.GH[k]))
    # the normal form at the located c3 against the restatement refined at the same c3
    bt = codim2.get_normal_form(br, 0, prob, ls, tol=tol, max_iterations=15)
    m = y["model"]
    a, b = loc["w"] / np.linalg.norm(loc["w"]), loc["v"] / np.linalg.norm(loc["v"])
    l2 = {}
    for name, t in (("fine", 1e-12), ("coarse", 1e-5)):
        s = R.newton_hopf(m, loc["u"], loc["p1"], loc["omega"], a, b, p2=sp["p2"], tol=t, max_iterations=20)
        zz, zs = NF.normalise(s["v"], s["w"])
        l2[name] = (BR.bautin_normal_form(m, NF.cgl_d3F, BR.cgl_d4F, BR.cgl_d5F, s["u"], m.at(s["p"], sp["p2"]), s["omega"], zz, zs)["l2"],
                    s["residuals"][-1] if name == "coarse" else 0.0, s)
    per_residual = abs(l2["coarse"][0] - l2["fine"][0]) / max(l2["coarse"][1], 1e-300)
    bound = allowed["l2"] + 10 * per_residual * tol
    print(f"gh: c3 = {sp['p2']:.12g} in [{lo:.12g}, {hi:.12g}] (restatement root {loc['p2']:.12g}), l2 = {bt.nf.l2:.12g} "
          f"(restatement {l2['fine'][0]:.12g}), bound {bound:.3e}, itlinear {bt.itlinear}, converged {bt.converged}")
    probe("bautin.end_to_end_l2", abs(bt.nf.l2 - l2["fine"][0]), bound, relative=abs(bt.nf.l2 - l2["fine"][0]) / abs(l2["fine"][0]))
    assert isinstance(bt, codim2.Bautin) and bt.type == "Supercritical" and bt.lens == ("r", "c3")
    assert bt.params[3] == sp["p2"] and abs(bt.params[0] - l2["fine"][2]["p"]) <= 1e-8
    assert prob.params["c3"] == BR.cgl_curve_start()[1]["c3"]               # the problem's own parameters are untouched
    # detection off: the same points, bit for bit
    _, _, br0 = _curve(codim2, hip, Cn, 0, tol)
    assert br0.l1 == [] and br0.GH == [] and br0.specialpoint == []
    assert br0.p1 == br.p1 and br0.p2 == br.p2 and br0.omega == br.omega, (br0.p2, br.p2)
    _, _, br1 = _curve(codim2, hip, Cn, 1, tol)
    assert br1.p2 == br.p2 and len(br1.specialpoint) == 1 and br1.specialpoint[0]["bisection_steps"] == 0
    assert br1.specialpoint[0]["interval"] == tuple(sorted((br.p2[i - 1], br.p2[i])))


# ------------------------------------------------------------------------------------------ 6: errors
def test_bautin_errors():
    """Any Swift-Hohenberg problem: the error of the Hopf formulation, from the passes and from the library call.  Five
    parameters instead of six: the parameter-count error.  <zeta, zeta*> = 0.5: the normalisation error (native and mirror).  An
    output that is one of the inputs: the aliasing error."""
    codim2, hip = _lib()
    from bk_amd import _lib as L
    ctx = hip.Context(0)
    sh = hip.SwiftHohenberg(ctx, (8, 8), (1.0, 1.0))
    x = sh.vec(np.zeros(sh.nglobal))
    ls0 = hip.GMRESIterativeSolvers(reltol=1e-8, restart=10, maxiter=10, Pl=None)
    xx = (x, x)
    hp0 = codim2.Hopf(x0=x, p=0.1, omega=1.0, zeta=xx, zeta_star=xx, nf=codim2.HopfNormalForm(0j, 1e-3 + 0j, x, x, xx),
                      params=sh._pvec(0.1), lens="l")
    with pytest.raises(L.BkHipError, match="Hopf formulation"):
        codim2.bautin_rhs3(sh, x, sh._pvec(0.1), xx, xx, x, 1 + 0j)
    with pytest.raises(L.BkHipError, match="Hopf formulation"):
        codim2.bautin_rhs4(sh, x, sh._pvec(0.1), xx, xx, x, xx, xx, 1 + 0j)
    with pytest.raises(L.BkHipError, match="Hopf formulation"):
        codim2.bautin_contract(sh, x, sh._pvec(0.1), xx, xx, xx, x, xx, xx, xx, x)
    with pytest.raises(L.BkHipError, match="Hopf formulation"):
        codim2.bautin_normal_form_native(sh, hp0, ls0)
    pars = dict(PARS)
    prob = hip.CGL2d(ctx, (8, 6), LS, **pars)
    rng = np.random.default_rng(2)
    n = prob.nlocal
    V = lambda: prob.vec(rng.standard_normal(n))
    u, q, p0 = V(), (V(), V()), (V(), V())
    with pytest.raises(L.BkHipError, match="takes params"):
        codim2.bautin_rhs3(prob, u, _pv(pars)[:5], q, p0, u, 1 + 0j)
    with pytest.raises(L.BkHipError, match="takes params"):
        codim2.bautin_contract(prob, u, _pv(pars)[:5], q, p0, q, u, q, q, q, u)
    hp = codim2.Hopf(x0=u, p=0.5, omega=1.0, zeta=q, zeta_star=p0, nf=codim2.HopfNormalForm(0j, 1e-3 + 0j, V(), V(), (V(), V())),
                     params=_pv(pars), lens="r")
    ls = _solver(hip, prob, 0.5)
    with pytest.raises(L.BkHipError, match="normalization"):
        codim2.bautin_normal_form_native(prob, hp, ls)
    with pytest.raises(ValueError, match="normalization"):
        codim2.bautin_normal_form(prob, hp, ls)
    hp.params = _pv(pars)[:5]
    with pytest.raises(L.BkHipError, match="takes params"):
        codim2.bautin_normal_form_native(prob, hp, ls)
    with pytest.raises(L.BkHipError, match="aliases an input"):
        import ctypes as C
        P = lambda v: v.t.data_ptr()
        g = (C.c_double * 2)(1.0, 0.0)
        pv = (C.c_double * 6)(*_pv(pars))
        ctx.check(ctx.lib.bk_bautin_rhs3(prob.h, P(u), pv, 6, P(q[0]), P(q[1]), P(p0[0]), P(p0[1]), P(u), g, P(q[0]), P(p0[0]),
                                         P(hp.nf.Psi001), P(hp.nf.Psi110)), "bk_bautin_rhs3")
    ctx.close()
