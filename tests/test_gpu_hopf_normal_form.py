"""GPU tests of the Hopf normal form and the periodic-orbit predictor of cGL (bk_hopf_d3f, bk_hopf_nf_rhs, bk_hopf_nf_contract,
bk_hopf_normal_form, bk_hopf_orbit; bk_amd.codim2): the pointwise kernels against NumPy in extended precision, the fused
contraction against an exact sum, the orbit kernel against NumPy, and the normal form -- native, call-by-call mirror and the dense
CPU restatement (tests/normal_form_ref.py) -- at a Hopf point known in closed form and at one off the trivial state.

Closed form: on the trivial state u = 0 (gamma = 0) at r* = -lam_11, omega = +nu, with zeta = zeta* = phi (1, -i) / sqrt 2, phi the
unit-norm first sine mode, d2F(0) = 0, so every Psi vanishes and only the d3F term survives:
a = 1, b = 2 (-c3 + i mu) 9 / (4 (Nx + 1)(Ny + 1))."""
import ctypes as C
import math

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import minaug_hopf_ref as R
import normal_form_ref as NF
from conftest import probe
from test_gpu_hopf import DIMS, LS, PARS, _dirichlet_lap, _hopf_mode, _nontrivial_hopf_point, _pair, _solver, _vec_at

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
LD = np.longdouble


def _lib():
    from bk_amd import codim2, hip
    return codim2, hip


def _pv(pars):
    return [pars[k] for k in R.CGL_PARAMS]


def _model(pars, lens="r"):
    """The pointwise cGL tensors as a HopfModel (no F, no J: hopf_terms needs neither)."""
    return R.HopfModel(None, None, R.cgl_d2F, R.cgl_dFdp, R.cgl_dJvdp, pars, lens)


# ------------------------------------------------------------------------------------------ 1, 2: the pointwise kernels
def test_hopf_d3F_matches_numpy_and_differences_of_the_device_hessian(ctx):
    """bk_hopf_d3f on a ragged grid with gamma != 0 against the formula in extended precision, in units of eps * (sum of the
    moduli of the monomials): a monomial passes through at most 10 roundings of eps / 2 on the device (4 in the coefficient, 2 in
    T . c, 4 in a' M b), so 5 units is the worst case and 16 the bound.  Then against central differences of bk_hopf_d2f in the
    third argument, bounded as test_hopf_d2F_matches_differences_of_the_device_jacobian without the Laplacian term (d2F is
    pointwise): the rounding of the two Hessian evaluations over eps, and the O(eps^2) of the quintic term."""
    codim2, hip = _lib()
    rng = np.random.default_rng(21)
    pars = dict(PARS, r=0.3, gamma=0.2)
    prob = hip.CGL2d(ctx, (23, 17), LS, **pars)
    pv, n = _pv(pars), prob.nlocal
    u, a, b, c = 0.5 * rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
    U, A, B, Cv = (prob.vec(x) for x in (u, a, b, c))
    got = codim2.hopf_d3F(prob, U, pv, A, B, Cv).numpy()
    ref = NF.cgl_d3F(u.astype(LD), pars, a.astype(LD), b.astype(LD), c.astype(LD))
    scale = NF.cgl_d3F_abs(u, pars, a, b, c)
    probe("hopf_nf.d3F_ulps", float((np.abs(got - ref) / (EPS * scale)).max()), 16.0, tight=1.0)
    eps = 1e-4
    Hp = codim2.hopf_d2F(prob, prob.vec(u + eps * c), pv, A, B).numpy()
    Hm = codim2.hopf_d2F(prob, prob.vec(u - eps * c), pv, A, B).numpy()
    fd = (Hp - Hm) / (2 * eps)
    bound = 8 * EPS * NF.cgl_d2F_abs(u, pars, a, b).max() / eps + 1e-6 * np.abs(got).max()
    probe("hopf_nf.d3F_vs_d2F_fd", np.abs(fd - got).max(), bound)


def test_hopf_nf_rhs_matches_the_restatement(ctx):
    """bk_hopf_nf_rhs against R.cgl_d2F with complex arguments in extended precision, in units of eps * (sum of the moduli of the
    monomials): at most 13 roundings per monomial on the device (8 in a quintic Hessian coefficient, 2 in H x, 2 in x' H x, 1 in
    the final sum), 6.5 units; bound 16.  Aligned, misaligned and odd-point-count layouts."""
    codim2, hip = _lib()
    pars = dict(PARS, r=0.3, gamma=0.2)
    for dims, offset in (((24, 16), 0), ((24, 16), 1), ((23, 17), 0)):
        rng = np.random.default_rng(31 + offset + dims[0])
        prob = hip.CGL2d(ctx, dims, LS, **pars)
        n = prob.nlocal
        u, zr, zi = 0.6 * rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
        dev = lambda x: _vec_at(ctx, hip, x, offset)
        (r20r, r20i), r11 = codim2.hopf_nf_rhs(prob, dev(u), _pv(pars), (dev(zr), dev(zi)))
        z = zr.astype(LD) + 1j * zi.astype(LD)
        ref20 = 0.5 * R.cgl_d2F(u.astype(LD), pars, z, z)
        ref11 = R.cgl_d2F(u.astype(LD), pars, z, np.conj(z))
        zabs = np.abs(zr) + np.abs(zi)
        unit = EPS * NF.cgl_d2F_abs(u, pars, zabs, zabs)
        tag = f"{dims[0]}x{dims[1]}+{offset}"
        probe(f"hopf_nf.rhs_r20_re_ulps.{tag}", float((np.abs(r20r.numpy() - ref20.real) / unit).max()), 16.0, tight=2.0)
        probe(f"hopf_nf.rhs_r20_im_ulps.{tag}", float((np.abs(r20i.numpy() - ref20.imag) / unit).max()), 16.0, tight=2.0)
        probe(f"hopf_nf.rhs_r11_ulps.{tag}", float((np.abs(r11.numpy() - ref11.real) / unit).max()), 16.0, tight=2.0)
        assert float(np.abs(ref11.imag).max()) <= 1e-17 * float(np.abs(ref11.real).max())


# ------------------------------------------------------------------------------------------ 3: the fused contraction
def _contract_terms(u, pars, lens, z, zs, P001, P110, P200):
    """Per element of the stacked fields the terms whose sums are a and b: conj(av) zeta*, conj(bv) zeta*."""
    av, bv = NF.hopf_terms(_model(pars, lens), NF.cgl_d3F, u, pars, lens, z, zs, P001, P110, P200)
    return np.conj(av) * zs, np.conj(bv) * zs


def _check_contract(name, n, got, terms):
    for part in ("real", "imag"):
        t = getattr(terms, part)
        bound = 4 * n * EPS * np.abs(t).sum() + 1e-300
        probe(f"hopf_nf.contract_{name}_{part}", abs(getattr(got, part) - math.fsum(t)) / bound, 1.0)


def _random_contract_inputs(rng, n):
    return [rng.standard_normal(n) for _ in range(9)]


@pytest.mark.parametrize("Nx", [2, 3, 127, 128, 4099, 65537])
@pytest.mark.parametrize("offset", [0, 1])
def test_hopf_nf_contract_matches_an_exact_sum(ctx, Nx, offset):
    """a and b within the summation-rounding bound of the fp64 sum, 4 n eps sum |terms| per component, against math.fsum of the
    restatement's per-point terms on random u, zeta, zeta*, Psi: the grid / alignment matrix of
    test_hopf_contract_matches_an_exact_sum (Ny = 2 for even Nx, 3 for odd Nx: an odd point count misaligns the second field),
    every parameter index."""
    codim2, hip = _lib()
    rng = np.random.default_rng(100 + Nx + offset)
    Ny = 2 if Nx % 2 == 0 else 3
    N = Nx * Ny
    prob = hip.CGL2d(ctx, (Nx, Ny), (1.0, 1.0), **PARS)
    pars, n = dict(PARS), 2 * N
    u, zr, zi, sr, si, p, q, gr, gi = _random_contract_inputs(rng, n)
    dev = lambda x: _vec_at(ctx, hip, x, offset)
    U, Z, ZS, P, Q, G = dev(u), (dev(zr), dev(zi)), (dev(sr), dev(si)), dev(p), dev(q), (dev(gr), dev(gi))
    for ip, name in enumerate(R.CGL_PARAMS):
        a, b = codim2.hopf_nf_contract(prob, U, _pv(pars), ip, Z, ZS, P, Q, G)
        ta, tb = _contract_terms(u, pars, name, zr + 1j * zi, sr + 1j * si, p, q, gr + 1j * gi)
        _check_contract(f"a.{name}.N{N}+{offset}", n, a, ta)
        _check_contract(f"b.{name}.N{N}+{offset}", n, b, tb)


def test_hopf_nf_contract_non_temporal_path_at_2048_squared(ctx):
    """n = 2 * 2048^2 = 2^23 >= 2^22 selects the non-temporal 16-B instantiation: exact sums as for the small lengths."""
    codim2, hip = _lib()
    prob = hip.CGL2d(ctx, (2048, 2048), (1.0, 1.0), **PARS)
    n = prob.nlocal
    assert n >= 1 << 22
    rng = np.random.default_rng(12)
    pars = dict(PARS)
    u, zr, zi, sr, si, p, q, gr, gi = _random_contract_inputs(rng, n)
    V = prob.vec
    a, b = codim2.hopf_nf_contract(prob, V(u), _pv(pars), 1, (V(zr), V(zi)), (V(sr), V(si)), V(p), V(q), (V(gr), V(gi)))
    ta, tb = _contract_terms(u, pars, "mu", zr + 1j * zi, sr + 1j * si, p, q, gr + 1j * gi)
    _check_contract("nt_a", n, a, ta)
    _check_contract("nt_b", n, b, tb)


# ------------------------------------------------------------------------------------------ 4: the orbit kernel
def _orbit_terms(x0, zr, zi, p, q, gr, gi, ds, amp, t):
    """The seven terms of orbit(t) (NormalForms.jl:1262-1271) in extended precision."""
    x0, zr, zi, p, q, gr, gi = (v.astype(LD) for v in (x0, zr, zi, p, q, gr, gi))
    amp, t, ds = LD(amp), LD(t), LD(ds)
    ar, ai, a2 = amp * np.cos(t), amp * np.sin(t), amp * amp
    return [x0, 2 * ar * zr, -2 * ai * zi, ds * p, a2 * q, 2 * a2 * np.cos(2 * t) * gr, -2 * a2 * np.sin(2 * t) * gi]


def _check_orbit(name, got, terms):
    ref = sum(terms)
    unit = EPS * sum(np.abs(t) for t in terms)
    probe(name, float((np.abs(got.astype(LD) - ref) / unit).max()), 8.0, tight=4.0)


@pytest.mark.parametrize("n, offset", [(1000, 0), (1001, 0), (1000, 1), (1 << 22, 0)])
@pytest.mark.parametrize("M", [1, 3, 8, 11])
def test_hopf_orbit_matches_numpy(ctx, n, offset, M):
    """bk_hopf_orbit against the seven terms summed in extended precision, bound 8 eps sum |terms| per element: the coefficients
    2 amp cos t, ..., 2 amp^2 sin 2t carry at most 2 eps (one libm call, two products), their products with the vectors eps / 2,
    and the six additions 3 eps in all.  16-B, scalar (odd length, misaligned) and non-temporal paths; M = 11 takes two passes."""
    codim2, hip = _lib()
    rng = np.random.default_rng(n % 1000 + offset + M)
    x0, zr, zi, p, q, gr, gi = (rng.standard_normal(n) for _ in range(7))
    dev = lambda x: _vec_at(ctx, hip, x, offset)
    ds, amp = -0.037, 0.61
    ts = [0.3 + 2 * math.pi * m / M for m in range(M)]
    outs = codim2.hopf_orbit(dev(x0), (dev(zr), dev(zi)), dev(p), dev(q), (dev(gr), dev(gi)), ds, amp, ts)
    assert len(outs) == M
    for m, (o, t) in enumerate(zip(outs, ts)):
        _check_orbit(f"hopf_nf.orbit.n{n}+{offset}.M{M}.{m}", o.numpy(), _orbit_terms(x0, zr, zi, p, q, gr, gi, ds, amp, t))


# ------------------------------------------------------------------------------------------ 5: the closed form
@pytest.mark.parametrize("c3", [0.8, PARS["c3"]])
def test_normal_form_native_and_mirror_give_the_closed_form_on_the_trivial_state(ctx, c3):
    """41 x 21 (the example's grid), u = 0, gamma = 0, r* = -lam_11, omega = nu: |a - 1| and |b - b_closed| within the summation
    bound of the contraction pass evaluated on the actual terms; supercritical for c3 > 0, subcritical for the repository's
    c3 = -1.  All three right-hand sides are exactly zero: the solves converge at once and the Psi are exactly zero."""
    codim2, hip = _lib()
    pars = dict(PARS, c3=c3)
    rstar, nu = -_dirichlet_lap(DIMS, LS)[0], pars["nu"]
    pars["r"] = rstar
    prob = hip.CGL2d(ctx, DIMS, LS, **pars)
    n = prob.nlocal
    ls = _solver(hip, prob, rstar)
    zr, zi = _hopf_mode(DIMS)
    z = zr + 1j * zi
    X = codim2.HopfVec(prob.vec(np.zeros(n)), [rstar, nu])
    a0, b0 = NF.cgl_closed_form(DIMS, pars["mu"], c3)
    zero = np.zeros(n)
    ta, tb = _contract_terms(zero, pars, "r", z, z, zero, zero, zero + 0j)
    bound_a = 4 * n * EPS * (np.abs(ta.real).sum() + np.abs(ta.imag).sum())
    bound_b = 4 * n * EPS * (np.abs(tb.real).sum() + np.abs(tb.imag).sum())
    its = []
    for kind, f in (("native", codim2.hopf_normal_form_native), ("mirror", codim2.hopf_normal_form)):
        Z = _pair(prob, zr, zi)
        hp = f(prob, X, Z, Z, ls)
        probe(f"hopf_nf.closed_form_a.{kind}.c3={c3}", abs(hp.nf.a - a0), bound_a)
        probe(f"hopf_nf.closed_form_b.{kind}.c3={c3}", abs(hp.nf.b - b0), bound_b, relative=abs(hp.nf.b - b0) / abs(b0))
        assert hp.type == ("SuperCritical" if c3 > 0 else "SubCritical"), (kind, hp.nf.b)
        assert hp.converged, (kind, hp.itlinear)
        its.append(hp.itlinear)
        assert kind == "mirror" or hp.unconverged_solves == 0
        for v in (hp.nf.Psi001, hp.nf.Psi110, *hp.nf.Psi200):
            assert np.abs(v.numpy()).max() == 0.0, kind
        assert hp.p == rstar and hp.omega == nu and hp.lens == "r" and hp.params == _pv(pars)
    assert its[0] == its[1], its
    # omega = -nu with the conjugate eigenvectors: the conjugate coefficients
    Zc = _pair(prob, zr, -zi)
    hc = codim2.hopf_normal_form_native(prob, codim2.HopfVec(X.u, [rstar, -nu]), Zc, Zc, ls)
    probe(f"hopf_nf.closed_form_b.conjugate.c3={c3}", abs(hc.nf.b - np.conj(b0)), bound_b)
    probe(f"hopf_nf.closed_form_a.conjugate.c3={c3}", abs(hc.nf.a - np.conj(a0)), bound_a)


# ------------------------------------------------------------------------------------------ 6: off the trivial state
def _gmres_solver(reltol):
    """solver(A, rhs) for NF.hopf_normal_form: SciPy's GMRES at ``reltol`` as it comes (restart 20, no preconditioner)."""
    def solve(A, rhs):
        x, info = spla.gmres(A, rhs, rtol=reltol, atol=0.0)
        assert info == 0, info
        return x
    return solve


def test_normal_form_off_the_trivial_state_native_mirror_and_restatement():
    """The Hopf point of _nontrivial_hopf_point (gamma = 0.1, 41 x 21, u != 0), where every term of a and b is alive; zeta, zeta*
    from its null vectors.  Native and mirror run the same solves on fresh contexts: a, b to 1e-12 relative, equal GMRES counts.
    Against the dense restatement the deviation is set by the GMRES tolerance times the conditioning of J and 2 i omega - J.  The
    bound comes from the restatement itself: its three systems solved by SciPy GMRES (default restart) at the device's reltol
    (1e-13) instead of LU change a, b and the Psi by some amount; 10 x that amount is allowed (the device solves run on the real-equivalent 2n system
    with another preconditioner).  Every value is logged next to its bound by ``probe``; the measured margins are in DESIGN section 9d."""
    codim2, hip = _lib()
    reltol = 1e-13
    op, s = _nontrivial_hopf_point()
    pars = dict(PARS, gamma=0.1, r=s["p"])
    model = R.cgl_model(op, pars, "r")
    z, zs = NF.normalise(s["v"], s["w"])
    lu = NF.hopf_normal_form(model, NF.cgl_d3F, s["u"], dict(pars), "r", s["omega"], z, zs)
    gm = NF.hopf_normal_form(model, NF.cgl_d3F, s["u"], dict(pars), "r", s["omega"], z, zs, solver=_gmres_solver(reltol))
    assert all(np.abs(lu[k]).max() > 1e-6 for k in ("Psi001", "Psi110", "Psi200")) and abs(lu["a"]) > 1e-3 and abs(lu["b"]) > 1e-3
    allowed = {k: 10 * abs(gm[k] - lu[k]) for k in ("a", "b")}
    allowed.update({k: 10 * np.abs(gm[k] - lu[k]).max() for k in ("Psi001", "Psi110", "Psi200")})
    print(f"restatement: a = {lu['a']:.12g}, b = {lu['b']:.12g}, type {lu['type']}; allowed deviations {allowed}")
    out = {}
    for kind in ("native", "mirror"):
        ctx = hip.Context(0)
        prob = hip.CGL2d(ctx, DIMS, LS, **pars)
        ls = _solver(hip, prob, s["p"], reltol=reltol)
        X = codim2.HopfVec(prob.vec(s["u"]), [s["p"], s["omega"]])
        Z, ZS = _pair(prob, z.real, z.imag), _pair(prob, zs.real, zs.imag)
        f = codim2.hopf_normal_form_native if kind == "native" else codim2.hopf_normal_form
        out[kind] = hp = f(prob, X, Z, ZS, ls)
        print(f"{kind}: a = {hp.nf.a:.12g}, b = {hp.nf.b:.12g}, type {hp.type}, converged {hp.converged}, itlinear {hp.itlinear}")
        assert hp.converged and hp.type == lu["type"], (kind, hp.itlinear)
        probe(f"hopf_nf.nontrivial_a.{kind}", abs(hp.nf.a - lu["a"]), allowed["a"], relative=abs(hp.nf.a - lu["a"]) / abs(lu["a"]))
        probe(f"hopf_nf.nontrivial_b.{kind}", abs(hp.nf.b - lu["b"]), allowed["b"], relative=abs(hp.nf.b - lu["b"]) / abs(lu["b"]))
        P200 = hp.nf.Psi200[0].numpy() + 1j * hp.nf.Psi200[1].numpy()
        for name, got in (("Psi001", hp.nf.Psi001.numpy()), ("Psi110", hp.nf.Psi110.numpy()), ("Psi200", P200)):
            probe(f"hopf_nf.nontrivial_{name}.{kind}", np.abs(got - lu[name]).max(), allowed[name],
                  relative=np.abs(got - lu[name]).max() / np.abs(lu[name]).max())
    na, mi = out["native"], out["mirror"]
    assert na.itlinear == mi.itlinear, (na.itlinear, mi.itlinear)
    assert abs(na.nf.a - mi.nf.a) <= 1e-12 * abs(mi.nf.a) and abs(na.nf.b - mi.nf.b) <= 1e-12 * abs(mi.nf.b), (na.nf, mi.nf)


# ------------------------------------------------------------------------------------------ 7: end to end
def test_bisected_hopf_point_to_normal_form_and_predictor_end_to_end(ctx):
    """The branch of test_bisected_hopf_point_refines_end_to_end -> get_normal_form -> the closed-form a, b (the point is refined,
    so the closed form applies) -> predictor.  Bound, relative: 40 (tol_newton + reltol_gmres) / gap with gap the distance from
    i nu to the nearest other eigenvalue of J(r*), the test's ``width`` -- first-order eigenvector perturbation, b cubic in
    (zeta, conj zeta, zeta*), and a factor 10."""
    codim2, hip = _lib()
    from bk_amd import continuation as Cn
    lap = _dirichlet_lap(DIMS, LS)
    rstar = -lap[:2]
    width = float(rstar[1] - rstar[0])
    tol_newton, reltol = 1e-10, 1e-10
    prob = hip.CGL2d(ctx, DIMS, LS, r=0.5)
    n = prob.nlocal
    ls = _solver(hip, prob, float(rstar[0]), reltol=reltol)
    lse = _solver(hip, prob, float(rstar[0]) - 1.0, reltol=reltol)
    eig = hip.ShiftInvert(1.0, lse, tol=1e-8, maxiter=300, hermitian=False, save_vectors=False)
    nopt = Cn.NewtonPar(tol=tol_newton, max_iterations=20, linsolver=ls, eigsolver=eig)
    cp = Cn.ContinuationPar(ds=0.5 * width, dsmin=1e-3 * width, dsmax=0.6 * width, p_min=float(rstar[0] - 2 * width),
                            p_max=float(rstar[1]), max_steps=3, nev=6, newton_options=nopt, n_inversion=2,
                            max_bisection_steps=4, dsmin_bisection=1e-4 * width)
    alg = Cn.PALC(tangent="secant", theta=0.5, bls=hip.BorderingBLS(None, check_precision=False))
    br = Cn.continuation_native(prob, prob.vec(np.zeros(n)), float(rstar[0] - 0.7 * width), alg, cp, normC=Cn.norminf,
                                bisection=True, save_sol=True)
    ih = [i for i, sp in enumerate(br.specialpoint) if sp.get("type") == "hopf"]
    assert ih, br.specialpoint
    hp = codim2.get_normal_form(br, ih[0], prob, ls, tol=tol_newton, max_iterations=15)
    a0, b0 = NF.cgl_closed_form(DIMS, PARS["mu"], PARS["c3"])
    bound = 40 * (tol_newton + reltol) / width
    print(f"end to end: p = {hp.p:.15g} (r* = {rstar[0]:.15g}), omega = {hp.omega:.15g}, a = {hp.nf.a:.15g}, b = {hp.nf.b:.15g} "
          f"(closed form {b0:.15g}), type {hp.type}, itlinear {hp.itlinear}, bound {bound:.3e}")
    assert abs(hp.p - rstar[0]) <= 1e-9 * abs(rstar[0]) and abs(hp.omega - PARS["nu"]) <= 1e-9, (hp.p, hp.omega)
    assert abs(codim2.cinner(hp.zeta, hp.zeta_star) - 1) <= 1e-12 and abs(codim2.cnorm(hp.zeta) - 1) <= 1e-12
    probe("hopf_nf.end_to_end_a", abs(hp.nf.a - a0), bound)
    probe("hopf_nf.end_to_end_b", abs(hp.nf.b - b0) / abs(b0), bound)
    assert hp.type == "SubCritical" and hp.converged
    # predictor: the formulas with the closed-form coefficients; p and omega of the point carry the 1e-9 of the refinement
    ds = 0.01
    rec, ref = codim2.predictor(hp, ds), NF.predictor(float(rstar[0]), PARS["nu"], a0, b0, ds)
    g = abs(a0) + 3 * abs(b0.imag * a0.real / b0.real)                     # sensitivity of Im a - Im b Re a / Re b
    tol_om = 1e-9 + abs(ds) * bound * g
    assert rec["dsfactor"] == ref["dsfactor"] == -1                        # Re a Re b > 0: the orbits live below r*
    assert abs(rec["p"] - ref["p"]) <= 1e-9 * abs(rstar[0]), (rec["p"], ref["p"])
    assert abs(rec["amp"] / ref["amp"] - 1) <= bound, (rec["amp"], ref["amp"])
    assert abs(rec["omega"] - ref["omega"]) <= tol_om, (rec["omega"], ref["omega"])
    assert abs(rec["period"] / ref["period"] - 1) <= 2 * tol_om / abs(ref["omega"]), (rec["period"], ref["period"])
    # the orbit through the fused kernel: one phase and the M equidistant slices against the restatement on the same vectors
    vecs = [v.numpy() for v in (hp.x0, hp.zeta[0], hp.zeta[1], hp.nf.Psi001, hp.nf.Psi110, hp.nf.Psi200[0], hp.nf.Psi200[1])]
    amp = rec["amp"] / 2
    _check_orbit("hopf_nf.end_to_end_orbit_t", rec["orbit"](0.7).numpy(), _orbit_terms(*vecs, ds, amp, 0.7))
    sl = rec["orbit"].slices(5)
    assert len(sl) == 5
    for m, o in enumerate(sl):
        _check_orbit(f"hopf_nf.end_to_end_orbit_slice{m}", o.numpy(), _orbit_terms(*vecs, ds, amp, 2 * math.pi * m / 5))
    with pytest.raises(NotImplementedError, match="newton_fold"):
        codim2.get_normal_form(type("B", (), dict(specialpoint=[dict(type="bp")]))(), 0, prob, ls)


# ------------------------------------------------------------------------------------------ 8: errors and flags
def test_normal_form_errors_and_unconverged_solves():
    """Any Swift-Hohenberg problem: the error of the Hopf formulation.  <zeta, zeta*> = 0.5: the normalisation error (native and
    mirror).  maxiter = 1 at the Hopf point off the trivial state, where all three right-hand sides are non-zero: converged is
    False, no error, and the counter equals the three solves."""
    codim2, hip = _lib()
    from bk_amd import _lib as L
    ctx = hip.Context(0)
    sh = hip.SwiftHohenberg(ctx, (8, 8), (1.0, 1.0))
    x = sh.vec(np.zeros(sh.nglobal))
    ls0 = hip.GMRESIterativeSolvers(reltol=1e-8, restart=10, maxiter=10, Pl=None)
    with pytest.raises(L.BkHipError, match="Hopf formulation"):
        codim2.hopf_d3F(sh, x, sh._pvec(0.1), x, x, x)
    with pytest.raises(L.BkHipError, match="Hopf formulation"):
        codim2.hopf_nf_rhs(sh, x, sh._pvec(0.1), (x, x))
    with pytest.raises(L.BkHipError, match="Hopf formulation"):
        codim2.hopf_nf_contract(sh, x, sh._pvec(0.1), 0, (x, x), (x, x), x, x, (x, x))
    with pytest.raises(L.BkHipError, match="Hopf formulation"):
        codim2.hopf_normal_form_native(sh, codim2.HopfVec(x, [0.1, 1.0]), (x, x), (x, x), ls0)
    op, s = _nontrivial_hopf_point()
    pars = dict(PARS, gamma=0.1, r=s["p"])
    prob = hip.CGL2d(ctx, DIMS, LS, **pars)
    z, zs = NF.normalise(s["v"], s["w"])
    X = codim2.HopfVec(prob.vec(s["u"]), [s["p"], s["omega"]])
    Z, ZS = _pair(prob, z.real, z.imag), _pair(prob, zs.real, zs.imag)
    half = _pair(prob, 0.5 * zs.real, 0.5 * zs.imag)
    ls = _solver(hip, prob, s["p"])
    with pytest.raises(L.BkHipError, match="normalization"):
        codim2.hopf_normal_form_native(prob, X, Z, half, ls)
    with pytest.raises(ValueError, match="normalization"):
        codim2.hopf_normal_form(prob, X, Z, half, ls)
    with pytest.raises(L.BkHipError, match="aliases an input"):                 # an output that is one of the inputs
        t0, outp = (C.c_double * 1)(0.0), (C.c_void_p * 1)(X.u.t.data_ptr())
        ctx.check(ctx.lib.bk_hopf_orbit(ctx.h, X.u.n, X.u.t.data_ptr(), Z[0].t.data_ptr(), Z[1].t.data_ptr(), ZS[0].t.data_ptr(),
                                        ZS[0].t.data_ptr(), ZS[0].t.data_ptr(), ZS[1].t.data_ptr(), 0.1, 0.1, 1, t0, outp),
                  "bk_hopf_orbit")
    ls1 = hip.GMRESIterativeSolvers(reltol=1e-13, restart=2, maxiter=1, Pl=hip.LaplacePreconditioner(prob, 1.0))
    hp = codim2.hopf_normal_form_native(prob, X, Z, ZS, ls1)
    assert hp.converged is False and hp.unconverged_solves == 3, (hp.converged, hp.unconverged_solves, hp.itlinear)
    assert np.isfinite([hp.nf.a.real, hp.nf.a.imag, hp.nf.b.real, hp.nf.b.imag]).all()
    ctx.close()
