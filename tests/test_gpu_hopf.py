"""GPU tests of the minimally augmented Hopf formulation (bk_hopf_d2f, bk_hopf_djdp, bk_hopf_contract, bk_hopf_terms,
bk_hopf_linsolve, bk_newton_hopf; bk_amd.codim2): the Hessian kernels against NumPy, the fused contraction against an exact sum,
d2F against differences of the device Jacobian, and newton_hopf -- native against the call-by-call mirror and the CPU
restatement -- at Hopf points known in closed form: on the trivial state u = 0 (gamma = 0) of cGL the Jacobian is
Lap (x) I + [[r, -nu], [nu, r]], with eigenvalues lam_ij + r +- i nu, so r* = -lam_ij is a Hopf point with omega = nu."""
import math
import time

import numpy as np
import pytest
import torch

import minaug_hopf_ref as R
from conftest import probe
from oracle import operators

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
DIMS, LS = (41, 21), (np.pi, np.pi / 2)            # the grid of examples/cGL2d.jl
PARS = dict(r=0.5, mu=0.1, nu=1.0, c3=-1.0, c5=1.0, gamma=0.0)


def _lib():
    from bk_amd import codim2, hip
    return codim2, hip


def _ulps(a, b):
    return np.abs(a - b) / np.maximum(np.spacing(np.maximum(np.abs(a), np.abs(b))), np.finfo(float).tiny)


def _dirichlet_lap(dims, ls):
    lam = []
    for n, l in zip(dims, ls):
        h = 2 * l / n
        lam.append(-(4 / h ** 2) * np.sin(np.pi * np.arange(1, n + 1) / (2 * (n + 1))) ** 2)
    return np.sort((lam[0][:, None] + lam[1][None, :]).ravel())[::-1]


def _hopf_mode(dims):
    """(re, im) of the eigenvector (phi, -i phi) of J(0) for lam_11 + r + i nu (phi = the first sine mode), unit norm."""
    x = np.sin(np.pi * np.arange(1, dims[0] + 1) / (dims[0] + 1))
    y = np.sin(np.pi * np.arange(1, dims[1] + 1) / (dims[1] + 1))
    phi = np.outer(y, x).reshape(-1)
    phi /= np.linalg.norm(phi) * math.sqrt(2)
    z = np.zeros_like(phi)
    return np.concatenate([phi, z]), np.concatenate([z, -phi])


def _pair(prob, re, im):
    return prob.vec(re), prob.vec(im)


def _solver(hip, prob, r0, maxiter=600, restart=60, reltol=1e-13):
    return hip.GMRESIterativeSolvers(reltol=reltol, restart=restart, maxiter=maxiter,
                                     Pl=hip.CGLBlockPreconditioner(prob, r0, PARS["nu"]))


def test_hopf_d2F_and_dJdp_match_numpy(ctx):
    codim2, hip = _lib()
    rng = np.random.default_rng(1)
    pars = dict(PARS, r=0.3, gamma=0.2)
    prob = hip.CGL2d(ctx, (23, 17), LS, **pars)
    pv = [pars[k] for k in R.CGL_PARAMS]
    n = prob.nlocal
    u, a, b = (rng.standard_normal(n) for _ in range(3))
    U, A, B = prob.vec(u), prob.vec(a), prob.vec(b)
    got = codim2.hopf_d2F(prob, U, pv, A, B).numpy()
    probe("hopf.d2F_ulps", _ulps(got, R.cgl_d2F(u, pars, a, b)).max(), 1.0, tight=0.0)
    for ip, name in enumerate(R.CGL_PARAMS):
        got = codim2.hopf_dJdp(prob, U, pv, ip, A).numpy()
        probe(f"hopf.dJdp_ulps.{name}", _ulps(got, R.cgl_dJvdp(u, pars, name, a)).max(), 1.0, tight=0.0)


def test_hopf_d2F_matches_differences_of_the_device_jacobian(ctx):
    codim2, hip = _lib()
    rng = np.random.default_rng(5)
    prob = hip.CGL2d(ctx, (64, 48), LS, **PARS)
    pv = [PARS[k] for k in R.CGL_PARAMS]
    n = prob.nlocal
    u, a, b = 0.5 * rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
    eps = 1e-4
    Jp = prob.jacobian(prob.vec(u + eps * a), PARS["r"])(prob.vec(b)).numpy()
    Jm = prob.jacobian(prob.vec(u - eps * a), PARS["r"])(prob.vec(b)).numpy()
    fd = (Jp - Jm) / (2 * eps)
    got = codim2.hopf_d2F(prob, prob.vec(u), pv, prob.vec(a), prob.vec(b)).numpy()
    # the Laplacian cancels up to rounding (eps_mach |Lap|_inf |b|_inf / eps); the cubic / quintic terms leave O(eps^2)
    h = 2 * np.pi / 64
    bound = 8 * EPS * (8 / h ** 2) * np.abs(b).max() / eps + 1e-6 * np.abs(got).max()
    probe("hopf.d2F_vs_jacobian_fd", np.abs(fd - got).max(), bound)


def _vec_at(ctx, hip, x, offset):
    """x on the device, starting `offset` doubles into its allocation (offset 1: every 16-B vector load is misaligned)."""
    t = torch.empty(len(x) + offset, dtype=torch.float64, device=ctx.torch_device)
    v = t[offset:]
    v.copy_(torch.from_numpy(np.asarray(x, dtype=np.float64)))
    return hip.HipVec(ctx, v)


@pytest.mark.parametrize("Nx", [2, 3, 127, 128, 4099, 65537])
@pytest.mark.parametrize("offset", [0, 1])
def test_hopf_contract_matches_an_exact_sum(ctx, Nx, offset):
    """S_k = w^H d2F[v, X_k], P = w^H dJ/dp v and Q = w^H v within the summation-rounding bound of the fp64 sum on Nx x Ny grids
    (Ny = 2 for even Nx, 3 for odd Nx: an odd point count misaligns the second field), aligned and misaligned allocations,
    m = 0 .. 3, every parameter."""
    codim2, hip = _lib()
    rng = np.random.default_rng(Nx + offset)
    Ny = 2 if Nx % 2 == 0 else 3
    N = Nx * Ny
    prob = hip.CGL2d(ctx, (Nx, Ny), (1.0, 1.0), **PARS)
    pars = dict(PARS)
    pv = [pars[k] for k in R.CGL_PARAMS]
    n = 2 * N
    u, vr, vi, wr, wi = (rng.standard_normal(n) for _ in range(5))
    Xs = [rng.standard_normal(n) for _ in range(3)]
    dev = lambda x: _vec_at(ctx, hip, x, offset)
    U, V, W, XV = dev(u), (dev(vr), dev(vi)), (dev(wr), dev(wi)), [dev(x) for x in Xs]
    v, w = vr + 1j * vi, wr + 1j * wi

    def check(name, got, terms):
        for part, t in (("re", terms.real), ("im", terms.imag)):
            bound = 4 * n * EPS * np.abs(t).sum() + 1e-300
            val = getattr(got, "real" if part == "re" else "imag")
            probe(f"hopf.contract_{name}_{part}.N{N}", abs(val - math.fsum(t)) / bound, 1.0)

    for ip, name in enumerate(R.CGL_PARAMS):
        tp = np.conj(w) * R.cgl_dJvdp(u, pars, name, v)
        tq = np.conj(w) * v
        for m in range(4):
            S, P, Q = codim2.hopf_contract(prob, U, pv, ip, V, W, XV[:m])
            for k in range(m):
                check(f"S{k}", S[k], np.conj(w) * R.cgl_d2F(u, pars, v, Xs[k]))
            if name == "gamma":
                assert P == 0
            else:
                check("P", P, tp)
            check("Q", Q, tq)


def test_sh_problems_have_no_hopf_formulation(ctx):
    codim2, hip = _lib()
    from bk_amd import _lib as L
    prob = hip.SwiftHohenberg(ctx, (8, 8), (1.0, 1.0))
    x = prob.vec(np.zeros(prob.nglobal))
    with pytest.raises(L.BkHipError, match="Hopf formulation"):
        codim2.hopf_d2F(prob, x, prob._pvec(0.1), x, x)
    with pytest.raises(L.BkHipError, match="Hopf formulation"):
        codim2.hopf_contract(prob, x, prob._pvec(0.1), 0, (x, x), (x, x))
    prob1 = hip.SwiftHohenberg1D(ctx, 64, 6.0)
    x1 = prob1.vec(np.zeros(64))
    with pytest.raises(L.BkHipError, match="Hopf formulation"):
        codim2.hopf_dJdp(prob1, x1, prob1._pvec(0.1), 0, x1)


def _trivial_case(ctx, hip, dims=DIMS, ls=LS):
    lap = _dirichlet_lap(dims, ls)
    rstar = -lap[0]
    prob = hip.CGL2d(ctx, dims, ls, **dict(PARS, r=rstar + 0.02))
    return prob, rstar, lap


def test_newton_hopf_native_mirror_and_restatement_land_on_the_closed_form_hopf_point():
    """41 x 21 (the example's grid), u = 0, gamma = 0: from (r* + 0.02, 0.95 nu) with the reference's default start vectors
    (random a, b, then the bordered vectors).  Native and mirror each run on a fresh context (equal solver states)."""
    codim2, hip = _lib()
    op = operators.CGL2d(DIMS, LS)
    n = 2 * DIMS[0] * DIMS[1]
    lap = _dirichlet_lap(DIMS, LS)
    rstar, nu = -lap[0], PARS["nu"]
    model = R.cgl_model(op, dict(PARS), "r")
    x0 = np.zeros(n)
    a, b = R.start_vectors(model, x0, model.at(rstar + 0.02), 0.95 * nu, seed=3)
    ref = R.newton_hopf(model, x0, rstar + 0.02, 0.95 * nu, a, b, tol=1e-12, max_iterations=15)
    assert ref["converged"], ref["residuals"]
    out = {}
    for kind in ("native", "mirror"):
        ctx = hip.Context(0)
        prob = hip.CGL2d(ctx, DIMS, LS, **dict(PARS, r=rstar + 0.02))
        ls = _solver(hip, prob, rstar + 0.02)
        X0 = codim2.HopfVec(prob.vec(x0), [rstar + 0.02, 0.95 * nu])
        A, B = _pair(prob, a.real, a.imag), _pair(prob, b.real, b.imag)
        f = codim2.newton_hopf_native if kind == "native" else codim2.newton_hopf
        out[kind] = s = f(prob, X0, A, B, ls, tol=1e-12, max_iterations=15)
        assert s["converged"], (kind, s["residuals"])
        assert np.abs(s["u"].u.numpy()).max() == 0.0
        print(f"{kind}: itnewton {s['itnewton']}, GMRES {s['itlineartot']}, unconverged {s['unconverged_solves']}, "
              f"residuals {s['residuals']}")
    for name, (p, om) in (("native", out["native"]["u"].p), ("mirror", out["mirror"]["u"].p), ("ref", (ref["p"], ref["omega"]))):
        probe(f"hopf.closed_form_r.{name}", abs(p - rstar) / abs(rstar), 1e-11)
        probe(f"hopf.closed_form_omega.{name}", abs(om - nu) / nu, 1e-11)
    assert out["native"]["itnewton"] == out["mirror"]["itnewton"]
    assert out["native"]["unconverged_solves"] == out["mirror"]["unconverged_solves"]
    assert np.abs(out["native"]["u"].p - out["mirror"]["u"].p).max() <= 1e-13


def test_newton_hopf_native_at_c3_size(ctx):
    """The first Hopf point of the trivial state at 1024 x 1024 (config C3: the example's mesh width on a 25x larger domain),
    from (r* + 0.02 width, 0.95 nu) with a = b = the closed-form Hopf mode.  Records the GMRES counts and the time per Newton
    iteration."""
    codim2, hip = _lib()
    n1 = 1024
    dims, ls_ = (n1, n1), (np.pi * n1 / 41, (np.pi / 2) * n1 / 21)
    lap = _dirichlet_lap(dims, ls_)
    rstar, width, nu = -lap[0], lap[0] - lap[1], PARS["nu"]
    r0 = rstar + 0.02 * width
    prob = hip.CGL2d(ctx, dims, ls_, **dict(PARS, r=r0))
    ls = _solver(hip, prob, r0, reltol=1e-12)
    zr, zi = _hopf_mode(dims)
    Z = _pair(prob, zr, zi)
    X0 = codim2.HopfVec(prob.vec(np.zeros(prob.nlocal)), [r0, 0.95 * nu])
    codim2.newton_hopf_native(prob, X0, Z, Z, ls, tol=1e-10, max_iterations=1)          # warm-up (pools, kernels)
    ctx.sync()
    t0 = time.perf_counter()
    s = codim2.newton_hopf_native(prob, X0, Z, Z, ls, tol=1e-10, max_iterations=15)
    ctx.sync()
    dt = time.perf_counter() - t0
    assert s["converged"], s["residuals"]
    p, om = s["u"].p
    print(f"C3 1024^2 Hopf: r = {p:.15g} (r* = {rstar:.15g}), omega = {om:.15g}, itnewton {s['itnewton']}, GMRES "
          f"{s['itlineartot']}, {1e3 * dt / max(s['itnewton'], 1):.1f} ms per Newton iteration, unconverged "
          f"{s['unconverged_solves']}")
    assert abs(p - rstar) <= 1e-9 * abs(rstar) and abs(om - nu) <= 1e-9


def test_hopf_curve_in_gamma_leaves_the_trivial_state_and_matches_the_restatement():
    """continuation_hopf in gamma from the closed-form Hopf point, 6 steps of ds = 0.01 (the example's ds): every point is a
    Hopf point of the dense Jacobian, matches the restatement, and the state is non-zero (the Hessian terms act)."""
    codim2, hip = _lib()
    from bk_amd import continuation as Cn
    import scipy.linalg as sla
    op = operators.CGL2d(DIMS, LS)
    n = 2 * DIMS[0] * DIMS[1]
    lap = _dirichlet_lap(DIMS, LS)
    rstar, nu = -lap[0], PARS["nu"]
    tol = 1e-10
    model = R.cgl_model(op, dict(PARS), "r", "gamma")
    zr, zi = _hopf_mode(DIMS)
    z = zr + 1j * zi
    ds_seq = [0.01] * 6
    ref = R.continuation_hopf(model, np.zeros(n), rstar, nu, 0.0, z, z, ds=0.01, dsmax=0.01, tol=tol, max_iterations=10,
                              ds_sequence=ds_seq)
    ctx = hip.Context(0)
    prob = hip.CGL2d(ctx, DIMS, LS, **dict(PARS, r=rstar))
    ls = _solver(hip, prob, rstar)
    Z = _pair(prob, zr, zi)
    cp = Cn.ContinuationPar(ds=0.01, dsmin=1e-4, dsmax=0.01, p_min=-1.0, p_max=1.0, max_steps=10,
                            newton_options=Cn.NewtonPar(tol=tol, max_iterations=10))
    br = codim2.continuation_hopf(prob, codim2.HopfVec(prob.vec(np.zeros(n)), [rstar, nu]), 0.0, "gamma", Z, Z, ls, cp,
                                  save_sol=True, ds_sequence=ds_seq)
    assert len(br.p2) == len(ref["p2"]) == 7
    for i, zz in enumerate(br.sol):
        x = zz.u.u.numpy()
        r, om, g = zz.u.p[0], zz.u.p[1], zz.p
        q = dict(PARS, r=r, gamma=g)
        assert np.abs(op.F(x, **q)).max() <= tol
        ev = sla.eigvals(op.J(x, **q).toarray())
        k = np.argmin(np.abs(ev - 1j * om))
        print(f"point {i}: gamma {g:+.4f} r {r:.12f} omega {om:.12f} |x|_inf {np.abs(x).max():.3e} nearest eigenvalue "
              f"{ev[k]:.3e} itlinear {br.itlinear[i]}")
        assert abs(ev[k].real) <= 1e-8 and abs(ev[k].imag - om) <= 1e-8, ev[k]
        assert max(abs(r - ref["p1"][i]), abs(g - ref["p2"][i]), abs(om - ref["omega"][i])) <= 1e-8, (i, r, g, om, ref)
    last = br.sol[-1]
    assert np.abs(last.u.u.numpy()).max() > 1e-3
    H = codim2.HopfProblem(prob, "gamma", Z, Z, ls)
    v, w, _ = H.terms(last.u, last.p)
    S, _, _ = codim2.hopf_contract(prob, last.u.u, H.pvec(last.u.p[0], last.p), 0, v, w, [last.u.u])
    assert abs(S[0]) > 1e-8, S


def test_bisected_hopf_point_refines_end_to_end(ctx):
    """continuation_native(..., bisection = True, save_sol = True) across the first Hopf point of the trivial branch, then
    hopf_point and newton_hopf_native from the reference's default start vectors and from start_with_eigen (ShiftInvert with
    save_vectors: b = the eigenvector of +i omega, a = zeta* with a^H b = 1).  The eigen start must be the Hopf mode itself, not
    its conjugate: |v^H b| ~ 1 for the null vector v of J - i omega at the refined point (the conjugate mode is orthogonal)."""
    codim2, hip = _lib()
    from bk_amd import continuation as Cn
    lap = _dirichlet_lap(DIMS, LS)
    rstar = -lap[:2]
    width = float(rstar[1] - rstar[0])
    prob = hip.CGL2d(ctx, DIMS, LS, r=0.5)
    n = prob.nlocal
    ls = _solver(hip, prob, float(rstar[0]), reltol=1e-10)
    lse = _solver(hip, prob, float(rstar[0]) - 1.0, reltol=1e-10)
    eig = hip.ShiftInvert(1.0, lse, tol=1e-8, maxiter=300, hermitian=False, save_vectors=False)
    nopt = Cn.NewtonPar(tol=1e-10, max_iterations=20, linsolver=ls, eigsolver=eig)
    cp = Cn.ContinuationPar(ds=0.5 * width, dsmin=1e-3 * width, dsmax=0.6 * width, p_min=float(rstar[0] - 2 * width),
                            p_max=float(rstar[1]), max_steps=3, nev=6, newton_options=nopt, n_inversion=2,
                            max_bisection_steps=4, dsmin_bisection=1e-4 * width)
    alg = Cn.PALC(tangent="secant", theta=0.5, bls=hip.BorderingBLS(None, check_precision=False))
    br = Cn.continuation_native(prob, prob.vec(np.zeros(n)), float(rstar[0] - 0.7 * width), alg, cp, normC=Cn.norminf,
                                bisection=True, save_sol=True)
    ih = [i for i, s in enumerate(br.specialpoint) if s.get("type") == "hopf"]
    assert ih, br.specialpoint
    X = codim2.hopf_point(br, ih[0])
    assert abs(X.p[1] - PARS["nu"]) <= 1e-6, X.p
    eigv = hip.ShiftInvert(1.0, lse, tol=1e-10, maxiter=300, hermitian=False, save_vectors=True)
    for start in ("random", "eigen"):
        a, b = codim2.hopf_start_vectors(prob, X, ls, eig=eigv if start == "eigen" else None, nev=6)
        s = codim2.newton_hopf_native(prob, X, a, b, ls, tol=1e-10, max_iterations=15)
        assert s["converged"], (start, s["residuals"])
        assert abs(s["u"].p[0] - rstar[0]) <= 1e-9 * abs(rstar[0]) and abs(s["u"].p[1] - PARS["nu"]) <= 1e-9, (start, s["u"].p)
        if start == "eigen":
            ab = codim2.cinner(a, b)
            assert abs(ab - 1) <= 1e-10, ab
            al = abs(codim2.cinner(s["v"], b)) / (codim2.cnorm(s["v"]) * codim2.cnorm(b))
            print(f"start_with_eigen: a^H b = {ab:.3e}, |v^H b| / |v||b| = {al:.12f}, itnewton {s['itnewton']}")
            assert al >= 0.999, al


def _nontrivial_hopf_point():
    """A Hopf point with u != 0 (gamma = 0.1, refined in r by the restatement from u = 0): (state, r, omega, v, w)."""
    op = operators.CGL2d(DIMS, LS)
    rstar = -_dirichlet_lap(DIMS, LS)[0]
    zr, zi = _hopf_mode(DIMS)
    m = R.cgl_model(op, dict(PARS, gamma=0.1), "r")
    s = R.newton_hopf(m, np.zeros(2 * DIMS[0] * DIMS[1]), rstar, PARS["nu"], zr + 1j * zi, zr + 1j * zi, tol=1e-12,
                      max_iterations=20)
    assert s["converged"] and np.abs(s["u"]).max() > 0.1, s["residuals"]
    return op, s


@pytest.mark.parametrize("lens", ["mu", "c3"])
def test_newton_hopf_in_a_hessian_coefficient_matches_mirror_and_restatement(lens):
    """Newton in mu or c3 -- parameters that enter d2F -- at a Hopf point off the trivial state (gamma = 0.1, r fixed), started
    0.3 away: the Hessian terms of every step must be those of the current parameter value.  Native, mirror and restatement
    take the same number of Newton iterations with the same residual history and land on the start point's parameter.  (With
    the coefficients of the start value the native solve needs one more iteration in mu, and reaches 2e-9 instead of 1e-11 at
    the second step in c3.)"""
    codim2, hip = _lib()
    op, base = _nontrivial_hopf_point()
    pars = dict(PARS, gamma=0.1, r=base["p"])
    p0 = PARS[lens] + 0.3
    a, b = base["w"] / np.linalg.norm(base["w"]), base["v"] / np.linalg.norm(base["v"])
    model = R.cgl_model(op, pars, lens)
    ref = R.newton_hopf(model, base["u"], p0, base["omega"], a, b, tol=1e-12, max_iterations=15)
    assert ref["converged"] and abs(ref["p"] - PARS[lens]) <= 1e-11, ref
    out = {}
    for kind in ("native", "mirror"):
        ctx = hip.Context(0)
        prob = hip.CGL2d(ctx, DIMS, LS, lens=lens, **dict(pars, **{lens: p0}))
        ls = _solver(hip, prob, base["p"])
        X0 = codim2.HopfVec(prob.vec(base["u"]), [p0, base["omega"]])
        A, B = _pair(prob, a.real, a.imag), _pair(prob, b.real, b.imag)
        f = codim2.newton_hopf_native if kind == "native" else codim2.newton_hopf
        out[kind] = s = f(prob, X0, A, B, ls, tol=1e-12, max_iterations=15)
        print(f"{lens} {kind}: itnewton {s['itnewton']}, GMRES {s['itlineartot']}, residuals {s['residuals']}")
        assert s["converged"], (kind, s["residuals"])
        assert s["itnewton"] == ref["itnewton"], (kind, s["residuals"], ref["residuals"])
        for rg, rr in zip(s["residuals"], ref["residuals"]):
            if max(rg, rr) >= 1e-10:                            # below that the GMRES tolerance, not the step, sets the value
                assert abs(math.log10(rg) - math.log10(rr)) <= 0.5, (kind, s["residuals"], ref["residuals"])
        p, om = s["u"].p
        assert abs(p - ref["p"]) <= 1e-11 and abs(om - ref["omega"]) <= 1e-11, (kind, p, om, ref["p"], ref["omega"])
        assert np.abs(s["u"].u.numpy() - ref["u"]).max() <= 1e-10
    assert out["native"]["itnewton"] == out["mirror"]["itnewton"]
    assert np.abs(out["native"]["u"].p - out["mirror"]["u"].p).max() <= 1e-13


def test_hopf_contract_non_temporal_path_at_2048_squared(ctx):
    """n = 2 * 2048^2 = 2^23 >= 2^22 selects the non-temporal 16-B instantiation: exact sums as for the small lengths."""
    codim2, hip = _lib()
    dims = (2048, 2048)
    prob = hip.CGL2d(ctx, dims, (1.0, 1.0), **PARS)
    assert prob.nlocal >= 1 << 22
    rng = np.random.default_rng(11)
    n = prob.nlocal
    pars = dict(PARS)
    pv = [pars[k] for k in R.CGL_PARAMS]
    u, vr, vi, wr, wi = (rng.standard_normal(n) for _ in range(5))
    Xs = [rng.standard_normal(n) for _ in range(3)]
    S, P, Q = codim2.hopf_contract(prob, prob.vec(u), pv, 1, (prob.vec(vr), prob.vec(vi)), (prob.vec(wr), prob.vec(wi)),
                                   [prob.vec(x) for x in Xs])
    v, w = vr + 1j * vi, wr + 1j * wi
    terms = [np.conj(w) * R.cgl_d2F(u, pars, v, x) for x in Xs] + [np.conj(w) * R.cgl_dJvdp(u, pars, "mu", v), np.conj(w) * v]
    for name, got, t in zip(("S0", "S1", "S2", "P", "Q"), list(S) + [P, Q], terms):
        for part in ("real", "imag"):
            tt = getattr(t, part)
            bound = 4 * n * EPS * np.abs(tt).sum()
            probe(f"hopf.contract_nt_{name}_{part}", abs(getattr(got, part) - math.fsum(tt)) / bound, 1.0)


def test_hopf_unconverged_solves_are_counted():
    """With maxiter = 1 every bordered-vector solve stops early: the native counter equals the mirror's count, one per point.
    On u = 0 the step's solves J \\ F and J \\ dpF have zero right-hand sides and converge at once."""
    codim2, hip = _lib()
    n = 2 * DIMS[0] * DIMS[1]
    rstar = -_dirichlet_lap(DIMS, LS)[0]
    zr, zi = _hopf_mode(DIMS)
    counts = {}
    for kind in ("native", "mirror"):
        ctx = hip.Context(0)
        prob = hip.CGL2d(ctx, DIMS, LS, **dict(PARS, r=rstar + 0.02))
        ls = hip.GMRESIterativeSolvers(reltol=1e-13, restart=2, maxiter=1, Pl=hip.LaplacePreconditioner(prob, 1.0))
        Z = _pair(prob, zr, zi)
        X0 = codim2.HopfVec(prob.vec(np.zeros(n)), [rstar + 0.02, 0.95])
        f = codim2.newton_hopf_native if kind == "native" else codim2.newton_hopf
        s = f(prob, X0, Z, Z, ls, tol=1e-14, max_iterations=2)
        counts[kind] = (s["unconverged_solves"], s["itnewton"])
    assert counts["native"] == counts["mirror"], counts
    assert counts["native"][1] == 2 and counts["native"][0] == counts["native"][1] + 1, counts
