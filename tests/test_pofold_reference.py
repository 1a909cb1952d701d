"""CPU pins of tests/pofold_ref.py, the restatement the GPU tests of the adjoint orbit Jacobian (test_gpu_pofold.py) compare with:
the assembled Jacobian transposed, sparse LU of the transposed preconditioner matrix, sparse LU of the transposed Jacobian for
the preconditioned GMRES, differences of the long-double JVP for the second derivatives, the closed-form fold of limit cycles on
one grid point, and the recorded bordered Newton at 16 x 12."""
import math

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import pofold_ref as F
import potrap_ref as R

LS = (np.pi, np.pi / 2)
PARS = dict(r=0.5, mu=0.1, nu=1.0, c3=-1.0, c5=1.0, gamma=0.0)
EPS = np.finfo(float).eps
# the GPU cases of test_gpu_pofold.py: (dims, M)
CASES = [((12, 9), 7), ((23, 17), 9), ((16, 12), 12), ((12, 9), 3)]


def _rstar(m):
    return -m.lam.max()


def _random(m, M, seed, amp=0.5):
    rng = np.random.default_rng(seed)
    return (amp * rng.standard_normal((M, m.N)), rng.standard_normal((M, m.N)), rng.standard_normal((M, m.N)), 1.0 + rng.random(),
            rng.standard_normal())


@pytest.mark.parametrize("dims,M", CASES)
def test_adjoint_application_is_the_transpose_of_the_assembled_jacobian(dims, M):
    """jvp_adjoint in double against jacobian_sparse(...).T @ y, entry by entry within 8 eps x (the sum of the moduli of the entry's
    terms): both evaluate the same few terms per entry in another order.  The tail, a sum over K N products, within the summation
    bound K N eps sum |terms|.  The long-double evaluation, the GPU yardstick, agrees with the double one to the same bound."""
    m = R.Model(dims, LS)
    pars = dict(PARS, gamma=0.2)
    U, W, phi, T, tau = _random(m, M, 11)
    out, tail = F.jvp_adjoint(m, U, T, pars, W, tau, phi)
    unit, utail = F.jvp_adjoint(m, U, T, pars, W, tau, phi, mod=True)
    ref = R.jacobian_sparse(m, U, T, pars, phi).T @ R.pack(W, tau)
    assert np.all(np.abs(out.reshape(-1) - ref[:-1]) <= 8 * EPS * unit.reshape(-1))
    assert abs(tail - ref[-1]) <= (M - 1) * m.N * EPS * utail
    ld, ldtail = F.jvp_adjoint(m, U.astype(R.LD), T, pars, W.astype(R.LD), tau, phi.astype(R.LD))
    assert np.all(np.abs(out - ld) <= 8 * EPS * unit)
    assert abs(tail - float(ldtail)) <= (M - 1) * m.N * EPS * utail


@pytest.mark.parametrize("dims,M", CASES[:3])
def test_adjoint_and_forward_applications_are_dual(dims, M):
    """<dG x, y> = <x, dG^T y> for the two restated applications in long double, to the rounding of the sums."""
    m = R.Model(dims, LS)
    pars = dict(PARS, gamma=0.2)
    U, W, phi, T, tau = _random(m, M, 12)
    rng = np.random.default_rng(13)
    X, dT = rng.standard_normal((M, m.N)), rng.standard_normal()
    L = lambda a: a.astype(R.LD)
    jx, jt = R.jvp(m, L(U), T, pars, L(X), dT, L(phi))
    ay, at = F.jvp_adjoint(m, L(U), T, pars, L(W), tau, L(phi))
    lhs = np.sum(jx * L(W)) + jt * R.LD(tau)
    rhs = np.sum(L(X) * ay) + R.LD(dT) * at
    scale = float(np.sum(np.abs(jx * W)) + np.sum(np.abs(X * ay)))
    assert abs(float(lhs - rhs)) <= M * m.N * float(np.finfo(R.LD).eps) * scale


@pytest.mark.parametrize("dims,M", CASES + [((41, 21), 3)])
def test_adjoint_modal_solve_matches_sparse_lu_of_A0_transposed(dims, M):
    """The backward recurrence per sine mode against sparse LU of A0_sparse(...).T at the GPU cases (a = r_hopf - 0.05, b = nu,
    T = 2 pi): the difference is the yardstick of the GPU adjoint time solve."""
    m = R.Model(dims, LS)
    a, b, T = _rstar(m) - 0.05, PARS["nu"], 2 * math.pi
    f = np.random.default_rng(3).standard_normal((M, m.N))
    A0T = R.A0_sparse(m, M, T, a, b).T.tocsc()
    lu = spla.splu(A0T).solve(f.reshape(-1)).reshape(M, -1)
    md = F.modal_solve_adjoint(m, M, T, a, b, f)
    diff = np.abs(md - lu).max() / np.abs(lu).max()
    print(f"adjoint modal vs LU {dims} M={M}: {diff:.3e}")
    assert diff <= 1e-10
    assert np.abs(A0T @ md.reshape(-1) - f.reshape(-1)).max() <= 1e-11 * np.abs(f).max() * max(1.0, np.abs(md).max())


def test_adjoint_gmres_solves_the_transposed_system():
    """At 16 x 12, M = 12 on a smooth orbit-like state: the preconditioned GMRES on dG^T at rtol 1e-9 against sparse LU of the
    assembled transpose; the iteration count is that of the forward system within a few (the spectra are equal)."""
    dims, M = (16, 12), 12
    m = R.Model(dims, LS)
    pars = dict(PARS, r=_rstar(m) - 0.1)
    x, y = np.meshgrid(np.arange(1, m.nx + 1) / (m.nx + 1), np.arange(1, m.ny + 1) / (m.ny + 1))
    mode = (np.sin(np.pi * x) * np.sin(np.pi * y)).reshape(-1)
    th = 2 * math.pi * np.arange(M) / (M - 1)
    U = 0.6 * np.stack([np.concatenate([math.cos(t) * mode, math.sin(t) * mode]) for t in th])
    T = 2 * math.pi * M / (M - 1)
    phi, _ = R.update_section(m, U, pars)
    rhs = np.random.default_rng(5).standard_normal(M * m.N + 1)
    a, b = pars["r"], pars["nu"]
    exact = spla.splu(R.jacobian_sparse(m, U, T, pars, phi).T.tocsc()).solve(rhs)
    xa, ita = F.gmres_solve_adjoint(m, U, T, pars, phi, rhs, a, b, T, 1e-9)
    _, itf = R.gmres_solve(m, U, T, pars, phi, rhs, a, b, T, 1e-9)
    print(f"adjoint gmres: {ita} iterations (forward {itf}), error {np.abs(xa - exact).max():.3e}")
    assert np.abs(xa - exact).max() <= 1e-6 * np.abs(exact).max()
    assert abs(ita - itf) <= 8


# ------------------------------------------------------------------------------------------ second derivatives
@pytest.mark.parametrize("name", ["r", "c5", "mu", "c3", "nu"])
def test_hessian_and_djdp_match_central_differences_of_the_jacobian(name):
    """B(u)[v, x] against (J(u + e v) x - J(u - e v) x) / 2e and D_p(u) v against the same difference in the parameter, in long
    double with e = 1e-6: the difference's own error is e^2 |d3| / 6 (truncation, the fifth-order polynomial has bounded
    derivatives: |d3|, |d2_p| below 1e3 here) plus eps_ld |J x| / e (cancellation), together below 1e-8 of the scale."""
    m = R.Model((7, 5), LS)
    pars = dict(PARS, gamma=0.2)
    rng = np.random.default_rng(21)
    u, v, x = (0.6 * rng.standard_normal(m.N)).astype(R.LD), rng.standard_normal(m.N).astype(R.LD), rng.standard_normal(m.N).astype(R.LD)
    e = R.LD(1e-6)
    fd = (m.Jv(u + e * v, pars, x) - m.Jv(u - e * v, pars, x)) / (2 * e)
    B = F.hess_apply(m, u, pars, v, x)
    assert np.abs(fd - B).max() <= 1e-8 * max(1.0, float(np.abs(B).max()))
    # (B[v, .])^T s is its transpose
    s_ = rng.standard_normal(m.N).astype(R.LD)
    assert abs(float(np.sum(F.hess_vT(m, u, pars, v, s_) * x) - np.sum(s_ * B))) <= 1e-15 * float(np.sum(np.abs(s_ * B)))
    pp, pm = dict(pars, **{name: pars[name] + 1e-6}), dict(pars, **{name: pars[name] - 1e-6})
    fdp = (m.Jv(u, pp, v) - m.Jv(u, pm, v)) / R.LD(2e-6)
    D = F.djdp_v(m, u, name, v)
    assert np.abs(fdp - D).max() <= 1e-8 * max(1.0, float(np.abs(D).max()))


@pytest.mark.parametrize("dims,M", CASES[:3])
@pytest.mark.parametrize("name", ["r", "c5"])
def test_fold_border_matches_differences_of_the_long_double_jvp(dims, M, name):
    """<sigma_x, X> = -<w, d2G[v, X]> and sigma_p = -<w, d_p(dG) v> with the second derivatives as central differences of the
    long-double JVP (e = 1e-6 in the state, 1e-6 in the parameter; error e^2 x third derivatives + eps_ld / e, below 1e-8
    relative to the sum of the moduli of the terms), for a random direction X with a T entry."""
    m = R.Model(dims, LS)
    pars = dict(PARS, gamma=0.2)
    U, W, phi, T, tau = _random(m, M, 31)
    rng = np.random.default_rng(32)
    V, X = rng.standard_normal((M, m.N)), rng.standard_normal((M, m.N))
    vT, xT = rng.standard_normal(), rng.standard_normal()
    L = lambda a: a.astype(R.LD)
    sx, sxT, sp = F.fold_border(m, L(U), T, pars, name, L(V), vT, L(W))
    e = R.LD(1e-6)
    jp, tp = R.jvp(m, L(U) + e * L(X), R.LD(T) + e * R.LD(xT), pars, L(V), vT, L(phi))
    jm, tm = R.jvp(m, L(U) - e * L(X), R.LD(T) - e * R.LD(xT), pars, L(V), vT, L(phi))
    d2 = (jp - jm) / (2 * e)
    ref = -(np.sum(L(W) * d2) + R.LD(tau) * (tp - tm) / (2 * e))
    got = np.sum(sx * L(X)) + sxT * R.LD(xT)
    scale = float(np.sum(np.abs(L(W) * d2)))
    assert abs(float(got - ref)) <= 1e-8 * scale, (float(got), float(ref))
    pp, pm = dict(pars, **{name: pars[name] + 1e-6}), dict(pars, **{name: pars[name] - 1e-6})
    dp = (R.jvp(m, L(U), T, pp, L(V), vT, L(phi))[0] - R.jvp(m, L(U), T, pm, L(V), vT, L(phi))[0]) / R.LD(2e-6)
    assert abs(float(sp + np.sum(L(W) * dp))) <= 1e-8 * float(np.sum(np.abs(L(W) * dp))), (float(sp), float(-np.sum(L(W) * dp)))
    # sigma_x has no closure row
    assert np.all(sx[M - 1] == 0)


# ------------------------------------------------------------------------------------------ the fold of limit cycles
def _fold_jacobian_dense(m, s, pars, name, phi):
    """The Jacobian of the fold system at a converged point, dense: [dG d_pG; sigma_x^T sigma_p]."""
    M = s["U"].shape[0]
    pp = dict(pars, **{name: s["p"]})
    A = R.jacobian_sparse(m, s["U"], s["T"], pp, phi).toarray()
    sx, sxT, sp = F.fold_border(m, s["U"], s["T"], pp, name, s["v"][:-1].reshape(M, -1), s["v"][-1], s["w"][:-1].reshape(M, -1))
    dpG = R.pack(R.dparam(m, s["U"], s["T"], pp, name), 0.0)
    return np.block([[A, dpG[:, None]], [R.pack(sx, sxT)[None, :], np.array([[sp]])]])


@pytest.mark.parametrize("M", [5, 7, 12, 30])          # M = 3: theta = pi, T = (2 M / omega) tan(pi / 2) is infinite
@pytest.mark.parametrize("c5", [1.0, 1.3])
def test_fold_of_the_discrete_stuart_landau_orbit_in_closed_form(M, c5):
    """On one grid point the exact discrete orbit has r_eff = c3 R^2 + c5 R^4 for any M, so the fold of the discrete functional is
    at r + lam_11 = -c3^2 / (4 c5), R^2 = -c3 / (2 c5).  Newton on the fold system (sparse LU) from the closed-form orbit at
    r_eff = -0.24, c5 = 1 (a = b = the branch tangent there by a difference of closed forms) lands there for c5 = 1 and for
    c5 = 1.3.  Bound: 8 eps cond_2(J_fold) max(1, |X|_inf) with J_fold the dense Jacobian of the fold system at the solution -- the
    last Newton update solves J_fold dX = residual with the residual at rounding, eps x (terms of order 1)."""
    m = R.Model((1, 1), LS)
    p0 = dict(PARS, r=-0.24 - m.lam[0])
    U, T, _ = R.stuart_landau_orbit(-0.24, p0, M)
    U2, T2, _ = R.stuart_landau_orbit(-0.24 + 1e-3, p0, M)
    tau = R.pack(U2 - U, T2 - T)
    tau /= np.linalg.norm(tau)
    pars = dict(p0, c5=c5)
    phi, xpi = R.update_section(m, U, pars)
    s = F.newton_fold(m, U, T, pars, "r", phi, xpi, tau, tau, F.lu_bsolver(m), tol=1e-12, max_iterations=15)
    assert s["converged"], s["residuals"]
    cond = np.linalg.cond(_fold_jacobian_dense(m, s, pars, "r", phi))
    bound = 8 * EPS * cond * max(1.0, float(np.abs(s["U"]).max()), s["T"])
    r_fold, R2 = -PARS["c3"] ** 2 / (4 * c5), -PARS["c3"] / (2 * c5)
    got_r, got_R2 = s["p"] + m.lam[0], float(np.max(s["U"][:, 0] ** 2 + s["U"][:, 1] ** 2))
    print(f"1x1 fold M={M} c5={c5}: r_eff {got_r:.15g} (exact {r_fold:.15g}), R^2 {got_R2:.15g} ({R2:.15g}), cond {cond:.3e}, "
          f"bound {bound:.3e}, residuals {s['residuals']}")
    assert abs(got_r - r_fold) <= bound and abs(got_R2 - R2) <= 2 * math.sqrt(R2) * bound + bound ** 2
    assert abs(s["sigma"]) <= 1e-12


# the figures of the recorded run below, the yardsticks of tests/test_gpu_pofold.py and the table of DESIGN 9m
RECORDED = dict(residuals=(1.17e-2, 3.69e-4, 1.84e-7), p=-0.2005157, T=7.349880, amplitude=0.846279, its=(9, 13))


def test_recorded_bordered_newton_at_16x12():
    """The fold run of test_gpu_floquet.py (16 x 12, M = 12, dr = 0.15, ds = -0.02, dsmax = 0.04) on the restatement with sparse LU;
    from its third step -- the point after the fold is crossed -- Newton on the fold system with every linear system a doubly
    bordered one, by sparse LU and by GMRES at rtol 1e-9 preconditioned by diag(A0^-1, 1, 1).  Both converge in three steps with
    the recorded residuals to the recorded fold; every bordered GMRES takes 9 to 13 iterations, the last as the first (the
    bordered systems stay regular at the fold); LU and GMRES agree to 1e-9."""
    dims, M, dr = (16, 12), 12, 0.15
    cp = dict(ds=-0.02, dsmin=1e-4, dsmax=0.04, a=0.5, eta=150.0, tol=1e-10, max_iterations=10)
    m = R.Model(dims, LS)
    rh = _rstar(m)
    pars = dict(PARS, r=rh - dr)
    pars_of = lambda p: dict(pars, r=p)
    U0, T0 = F.hopf_guess(m, M, dr, PARS)
    phi, xpi = R.section_from_guess(m, U0, pars)
    st = F.fold_start(m, U0, T0, pars, "r", phi, xpi, R.lu_solver(m, pars_of), cp, 3)
    pp = dict(pars, r=st["p"])
    lu = F.newton_fold(m, st["U"], st["T"], pp, "r", st["phi"], st["xpi"], st["tau"], st["tau"], F.lu_bsolver(m))
    gm = F.newton_fold(m, st["U"], st["T"], pp, "r", st["phi"], st["xpi"], st["tau"], st["tau"],
                       F.gmres_bsolver(m, pp["r"], pp["nu"], st["T"], 1e-9))
    print(f"fold Newton 16x12: LU residuals {lu['residuals']}, GMRES {gm['residuals']}; p - r_hopf {lu['p'] - rh:.9f} / "
          f"{gm['p'] - rh:.9f}, T {lu['T']:.9f} / {gm['T']:.9f}, amplitude {np.abs(lu['U']).max():.9f}; GMRES counts {gm['itlinear']} "
          f"{gm['last_terms_its']}; |dp| {abs(lu['p'] - gm['p']):.3e} |dT| {abs(lu['T'] - gm['T']):.3e}")
    for s in (lu, gm):
        assert s["converged"] and len(s["residuals"]) == 4 and s["residuals"][-1] < 1e-12, s["residuals"]
        for got, rec in zip(s["residuals"], RECORDED["residuals"]):
            assert abs(got - rec) <= 0.01 * rec, (got, rec)
        assert abs(s["p"] - rh - RECORDED["p"]) <= 1e-6 and abs(s["T"] - RECORDED["T"]) <= 1e-5
        assert abs(np.abs(s["U"]).max() - RECORDED["amplitude"]) <= 1e-5
    counts = [c for t in gm["itlinear"] for c in t] + list(gm["last_terms_its"])
    assert RECORDED["its"][0] <= min(counts) and max(counts) <= RECORDED["its"][1], counts
    assert abs(lu["p"] - gm["p"]) <= 1e-9 and abs(lu["T"] - gm["T"]) <= 1e-9 and np.abs(lu["U"] - gm["U"]).max() <= 1e-9
    # the fold curve in c5 from each refined point: three PALC steps (ds = 0.01, dsmin = 1e-3, dsmax = 0.05, cGL2d.jl:381) with the
    # natural step sizes, a and b renewed per point.  LU and GMRES agree to 1e-9; two Newton steps per point; 105 GMRES iterations
    # per step over its ten bordered solves; (p1 - r_hopf) c5 stays at -0.2005 .. -0.2006 (recorded: -0.200516, -0.200543,
    # -0.200578, -0.200623 at c5 = 1, 1.01397, 1.03243, 1.05681)
    cpf = dict(ds=0.01, dsmin=1e-3, dsmax=0.05, a=0.5, eta=150.0, tol=1e-10, max_iterations=10)
    curves = {}
    for key, s, bs in (("lu", lu, F.lu_bsolver(m)), ("gm", gm, F.gmres_bsolver(m, pp["r"], pp["nu"], st["T"], 1e-9))):
        curves[key] = F.palc_fold(m, s["U"], s["T"], dict(pp, r=s["p"]), "r", "c5", st["phi"], st["xpi"], st["tau"], st["tau"], bs, cpf, 3)
    cl, cg = curves["lu"], curves["gm"]
    prod = [(a - rh) * b for a, b in zip(cl["p1"], cl["p2"])]
    print(f"fold curve 16x12: p1 - r_hopf {[p - rh for p in cl['p1']]}, c5 {cl['p2']}, T {cl['T']}, newton {cl['itnewton']}, "
          f"GMRES per step {cg['itlinear']}, (p1 - r_hopf) c5 {prod}")
    for key in ("p1", "p2", "T", "amplitude"):
        assert np.abs(np.array(cl[key]) - np.array(cg[key])).max() <= 1e-9, key
    assert cl["itnewton"] == cg["itnewton"] == [0, 2, 2, 2]
    for got, rec in zip(cl["p2"], (1.0, 1.01397, 1.03243, 1.05681)):
        assert abs(got - rec) <= 1e-5
    for got, rec in zip(prod, (-0.200516, -0.200543, -0.200578, -0.200623)):
        assert abs(got - rec) <= 1e-6
    assert all(9 * 10 <= c <= 13 * 10 for c in cg["itlinear"][1:]), cg["itlinear"]
