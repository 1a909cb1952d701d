"""CPU pins of tests/potrap_ref.py, the restatement the GPU tests of the trapezoid periodic orbits (test_gpu_potrap.py) compare
with: a closed form, finite differences, the assembled Jacobian, sparse LU of the preconditioner matrix, the reference's own
Stuart-Landau setup and the oracle's vector field."""
import math

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import potrap_ref as R
from oracle import operators

LS = (np.pi, np.pi / 2)
PARS = dict(r=0.5, mu=0.1, nu=1.0, c3=-1.0, c5=1.0, gamma=0.0)
EPS = np.finfo(float).eps
# the GPU cases of test_gpu_potrap.py: (dims, M)
CASES = [((12, 9), 7), ((16, 12), 12), ((23, 17), 9), ((12, 9), 3), ((12, 9), 33)]


def _rstar(m):
    return -m.lam.max()


def _random_orbit(m, M, seed, amp=0.5):
    rng = np.random.default_rng(seed)
    return amp * rng.standard_normal((M, m.N)), rng.standard_normal((M, m.N)), 1.0 + rng.random(), rng.standard_normal()


@pytest.mark.parametrize("M", [3, 7, 100])
def test_closed_form_on_a_1x1_grid(M):
    """On one grid point cGL is Stuart-Landau with r_eff = r + lam_11 and the trapezoid scheme has the exact discrete solution
    u_i = R e^{i theta i}, theta = 2 pi / (M - 1) = 2 atan(h omega / 2): the residual vanishes to rounding at
    T = (2 M / omega) tan(pi / (M - 1)), with omega = nu - mu R^2 for NL's sign of mu (z' = (r + i nu) z - (c3 + i mu) |z|^2 z).
    A wrong T (the orbit's own period, M - 1 steps) leaves a residual of first order: the h = T / M convention is pinned."""
    m = R.Model((1, 1), LS)
    pars = dict(PARS, r=2.0)
    r_eff = pars["r"] + m.lam[0]
    assert r_eff != pars["r"]
    U, T, om = R.stuart_landau_orbit(r_eff, pars, M)
    phi, xpi = R.section_from_guess(m, U, pars)
    G, tail = R.residual(m, U.astype(R.LD), T, pars, phi, xpi)
    scale, _ = R.residual(m, U, T, pars, phi, xpi, mod=True)
    assert np.abs(G).max() <= 8 * EPS * scale.max(), (np.abs(G).max(), scale.max())
    assert abs(T * (M - 1) / M - (2 * (M - 1) / om) * math.tan(math.pi / (M - 1))) <= 4 * EPS * T
    Gbad, _ = R.residual(m, U, T * (M - 1) / M, pars, phi, xpi)
    assert np.abs(Gbad[:-1]).max() > 1e-3 / M


@pytest.mark.parametrize("dims,M", CASES[:3])
def test_jvp_matches_central_differences_and_the_assembled_jacobian(dims, M):
    m = R.Model(dims, LS)
    pars = dict(PARS, gamma=0.2)
    U, dU, T, dT = _random_orbit(m, M, 1)
    phi = np.random.default_rng(2).standard_normal((M, m.N))
    xpi = np.zeros_like(U)
    out, tail = R.jvp(m, U, T, pars, dU, dT, phi)
    e = 1e-5
    Gp, tp = R.residual(m, (U + e * dU).astype(R.LD), T + e * dT, pars, phi, xpi)
    Gm, tm = R.residual(m, (U - e * dU).astype(R.LD), T - e * dT, pars, phi, xpi)
    fd = ((Gp - Gm) / (2 * e)).astype(float)
    assert np.abs(fd - out).max() <= 1e-7 * np.abs(out).max()
    assert abs(float((tp - tm) / (2 * e)) - tail) <= 1e-9 * abs(tail)
    A = R.jacobian_sparse(m, U, T, pars, phi)
    got = A @ R.pack(dU, dT)
    ref = R.pack(out, tail)
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()


@pytest.mark.parametrize("dims,M", CASES)
def test_modal_solve_matches_sparse_lu_of_A0(dims, M):
    """The recurrence per sine mode against sparse LU of the assembled A0 at the GPU cases (a = r_hopf - 0.05, b = nu, T = 2 pi):
    the difference is the yardstick of the GPU time solve; both solve the system to a backward error of a few eps."""
    m = R.Model(dims, LS)
    a, b, T = _rstar(m) - 0.05, PARS["nu"], 2 * math.pi
    f = np.random.default_rng(3).standard_normal((M, m.N))
    A0 = R.A0_sparse(m, M, T, a, b)
    lu = spla.splu(A0).solve(f.reshape(-1)).reshape(M, -1)
    md = R.modal_solve(m, M, T, a, b, f)
    diff = np.abs(md - lu).max() / np.abs(lu).max()
    print(f"modal vs LU {dims} M={M}: {diff:.3e}")
    assert diff <= 1e-10
    assert np.abs(A0 @ md.reshape(-1) - f.reshape(-1)).max() <= 1e-11 * np.abs(f).max() * max(1.0, np.abs(md).max())
    amin, dmin = R.modal_guards(m, M, T, a, b)
    assert amin > R.PIVOT and dmin > R.PIVOT


@pytest.mark.parametrize("dims,M", CASES[:2])
def test_the_guard_case_is_below_the_threshold(dims, M):
    """a = -lam_11, b = nu, T = (2 M / nu) tan(pi / (M - 1)): the first sine mode is Hopf-critical and rho^K = 1."""
    m = R.Model(dims, LS)
    T = (2 * M / PARS["nu"]) * math.tan(math.pi / (M - 1))
    amin, dmin = R.modal_guards(m, M, T, _rstar(m), PARS["nu"])
    assert amin > R.PIVOT and dmin < R.PIVOT, (amin, dmin)


def test_stuart_landau_setup_of_the_reference_converges():
    """test/periodic_orbits_function_fd/stuartLandauTrap.jl:23-70: M = 100, circle guess, tol 1e-9, sup norm -- here through cGL on
    a 1 x 1 grid with r_eff = 1, nu = 1, c3 = 1, mu = 0, c5 = 0 (the Stuart-Landau field of that file), Newton with sparse LU."""
    m = R.Model((1, 1), LS)
    pars = dict(r=1.0 - m.lam[0], mu=0.0, nu=1.0, c3=1.0, c5=0.0, gamma=0.0)
    M = 100
    t = np.linspace(0, 2 * np.pi, M)
    U0 = np.stack([np.cos(t), np.sin(t)], axis=1)
    phi, xpi = R.section_from_guess(m, U0, pars)
    pars_of = lambda p: dict(pars, r=p)
    s = R.newton(m, U0, 2 * np.pi, pars["r"], pars_of, phi, xpi, R.lu_solver(m, pars_of), tol=1e-9, max_iterations=10)
    assert s["converged"], s["residuals"]
    # the discrete orbit of the closed form above: radius 1, omega = 1, T = 2 M tan(pi / (M - 1))
    assert abs(s["T"] - 2 * M * math.tan(math.pi / (M - 1))) <= 1e-9 and abs(np.abs(s["U"][:, 0] + 1j * s["U"][:, 1]) - 1.0).max() <= 1e-9


@pytest.mark.parametrize("dims,M", CASES[:2])
def test_functional_matches_the_oracle_slice_by_slice(dims, M):
    m = R.Model(dims, LS)
    op = operators.CGL2d(dims, LS)
    pars = dict(PARS, gamma=0.2)
    U, dU, T, dT = _random_orbit(m, M, 5)
    phi = np.random.default_rng(6).standard_normal((M, m.N))
    xpi = np.random.default_rng(7).standard_normal((M, m.N))
    G, tail = R.residual(m, U, T, pars, phi, xpi)
    dG, dtail = R.jvp(m, U, T, pars, dU, dT, phi)
    K, h = M - 1, T / M
    for i in range(K):
        j = K - 1 if i == 0 else i - 1
        Fi, Fj = op.F(U[i], **pars), op.F(U[j], **pars)
        ref = U[i] - U[j] - (h / 2) * (Fi + Fj)
        assert np.abs(G[i] - ref).max() <= 1e-12 * np.abs(ref).max()
        dref = dU[i] - dU[j] - (h / 2) * (op.J(U[i], **pars) @ dU[i] + op.J(U[j], **pars) @ dU[j]) - (dT / M / 2) * (Fi + Fj)
        assert np.abs(dG[i] - dref).max() <= 1e-12 * np.abs(dref).max()
    assert np.array_equal(G[K], U[K] - U[0]) and np.array_equal(dG[K], dU[K] - dU[0])
    assert abs(tail - np.sum((U - xpi) * phi)) <= 1e-12 * np.sum(np.abs((U - xpi) * phi))
    assert abs(dtail - np.sum(dU * phi)) <= 1e-12 * np.sum(np.abs(dU * phi))
    assert abs(m.J(U[0], pars) - op.J(U[0], **pars)).max() <= 1e-12 * abs(op.J(U[0], **pars)).max()


def _hopf_guess(m, M, dr, ampfactor=1.0):
    """The one-mode guess of the Hopf predictor at the trivial state in closed form: a = 1, b = 2 (-c3 + i mu) 9 / (4 (Nx + 1)
    (Ny + 1)), amp = sqrt(dr / Re b), slices 2 Re(zeta amp e^{i t_m}) with zeta = phi (1, -i) / sqrt 2, T entry 2 pi / omega."""
    b = 2 * (-PARS["c3"] + 1j * PARS["mu"]) * 9 / (4 * (m.nx + 1) * (m.ny + 1))
    amp = ampfactor * math.sqrt(dr / b.real)
    om = PARS["nu"] + (0.0 - b.imag * 1.0 / b.real) * dr
    phi = np.outer(np.sin(np.pi * np.arange(1, m.ny + 1) / (m.ny + 1)), np.sin(np.pi * np.arange(1, m.nx + 1) / (m.nx + 1))).reshape(-1)
    phi /= np.linalg.norm(phi) * math.sqrt(2)
    t = 2 * np.pi * np.arange(M) / M
    U = np.stack([np.concatenate([2 * amp * np.cos(tm) * phi, 2 * amp * np.sin(tm) * phi]) for tm in t])
    return U, abs(2 * np.pi / om)


def test_newton_from_the_m12_guess_at_dr_001_lands_on_the_trivial_state():
    """Why the M = 12 Newton case of the GPU tests starts from dr = 0.1: at 16 x 12, M = 12, dr = 0.01 the reference's guess -- M
    slices on the whole circle, the orbit's own period as the T entry -- sends Newton with sparse LU to u = 0 (amplitude at
    rounding, from a guess amplitude of 0.13)."""
    m = R.Model((16, 12), LS)
    dr, M = 0.01, 12
    r = _rstar(m) - dr
    pars = dict(PARS, r=r)
    pars_of = lambda p: dict(pars, r=p)
    U0, T0 = _hopf_guess(m, M, dr)
    phi, xpi = R.section_from_guess(m, U0, pars)
    lu = R.newton(m, U0, T0, r, pars_of, phi, xpi, R.lu_solver(m, pars_of), tol=1e-10, max_iterations=12)
    assert lu["converged"] and np.abs(U0).max() > 0.1 and np.abs(lu["U"]).max() < 1e-10, (lu["residuals"], np.abs(lu["U"]).max())


@pytest.mark.parametrize("dims,M,dr", [((16, 12), 12, 0.1), ((16, 12), 30, 0.01)])
def test_newton_with_lu_and_with_preconditioned_gmres_agree(dims, M, dr):
    """Newton from the one-mode guess at r = r_hopf - dr: sparse LU against GMRES with the modal preconditioner (a = r, b = nu,
    rtol 1e-9): both converge to 1e-10 in a handful of steps to the orbit, not to the trivial state, and the difference of the two
    orbits is the yardstick of the GPU Newton test.  (The guess has M slices on the full circle and the orbit's own period as
    the T entry, as examples/cGL2d.jl:172-174 builds it, while the closure wants slice M = slice 1: at M = 12 it is far enough off
    that Newton from dr = 0.01 lands on the trivial state, so the M = 12 case starts from dr = 0.1.)"""
    m = R.Model(dims, LS)
    r = _rstar(m) - dr
    pars = dict(PARS, r=r)
    pars_of = lambda p: dict(pars, r=p)
    U0, T0 = _hopf_guess(m, M, dr)
    phi, xpi = R.section_from_guess(m, U0, pars)
    lu = R.newton(m, U0, T0, r, pars_of, phi, xpi, R.lu_solver(m, pars_of), tol=1e-10, max_iterations=10)
    gm = R.newton(m, U0, T0, r, pars_of, phi, xpi, R.gmres_solver(m, pars_of, r, PARS["nu"], T0, 1e-9), tol=1e-10, max_iterations=10)
    assert lu["converged"] and gm["converged"], (lu["residuals"], gm["residuals"])
    assert len(lu["residuals"]) - 1 <= 6 and max(gm["itlinear"]) <= 25, (lu["residuals"], gm["itlinear"])
    assert np.abs(lu["U"]).max() > 0.5 * np.abs(U0).max()
    d = np.abs(lu["U"] - gm["U"]).max()
    print(f"LU vs GMRES Newton {dims} M={M}: orbit {d:.3e}, T {abs(lu['T'] - gm['T']):.3e}, gmres its {gm['itlinear']}")
    assert d <= 1e-8 and abs(lu["T"] - gm["T"]) <= 1e-8
