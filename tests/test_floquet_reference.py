"""CPU tests of the restatement tests/floquet_ref.py, the yardstick of tests/test_gpu_floquet.py: the dense monodromy against a
closed form on one grid point, the space-time solve against the dense monodromy, the modal solve of the initial-value preconditioner
against sparse LU of its matrix, and the classification of bifurcations of orbits (the product's pure function and the
restatement's) against the rows of src/Bifurcations.jl:103-131."""
import math

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import floquet_ref as Fq
import potrap_ref as R

LS = (np.pi, np.pi / 2)
PARS = dict(r=0.5, mu=0.1, nu=1.0, c3=-1.0, c5=1.0, gamma=0.0)
EPS = np.finfo(float).eps
# the shapes of the GPU tests of the marching kernel and the preconditioner; M = 3 is the smallest bk_potrap_create accepts
GPU_SHAPES = [((12, 9), 7), ((23, 17), 9), ((16, 12), 12), ((12, 9), 3), ((41, 21), 3)]
# (dims, M, dr, Newton steps): the three cases of DESIGN 9l's table; the first stops Newton before convergence (operator only)
TABLE = [((12, 9), 7, 0.1), ((16, 12), 12, 0.1), ((16, 12), 30, 0.01)]


def _rot(t):
    return np.array([[math.cos(t), -math.sin(t)], [math.sin(t), math.cos(t)]])


@pytest.mark.parametrize("M", [4, 7, 30, 100])       # M = 3: theta = pi, T = (2 M / omega) tan(pi / 2) is infinite
def test_dense_monodromy_closed_form_on_a_1x1_grid(M):
    """Stuart-Landau on one grid point, the exact discrete orbit u_i = Rot(i theta) u_0, theta = 2 pi / K.  The vector field is
    equivariant, J_i = Rot(i theta) J_0 Rot(-i theta), so with C = (I - hh J_0)^-1 Rot(-theta) (I + hh J_0) step i >= 1 is
    Rot(i theta) C Rot(-(i - 1) theta), step 0 is C Rot(theta) (prev(0) = K - 1 and Rot(K theta) = I), and the product telescopes:

        monodromy = Rot(-theta) C^K Rot(theta)

    -- C^K itself up to the similarity by Rot(theta) (J_0 does not commute with rotations, so the similarity stays).  Agreement at
    rounding: the bound is 8 eps cond with cond = K cond_2(I - hh J_0) max(1, |C|_2)^K, the K solves with one matrix class and the
    growth of the K-fold product; printed.  The tangent of the orbit is an exact eigenvector, so 1 is an eigenvalue within the same
    bound times the eigenvalue's own condition number 1 / |y^H x|."""
    m = R.Model((1, 1), LS)
    pars = dict(PARS, r=2.0)
    U, T, _ = R.stuart_landau_orbit(pars["r"] + m.lam[0], pars, M)
    K, hh = M - 1, R._hh(T, M, float)
    th = 2 * math.pi / K
    J0 = m.J(U[0], pars).toarray()
    A0 = np.eye(2) - hh * J0
    Cm = np.linalg.solve(A0, _rot(-th) @ (np.eye(2) + hh * J0))
    closed = _rot(-th) @ np.linalg.matrix_power(Cm, K) @ _rot(th)
    mono = Fq.dense_monodromy(m, U, T, pars)
    cond = K * np.linalg.cond(A0) * max(1.0, np.linalg.norm(Cm, 2)) ** K
    err = np.abs(mono - closed).max()
    w, _, kap = Fq.leading_multipliers(mono, 2)
    k1 = int(np.argmin(np.abs(w - 1)))
    print(f"1x1 M={M}: |mono - closed| {err:.3e}, cond {cond:.3e}, bound {8 * EPS * cond:.3e}; multipliers {w}, kappa {kap}")
    assert err <= 8 * EPS * cond
    assert abs(w[k1] - 1) <= 8 * EPS * cond * kap[k1]
    # the sequential form and the initial-value system give the same last slice
    x = np.array([0.3, -0.8])
    ys = Fq.monodromy_sequential(m, U, T, pars, x)
    assert np.abs(ys[-1] - mono @ x).max() <= 8 * EPS * cond * np.abs(x).max()
    unit = Fq.ivp_apply(m, U, T, pars, ys, mod=True).max()
    assert np.abs(Fq.ivp_apply(m, U, T, pars, ys) - Fq.ivp_rhs(m, U, T, pars, x)).max() <= 8 * EPS * cond * unit


# iterations at rtol 1e-3 / 1e-6 / 1e-9 and the error at 1e-9, measured with x = the unit random vector of seed 5
MEASURED = {((12, 9), 7, 0.1): ((6, 10, 14), 8.6e-11), ((16, 12), 12, 0.1): ((4, 7, 9), 3.1e-11), ((16, 12), 30, 0.01): ((2, 4, 5), 3.7e-11)}


@pytest.mark.parametrize("dims,M,dr", TABLE)
def test_spacetime_solve_matches_the_dense_monodromy(dims, M, dr):
    """The last slice of the space-time GMRES solution (preconditioner a = r, b = nu) equals the dense monodromy applied to x; the
    counts and errors are the yardsticks of the GPU tests and the rows of DESIGN 9l's table.  The error bound is the stopping rule's:
    |A0^-1 (f - A y)| <= rtol |A0^-1 f| bounds the error by cond(A0^-1 A) rtol |y|, and cond(A0^-1 A) is below 10 on these orbits
    (measured 2.5 .. 6), so 10 rtol |y|_2; iteration counts within 1 of the recorded ones (another BLAS may round the Arnoldi
    process differently near a threshold).  At (12, 9), M = 7 Newton (10 steps) has not converged: the monodromy of a non-orbit
    is as good an operator, its largest multiplier just is not 1."""
    m = R.Model(dims, LS)
    s, pars, _, _, _ = Fq.converged_orbit(m, M, dr, PARS)
    assert s["converged"] == (dims != (12, 9))
    U, T = s["U"], s["T"]
    mono = Fq.dense_monodromy(m, U, T, pars)
    x = np.random.default_rng(5).standard_normal(m.N)
    x /= np.linalg.norm(x)
    its, errs = [], []
    for rtol in (1e-3, 1e-6, 1e-9):
        Y, it = Fq.spacetime_solve(m, U, T, pars, x, pars["r"], pars["nu"], rtol)
        its.append(it)
        errs.append(float(np.abs(Y[-1] - mono @ x).max()))
        assert errs[-1] <= 10 * rtol * np.linalg.norm(Y)
    w, _, kap = Fq.leading_multipliers(mono, 6)
    print(f"space-time {dims} M={M} dr={dr}: iterations {its}, errors {errs}; multipliers {w}; kappa {kap}")
    rec_its, rec_err = MEASURED[(dims, M, dr)]
    assert all(abs(a - b) <= 1 for a, b in zip(its, rec_its)), (its, rec_its)
    assert errs[-1] <= 4 * rec_err
    # the sequential form with dense solves is the dense monodromy at rounding, and its slices solve the initial-value rows
    ys = Fq.monodromy_sequential(m, U, T, pars, x)
    assert np.abs(ys[-1] - mono @ x).max() <= 1e-13
    if s["converged"]:
        assert abs(w[1] - 1) <= 1e-8 if abs(w[0]) > 1.05 else abs(w[0] - 1) <= 1e-8


@pytest.mark.parametrize("dims,M,dr,nev", [((16, 12), 12, 0.1, 2), ((16, 12), 30, 0.01, 4)])
def test_recorded_delta_of_the_gmres_monodromy(dims, M, dr, nev):
    """delta = |M_gmres - M_dense|_2 with M_gmres assembled column by column by the space-time GMRES at rtol 1e-9: the perturbation
    in the eigenvalue bound 10 kappa (delta + tol_eig) of the GPU multiplier tests.  floquet_ref.DELTA records it; here it is
    recomputed and has to sit within a factor 2.  The leading multipliers are simple and well conditioned (kappa printed)."""
    m = R.Model(dims, LS)
    s, pars, _, _, _ = Fq.converged_orbit(m, M, dr, PARS)
    mono = Fq.dense_monodromy(m, s["U"], s["T"], pars)
    Mg, its = Fq.monodromy_by_gmres(m, s["U"], s["T"], pars, pars["r"], pars["nu"], 1e-9)
    delta = float(np.linalg.norm(Mg - mono, 2))
    w, _, kap = Fq.leading_multipliers(mono, nev)
    print(f"delta {dims} M={M}: {delta:.3e} (recorded {Fq.DELTA[(dims, M, dr)]:.3e}), iterations {min(its)}..{max(its)}, "
          f"multipliers {w}, kappa {kap}, bounds {10 * kap * (delta + 1e-8)}")
    assert 0.5 * Fq.DELTA[(dims, M, dr)] <= delta <= 2 * Fq.DELTA[(dims, M, dr)]
    assert kap.max() < 2 and np.abs(w.imag).max() == 0


@pytest.mark.parametrize("dims,M", GPU_SHAPES)
def test_ivp_modal_solve_matches_sparse_lu_of_A0(dims, M):
    """The initial-value modal solve against sparse LU of A0 at every shape of the GPU tests, a = r_hopf - 0.05, b = nu, T = 2 pi,
    a random right-hand side: the difference is the yardstick of the GPU preconditioner test (10 x, floored at 8 eps |solution|).
    Bound here: 64 eps cond_est |solution|, cond_est = (1 + |beta / alpha|_max + ... ) <= K max(1, |rho|)^K / min |alpha| -- the
    forward substitution's growth."""
    m = R.Model(dims, LS)
    a, b, T = -m.lam.max() - 0.05, PARS["nu"], 2 * math.pi
    K = M - 1
    f = np.random.default_rng(3 + M).standard_normal((K, m.N))
    lu = spla.splu(Fq.A0_ivp_sparse(m, M, T, a, b)).solve(f.reshape(-1)).reshape(K, -1)
    md = Fq.modal_solve_ivp(m, M, T, a, b, f)
    hh = R._hh(T, M, float)
    mu = a + m.lam + 1j * b
    rho = np.abs((1 + hh * mu) / (1 - hh * mu)).max()
    cond = K * max(1.0, rho) ** K / Fq.modal_min_alpha(m, M, T, a, b)
    d = float(np.abs(md - lu).max())
    print(f"ivp modal vs LU {dims} M={M}: {d:.3e} (|solution| {np.abs(lu).max():.3e}, cond_est {cond:.3e})")
    assert d <= 64 * EPS * cond * np.abs(lu).max()
    # the matrix is what the operator applies when the orbit is the trivial state and (r, nu) = (a, b)
    U = np.zeros((M, m.N))
    o = Fq.ivp_apply(m, U, T, dict(PARS, r=a, nu=b), lu)
    assert np.abs(o - f).max() <= 1e-9 * np.abs(f).max()


def test_ivp_guard_names_a_small_alpha():
    """alpha = 1 - hh (a + lam + i b) vanishes only for b = 0: with b = 0 and a = 1 / hh - lam_11 the (1, 1) mode is below the pivot
    threshold -- the guard case of the GPU test."""
    m = R.Model((16, 12), LS)
    M, T = 12, 2 * math.pi
    hh = R._hh(T, M, float)
    assert Fq.modal_min_alpha(m, M, T, 1 / hh - m.lam.max(), 0.0) < R.PIVOT
    assert Fq.modal_min_alpha(m, M, T, -m.lam.max() - 0.05, PARS["nu"]) > 0.1


# rows of src/Bifurcations.jl:103-131 for a Floquet solver: (n_unstable, n_unstable_prev, n_imag, n_imag_prev) -> type
ROWS = [((1, 0, 0, 0), "bp"),          # one real exponent crosses
        ((0, 1, 0, 0), "bp"),          # ... and back: the fold of limit cycles
        ((1, 0, 1, 0), "pd"),          # one exponent with a nonzero imaginary part: the multiplier crosses at -1
        ((3, 2, 2, 0), "nd"),          # delta n_unstable = 1, delta n_imag = 2: the conjugate is missing (:127-131)
        ((2, 0, 2, 0), "ns"),          # a pair
        ((2, 0, 0, 0), "nd"),          # two real ones at once
        ((2, 0, 1, 0), "nd"),
        ((3, 0, 2, 0), "nd"),          # more than two
        ((1, -1, 0, -1), "nd")]        # counts not populated yet (:133-137)


@pytest.mark.parametrize("counts,tp", ROWS)
def test_classification_follows_the_table_of_the_reference(counts, tp):
    from bk_amd.periodic_orbit import classify_po_bifurcation
    nu, nup, ni, nip = counts
    got = classify_po_bifurcation(nu, nup, ni, nip)
    assert got["type"] == tp and Fq.classify(nu, nup, ni, nip) == tp
    assert got["delta"] == (nu - nup, ni - nip)
    assert got["ind_ev"] == (nup if nu < nup else nu)                    # :95


def test_no_change_of_n_unstable_is_no_point_and_counts_ignore_nan():
    from bk_amd.periodic_orbit import classify_po_bifurcation, floquet_exponents, stability_counts
    assert classify_po_bifurcation(1, 1, 0, 0) is None and Fq.classify(1, 1, 0, 0) is None
    mults = np.array([2.0, 1.0 + 1e-12, -1.5, 0.3 + 0.4j, complex("nan")])
    s = floquet_exponents(mults)
    assert stability_counts(s, 1e-10) == Fq.stability_counts(Fq.floquet_exponents(mults[:4]), 1e-10) == (2, 1)
    assert stability_counts(s, 1e-13) == (3, 1)
