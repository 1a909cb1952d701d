"""The cases of tests/test_gpu_eig_exhaustion.py are what they claim to be: established on the reference alone (no GPU, writes nothing).

For every case of tests/eig_exhaustion_ref.py:

  * the eigenvalues of the A cases are pairwise distinct and the start vector has a component along every eigenvector, so the Krylov space
    of the start vector is the whole space, d = n; the B start vectors have d = 6 and d = 1;
  * in the float64 restatement of the two-pass Arnoldi step (eig_exhaustion_ref.arnoldi) the remainder ratio nn / ww is at least 1e-20 at
    every step before d and drops below the breakdown threshold 1e-30 at step d -- by the factor recorded in RATIO_AT_D below, which is the
    margin the breakdown test lives on;
  * every wanted set ends at a clear gap (GAP_RATIO = 1.05, the rule of tests/test_gpu_eigensolve_at_size.py); nev values that end inside
    a cluster were moved (NEV_GRID), not the rule;
  * with the breakdown test taken out, the restatement grown to 45 vectors returns Ritz values that match no dense eigenvalue of their
    own, the count of values with positive real part goes up, and the number of operator applications is 45, not d: a solver that
    misses the breakdown fails checks 3, 4, 6 and 8 of the GPU test.
"""
import numpy as np
import pytest

import eig_exhaustion_ref as R

A_IDS = list(R.A_CASES)

# nn / ww at step d = n of the restatement per case and mode, as measured on the CPU this file was written on (float64, NumPy's
# summation order); the test asserts the value of the day within a factor 8 of it.  All sit a factor 6 to 40 below the threshold 1e-30.
RATIO_AT_D = {
    "sh-4x3x2": dict(si=1.6e-31, lr=2.5e-32, lm=2.5e-32),
    "sh-6x5": dict(si=6.8e-32, lr=3.1e-32, lm=3.1e-32),
    "sh-8x4": dict(si=5.6e-32, lr=1.1e-31, lm=1.1e-31),
    "cgl-4x3-zero": dict(si=1.5e-31, lr=5.6e-32, lm=5.6e-32),
    "cgl-4x3-rand": dict(si=4.2e-32, lr=6.2e-32, lm=6.2e-32),
}
# the nev grid per case and mode: {1, 6, n - 2} with a value moved where its set ends inside a cluster
NEV_GRID = {
    "sh-4x3x2": dict(si=(1, 6, 22), lr=(1, 6, 22), lm=(1, 6, 22)),
    "sh-6x5": dict(si=(1, 6, 27), lr=(1, 6, 27), lm=(1, 6, 28)),
    "sh-8x4": dict(si=(1, 6, 29), lr=(1, 6, 29), lm=(1, 6, 30)),
    "cgl-4x3-zero": dict(si=(1, 6, 22), lr=(1, 6, 22), lm=(1, 6, 22)),
    "cgl-4x3-rand": dict(si=(1, 6, 22), lr=(1, 6, 22), lm=(1, 6, 20)),
}


def test_case_list_is_what_the_gpu_test_runs():
    assert sorted(R.case(c).n for c in A_IDS) == [24, 24, 24, 30, 32]
    assert [R.case(c).hermitian for c in A_IDS] == [True, True, True, False, False]
    assert R.case("sh-8x8x6/eig1/nev3").n == 384 and len(R.B_CASES) == 3
    assert {R.case(c).start for c in A_IDS} == {"random", "upload"}
    assert max(R.case(c).n for c in A_IDS) < 45 <= R.KRYLOVDIM_MAX


def test_library_random_restatement_is_a_uniform_draw():
    x = R.library_random(4096)
    assert x.min() >= 0.0 and x.max() < 1.0 and abs(x.mean() - 0.5) < 0.02 and len(np.unique(x)) == 4096
    assert not np.array_equal(R.library_random(8, seed=1), R.library_random(8, seed=2))
    assert np.array_equal(R.library_random(8, goff=3), R.library_random(11)[3:])


@pytest.mark.parametrize("cid", A_IDS)
def test_a_case_exhausts_the_whole_space(cid):
    c, sp = R.case(cid), R.spectrum(cid)
    lam = np.asarray(sp.lam, dtype=complex)
    sep = np.abs(lam[:, None] - lam[None, :]) + np.diag(np.full(c.n, np.inf))
    # distinct by eight orders more than the rounding of a dense eigensolve (64 n eps |J| ~ 5e-13 |J|)
    assert sep.min() >= 1e-4 * sp.normJ, ("eigenvalues not pairwise distinct", sep.min())
    comp = R.components(cid)
    assert comp.min() >= 1e-4, ("the start vector misses an eigen-direction", comp.min())
    assert R.grade(cid) == c.n
    assert (sp.kappa == 1.0) if c.hermitian else (sp.kappa >= 1.0)
    if c.state == "random":
        assert sp.kappa > 1.5                                 # the non-normal case is non-normal
    # the dense pairs are eigenpairs: true residuals in extended precision at rounding level
    worst = max(R.residual(cid, lam[i], sp.V[:, i]) for i in range(c.n))
    assert worst <= 64 * c.n * R.EPS * sp.kappa * sp.normJ, worst


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("cid", A_IDS)
def test_remainder_ratio_drops_at_step_d_and_not_before(cid, mode):
    n = R.case(cid).n
    x, _ = R.start_vector(cid)
    a = R.arnoldi(R.operator(cid, mode), x, R.KRYLOVDIM_MAX)
    assert a.breakdown == n and a.applied == n, (a.breakdown, a.applied)
    assert min(a.first[:n - 1]) >= 1e-20 and np.nanmin(a.second[:n - 1]) >= 1e-20, (min(a.first[:n - 1]), np.nanmin(a.second[:n - 1]))
    at = a.first[n - 1]
    assert at < R.BREAKDOWN, at
    rec = RATIO_AT_D[cid][mode]
    assert rec / 8 <= at <= 8 * rec, (cid, mode, at, rec)
    # exact pairs after the breakdown: the Ritz values of the n x n Rayleigh quotient are the spectrum, within the mode's bound
    ritz = R.ritz_values(cid, mode, a.H)
    assert R.off_spectrum(cid, mode, ritz) == 0


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("cid", A_IDS)
def test_every_wanted_set_ends_at_a_clear_gap(cid, mode):
    c = R.case(cid)
    grid = R.nev_grid(cid, mode)
    assert grid == NEV_GRID[cid][mode]
    assert len(set(grid)) == 3 and all(abs(a - b) <= 2 for a, b in zip(grid, R.NEV_ASKED(c.n)))
    for nev in grid:
        w = R.wanted(cid, mode, nev)
        assert w.gap >= R.GAP_RATIO, (cid, mode, nev, w.gap)
        assert w.nvals in (nev, nev + 1) and len(w.values) == w.nvals
        if c.hermitian:
            assert w.nvals == nev and np.all(w.values.imag == 0.0)
        key = np.abs(w.values) if mode == "lm" else w.values.real
        assert np.all(np.diff(key) <= 64 * R.EPS * np.abs(key).max())
        # complex values come in whole pairs
        for z in w.values[np.abs(w.values.imag) > 0]:
            assert np.abs(w.values - np.conj(z)).min() <= 64 * R.EPS * abs(z)


def test_group_c_position_nev_splits_a_pair():
    nev = R.pair_split_nev(R.C_CASE)
    w = R.wanted(R.C_CASE, "si", nev)
    assert nev == 3 and w.nvals == nev + 1 and w.gap >= R.GAP_RATIO
    assert np.all(np.abs(w.values.imag) > 0.5)                # u = 0: every eigenvalue is r + lap_k +- i nu
    lam = np.asarray(R.spectrum(R.C_CASE).lam, dtype=complex)
    d = np.sort(np.abs(lam - R.case(R.C_CASE).sigma))
    assert abs(d[nev - 1] - d[nev]) <= 64 * R.EPS * d[nev]      # positions nev and nev + 1 are the two members of one pair


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("cid", A_IDS)
def test_a_solver_that_misses_the_breakdown_returns_ghosts(cid, mode):
    c = R.case(cid)
    x, _ = R.start_vector(cid)
    a = R.arnoldi(R.operator(cid, mode), x, 45, detect=False)
    assert a.breakdown == 0 and a.applied == 45 > c.n                      # check 8 would fail
    ritz = R.ritz_values(cid, mode, a.H)
    assert len(ritz) == 45 > c.n                                           # check 2: more values than the space has dimensions
    assert R.off_spectrum(cid, mode, ritz) >= 45 - c.n                     # check 3: no dense eigenvalue of their own
    lam = np.asarray(R.spectrum(cid).lam, dtype=complex)
    assert np.sum(ritz.real > R.TOL_STABILITY) > np.sum(lam.real > R.TOL_STABILITY)        # check 6: the raw count goes up
    # check 4: the most wanted values of the polluted set are not the wanted set
    nev = R.nev_grid(cid, mode)[1]
    w = R.wanted(cid, mode, nev)
    key = 1.0 / np.abs(ritz - c.sigma) if mode == "si" else (ritz.real if mode == "lr" else np.abs(ritz))
    top = ritz[np.argsort(-key)][:w.nvals]
    _, dist = R.match(top, w.values)
    E, _ = R.bounds(cid, mode, w.values, eta=1e-12)
    assert dist.max() > E.max(), (dist.max(), E.max())


@pytest.mark.parametrize("cid", list(R.B_CASES))
def test_b_start_vector_lies_in_an_invariant_subspace(cid):
    start, nev = R.B_CASES[cid]
    d = {"eigsum6": 6, "eig1": 1}[start]
    assert R.grade(cid) == d
    comp = np.sort(R.components(cid))[::-1]
    assert comp[d] <= 1e-12 * comp[0]                          # invariant to the eigenvectors' accuracy only ...
    x, _ = R.start_vector(cid)
    a = R.arnoldi(R.operator(cid, "si"), x, d + 4)
    assert a.breakdown == 0                                    # ... which is far above the breakdown threshold: no claim on counts
    assert min(a.first[:d - 1], default=1.0) >= 1e-3 and 1e-28 <= a.first[d - 1] <= 1e-18, a.first
    w = R.wanted(cid, "si", nev)
    assert w.gap >= R.GAP_RATIO and w.nvals == nev
    lam = R.spectrum(cid).lam
    near = lam[np.argsort(np.abs(lam - 0.1), kind="stable")]
    assert set(near[:min(d, nev)]) <= set(w.values.real)       # the subspace's values are among the wanted ones
    if start == "eig1":
        assert near[0] in w.values.real and x @ R.spectrum(cid).V[:, np.argmin(np.abs(lam - near[0]))] > 0.999


def test_native_branch_crosses_lstar_between_two_step_points():
    params, counts, br = R.branch_reference()
    ls = R.branch_lstar()
    assert len(params) == R.BRANCH_STEPS + 1 and np.all(np.diff(params) > 0)
    k = int(np.searchsorted(params, ls))
    assert 0 < k < len(params) and params[k - 1] < ls < params[k]
    for p in params:
        assert np.abs(R.branch_spectrum(p)).min() >= 5 * R.TOL_STABILITY, p
    assert counts == [0] * k + [1] * (len(params) - k) and list(br["n_unstable"]) == counts
    assert [sp["step"] for sp in br["specialpoint"]] == [k]
    # the default Krylov dimension of the native branch exceeds the space: max(30, nev + 30) = 36 > 32
    assert max(30, R.BRANCH_NEV + 30) > int(np.prod(R.BRANCH_DIMS))
    # and the nev values nearest sigma hold every unstable one at every point
    for p in params:
        ev = R.branch_spectrum(p)
        near = ev[np.argsort(np.abs(ev - 0.1), kind="stable")]
        assert np.abs(near[R.BRANCH_NEV] - 0.1) >= R.GAP_RATIO * np.abs(near[R.BRANCH_NEV - 1] - 0.1)
        assert np.sum(near[:R.BRANCH_NEV] > R.TOL_STABILITY) == np.sum(ev > R.TOL_STABILITY)
