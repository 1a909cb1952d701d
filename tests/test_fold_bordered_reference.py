"""CPU checks of the restatement tests/minaug_bordered_ref.py -- the fold formulation on the bordered systems that stay regular at
the fold -- against tests/minaug_fold_ref.py (the elimination path), SciPy GMRES and dense matrices.  No device."""
import numpy as np
import pytest

import minaug_bordered_ref as B
import minaug_fold_ref as R
from oracle import operators

EPS = np.finfo(float).eps


def _small(kind):
    rng = np.random.default_rng(3)
    if kind == "sh":
        op, pars = operators.SwiftHohenberg((6, 5), (np.pi, 1.3 * np.pi)), dict(l=-0.2, nu=1.3)
    else:
        op, pars = operators.SwiftHohenberg1D(17, 6.0), dict(lam=-0.7, nu=2.0)
    names = list(pars)
    return op, R.sh_model(op, kind, pars, names[0]), pars, rng


@pytest.mark.parametrize("kind", ["sh", "sh1d"])
def test_border_row_is_minus_w_d2F_v_column_by_column(kind):
    op, model, pars, rng = _small(kind)
    n = op.L1.shape[0]
    x, v, w = (rng.standard_normal(n) for _ in range(3))
    sigx = B.border_row(kind, pars["nu"], x, v, w)
    h, _ = R.sh_polys(kind, pars["nu"], 0)
    for j in range(n):
        e = np.zeros(n)
        e[j] = 1.0
        col = -np.dot(w, model.d2F(x, pars, v, e))
        # three factors multiplied in another order, n - 1 exact zeros added: 4 eps of the one nonzero term
        assert abs(col - sigx[j]) <= 4 * EPS * abs(w[j] * R.horner(h, x[j]) * v[j]), (j, col, sigx[j])


def test_full_fold_matrix_agrees_with_the_elimination_path_off_the_fold():
    """[J dpF; sigma_x' sigma_p] solved directly against x1 - dsig x2 at l = l* + 1e-2, x = 0, a random right-hand side.
    Bound, from the rounding of the two direct solves (backward-stable LU: relative error n eps cond): the full solve carries
    n eps cond(M) |y|; the elimination carries n eps cond(J) on x1 and on x2, and dsig = (rhsp - sx1) / (sp - sx2) passes the
    errors of sx1 = <sigx, x1>, sx2 = <sigx, x2> on with the factor |sigx| / |sp - sx2|, once more into dX through |x2|."""
    op, lstar, a = B.trivial_case((16, 8))
    n = a.size
    pars = dict(l=lstar + 1e-2, nu=1.3)
    model = R.sh_model(op, "sh", pars, "l")
    x = np.zeros(n)
    v, w, _ = R.bordered_vectors(model, x, pars, a, a)
    rng = np.random.default_rng(5)
    rhsu, rhsp = rng.standard_normal(n), float(rng.standard_normal())
    dX1, ds1 = B.fold_linsolve_full(model, x, pars, v, w, rhsu, rhsp, "sh")
    dX2, ds2 = R.fold_linsolve(model, x, pars, v, w, rhsu, rhsp)
    M = B.fold_matrix(model, x, pars, v, w, "sh")
    Jd = model.J(x, pars).toarray()
    sigx, sigp, dpF = B._terms(model, x, pars, v, w, "sh")
    x1, x2 = np.linalg.solve(Jd, rhsu), np.linalg.solve(Jd, dpF)
    den = abs(sigp - np.dot(sigx, x2))
    ny = np.linalg.norm(np.append(dX1, ds1))
    e_full = n * EPS * np.linalg.cond(M) * ny
    e_x = n * EPS * np.linalg.cond(Jd)
    e_ds = np.linalg.norm(sigx) * e_x * (np.linalg.norm(x1) + abs(ds2) * np.linalg.norm(x2)) / den
    e_elim = e_x * (np.linalg.norm(x1) + abs(ds2) * np.linalg.norm(x2)) + e_ds * np.linalg.norm(x2)
    err = max(np.linalg.norm(dX1 - dX2), abs(ds1 - ds2))
    print("full vs elimination:", err, "bound", e_full + e_elim + e_ds, "cond M", np.linalg.cond(M), "cond J", np.linalg.cond(Jd))
    assert err <= e_full + e_elim + e_ds


DISTANCES = [5e-3, 1e-5, 1e-9, 0.0]


@pytest.fixture(scope="module")
def table():
    op, lstar, a = B.trivial_case()
    pl = operators.dct_preconditioner(op.dims, op.ls, 1.0)
    rows = {}
    for d in DISTANCES:
        J = op.J(np.zeros(a.size), lstar + d, 1.3)
        v, sg, info, it = B.bordered_gmres(J, a, a, 0.0, np.zeros(a.size), 1.0, pl)
        row = dict(b_info=info, b_it=it, sigma=sg)
        if d in (1e-5, 0.0):
            _, sinfo, sit, srel = B.singular_gmres(J, a, pl)
            row.update(s_info=sinfo, s_it=sit, s_rel=srel)
        rows[d] = row
        print("l - l* =", d, row)
    return rows


def test_bordered_gmres_converges_where_the_singular_solve_fails(table):
    """SciPy GMRES(40) x 50, rtol 1e-10, Pl = lu(L1 + I), 64 x 64 trivial singular case: the issue's table."""
    for d in (1e-5, 0.0):
        assert table[d]["b_info"] == 0, table[d]
        assert table[d]["s_info"] != 0, table[d]


def test_bordered_gmres_count_does_not_depend_on_the_distance_to_the_fold(table):
    its = [table[d]["b_it"] for d in DISTANCES]
    assert all(table[d]["b_info"] == 0 for d in DISTANCES)
    assert max(its) - min(its) <= 2, its


def _close(rb, rr, what):
    assert rb["converged"] and rr["converged"], (what, rb["residuals"], rr["residuals"])
    # the bounds tests/test_gpu_fold.py holds the device against the restatement with
    assert abs(rb["p"] - rr["p"]) <= 1e-10 * max(1.0, abs(rr["p"])), (what, rb["p"], rr["p"])
    assert np.abs(rb["u"] - rr["u"]).max() <= 1e-8, what


def test_newton_fold_on_the_bordered_path_lands_on_the_trivial_singular_point():
    op, lstar, a = B.trivial_case()
    n = a.size
    model = R.sh_model(op, "sh", dict(l=lstar + 0.005, nu=1.3), "l")
    kw = dict(tol=1e-10, max_iterations=20, normN=lambda z: np.abs(z).max())
    rb = B.newton_fold(model, np.zeros(n), lstar + 0.005, a, a, "sh", **kw)
    rr = R.newton_fold(model, np.zeros(n), lstar + 0.005, a, a, **kw)
    _close(rb, rr, "trivial")
    assert abs(rb["p"] - lstar) <= 1e-10


def test_newton_fold_on_the_bordered_path_lands_on_the_hexagon_fold():
    hb = B.hex_fold_case()
    x0, p0, z0 = B.hex_fold_guess(hb)
    model = R.sh_model(hb["op"], "sh", dict(l=p0, nu=B.NU_HEX), "l")
    kw = dict(tol=1e-9, max_iterations=15, normN=lambda z: np.abs(z).max())
    rb = B.newton_fold(model, x0, p0, z0, z0, "sh", **kw)
    rr = R.newton_fold(model, x0, p0, z0, z0, **kw)
    _close(rb, rr, "hexagon")
    assert np.abs(rb["u"]).max() > 0.5


@pytest.mark.parametrize("shift,alpha1", [(0.0, 1.0), (0.37, 1.0), (0.37, 0.5)])
def test_stencil_free_border_identity_with_dense_matrices(shift, alpha1):
    """alpha0 I + alpha1 [T atil/alpha1; kappa b'/alpha1 (c - alpha0)/alpha1] = diag(Pl^-1, 1) [J + shift, a; kappa b' c] with T built from
    its definition: Pl = L1 + s I, J = -L1 + diag(g), Pl^-1 (shift + J) = -I + Pl^-1 diag(shift + s + g), so T = Pl^-1 diag(.)
    for (alpha0, alpha1) = (-1, 1) -- the pair the device takes in both orders -- and T / alpha1 for any other alpha1."""
    op, model, pars, rng = _small("sh")
    n = op.L1.shape[0]
    s = 1.0
    u = 0.3 * rng.standard_normal(n)
    L1 = op.L1.toarray()
    g = pars["l"] + 2.0 * pars["nu"] * u - 3.0 * u * u
    Jd = -L1 + np.diag(g) + shift * np.eye(n)
    Pinv = np.linalg.inv(L1 + s * np.eye(n))
    alpha0 = -1.0
    T = Pinv @ np.diag(shift + s + g) / alpha1
    a, b = rng.standard_normal(n), rng.standard_normal(n)
    c, kappa = 0.7, 1.0 / n
    lhs, rhs = B.tmode_matrices(T, Jd, Pinv, a, b, c, kappa, alpha0, alpha1)
    z = rng.standard_normal(n + 1)
    # every entry is a sum of at most n + 2 products: n eps of the sums of moduli, through both products Pl^-1 (J z)
    bound = 8 * n * EPS * (np.abs(Pinv) @ (np.abs(Jd) @ np.abs(z[:-1]) + np.abs(a) * abs(z[-1]))).max() + 8 * n * EPS * np.abs(z).max()
    assert np.abs(lhs @ z - rhs @ z).max() <= bound
