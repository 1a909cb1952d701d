"""CPU tests of the dense restatement of the normal form at branch points with 2-d and 3-d kernels (tests/normal_form_nd_ref.py):
it is pinned to the answers the reference's own tests hold for the vector fields Fbp2d and FbpD6 (test/normal_forms/testNF.jl),
to closed forms on the trivial branch of 2-D and 3-D Swift-Hohenberg, to the transformation of its tensors under a rotation of
the kernel basis, and its predictor to the closed-form zeros of the reduced equation.  The GPU tests compare the library against
this restatement.  Also here: the host side of bk_amd.normal_form_nd (record, reduced equation, predictor, argument checks) and
the C boundary of the new entries."""
import json
import os

import numpy as np
import pytest

import minaug_fold_ref as R
import normal_form1d_ref as N1R
import normal_form_nd_ref as M
from oracle import operators

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "normal_form_nd_answers.json")))
EPS = np.finfo(float).eps


# ------------------------------------------------------------------------------------------ 1: the reference's own answers
@pytest.mark.parametrize("ans", GOLD["Fbp2d"]["answers"], ids=lambda a: f"gamma={a['gamma']}")
def test_restatement_reproduces_the_references_answers_for_Fbp2d(ans):
    """testNF.jl:277-285 at mu = 0 with zeta = e1, e2 and zeta* = (1, 0, 1), (0, 1, 0), every assertion at the reference's 1e-10;
    the expected values are the fixture's."""
    g = GOLD["Fbp2d"]
    gamma = ans["gamma"]
    p = dict(g["params"], gamma=gamma)
    model, d3F = M.cubic_model(M.Fbp2d, p, g["lens"])
    nf = M.normal_form_nd(model, d3F, np.array(g["x0"]), model.at(p["mu"]), g["lens"], g["zetas"], g["zeta_stars"])
    tol = g["atol"]
    assert abs(nf["b30"][0, 0, 0, 0] / 6 - ans["b30_0000_over_6"]) <= tol
    assert abs(nf["b30"][0, 0, 1, 1] / 2 - ans["b30_0011_over_2"]) <= tol
    assert abs(nf["b30"][0, 0, 0, 1] / 2 - ans["b30_0001_over_2"]) <= tol
    assert abs(nf["b30"][1, 0, 0, 1] / 2 - ans["b30_1001_over_2"]) <= tol
    assert np.abs(nf["b20"][:, :, 0]).max() <= tol
    assert np.abs(nf["b20"][0] / 2 - np.array(ans["b20_0_over_2"])).max() <= tol
    assert np.abs(nf["b11"] - np.array(ans["b11"])).max() <= tol
    assert np.abs(nf["a01"] - np.array(ans["a01"])).max() <= tol
    assert nf["type"] == "2-d"
    # :271-275: the reduced equation is the vector field on the centre manifold x3 = gamma (x1^3 + x2^2), at mu = 0
    for x in ([0.3, 0.7], [1.0, 0.0], [0.0, 1.0]):
        full = M.Fbp2d(np.array(x + [0.0]), p)[:2] + gamma * np.array([x[0] ** 3 + x[1] ** 2, 0.0])
        assert np.abs(M.reduced_form(nf, np.array(x), 0.0) - full).max() < 1e-9


def test_restatement_reproduces_the_references_answers_for_FbpD6():
    """testNF.jl:344-351: J = 0 at mu = 0, the kernel is the whole space and the border has all three columns."""
    g = GOLD["FbpD6"]
    p = dict(g["params"])
    model, d3F = M.cubic_model(M.FbpD6, p, g["lens"])
    nf = M.normal_form_nd(model, d3F, np.array(g["x0"]), model.at(p["mu"]), g["lens"], g["zetas"])
    tol, ans = g["atol"], g["answers"]
    assert np.all(nf["a01"] == np.array(ans["a01"]))
    assert np.abs(nf["b11"] - np.array(ans["b11"])).max() <= tol
    assert abs(nf["b30"][0, 0, 0, 0] / 6 - ans["b30_0000_over_6"]) <= tol
    assert abs(nf["b30"][0, 0, 1, 1] / 2 - ans["b30_0011_over_2"]) <= tol
    assert abs(nf["b20"][0, 1, 2] - ans["b20_012"]) <= tol
    x0 = np.random.default_rng(0).random(3)
    dp = g["reduced_form_dp"]
    assert np.abs(M.FbpD6(x0, dict(p, mu=dp)) - M.reduced_form(nf, x0, dp)).max() < g["reduced_form_atol"]


def test_biorthonormality_is_checked():
    g = GOLD["Fbp2d"]
    model, d3F = M.cubic_model(M.Fbp2d, dict(g["params"], gamma=0.0), g["lens"])
    with pytest.raises(ValueError, match="biorthonormal"):
        M.normal_form_nd(model, d3F, np.zeros(3), model.at(0.0), "mu", g["zetas"], [[1, 0, 1.0], [1e-6, 1, 0.0]])


# ------------------------------------------------------------------------------------------ 2: closed form on u = 0
def _sh2d():
    g = GOLD["sh2d"]
    dims, ls, nu = tuple(g["dims"]), tuple(np.pi * a for a in g["half_lengths_over_pi"]), g["nu"]
    (l1, z1), (l2, z2) = (M.sh_cos_mode(dims, ls, m) for m in g["modes"])
    op = operators.SwiftHohenberg(dims, ls)
    model = R.sh_model(op, "sh", dict(l=l1, nu=nu), "l")
    return g, dims, ls, nu, l1, l2, z1, z2, op, model, N1R.sh_d3F("sh", ["l", "nu"])


@pytest.fixture(scope="module")
def sh2d():
    g, dims, ls, nu, l1, l2, z1, z2, op, model, d3F = _sh2d()
    nf = M.normal_form_nd(model, d3F, np.zeros(z1.shape[0]), model.at(l1), "l", [z1, z2])
    return dict(g=g, dims=dims, ls=ls, nu=nu, lstar=l1, l2=l2, z=[z1, z2], op=op, model=model, d3F=d3F, nf=nf)


def test_sh_trivial_branch_closed_form_two_modes(sh2d):
    """16 x 16, half-lengths (pi, pi), modes (1, 2) and (2, 1), nu = 1.3 at p = l* exactly: the bordered matrix is regular there."""
    g, nf = sh2d["g"], sh2d["nf"]
    assert sh2d["lstar"] == sh2d["l2"] and abs(sh2d["lstar"] - g["lstar"]) <= 1e-15
    w = np.sort(np.abs(np.linalg.eigvalsh(sh2d["op"].J(np.zeros(256), sh2d["lstar"], sh2d["nu"]).toarray())))
    assert w[0] < 1e-12 and w[1] < 1e-12 and abs(w[2] - g["smallest_abs_eigenvalues"][2]) < 1e-3, w[:3]
    assert np.abs(nf["a01"]).max() == 0.0 and np.abs(nf["a02"]).max() == 0.0
    assert np.abs(nf["b20"]).max() <= 1e-14                      # <zeta^3> = 0: rounding of a sum of 256 terms of size <= 3e-3
    assert np.abs(nf["b11"] - np.eye(2)).max() <= 4 * EPS         # <zeta_i, zeta_j>
    cf = N1R.sh_trivial_closed_form(sh2d["dims"], sh2d["ls"], tuple(g["modes"][0]), sh2d["nu"])
    assert abs(cf["b30"] - g["b30_diag"]) <= 1e-12
    for i in range(2):
        assert abs(nf["b30"][i, i, i, i] / cf["b30"] - 1) <= g["b30_diag_rtol"], (i, nf["b30"][i, i, i, i], cf["b30"])
    for I in ((0, 0, 1, 1), (1, 0, 0, 1)):
        assert abs(nf["b30"][I] - g["b30_cross"]) <= g["b30_cross_atol"], (I, nf["b30"][I])
    assert abs(nf["b30"][0, 0, 0, 1]) <= 1e-13 and abs(nf["b30"][1, 1, 1, 0]) <= 1e-13
    assert nf["type"] == "2-d"


def test_packed_layouts_and_pass_restatements_agree_with_the_tensors(sh2d):
    """The per-point terms the GPU tests sum (dots_terms, rhs_exact, contract_terms) are the tensors of the restatement, at a
    generic state where every coefficient is alive: sums against the packed arrays to the rounding 4 n eps sum |terms|."""
    rng = np.random.default_rng(5)
    op, d3F, nu = sh2d["op"], sh2d["d3F"], sh2d["nu"]
    n = 256
    for lens, ip in (("l", 0), ("nu", 1)):
        model = R.sh_model(op, "sh", dict(l=0.05, nu=nu), lens)
        u = 0.3 * rng.standard_normal(n)
        zs = list(np.linalg.qr(rng.standard_normal((n, 3)))[0].T)
        q = model.at(0.05 if lens == "l" else nu)
        nf = M.normal_form_nd(model, d3F, u, q, lens, zs)
        a01, a02, b11, b20p, b30p = M.pack(nf)
        ta01, tb20, tg = M.dots_terms("sh", nu, ip, u, zs)
        qs = [nf["Psi2"][jk] for jk in M.pairs(3)]
        tb11, ta02, tb30 = M.contract_terms("sh", nu, ip, u, zs, nf["Psi01"], qs)
        close = lambda v, t: abs(v - t.sum()) <= 4 * n * EPS * np.abs(t).sum()
        for i in range(3):
            assert close(a01[i], ta01[i]) and close(a02[i], ta02[i])
            assert all(close(b11[i, j], tb11[i][j]) for j in range(3))
            assert all(close(b20p[i, k], tb20[i][k]) for k in range(6))
            assert all(close(b30p[i, k], tb30[i][k]) for k in range(10))
        assert min(np.abs(v).min() for v in (a01, a02, b11, b20p, b30p)) > 1e-6          # all alive
        for r, e in zip(M.rhs_exact("sh", nu, ip, u, zs, a01, b20p), nf["rhs"]):
            assert np.abs(r - e).max() <= 16 * EPS * (np.abs(e).max() + 1)


# ------------------------------------------------------------------------------------------ 3: basis independence
def test_rotated_basis_gives_the_transformed_tensors(sh2d):
    """The same point in the basis rotated by theta = 0.3, where every entry of b30 is alive.  Both sides come from direct solves
    with the bordered matrix B, backward stable: Psi carries a relative error kappa(B) eps, and it enters b30 linearly.  So the
    two may differ by kappa(B) eps S (|cos| + |sin|)^4 with S the largest sum of absolute per-point terms of a b30 entry."""
    g, nf = sh2d["g"], sh2d["nf"]
    th = g["rotation_theta"]
    Rm = np.array([[np.cos(th), np.sin(th)], [-np.sin(th), np.cos(th)]])
    z1, z2 = sh2d["z"]
    zr = [Rm[i, 0] * z1 + Rm[i, 1] * z2 for i in range(2)]
    model, d3F = sh2d["model"], sh2d["d3F"]
    zero = np.zeros(z1.shape[0])
    nfr = M.normal_form_nd(model, d3F, zero, model.at(sh2d["lstar"]), "l", zr)
    want = M.rotate(nf, Rm)
    kappa = np.linalg.cond(nf["B"].toarray())
    tb30 = M.contract_terms("sh", sh2d["nu"], 0, zero, zr, nfr["Psi01"], [nfr["Psi2"][jk] for jk in M.pairs(2)])[2]
    S = max(np.abs(t).sum() for row in tb30 for t in row)
    tol = kappa * EPS * S * (abs(np.cos(th)) + abs(np.sin(th))) ** 4
    print(f"kappa(B) = {kappa:.3e}, S = {S:.3e}, allowed {tol:.3e}, measured {np.abs(nfr['b30'] - want['b30']).max():.3e}")
    assert np.abs(want["b30"]).min() > 1e-2                                           # every entry alive
    assert np.abs(nfr["b30"] - want["b30"]).max() <= tol
    assert np.abs(nfr["b11"] - want["b11"]).max() <= 8 * EPS and np.abs(nfr["b20"] - want["b20"]).max() <= 1e-14
    assert np.abs(nfr["a01"]).max() == 0.0 and np.abs(nfr["a02"]).max() == 0.0


def test_gmres_bordered_solve_agrees_with_the_direct_one(sh2d):
    """The yardstick of the solver-dependent GPU tolerances: the (n + N) system by SciPy GMRES, left-preconditioned by
    diag((L1 + I)^-1, I) and stopped on the preconditioned residual at reltol, against the direct solve.  A solve stopped at
    |P (b - B x)| <= reltol |P b| is within kappa(P B) reltol of the solution, and b30 is linear in Psi."""
    model, d3F, nf = sh2d["model"], sh2d["d3F"], sh2d["nf"]
    reltol = 1e-10
    Pl = operators.dct_preconditioner(sh2d["dims"], sh2d["ls"], 1.0)
    zero = np.zeros(256)
    gm = M.normal_form_nd(model, d3F, zero, model.at(sh2d["lstar"]), "l", sh2d["z"], solver="gmres", reltol=reltol, Pl=Pl)
    B = nf["B"].toarray()
    PB = np.vstack([np.stack([Pl(B[:256, j]) for j in range(258)], axis=1), B[256:]])
    kappa = np.linalg.cond(PB)
    for jk in M.pairs(2):
        d = np.linalg.norm(gm["Psi2"][jk] - nf["Psi2"][jk]) / np.linalg.norm(nf["Psi2"][jk])
        assert d <= kappa * reltol, (jk, d, kappa)
    assert np.abs(gm["b30"] - nf["b30"]).max() <= 3 * kappa * reltol * np.abs(nf["b30"]).max()


# ------------------------------------------------------------------------------------------ 4: predictor
def _sh3d():
    g = GOLD["sh3d"]
    dims, ls, nu = tuple(g["dims"]), tuple(g["half_lengths"]), g["nu"]
    lz = [M.sh_cos_mode(dims, ls, m) for m in g["modes"]]
    op = operators.SwiftHohenberg(dims, ls)
    model = R.sh_model(op, "sh", dict(l=lz[0][0], nu=nu), "l")
    nf = M.normal_form_nd(model, N1R.sh_d3F("sh", ["l", "nu"]), np.zeros(op.N), model.at(lz[0][0]), "l", [z for _, z in lz])
    return g, lz, nf


@pytest.fixture(scope="module")
def sh3d():
    return _sh3d()


def test_sh_trivial_branch_three_modes(sh3d):
    """8 x 8 x 8, half-lengths 2.5, modes (2,0,0), (0,2,0), (0,0,2), nu = 0.9: one l*, b30 diagonal and cross terms positive."""
    g, lz, nf = sh3d
    assert lz[0][0] == lz[1][0] == lz[2][0]
    assert np.abs(nf["a01"]).max() == 0.0 and np.abs(nf["a02"]).max() == 0.0 and np.abs(nf["b20"]).max() <= 1e-14
    assert np.abs(nf["b11"] - np.eye(3)).max() <= 4 * EPS
    for i in range(3):
        assert abs(nf["b30"][i, i, i, i] - g["b30_diag"]) <= 1e-10
        for j in range(3):
            if j != i:
                assert abs(nf["b30"][i, i, j, j] - g["b30_cross"]) <= 1e-9 and abs(nf["b30"][j, i, i, j] - g["b30_cross"]) <= 1e-9
    assert abs(nf["b30"][0, 0, 1, 2]) <= 1e-15 and abs(nf["b30"][0, 1, 1, 2]) <= 1e-15


def _closed_roots(nf, dp):
    """Zeros of dp x_i + x_i (d x_i^2 / 6 + c sum_{j != i} x_j^2 / 2) = 0 (b11 = I, b30 diagonal d, cross terms c): m non-zero
    coordinates of equal size s, s^2 = -dp / (d / 6 + (m - 1) c / 2)."""
    import itertools
    N = len(nf["a01"])
    d, c = nf["b30"][0, 0, 0, 0], nf["b30"][0, 0, 1, 1]
    out = [np.zeros(N)]
    for m in range(1, N + 1):
        s2 = -dp / (d / 6 + (m - 1) * c / 2)
        if s2 > 0:
            for idx in itertools.combinations(range(N), m):
                for sg in itertools.product((-1, 1), repeat=m):
                    x = np.zeros(N)
                    x[list(idx)] = np.array(sg) * np.sqrt(s2)
                    out.append(x)
    return out


def _match(found, closed):
    """Every found zero is a closed-form one, each once; returns the largest distance."""
    assert len(found) == len(closed), (len(found), len(closed))
    used, worst = set(), 0.0
    for r in found:
        k = int(np.argmin([np.abs(r - c).max() for c in closed]))
        assert k not in used, (r, k)
        used.add(k)
        worst = max(worst, np.abs(r - closed[k]).max())
    return worst


# Defaults (scale = sqrt |dp|, starts at 1 and 2 in those units): the zeros lie at 2.99 (rolls) and 3.81 per coordinate (squares)
# in sh2d and at 26.9, 26.5 and 26.1 per coordinate in sh3d, so no start is on or next to a zero; a step of 1e-5 besides.  Then
# the reference's iteration (scale 1) where its zeros are of order one -- best-case settings: sh2d at dp = 0.1 has its rolls at
# 0.94 next to the first shell, sh3d at 5e-3 its zeros at 1.9 next to the second -- and starts moved onto the zeros (amp_igs).
PRED_CASES = [("sh2d", 0.01, {}), ("sh2d", 1e-5, {}), ("sh3d", 5e-3, {}), ("sh3d", 1e-4, {}),
              ("sh2d", 0.1, dict(scale=1.0)), ("sh3d", 5e-3, dict(scale=1.0)), ("sh3d", 1e-4, dict(scale=1e-2, amp_igs=25.0))]
PRED_IDS = ["sh2d-0.01", "sh2d-1e-5", "sh3d-5e-3", "sh3d-1e-4", "sh2d-0.1-unscaled", "sh3d-5e-3-unscaled", "sh3d-1e-4-starts-on-zeros"]


@pytest.mark.parametrize("name,dp,kw", PRED_CASES, ids=PRED_IDS)
def test_predictor_finds_every_zero_of_the_reduced_equation(name, dp, kw, sh2d, sh3d):
    """Case 2: 1 zero before and 9 after (the trivial one, 4 rolls x^2 = 6 dp / 0.67311 and 4 squares); the 3-D case: 27 before and
    1 after.  Counts, and the amplitudes against the closed-form zeros at 1e-10."""
    nf = sh2d["nf"] if name == "sh2d" else sh3d[2]
    g = GOLD[name]
    pr = M.predictor(nf, dp, **kw)
    assert len(pr["before"]) == g["roots_before"] and len(pr["after"]) == g["roots_after"]
    assert np.all(pr["before"][0] == 0) and np.all(pr["after"][0] == 0)
    assert _match(pr["before"], _closed_roots(nf, -dp)) <= 1e-10
    assert _match(pr["after"], _closed_roots(nf, dp)) <= 1e-10
    if name == "sh2d":
        rolls = [r for r in pr["after"] if np.count_nonzero(np.abs(r) > 1e-8) == 1]
        assert len(rolls) == 4 and all(abs(np.abs(r).max() ** 2 - 6 * dp / 0.67311) <= 1e-5 for r in rolls)


@pytest.mark.parametrize("theta", [0.3, 0.7, 1.1])
def test_predictor_in_a_rotated_basis_with_default_starts(theta, sh2d):
    """Case 2 in the basis rotated by theta, where no zero lies on an axis or a diagonal the starts sit on: the same 1 and 9 zeros,
    the closed-form ones in the rotated coordinates x' = R x."""
    Rm = np.array([[np.cos(theta), np.sin(theta)], [-np.sin(theta), np.cos(theta)]])
    nfr = M.rotate(sh2d["nf"], Rm)
    dp = 0.008
    pr = M.predictor(nfr, dp)
    assert _match(pr["before"], [Rm @ r for r in _closed_roots(sh2d["nf"], -dp)]) <= 1e-10
    assert _match(pr["after"], [Rm @ r for r in _closed_roots(sh2d["nf"], dp)]) <= 1e-10
    assert len(pr["before"]) == 1 and len(pr["after"]) == 9


def test_predictor_start_on_a_deflated_zero_is_not_converged():
    """A start equal to a zero already found (here the trivial one, deflated from the start, and a user start on a found zero):
    the deflation is infinite there; the start is dropped, nothing raises, and the other zeros are found."""
    from bk_amd import normal_form_nd as ND
    nf = dict(a01=np.zeros(2), a02=np.zeros(2), b11=np.eye(2), b20=np.zeros((2, 2, 2)), b30=np.zeros((2, 2, 2, 2)))
    for i in range(2):
        nf["b30"][i, i, i, i] = -6.0                                  # x_i (dp - x_i^2) = 0
    bp = _record(nf, 2)
    igs = [(1e-60, 0.0), (1.0, 0.0), (1.0, 0.0), (0.0, 1.0)]       # |x|^2 = 1e-120 on the trivial zero; (1, 0) twice
    for pr in (ND.predictor(bp, 1.0, igs=igs, scale=1.0), M.predictor(nf, 1.0, igs=igs, scale=1.0)):
        assert _match(pr["after"], [np.zeros(2), np.array([1.0, 0.0]), np.array([0.0, 1.0])]) <= 1e-12
        assert len(pr["before"]) == 1


# ------------------------------------------------------------------------------------------ the library's host side
def _record(nf, N):
    from bk_amd import normal_form_nd as ND
    return ND.NdBranchPoint(x0=None, tau=None, p=0.0, params=[0.0, 1.3], lens="l", zeta=[None] * N, zeta_star=[None] * N,
                            nf=ND.NdBPNormalForm(nf["a01"], nf["a02"], nf["b11"], nf["b20"], nf["b30"]), type=f"{N}-d")


@pytest.mark.parametrize("name,dp,kw", PRED_CASES, ids=PRED_IDS)
def test_library_predictor_and_reduced_form_match_the_restatement(name, dp, kw, sh2d, sh3d):
    """The record's reduced equation against the reference's loops, and the library's predictor against the restatement's: the
    same zeros (as sets: the two evaluate the cubic in different orders, and a Newton path may end at another zero)."""
    from bk_amd import normal_form_nd as ND
    nf = sh2d["nf"] if name == "sh2d" else sh3d[2]
    N = len(nf["a01"])
    bp = _record(nf, N)
    x = np.random.default_rng(1).standard_normal(N)
    ref = M.reduced_form(nf, x, 0.37)
    assert np.abs(bp.reduced_form(x, 0.37) - ref).max() <= 64 * EPS * max(1.0, np.abs(ref).max())
    with pytest.raises(ValueError, match="should match"):
        bp.reduced_form(np.zeros(N + 1), 0.1)
    got, want = ND.predictor(bp, dp, **kw), M.predictor(nf, dp, **kw)
    for side in ("before", "after"):
        assert len(got[side]) == len(want[side]) == GOLD[name]["roots_" + side]
        assert np.all(got[side][0] == 0)
        assert _match(got[side], want[side]) <= 1e-10
    two = ND.predictor(bp, dp, ampfactor=2.0, **kw)
    assert _match(two["before"], [2.0 * r for r in got["before"]]) <= 1e-10


def test_library_packed_layouts_expand_to_the_references_arrays():
    """expand_b20 / expand_b30 put the pair and triple columns at every permutation; a full model checks all of them."""
    from bk_amd import normal_form_nd as ND
    g = GOLD["FbpD6"]
    model, d3F = M.cubic_model(M.FbpD6, dict(g["params"]), g["lens"])
    rng = np.random.default_rng(2)
    Q = np.linalg.qr(rng.standard_normal((3, 3)))[0]
    nf = M.normal_form_nd(model, d3F, np.zeros(3), model.at(0.0), "mu", list(Q.T))
    a01, a02, b11, b20p, b30p = M.pack(nf)
    assert ND.pairs(3) == M.pairs(3) and ND.triples(3) == M.triples(3) and len(ND.pairs(2)) == 3 and len(ND.triples(2)) == 4
    assert np.array_equal(ND.expand_b20(b20p), nf["b20"]) and np.array_equal(ND.expand_b30(b30p), nf["b30"])
    assert np.abs(nf["b30"]).min() > 1e-3
    assert ND.classify_nd(a01, a02, b11, 3) == "3-d" and ND.classify_nd(a01, a02, 1e-4 * b11, 3) == "NonQuadraticParameter"


def test_get_normal_form_nd_checks_its_arguments():
    """ValueError for a point that is not "nd", NotImplementedError for N > 3, TypeError for a problem without the formulation;
    codim2.get_normal_form and continuation_from_branch_point keep raising for "nd" points."""
    from bk_amd import codim2, hip
    from bk_amd import normal_form1d as N1
    from bk_amd import normal_form_nd as ND
    sh = hip.SwiftHohenberg.__new__(hip.SwiftHohenberg)
    cgl = hip.CGL2d.__new__(hip.CGL2d)
    br = type("B", (), dict(specialpoint=[dict(type="bp", n_unstable=(0, 1)), dict(type="nd", n_unstable=(0, 4), step=1),
                                          dict(type="nd", n_unstable=(0, 2), step=1)], sol=[], param=[]))()
    with pytest.raises(ValueError, match="kernel of dimension > 1"):
        ND.get_normal_form_nd(br, 0, sh, None)
    with pytest.raises(NotImplementedError, match="N = 4"):
        ND.get_normal_form_nd(br, 1, sh, None)
    with pytest.raises(TypeError, match="SwiftHohenberg"):
        ND.get_normal_form_nd(br, 2, cgl, None)
    with pytest.raises(NotImplementedError, match="newton_fold"):
        codim2.get_normal_form(br, 2, sh, None)
    with pytest.raises(NotImplementedError, match="multicontinuation"):
        N1.continuation_from_branch_point(br, 2, sh, None, None)


def test_get_normal_form_nd_names_the_count_of_eigenvalues_near_zero():
    """Fewer than N eigenvalues within the stability tolerance (plus ten widths of the bisection interval) of 0: RuntimeError with
    the count; without eigenvectors, or with a wrong number of user vectors: ValueError.  Host logic only, on stand-in vectors."""
    from bk_amd import hip
    from bk_amd import normal_form_nd as ND

    class Vec:
        def __init__(self, a):
            self.a = np.asarray(a, dtype=float)

        def copy(self):
            return Vec(self.a.copy())

        def add_(self, x, a=1.0, b=1.0):
            self.a = b * self.a + a * x.a
            return self

        def norm(self):
            return float(np.linalg.norm(self.a))

        def scale_(self, c):
            self.a *= c
            return self

    sh = hip.SwiftHohenberg.__new__(hip.SwiftHohenberg)
    sh.jacobian = lambda x, p: None
    sp = dict(type="nd", n_unstable=(0, 2), step=1, interval=(0.1 - 1e-9, 0.1 + 1e-9), param=0.1)
    br = type("B", (), dict(specialpoint=[sp], sol=[Vec([0, 0]), Vec([0, 0]), Vec([0, 0])], param=[0.0, 0.1, 0.2]))()
    vecs = [(Vec([1, 0]),), (Vec([0, 1]),), (Vec([1, 1]),), (Vec([1, -1]),)]
    eig = lambda J, nev: (np.array([0.3, 5e-9, -0.2, -0.5]), vecs, True, 1)
    with pytest.raises(RuntimeError, match="returned 1 eigenvalues within"):
        ND.get_normal_form_nd(br, 0, sh, None, eig=eig)
    with pytest.raises(ValueError, match="eigenvectors"):
        ND.get_normal_form_nd(br, 0, sh, None, eig=lambda J, nev: (np.array([1e-9, -1e-9, 1, 2]), None, True, 1))
    with pytest.raises(ValueError, match="3 kernel vectors given"):
        ND.get_normal_form_nd(br, 0, sh, None, zetas=[Vec([1, 0])] * 3)
    with pytest.raises(ValueError, match="eigensolver"):
        ND.get_normal_form_nd(br, 0, sh, None)


# ------------------------------------------------------------------------------------------ 5: the C boundary
def test_library_exports_the_nd_normal_form_entries():
    """The four entries are declared in the header, bound by ctypes and exported by the built library; the ABI version stays."""
    import ctypes
    import re

    from bk_amd import _lib
    names = ["bk_nfnd_dots", "bk_nfnd_rhs", "bk_nfnd_contract", "bk_normal_form_nd"]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "bkhip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in names:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert len(_lib.SIGNATURES["bk_normal_form_nd"][1]) == 15
    assert re.search(r"#define\s+BK_ABI_VERSION\s+6\b", hdr)
