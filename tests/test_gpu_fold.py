"""GPU tests of the minimally augmented fold formulation (bk_d2f, bk_djdp, bk_fold_contract, bk_fold_terms, bk_fold_linsolve,
bk_newton_fold; bk_amd.codim2): the Hessian kernels against NumPy, the fused contraction against an exact sum, d2F against
differences of bk_jacobian, and newton_fold -- native against the call-by-call mirror and the CPU restatement -- at singular
points whose parameter is known in closed form: the symmetry-breaking points of the trivial branch u = 0, where
J = -L1 + l (SH) or L1 + lam (SH1D) is singular exactly when l (-lam) is an eigenvalue of L1 (-L1).  There the fold system
G = (F, sigma) vanishes, so its Newton solve must land on that eigenvalue."""
import math

import numpy as np
import pytest

import minaug_fold_ref as R
from conftest import probe
from oracle import operators

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps


def _lib():
    from bk_amd import codim2, hip
    return codim2, hip


def _ulps(a, b):
    return np.abs(a - b) / np.maximum(np.spacing(np.maximum(np.abs(a), np.abs(b))), np.finfo(float).tiny)


@pytest.mark.parametrize("kind", ["sh", "sh1d"])
def test_d2F_and_dJdp_match_numpy(ctx, kind):
    codim2, hip = _lib()
    rng = np.random.default_rng(1)
    if kind == "sh":
        prob, pars = hip.SwiftHohenberg(ctx, (23, 17), (np.pi, np.pi), l=-0.2, nu=1.3), [-0.2, 1.3]
    else:
        prob, pars = hip.SwiftHohenberg1D(ctx, 391, 6.0, lam=-0.7, nu=2.0), [-0.7, 2.0]
    n = prob.nlocal
    u, a, b = (rng.standard_normal(n) for _ in range(3))
    U, A, B = prob.vec(u), prob.vec(a), prob.vec(b)
    h, _ = R.sh_polys(kind, pars[1], 0)
    got = codim2.d2F(prob, U, pars, A, B).numpy()
    probe("fold.d2F_ulps." + kind, _ulps(got, R.horner(h, u) * a * b).max(), 1.0, tight=0.0)
    for ip in (0, 1):
        _, g = R.sh_polys(kind, pars[1], ip)
        got = codim2.dJdp(prob, U, pars, ip, A).numpy()
        probe(f"fold.dJdp_ulps.{kind}.{ip}", _ulps(got, R.horner(g, u) * a).max(), 1.0, tight=0.0)


@pytest.mark.parametrize("n", [2, 3, 127, 128, 4099, 4100, 65537])
def test_fold_contract_matches_an_exact_sum(ctx, n):
    """s_k = sum w h(u) v X_k and sigma_p = -sum w g(u) v within the summation-rounding bound of the fp64 sum: odd lengths,
    multiples of the 16-byte vector width, m = 0 .. 3."""
    codim2, hip = _lib()
    rng = np.random.default_rng(n)
    prob = hip.SwiftHohenberg1D(ctx, n, 6.0, lam=-0.7, nu=2.0)
    pars = [-0.7, 2.0]
    u, v, w = (rng.standard_normal(n) for _ in range(3))
    Xs = [rng.standard_normal(n) for _ in range(3)]
    U, V, W = prob.vec(u), prob.vec(v), prob.vec(w)
    XV = [prob.vec(x) for x in Xs]
    for ip in (0, 1):
        h, g = R.sh_polys("sh1d", pars[1], ip)
        th = w * v * R.horner(h, u)
        tg = w * v * R.horner(g, u)
        for m in range(4):
            s, sp = codim2.fold_contract(prob, U, pars, ip, V, W, XV[:m])
            for k in range(m):
                t = th * Xs[k]
                bound = 4 * n * EPS * np.abs(t).sum() + 1e-300
                probe(f"fold.contract_rel.n{n}", abs(s[k] - math.fsum(t)) / bound, 1.0)
            bound = 4 * n * EPS * np.abs(tg).sum() + 1e-300
            probe(f"fold.contract_sp_rel.n{n}", abs(sp + math.fsum(tg)) / bound, 1.0)


def test_d2F_matches_differences_of_the_device_jacobian(ctx):
    codim2, hip = _lib()
    rng = np.random.default_rng(5)
    prob = hip.SwiftHohenberg(ctx, (64, 48), (np.pi, 0.75 * np.pi), l=-0.1, nu=1.3)
    pars = [-0.1, 1.3]
    n = prob.nlocal
    u, a, b = 0.3 * rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
    eps = 1e-3
    Jp = prob.jacobian(prob.vec(u + eps * a), -0.1)(prob.vec(b)).numpy()
    Jm = prob.jacobian(prob.vec(u - eps * a), -0.1)(prob.vec(b)).numpy()
    fd = (Jp - Jm) / (2 * eps)
    got = codim2.d2F(prob, prob.vec(u), pars, prob.vec(a), prob.vec(b)).numpy()
    # the stencil parts cancel up to rounding: eps_mach |L1|_inf |b|_inf / eps
    h = 2 * np.pi / 64
    bound = 8 * EPS * (1 + 8 / h**2) ** 2 * np.abs(b).max() / eps
    probe("fold.d2F_vs_jacobian_fd", np.abs(fd - got).max(), bound)


def test_cgl_has_no_fold_formulation(ctx):
    codim2, hip = _lib()
    from bk_amd import _lib as L
    prob = hip.CGL2d(ctx, (8, 8), (1.0, 1.0))
    x = prob.vec(np.zeros(prob.nglobal))
    with pytest.raises(L.BkHipError, match="fold formulation"):
        codim2.d2F(prob, x, prob._pvec(0.5), x, x)


def _trivial_singular_case(ctx, kind):
    """(problem, preconditioner, exact parameter, mode vector) at the symmetry-breaking point of u = 0 nearest the start."""
    codim2, hip = _lib()
    if kind == "sh1d":
        N, l = 200, 6.0
        op = operators.SwiftHohenberg1D(N, l)
        ev, V = np.linalg.eigh(op.L1.toarray())              # L1 = -(I + D)^2 <= 0: J = L1 + lam singular at lam = -ev
        k = np.argmax(ev)
        prob = hip.SwiftHohenberg1D(ctx, N, l, lam=-ev[k] + 0.02, nu=2.0)
        return op, prob, None, -ev[k], V[:, k], [-ev[k] + 0.02, 2.0], ev
    dims, ls = (64, 64), (np.pi, 1.3 * np.pi)                # unequal sides: a simple eigenvalue
    op = operators.SwiftHohenberg(dims, ls)
    # J = -L1 + l with L1 = (I + Lap)^2 diagonal in the DCT-II basis: Lap eigenvalues per axis -(2/h)^2 sin^2(pi k / (2 N))
    lam = [-(2 * n / (2 * L)) ** 2 * np.sin(np.pi * np.arange(n) / (2 * n)) ** 2 for n, L in zip(dims, ls)]
    L1 = (1 + lam[0][:, None] + lam[1][None, :]) ** 2
    i, j = np.unravel_index(np.argmin(L1), L1.shape)
    x = np.cos(np.pi * i * (np.arange(dims[0]) + 0.5) / dims[0])
    y = np.cos(np.pi * j * (np.arange(dims[1]) + 0.5) / dims[1])
    mode = np.outer(y, x).reshape(-1)                          # x fastest
    prob = hip.SwiftHohenberg(ctx, dims, ls, l=L1[i, j] + 0.005, nu=1.3)
    return op, prob, hip.DCTPreconditioner(prob, 1.0), float(L1[i, j]), mode / np.linalg.norm(mode), [L1[i, j] + 0.005, 1.3], None


@pytest.mark.parametrize("kind", ["sh"])
def test_newton_fold_native_mirror_and_restatement_agree_on_an_exact_singular_point(kind):
    """SH 2-D 64 x 64 with Pl = lu(L1 + I) (SH2d-fronts.jl:121).  Native and mirror each run on a fresh context: the GMRES
    solves carry state from one solve to the next (speculation ramp, Newton shifts), so equal iteration counts need equal
    starting states."""
    codim2, hip = _lib()
    ctx = hip.Context(0)
    op, prob, Pl, pstar, mode, pars, spec = _trivial_singular_case(ctx, kind)
    n = prob.nlocal
    rng = np.random.default_rng(7)
    a0 = mode + 0.05 * rng.standard_normal(n)
    a0 /= np.linalg.norm(a0)
    A = prob.vec(a0)
    x0 = prob.vec(np.zeros(n))
    ls = hip.GMRESKrylovKit(dim=40, rtol=1e-10, atol=1e-13, maxiter=50, Pl=Pl)
    kw = dict(tol=1e-10, max_iterations=20, norm_inf=True)
    sn = codim2.newton_fold_native(prob, x0, pars[0], A, A, ls, **kw)
    ctx2 = hip.Context(0)
    _, prob2, Pl2, _, _, _, _ = _trivial_singular_case(ctx2, kind)
    ls2 = hip.GMRESKrylovKit(dim=40, rtol=1e-10, atol=1e-13, maxiter=50, Pl=Pl2)
    A2 = prob2.vec(a0)
    sm = codim2.newton_fold(prob2, prob2.vec(np.zeros(n)), pars[0], A2, A2, ls2, **kw)
    print(kind, "newton_fold: itnewton", sn["itnewton"], "itlinear", sn["itlineartot"], "residuals", sn["residuals"])
    assert sn["converged"] and sm["converged"], (sn["residuals"], sm["residuals"])
    assert sn["itnewton"] == sm["itnewton"]
    # here x stays 0, so only sigma_p enters the step: the fused pass and inner(w, dJdp v) sum -<w, v> in different orders, and the
    # last-bit difference in dsig moves the counts of the bordered solves J \\ a on the ever more singular J by a few iterations
    probe(f"fold.native_vs_mirror_itlinear.{kind}", abs(sn["itlineartot"] - sm["itlineartot"]) / sn["itlineartot"], 2e-3)
    probe(f"fold.native_vs_mirror_p.{kind}", abs(sn["u"].p - sm["u"].p), 1e-12)
    probe(f"fold.native_vs_mirror_x.{kind}", np.abs(sn["u"].u.numpy() - sm["u"].u.numpy()).max(), 1e-12)
    probe(f"fold.p_vs_exact.{kind}", abs(sn["u"].p - pstar), 1e-10)
    # the CPU restatement (sparse direct solves) from the same start
    kind_r = "sh1d" if kind == "sh1d" else "sh"
    names = ["lam", "nu"] if kind == "sh1d" else ["l", "nu"]
    model = R.sh_model(op, kind_r, dict(zip(names, pars)), names[0])
    rr = R.newton_fold(model, np.zeros(n), pars[0], a0, a0, tol=1e-10, max_iterations=20, normN=lambda z: np.abs(z).max())
    assert rr["converged"]
    probe(f"fold.gpu_vs_restatement_p.{kind}", abs(sn["u"].p - rr["p"]), 1e-10)
    probe(f"fold.gpu_vs_restatement_x.{kind}", np.abs(sn["u"].u.numpy() - rr["u"]).max(), 1e-8)
    if spec is not None:
        # independent check: the dense J at the result has an eigenvalue ~ 0, well separated from the next one
        e = np.sort(np.abs(np.linalg.eigvalsh(op.J(sn["u"].u.numpy(), sn["u"].p, 2.0).toarray())))
        probe("fold.min_abs_eig.sh1d", e[0], 1e-8)
        assert e[1] >= 1e4 * e[0], e[:3]


def test_continuation_fold_follows_the_exact_fold_curve_and_the_restatement(ctx):
    """continuation_fold in nu from the singular point of u = 0 (SH 2-D 64 x 64, Pl = lu(L1 + I)): L1 does not depend on nu, so the
    curve is l = l* for every nu.  Three fixed steps; (p1, p2) match the CPU restatement run with the same ds sequence."""
    codim2, hip = _lib()
    from bk_amd import continuation as Cn
    op, prob, Pl, pstar, mode, pars, _ = _trivial_singular_case(ctx, "sh")
    n = prob.nlocal
    a0 = mode + 0.05 * np.random.default_rng(7).standard_normal(n)
    a0 /= np.linalg.norm(a0)
    A = prob.vec(a0)
    ls = hip.GMRESKrylovKit(dim=40, rtol=1e-10, atol=1e-13, maxiter=50, Pl=Pl)
    cp = Cn.ContinuationPar(ds=0.01, dsmax=0.05, p_min=0.5, p_max=2.0, max_steps=3,
                            newton_options=Cn.NewtonPar(tol=1e-10, max_iterations=10))
    dss = [0.01, 0.01, 0.02]
    br = codim2.continuation_fold(prob, hip.BorderedArray(prob.vec(np.zeros(n)), pstar + 1e-4), 1.3, "nu", A, A, ls, cp,
                                  ds_sequence=dss)
    print("continuation_fold: p1", br.p1, "p2", br.p2, "itnewton", br.itnewton, "itlinear", br.itlinear)
    assert len(br.p2) == len(dss) + 1 and all(np.diff(br.p2) > 0)
    probe("fold.curve_p1_vs_exact", max(abs(p - pstar) for p in br.p1), 1e-10)
    model = R.sh_model(op, "sh", dict(l=pars[0], nu=1.3), "l", "nu")
    rr = R.continuation_fold(model, np.zeros(n), pstar + 1e-4, 1.3, a0, a0, ds=0.01, max_steps=3, tol=1e-10, max_iterations=10,
                             ds_sequence=dss)
    probe("fold.curve_vs_restatement_p1", max(abs(a - b) for a, b in zip(br.p1, rr["p1"])), 1e-8)
    probe("fold.curve_vs_restatement_p2", max(abs(a - b) for a, b in zip(br.p2, rr["p2"])), 1e-8)


def test_fold_contract_unaligned_vectors(ctx):
    """Vectors that are not 16-byte aligned take the element-wise instantiation of the contraction kernel."""
    codim2, hip = _lib()
    import torch
    n = 4099
    rng = np.random.default_rng(11)
    prob = hip.SwiftHohenberg1D(ctx, n, 6.0, lam=-0.7, nu=2.0)
    pars = [-0.7, 2.0]
    arrs = [rng.standard_normal(n) for _ in range(6)]

    def shifted(a):                                   # a view starting 8 bytes into a fresh buffer
        t = torch.empty(n + 1, dtype=torch.float64, device=ctx.torch_device)
        t[1:] = torch.from_numpy(a).to(ctx.torch_device)
        return hip.HipVec(ctx, t[1:], n)
    u, v, w, *Xs = arrs
    U, V, W = shifted(u), shifted(v), shifted(w)
    assert U.t.data_ptr() % 16 == 8
    h, g = R.sh_polys("sh1d", pars[1], 1)
    s, sp = codim2.fold_contract(prob, U, pars, 1, V, W, [shifted(x) for x in Xs])
    th, tg = w * v * R.horner(h, u), w * v * R.horner(g, u)
    for k in range(3):
        t = th * Xs[k]
        probe("fold.contract_unaligned_rel", abs(s[k] - math.fsum(t)) / (4 * n * EPS * np.abs(t).sum()), 1.0)
    probe("fold.contract_unaligned_sp_rel", abs(sp + math.fsum(tg)) / (4 * n * EPS * np.abs(tg).sum()), 1.0)


# ------------------------------------------------------------------------------------------ a fold of a nonzero state
NU_HEX = 1.2


@pytest.fixture(scope="module")
def hex_branch():
    """The z-invariant hexagons of the bench cell (tests/golden/bench_cell_states.npz: l = 0.1, nu = 1.2, examples/SH3d.jl:127)
    as a 2-D field reflected once in y -- 64 x 64 on (2 pi, 4 pi / sqrt 3), so the fused LDS transform kernels run -- continued
    in l by the CPU oracle (PALC, sparse direct solves) past the first fold of the hexagon branch (l ~ -0.174)."""
    import os
    from oracle import bordered, palc
    d = np.load(os.path.join(os.path.dirname(__file__), "golden", "bench_cell_states.npz"))
    cx, cy, cz = (int(c) for c in d["cell"])
    u2 = d["u0"].reshape(cz, cy, cx)[0]
    u = np.concatenate([u2, u2[::-1]], axis=0).reshape(-1)
    dims, ls = (cx, 2 * cy), (float(d["cell_l"][0]), 2 * float(d["cell_l"][1]))
    op = operators.SwiftHohenberg(dims, ls)
    prob = palc.Problem(lambda x, p: op.F(x, p, NU_HEX), lambda x, p: op.J(x, p, NU_HEX), dparam_factor=lambda x, p: x)
    bls = lambda *a, **k: bordered.bordering_bls(bordered.default_ls, *a, check_precision=False, **k)
    kw = dict(ls=bordered.default_ls, bls=bls, dsmin=1e-5, p_min=-1.0, p_max=1.0, keep_solutions=True, normC=palc.norminf,
              tol=1e-11)
    br = palc.continuation(prob, u, float(d["p0"]), ds=-0.01, dsmax=0.02, max_steps=20, **kw)
    dp = np.diff(br.param)
    k = [i for i in range(len(dp) - 1) if dp[i] * dp[i + 1] < 0][0] + 1             # middle point of the turn
    # fine-step branch through the turn, from two points before it: the independent turning-point check
    fine = palc.continuation(prob, br.sol[k - 2], br.param[k - 2], ds=-0.002, dsmax=0.002, max_steps=30, **kw)
    return dict(op=op, dims=dims, ls=ls, br=br, k=k, fine=fine, palc=palc)


def _turning_point(fine, palc):
    """p at the turn of the fine branch: the vertex of the quadratic through the three points around the sign change of the
    parameter increment, against the arclength (theta-norm, theta = 0.5) accumulated along the branch."""
    p = np.array(fine.param)
    s = np.concatenate([[0.0], np.cumsum([palc.norm_theta(fine.sol[i + 1] - fine.sol[i], p[i + 1] - p[i], 0.5)
                                          for i in range(len(p) - 1)])])
    dp = np.diff(p)
    i = [j for j in range(len(dp) - 1) if dp[j] * dp[j + 1] < 0][0]
    c = np.polyfit(s[i:i + 3], p[i:i + 3], 2)
    return float(np.polyval(c, -c[1] / (2 * c[0])))


def _eig_near_zero(op, x, l, nu):
    import scipy.sparse.linalg as spla
    e = np.sort(np.abs(spla.eigsh(op.J(x, l, nu).tocsc(), k=3, sigma=0.0, which="LM", return_eigenvectors=False)))
    return e


def _hex_problem(hip, hb, ctx):
    prob = hip.SwiftHohenberg(ctx, hb["dims"], hb["ls"], l=hb["br"].param[hb["k"]], nu=NU_HEX)
    Pl = hip.DCTPreconditioner(prob, 1.0)                  # Pl = lu(L1 + I), examples/SH2d-fronts.jl:121
    return prob, hip.GMRESKrylovKit(dim=40, rtol=1e-10, atol=1e-13, maxiter=200, Pl=Pl)


def _fold_guess(codim2, hb, prob):
    """fold_point on a Python branch record holding the oracle's states: continuation.locate_fold flags the turn."""
    from bk_amd import continuation as Cn
    rec, cp = Cn.ContResult(), Cn.ContinuationPar(detect_bifurcation=0)
    for p, x in zip(hb["br"].param, hb["br"].sol):
        Cn.locate_fold(rec, cp, p)
        rec.param.append(p)
        rec.sol.append(prob.vec(x))
    assert len(rec.specialpoint) == 1 and rec.specialpoint[0]["idx"] == hb["k"]
    return codim2.fold_point(rec, 0)


def test_newton_fold_refines_the_hexagon_fold(hex_branch):
    """SH 2-D fold of a nonzero state: native and mirror (each on a fresh context, so that their GMRES solves start from the same
    solver state), the CPU restatement with sparse direct bordered solves, the spectrum of J and the turn of a fine-step branch."""
    codim2, hip = _lib()
    hb = hex_branch
    out = {}
    for name, fn in (("native", codim2.newton_fold_native), ("mirror", codim2.newton_fold)):
        c = hip.Context(0)
        prob, ls = _hex_problem(hip, hb, c)
        guess, zeta = _fold_guess(codim2, hb, prob)
        out[name] = fn(prob, guess.u, guess.p, zeta, zeta, ls, tol=1e-9, max_iterations=15, norm_inf=True)
        out[name]["x"] = out[name]["u"].u.numpy()
        if name == "native":
            g0, z0 = guess.u.numpy(), zeta.numpy()
    sn, sm = out["native"], out["mirror"]
    print("hexagon fold: native itnewton", sn["itnewton"], "itlinear", sn["itlineartot"], "residuals", sn["residuals"],
          "| mirror itlinear", sm["itlineartot"], "| unconverged solves", sn["unconverged_solves"], sm["unconverged_solves"])
    assert sn["converged"] and sm["converged"], (sn["residuals"], sm["residuals"])
    # J is singular at the fold by construction (MinAugFold.jl:149): measured, 3 of the 7 solve calls (a bordered-vector solve per
    # point, the pair J \\ F, J \\ dpF per step) stop at maxiter without reaching rtol, yet Newton converges quadratically and
    # lands on the restatement's fold.  Both paths must see the same number, and it is recorded.
    probe("fold.hex.unconverged_solves", sn["unconverged_solves"], 7)
    assert sn["unconverged_solves"] == sm["unconverged_solves"]
    assert sn["itnewton"] == sm["itnewton"]
    assert np.abs(sn["x"]).max() > 0.5                                        # a patterned state, not u = 0
    # the capped solves make the counts rounding-sensitive (fused sums vs d2F + inner): measured 4.3e-3
    probe("fold.hex.native_vs_mirror_itlinear", abs(sn["itlineartot"] - sm["itlineartot"]) / sn["itlineartot"], 1e-2)
    probe("fold.hex.native_vs_mirror_p", abs(sn["u"].p - sm["u"].p) / abs(sn["u"].p), 1e-12)          # measured 0
    probe("fold.hex.native_vs_mirror_x", np.abs(sn["x"] - sm["x"]).max(), 1e-12)                    # measured 2e-16
    model = R.sh_model(hb["op"], "sh", dict(l=hb["br"].param[hb["k"]], nu=NU_HEX), "l")
    rr = R.newton_fold(model, g0, hb["br"].param[hb["k"]], z0, z0, tol=1e-9, max_iterations=15,
                       normN=lambda z: np.abs(z).max())
    assert rr["converged"], rr["residuals"]
    probe("fold.hex.gpu_vs_restatement_p", abs(sn["u"].p - rr["p"]) / abs(rr["p"]), 1e-10)
    probe("fold.hex.gpu_vs_restatement_x", np.abs(sn["x"] - rr["u"]).max(), 1e-8)
    e = _eig_near_zero(hb["op"], sn["x"], sn["u"].p, NU_HEX)
    print("hexagon fold: |eig| nearest 0", e, "p", sn["u"].p)
    probe("fold.hex.min_abs_eig", e[0], 1e-7)
    assert e[1] >= 1e4 * e[0], e
    pt = _turning_point(hb["fine"], hb["palc"])
    probe("fold.hex.p_vs_turning_point", abs(sn["u"].p - pt), 1e-6)


def test_continuation_fold_of_the_hexagon_fold_in_nu(hex_branch):
    """continuation_fold in nu (SH2d-fronts.jl:105) from the hexagon fold: three fixed steps, (p1, p2) against the restatement run
    with the same ds sequence, and every point independently a fold of J (sparse shift-invert at 0)."""
    codim2, hip = _lib()
    from bk_amd import continuation as Cn
    hb = hex_branch
    c = hip.Context(0)
    prob, ls = _hex_problem(hip, hb, c)
    guess, zeta = _fold_guess(codim2, hb, prob)
    sn = codim2.newton_fold_native(prob, guess.u, guess.p, zeta, zeta, ls, tol=1e-9, max_iterations=15, norm_inf=True)
    assert sn["converged"]
    b = sn["v"].copy().scale_(1.0 / sn["v"].norm())
    dss = [0.01, 0.01, 0.01]
    cp = Cn.ContinuationPar(ds=0.01, dsmax=0.05, p_min=0.5, p_max=2.0, max_steps=3,
                            newton_options=Cn.NewtonPar(tol=1e-9, max_iterations=10))
    x0 = sn["u"].u.numpy()
    br = codim2.continuation_fold(prob, sn["u"], NU_HEX, "nu", b, b, ls, cp, save_sol=True, ds_sequence=dss)
    print("hexagon fold curve: l", br.p1, "nu", br.p2, "itnewton", br.itnewton, "itlinear", br.itlinear)
    assert len(br.p2) == len(dss) + 1 and all(np.diff(br.p2) > 0)
    assert abs(br.p1[-1] - br.p1[0]) > 1e-3                                   # the fold moves with nu
    model = R.sh_model(hb["op"], "sh", dict(l=sn["u"].p, nu=NU_HEX), "l", "nu")
    bn = b.numpy()
    rr = R.continuation_fold(model, x0, sn["u"].p, NU_HEX, bn, bn, ds=0.01, max_steps=3, tol=1e-9, max_iterations=10,
                             ds_sequence=dss)
    probe("fold.hex_curve_vs_restatement_p1", max(abs(a - q) for a, q in zip(br.p1, rr["p1"])), 1e-8)
    probe("fold.hex_curve_vs_restatement_p2", max(abs(a - q) for a, q in zip(br.p2, rr["p2"])), 1e-8)
    for z in br.sol:
        e = _eig_near_zero(hb["op"], z.u.u.numpy(), z.u.p, z.p)
        probe("fold.hex_curve_min_abs_eig", e[0], 1e-7)
        assert e[1] >= 1e4 * e[0], e
