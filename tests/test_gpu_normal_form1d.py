"""GPU tests of the normal form at simple branch points and folds of the Swift-Hohenberg problems (bk_d3f, bk_nf1d_dots,
bk_nf1d_rhs, bk_nf1d_contract, bk_nf1d_predict, bk_normal_form_1d; bk_amd.normal_form1d): the pointwise and fused passes against
NumPy and exact sums, the normal form -- native against the call-by-call mirror, a closed form and the dense restatement
(tests/normal_form1d_ref.py) -- on the trivial branch and at the hexagon fold, and detect -> normal form -> predictor -> second
branch end to end.

Tolerances of the solver-dependent comparisons follow DESIGN section 9e: the yardstick is the restatement's own spread at the
same point, its direct bordered solve against BorderingBLS with SciPy GMRES at the test's reltol; 10 x that spread is allowed,
plus the rounding 4 n eps sum |terms| of a coefficient's fixed-order sum and, on the trivial branch, 10 x the restatement's own
measured distance from the closed form (the two CPU solvers share one rounded J; the closed form does not).  Every bound is logged next to its measured value by ``probe``."""
import math
import os

import numpy as np
import pytest

import minaug_fold_ref as R
import normal_form1d_ref as N
from conftest import probe
from oracle import operators

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
LENGTHS = [2, 3, 127, 128, 4099, 4100, 65537]


def _lib():
    from bk_amd import codim2, hip
    from bk_amd import normal_form1d as N1
    return codim2, hip, N1


def _ulps(a, b):
    return np.abs(a - b) / np.maximum(np.spacing(np.maximum(np.abs(a), np.abs(b))), np.finfo(float).tiny)


def _polys(kind, nu, ip):
    h, g = R.sh_polys(kind, nu, ip)
    return h, g, N.sh_d3_poly(kind, nu), N.sh_dp_poly(kind, ip)


def _dots_terms(kind, nu, ip, u, z, zs):
    """The per-point terms of bk_nf1d_dots in the kernel's operation order: (a01, b20, <zeta, zeta*>)."""
    h, g, t, f = _polys(kind, nu, ip)
    return R.horner(f, u) * zs, ((R.horner(h, u) * z) * z) * zs, z * zs


def _contract_terms(kind, nu, ip, u, z, zs, p, q):
    """... of bk_nf1d_contract: (b11, a02, b30)."""
    h, g, t, f = _polys(kind, nu, ip)
    H, G, T = R.horner(h, u), R.horner(g, u), R.horner(t, u)
    hz = H * z
    return (G * z + hz * p) * zs, (2.0 * (G * p) + (H * p) * p) * zs, (((T * z) * z) * z + 3.0 * (hz * q)) * zs


def _shifted(hip, ctx, a):
    """A device vector starting 8 bytes into a fresh buffer: the element-wise instantiations of the kernels."""
    import torch
    n = a.shape[0]
    t = torch.empty(n + 1, dtype=torch.float64, device=ctx.torch_device)
    t[1:] = torch.from_numpy(a).to(ctx.torch_device)
    v = hip.HipVec(ctx, t[1:], n)
    assert v.t.data_ptr() % 16 == 8
    return v


# ------------------------------------------------------------------------------------------ 1: pointwise d3F
@pytest.mark.parametrize("kind", ["sh", "sh1d"])
def test_d3F_matches_numpy(ctx, kind):
    codim2, hip, N1 = _lib()
    rng = np.random.default_rng(2)
    if kind == "sh":
        prob, pars = hip.SwiftHohenberg(ctx, (23, 17), (np.pi, np.pi), l=-0.2, nu=1.3), [-0.2, 1.3]
    else:
        prob, pars = hip.SwiftHohenberg1D(ctx, 391, 6.0, lam=-0.7, nu=2.0), [-0.7, 2.0]
    n = prob.nlocal
    u, a, b, c = (rng.standard_normal(n) for _ in range(4))
    got = N1.d3F(prob, prob.vec(u), pars, prob.vec(a), prob.vec(b), prob.vec(c)).numpy()
    ref = ((R.horner(N.sh_d3_poly(kind, pars[1]), u) * a) * b) * c
    probe("nf1d.d3F_ulps." + kind, _ulps(got, ref).max(), 1.0, tight=0.0)


# ------------------------------------------------------------------------------------------ 2: the reducing passes
@pytest.mark.parametrize("n", LENGTHS)
def test_reducing_passes_match_exact_sums(ctx, n):
    """bk_nf1d_dots and bk_nf1d_contract within the summation-rounding bound 4 n eps sum |terms| of an fp64 sum of n terms: odd
    lengths and multiples of the vector width, both parameters, zeta* the same vector as zeta and a separate one."""
    codim2, hip, N1 = _lib()
    rng = np.random.default_rng(n)
    prob = hip.SwiftHohenberg1D(ctx, n, 6.0, lam=-0.7, nu=2.0)
    pars = [-0.7, 2.0]
    u, z, zs, p, q = (rng.standard_normal(n) for _ in range(5))
    U, Z, ZS, P, Q = (prob.vec(a) for a in (u, z, zs, p, q))
    for ip in (0, 1):
        for alias in (True, False):
            s_np, S = (z, Z) if alias else (zs, ZS)
            got = N1.nf1d_dots(prob, U, pars, ip, Z, S)
            for name, g, t in zip(("a01", "b20", "zz"), got, _dots_terms("sh1d", pars[1], ip, u, z, s_np)):
                probe(f"nf1d.dots_{name}_rel.n{n}", abs(g - math.fsum(t)) / (4 * n * EPS * np.abs(t).sum() + 1e-300), 1.0)
            got = N1.nf1d_contract(prob, U, pars, ip, Z, S, P, Q)
            for name, g, t in zip(("b11", "a02", "b30"), got, _contract_terms("sh1d", pars[1], ip, u, z, s_np, p, q)):
                probe(f"nf1d.contract_{name}_rel.n{n}", abs(g - math.fsum(t)) / (4 * n * EPS * np.abs(t).sum() + 1e-300), 1.0)


def test_reducing_passes_unaligned_vectors(ctx):
    """Streams that are not 16-byte aligned take the element-wise instantiation."""
    codim2, hip, N1 = _lib()
    prob = hip.SwiftHohenberg1D(ctx, 4099, 6.0, lam=-0.7, nu=2.0)
    n, pars = 4099, [-0.7, 2.0]
    rng = np.random.default_rng(12)
    u, z, zs, p, q = (rng.standard_normal(n) for _ in range(5))
    U, Z, ZS, P, Q = (_shifted(hip, ctx, a) for a in (u, z, zs, p, q))
    for ip in (0, 1):
        got = N1.nf1d_dots(prob, U, pars, ip, Z, ZS)
        for g, t in zip(got, _dots_terms("sh1d", pars[1], ip, u, z, zs)):
            probe("nf1d.dots_unaligned_rel", abs(g - math.fsum(t)) / (4 * n * EPS * np.abs(t).sum()), 1.0)
        got = N1.nf1d_contract(prob, U, pars, ip, Z, ZS, P, Q)
        for g, t in zip(got, _contract_terms("sh1d", pars[1], ip, u, z, zs, p, q)):
            probe("nf1d.contract_unaligned_rel", abs(g - math.fsum(t)) / (4 * n * EPS * np.abs(t).sum()), 1.0)
        # mixed: one misaligned stream is enough to leave the vector path
        got = N1.nf1d_contract(prob, prob.vec(u), pars, ip, prob.vec(z), prob.vec(zs), P, prob.vec(q))
        for g, t in zip(got, _contract_terms("sh1d", pars[1], ip, u, z, zs, p, q)):
            probe("nf1d.contract_mixed_alignment_rel", abs(g - math.fsum(t)) / (4 * n * EPS * np.abs(t).sum()), 1.0)


# ------------------------------------------------------------------------------------------ 3: the writing passes
@pytest.mark.parametrize("n", [3, 128, 4099, 65537])
def test_rhs_and_predict_match_numpy_elementwise(ctx, n):
    """bk_nf1d_rhs and bk_nf1d_predict have no reductions.  r1 = a01 z - f(u): Horner (<= 6 roundings on |f| terms), one product
    and one subtraction -- at most 8 eps (|a01 z| + |f(u)|) even if NumPy ordered the operations differently; r2 = b20 z - (h z) z:
    two more products, 10 eps (|b20 z| + |h z z|); out = ((x0 + a z) + b p) + c t: three products, three sums, 6 eps of the sum of
    the magnitudes.  Aligned and misaligned streams, every output count."""
    codim2, hip, N1 = _lib()
    rng = np.random.default_rng(100 + n)
    prob = hip.SwiftHohenberg1D(ctx, n, 6.0, lam=-0.7, nu=2.0)
    pars = [-0.7, 2.0]
    u, z, p, t = (rng.standard_normal(n) for _ in range(4))
    a01, b20 = 0.37, -1.9
    for mk in (prob.vec, lambda a: _shifted(hip, ctx, a)):
        U, Z, P, T = mk(u), mk(z), mk(p), mk(t)
        for ip in (0, 1):
            h, g, d3, f = _polys("sh1d", pars[1], ip)
            r1, r2 = N1.nf1d_rhs(prob, U, pars, ip, Z, a01, b20)
            e1, e2 = a01 * z - R.horner(f, u), b20 * z - (R.horner(h, u) * z) * z
            b1 = 8 * EPS * (np.abs(a01 * z) + np.abs(R.horner(np.abs(f), np.abs(u))))
            b2 = 10 * EPS * (np.abs(b20 * z) + np.abs(R.horner(np.abs(h), np.abs(u)) * z * z))
            probe(f"nf1d.rhs_r1.n{n}", (np.abs(r1.numpy() - e1) / b1).max(), 1.0, tight=0.0)
            probe(f"nf1d.rhs_r2.n{n}", (np.abs(r2.numpy() - e2) / b2).max(), 1.0, tight=0.0)
        coefs = [(0.7, -0.3, 1.1), (-0.7, 0.3, 0.0), (0.0, 2.5, -0.2), (1e-3, 0.0, 0.0)]
        for m in (1, 2, 3, 4):
            outs = N1.nf1d_predict(U, Z, P, T, coefs[:m])
            for (a, b, c), o in zip(coefs, outs):
                ref = ((u + a * z) + b * p) + c * t
                bound = 6 * EPS * (np.abs(u) + np.abs(a * z) + np.abs(b * p) + np.abs(c * t))
                probe(f"nf1d.predict.n{n}.m{m}", (np.abs(o.numpy() - ref) / bound).max(), 1.0, tight=0.0)
        (o,) = N1.nf1d_predict(U, Z, None, None, [(0.25, 0.0, 0.0)])            # absent streams are not read
        probe(f"nf1d.predict_two_streams.n{n}", (np.abs(o.numpy() - (u + 0.25 * z)) / (6 * EPS * (np.abs(u) + np.abs(0.25 * z)))).max(),
              1.0, tight=0.0)


# ------------------------------------------------------------------------------------------ 4: closed form, trivial branch
BOX = (2.0, 2.54)           # half-lengths: mode (1, 1) is the first to go unstable, l* ~ 1e-4, the next mode 0.14 away
NU = 1.3
RELTOL = 1e-10


def _solver(hip, prob, maxiter=50):
    return hip.GMRESKrylovKit(dim=40, rtol=RELTOL, atol=1e-13, maxiter=maxiter, Pl=hip.DCTPreconditioner(prob, 1.0))


def _closed_form_at(dims, p):
    """The closed form of normal_form1d_ref.sh_trivial_closed_form at the parameter p next to l*: zeta stays an eigenvector of
    J(p) = -L1 + p, so the bordered solves keep their closed form with lam_ab = p - (1 + mu_a + mu_b)^2."""
    cf = N.sh_trivial_closed_form(dims, BOX, (1, 1), NU)
    nx, ny = dims
    mu = N.sh_trivial_mode(dims, BOX, (1, 1))[2]
    xs, ys = (np.arange(nx) + 0.5) / nx, (np.arange(ny) + 0.5) / ny
    psi, s, w = np.zeros(nx * ny), 0.0, 1.0 / (nx * ny)
    for a, b in ((0, 0), (2, 0), (0, 2), (2, 2)):
        phi = np.outer(np.cos(np.pi * b * ys), np.cos(np.pi * a * xs)).reshape(-1)
        lam = p - (1 + mu[0][a] + mu[1][b]) ** 2
        psi += -2 * NU * w * phi / lam
        s += w * w * float(np.dot(phi, phi)) / lam
    cf.update(Psi20=psi, b30=-6.0 * 9.0 / (4.0 * nx * ny) - 12.0 * NU * NU * s)
    return cf


def _sum_rounding(kind, nu, ip, u, z, lu):
    """The rounding of the fixed-order sums themselves, 4 n eps sum |terms| per coefficient (the bound of test 2), evaluated on
    the restatement's vectors: what two exact solvers may still differ by in a coefficient."""
    n = z.shape[0]
    d = [4 * n * EPS * np.abs(t_).sum() for t_ in _dots_terms(kind, nu, ip, u, z, z)]
    c = [4 * n * EPS * np.abs(t_).sum() for t_ in _contract_terms(kind, nu, ip, u, z, z, lu["Psi01"], lu["Psi20"])]
    return dict(a01=d[0], b20=d[1], b11=c[0], a02=c[1], b30=c[2], Psi01=0.0, Psi20=0.0)


def _against_closed_form(lu, cf, zero):
    """10 x |dense restatement - closed form| per quantity: the second measured yardstick on the trivial branch.  Both solvers of
    _spread apply the same rounded matrix, so their spread is blind to the rounding of J itself; the closed form is not."""
    al = {k: 10 * abs(lu[k] - cf[k]) for k in ("a01", "a02", "b11", "b20", "b30")}
    al.update(Psi01=10 * np.abs(lu["Psi01"]).max(), Psi20=10 * np.abs(lu["Psi20"] - cf["Psi20"]).max())
    return al


def _few_ulp(name, a, b):
    """Native against mirror: the same kernels and solves in the same order, so equality up to a few ulp (measured: equal)."""
    probe(name, abs(a - b), 8 * EPS * max(abs(a), abs(b)), tight=0.0)


def _spread(model, d3F, op, x, q, lens, z, lu, Pl):
    """10 x |BorderingBLS with SciPy GMRES at RELTOL - direct bordered solve| of the restatement at this point, per quantity."""
    gm = N.normal_form1d(model, d3F, x, q, lens, z, z, solver="bordering", reltol=RELTOL, Pl=Pl)
    al = {k: 10 * abs(gm[k] - lu[k]) for k in ("a01", "a02", "b11", "b20", "b30")}
    al.update({k: 10 * np.abs(gm[k] - lu[k]).max() for k in ("Psi01", "Psi20")})
    return al


@pytest.mark.parametrize("dims", [(64, 64), (45, 27)], ids=["64x64-fused", "45x27-odd"])
def test_normal_form_on_the_trivial_branch_matches_the_closed_form(dims):
    """u = 0 of 2-D SH next to the first symmetry-breaking point (p = l* + 1e-8, as a bisection leaves it), zeta = the cosine mode
    (1, 1).  Native and mirror on fresh contexts against the closed form, and against each other to a few ulp.  Allowed against
    the closed form: 10 x the restatement's spread, plus 10 x the restatement's own distance from the closed form (measured here,
    6.4e-10 relative in b30 at 64 x 64), plus the rounding 4 n eps sum |terms| of the fixed-order sums."""
    codim2, hip, N1 = _lib()
    n = dims[0] * dims[1]
    lstar, z, mu = N.sh_trivial_mode(dims, BOX, (1, 1))
    p = lstar + 1e-8
    cf = _closed_form_at(dims, p)
    L1 = (1 + mu[0][:dims[0], None] + mu[1][None, :dims[1]]) ** 2
    gap = np.sort(np.abs(lstar - L1).ravel())
    assert gap[0] == 0.0 and gap[1] > 0.1, gap[:3]                              # simple, well separated
    op = operators.SwiftHohenberg(dims, BOX)
    model = R.sh_model(op, "sh", dict(l=p, nu=NU), "l")
    d3F = N.sh_d3F("sh", ["l", "nu"])
    zero = np.zeros(n)
    lu = N.normal_form1d(model, d3F, zero, model.at(p), "l", z, z)
    allowed = _spread(model, d3F, op, zero, model.at(p), "l", z, lu, operators.dct_preconditioner(dims, BOX, 1.0))
    acf = _against_closed_form(lu, cf, zero)
    rnd = _sum_rounding("sh", NU, 0, zero, z, dict(Psi01=zero, Psi20=cf["Psi20"]))
    allowed = {k: allowed[k] + acf[k] + rnd[k] for k in allowed}
    print(f"{dims}: l* = {lstar:.6e}, closed-form b30 = {cf['b30']:.15g}, restatement - closed form x 10 {acf}, allowed {allowed}")
    out = {}
    for kind in ("native", "mirror"):
        ctx = hip.Context(0)
        prob = hip.SwiftHohenberg(ctx, dims, BOX, l=p, nu=NU)
        ls = _solver(hip, prob)
        Z = prob.vec(z)
        f = N1.normal_form1d_native if kind == "native" else N1.normal_form1d
        out[kind] = bp = f(prob, prob.vec(zero), p, Z, Z, ls)
        nf = bp.nf
        print(f"{kind}: a01 {nf.a01:.3e} a02 {nf.a02:.3e} b11 {nf.b11:.15g} b20 {nf.b20:.3e} b30 {nf.b30:.15g} type {bp.type} "
              f"converged {bp.converged} itlinear {bp.itlinear}")
        assert bp.type == "Pitchfork" and nf.b11 * nf.b30 > 0                           # subcritical
        for k in ("a01", "a02", "b11", "b20", "b30"):
            probe(f"nf1d.trivial_{k}.{kind}.{dims[0]}", abs(getattr(nf, k) - cf[k]), allowed[k])
        probe(f"nf1d.trivial_Psi20.{kind}.{dims[0]}", np.abs(nf.Psi20.numpy() - cf["Psi20"]).max(), allowed["Psi20"],
              relative=np.abs(nf.Psi20.numpy() - cf["Psi20"]).max() / np.abs(cf["Psi20"]).max())
        probe(f"nf1d.trivial_Psi01.{kind}.{dims[0]}", np.abs(nf.Psi01.numpy()).max(), allowed["Psi01"])
        # J \ zeta* has the solution zeta / 1e-8: its residual cannot be evaluated to reltol in fp64 (eps |x| ~ 2e-8 |zeta|), so that
        # ONE solve may come back unconverged -- a flag, and the elimination removes the zeta component it is made of
        if kind == "native":
            probe(f"nf1d.trivial_unconverged_solves.{dims[0]}", bp.unconverged_solves, 1)
        assert bp.p == p and bp.lens == "l" and bp.params == [p, NU]
        ctx.close()
    na, mi = out["native"].nf, out["mirror"].nf
    for k in ("a01", "a02", "b11", "b20", "b30"):
        _few_ulp(f"nf1d.trivial_native_vs_mirror_{k}.{dims[0]}", getattr(na, k), getattr(mi, k))


# ------------------------------------------------------------------------------------------ 5: the hexagon fold
NU_HEX = 1.2


@pytest.fixture(scope="module")
def hex_branch():
    """The setup of tests/test_gpu_fold.py: the z-invariant hexagons of the bench cell as a 2-D field reflected once in y (64 x 64),
    continued in l by the CPU oracle past the first fold of the hexagon branch (l ~ -0.174)."""
    from oracle import bordered, palc
    d = np.load(os.path.join(os.path.dirname(__file__), "golden", "bench_cell_states.npz"))
    cx, cy, cz = (int(c) for c in d["cell"])
    u2 = d["u0"].reshape(cz, cy, cx)[0]
    u = np.concatenate([u2, u2[::-1]], axis=0).reshape(-1)
    dims, ls = (cx, 2 * cy), (float(d["cell_l"][0]), 2 * float(d["cell_l"][1]))
    op = operators.SwiftHohenberg(dims, ls)
    prob = palc.Problem(lambda x, p: op.F(x, p, NU_HEX), lambda x, p: op.J(x, p, NU_HEX), dparam_factor=lambda x, p: x)
    bls = lambda *a, **k: bordered.bordering_bls(bordered.default_ls, *a, check_precision=False, **k)
    br = palc.continuation(prob, u, float(d["p0"]), ds=-0.01, dsmax=0.02, max_steps=20, ls=bordered.default_ls, bls=bls, dsmin=1e-5,
                           p_min=-1.0, p_max=1.0, keep_solutions=True, normC=palc.norminf, tol=1e-11)
    dp = np.diff(br.param)
    k = [i for i in range(len(dp) - 1) if dp[i] * dp[i + 1] < 0][0] + 1             # middle point of the turn
    return dict(op=op, dims=dims, ls=ls, br=br, k=k)


def test_normal_form_at_the_hexagon_fold_in_both_parameters(hex_branch):
    """Every coefficient alive: the fold of the hexagon branch, refined with newton_fold_native; the normal form in l and in nu at
    the same (x, p, zeta), native and mirror against the dense restatement -- 10 x the restatement's spread allowed, for a
    coefficient plus the rounding 4 n eps sum |terms| of its fixed-order sum -- and against each other to a few ulp.  In l the type
    is "Fold" and the turn of the branch has the side a01 b20 implies: p - p* ~ -b20 s^2 / (2 a01), s = <x - x*, zeta>, on the
    saved neighbours of the fold."""
    codim2, hip, N1 = _lib()
    from bk_amd import continuation as Cn
    hb = hex_branch
    ctx = hip.Context(0)
    k = hb["k"]
    prob = hip.SwiftHohenberg(ctx, hb["dims"], hb["ls"], l=hb["br"].param[k], nu=NU_HEX)
    ls = hip.GMRESKrylovKit(dim=40, rtol=RELTOL, atol=1e-13, maxiter=200, Pl=hip.DCTPreconditioner(prob, 1.0))
    rec, cp = Cn.ContResult(), Cn.ContinuationPar(detect_bifurcation=0)
    for p_, x_ in zip(hb["br"].param, hb["br"].sol):
        Cn.locate_fold(rec, cp, p_)
        rec.param.append(p_)
        rec.sol.append(prob.vec(x_))
    assert len(rec.specialpoint) == 1 and rec.specialpoint[0]["idx"] == k
    guess, tau = codim2.fold_point(rec, 0)
    sn = codim2.newton_fold_native(prob, guess.u, guess.p, tau, tau, ls, tol=1e-9, max_iterations=15, norm_inf=True)
    assert sn["converged"], sn["residuals"]
    # the same through the public entry: codim2.get_normal_form on the "fold" point of the record refines it itself (start vector
    # from fold_point, zeta from the null vector of newton_fold_native); without refinement it needs an eigensolver
    gf = codim2.get_normal_form(rec, 0, prob, ls, tol=1e-9, max_iterations=15, norm_inf=True)
    assert isinstance(gf, N1.SimpleBranchPoint) and gf.type == "Fold" and gf.lens == "l" and gf.zeta_star is gf.zeta
    assert abs(gf.p - sn["u"].p) <= 2e-10 * abs(sn["u"].p), (gf.p, sn["u"].p)          # two refinements of one guess (test_gpu_fold: 1e-10 each)
    assert gf.nf.a01 * gf.nf.b20 < 0 and abs(gf.tau.norm() - 1) <= 1e-12
    with pytest.raises(ValueError, match="eigensolver"):
        codim2.get_normal_form(rec, 0, prob, ls, refine=False)
    x, pf = sn["u"].u.numpy(), float(sn["u"].p)
    z = sn["v"].numpy()
    z = z / np.linalg.norm(z)
    op, d3F = hb["op"], N.sh_d3F("sh", ["l", "nu"])
    Pl = operators.dct_preconditioner(hb["dims"], hb["ls"], 1.0)
    ctx.close()
    for lens, p in (("l", pf), ("nu", NU_HEX)):
        model = R.sh_model(op, "sh", dict(l=pf, nu=NU_HEX), lens)
        q = model.at(p)
        lu = N.normal_form1d(model, d3F, x, q, lens, z, z)
        allowed = _spread(model, d3F, op, x, q, lens, z, lu, Pl)
        rnd = _sum_rounding("sh", NU_HEX, 0 if lens == "l" else 1, x, z, lu)
        allowed = {c: allowed[c] + rnd[c] for c in allowed}
        print(f"hexagon fold in {lens}: restatement", {c: lu[c] for c in ("a01", "a02", "b11", "b20", "b30", "type")}, "allowed", allowed)
        assert all(abs(lu[c]) > 1e-6 for c in ("a01", "a02", "b11", "b20", "b30")), lu                 # all terms alive
        out = {}
        for kind in ("native", "mirror"):
            c = hip.Context(0)
            pr = hip.SwiftHohenberg(c, hb["dims"], hb["ls"], l=pf, nu=NU_HEX, lens=lens)
            lsk = hip.GMRESKrylovKit(dim=40, rtol=RELTOL, atol=1e-13, maxiter=200, Pl=hip.DCTPreconditioner(pr, 1.0))
            Z = pr.vec(z)
            f = N1.normal_form1d_native if kind == "native" else N1.normal_form1d
            out[kind] = bp = f(pr, pr.vec(x), p, Z, Z, lsk)
            nf = bp.nf
            print(f"{kind} in {lens}: a01 {nf.a01:.12g} a02 {nf.a02:.12g} b11 {nf.b11:.12g} b20 {nf.b20:.12g} b30 {nf.b30:.12g} type "
                  f"{bp.type} converged {bp.converged} itlinear {bp.itlinear} unconverged {bp.unconverged_solves}")
            assert bp.type == lu["type"], (kind, lens, bp.type)
            for cname in ("a01", "a02", "b11", "b20", "b30"):
                probe(f"nf1d.hex_{cname}.{lens}.{kind}", abs(getattr(nf, cname) - lu[cname]), allowed[cname],
                      relative=abs(getattr(nf, cname) - lu[cname]) / abs(lu[cname]))
            for name, got in (("Psi01", nf.Psi01.numpy()), ("Psi20", nf.Psi20.numpy())):
                probe(f"nf1d.hex_{name}.{lens}.{kind}", np.abs(got - lu[name]).max(), allowed[name],
                      relative=np.abs(got - lu[name]).max() / np.abs(lu[name]).max())
            c.close()
        for cname in ("a01", "a02", "b11", "b20", "b30"):
            _few_ulp(f"nf1d.hex_native_vs_mirror_{cname}.{lens}", getattr(out["native"].nf, cname), getattr(out["mirror"].nf, cname))
        if lens == "l":
            assert lu["type"] == "Fold"
            for i in (k - 1, k + 1):
                s = float(np.dot(hb["br"].sol[i] - x, z))
                side = -lu["b20"] * s * s / (2 * lu["a01"])
                assert (hb["br"].param[i] - pf) * side > 0, (i, hb["br"].param[i] - pf, side)
            assert out["native"].nf.a01 * out["native"].nf.b20 * (hb["br"].param[k - 1] - pf) < 0


# ------------------------------------------------------------------------------------------ 6: end to end
def test_branch_point_to_normal_form_predictor_and_second_branch_end_to_end(ctx):
    """continuation_native on u = 0 in l through l* with bisection -> codim2.get_normal_form -> the record -> predictor ->
    continuation_from_branch_point for three steps, once more with the deflated Newton.  The coefficients against the restatement
    at the same (x0, p, zeta) (10 x its spread, plus 10 x its own distance from the closed form at that p, plus the rounding of the
    sums); every point of the new branch converged, off the
    trivial state with |s| growing, on the side dsfactor says, and equal to the restatement's switched branch from the same
    predictor to the Newton tolerance: |dx|_inf <= 10 tol / |lambda_min(J)| at that point, |dp| alike."""
    codim2, hip, N1 = _lib()
    from dataclasses import replace

    import scipy.sparse.linalg as spla

    from bk_amd import continuation as Cn
    from oracle import bordered, palc
    dims = (64, 64)
    n = dims[0] * dims[1]
    lstar, zmode, _ = N.sh_trivial_mode(dims, BOX, (1, 1))
    tol = 1e-10
    prob = hip.SwiftHohenberg(ctx, dims, BOX, l=-0.05, nu=NU)
    P = hip.DCTPreconditioner(prob, 1.0)
    ls = hip.GMRESKrylovKit(dim=40, rtol=RELTOL, atol=1e-13, maxiter=50, Pl=P)
    els = hip.KrylovLSSymmetric("minres", rtol=1e-10, atol=1e-13, itmax=4000, Pl=P)
    eig = hip.ShiftInvert(0.2, els, tol=1e-10, maxiter=20, hermitian=True, save_vectors=True)       # J - 0.2 < 0 for l < 0.2
    nopt = Cn.NewtonPar(tol=tol, max_iterations=20, linsolver=ls, eigsolver=eig)
    cp = Cn.ContinuationPar(ds=0.02, dsmin=1e-4, dsmax=0.03, p_min=-0.1, p_max=0.1, max_steps=2, nev=4, newton_options=nopt,
                            n_inversion=4, max_bisection_steps=30, dsmin_bisection=1e-9)
    alg = Cn.PALC(tangent="secant", theta=0.5, bls=hip.BorderingBLS(None, check_precision=False))
    br = Cn.continuation_native(prob, prob.vec(np.zeros(n)), lstar - 0.03, alg, cp, normC=Cn.norminf, bisection=True, save_sol=True)
    ib = [i for i, sp in enumerate(br.specialpoint) if sp.get("type") == "bp"]
    assert ib, br.specialpoint
    sp = br.specialpoint[ib[0]]
    print("branch point:", sp, "l* =", lstar)
    assert sp["interval"][0] - 1e-9 <= lstar <= sp["interval"][1] + 1e-9
    bp = codim2.get_normal_form(br, ib[0], prob, ls, eig=eig)
    assert isinstance(bp, N1.SimpleBranchPoint) and bp.type == "Pitchfork" and bp.lens == "l"
    probe("nf1d.e2e_unconverged_solves", bp.unconverged_solves, 1)              # J \ zeta* at bisection accuracy: see test 4
    assert bp.p == sp["param"] and np.abs(bp.x0.numpy()).max() == 0.0
    z = bp.zeta.numpy()
    assert abs(np.linalg.norm(z) - 1) <= 1e-12 and bp.zeta_star is bp.zeta
    probe("nf1d.e2e_zeta_vs_mode", min(np.abs(z - zmode).max(), np.abs(z + zmode).max()), 1e-6)
    op = operators.SwiftHohenberg(dims, BOX)
    model = R.sh_model(op, "sh", dict(l=bp.p, nu=NU), "l")
    d3F = N.sh_d3F("sh", ["l", "nu"])
    zero = np.zeros(n)
    lu = N.normal_form1d(model, d3F, zero, model.at(bp.p), "l", z, z)
    allowed = _spread(model, d3F, op, zero, model.at(bp.p), "l", z, lu, operators.dct_preconditioner(dims, BOX, 1.0))
    acf = _against_closed_form(lu, _closed_form_at(dims, bp.p), zero)
    rnd = _sum_rounding("sh", NU, 0, zero, z, lu)
    allowed = {c: allowed[c] + acf[c] + rnd[c] for c in allowed}
    print("e2e: restatement", {c: lu[c] for c in ("a01", "a02", "b11", "b20", "b30", "type")}, "device",
          {c: getattr(bp.nf, c) for c in ("a01", "a02", "b11", "b20", "b30")}, "allowed", allowed, "itlinear", bp.itlinear)
    assert lu["type"] == "Pitchfork"
    for c in ("a01", "a02", "b11", "b20", "b30"):
        probe(f"nf1d.e2e_{c}", abs(getattr(bp.nf, c) - lu[c]), allowed[c])
    # predictor: the formulas of :457-487 with the device's coefficients, the vector from the fused pass
    ds = 0.01
    pr = codim2.predictor(bp, ds)
    side = 1.0 if bp.nf.b11 * bp.nf.b30 < 0 else -1.0
    amp = math.sqrt(-6 * ds * side * bp.nf.b11 / bp.nf.b30)
    assert pr["dsfactor"] == side == -1.0 and pr["p"] == bp.p + ds * side and abs(pr["amp"] / amp - 1) <= 4 * EPS
    assert np.abs(pr["x1"].numpy() - amp * z).max() <= 6 * EPS * amp * np.abs(z).max() and pr["x0"] is bp.x0
    # the second branch: constant steps (ds = dsmax), no eigensolves
    cps = replace(cp, ds=ds, dsmin=ds, dsmax=ds, max_steps=3, detect_bifurcation=0, p_min=bp.p - 0.2, p_max=bp.p + 0.2)
    oprob = palc.Problem(lambda x_, p_: op.F(x_, p_, NU), lambda x_, p_: op.J(x_, p_, NU), dparam_factor=lambda x_, p_: x_)
    obls = lambda *a, **k_: bordered.bordering_bls(bordered.default_ls, *a, check_precision=False, **k_)
    runs = {}
    for defl in (False, True):
        B = N1.continuation_from_branch_point(br, ib[0], prob, alg, cps, eig=eig, usedeflation=defl, normC=Cn.norminf, save_sol=True)
        assert isinstance(B, N1.Branch) and B.bp.type == "Pitchfork"
        nb = B.branch
        print(f"second branch (deflation {defl}): p", nb.param, "itnewton", nb.itnewton, "itlinear", nb.itlinear)
        assert len(nb.param) == 4 and nb.param[0] == B.bp.p and nb.ds[0] == -ds
        assert all(r[-1] <= tol for r in nb.residuals[1:])                          # every point converged
        zb = B.bp.zeta.numpy()
        s = np.array([float(np.dot(v.numpy(), zb)) for v in nb.sol])
        assert s[0] == 0.0 and np.all(np.diff(np.abs(s)) > 0) and abs(s[1]) > 1e-2, s      # off u = 0, |s| grows
        assert all((p_ - B.bp.p) * side > 0 for p_ in nb.param[1:])                  # the side dsfactor says
        prd = N1.predictor(B.bp, ds)
        x1 = prd["x1"].numpy()
        if defl:
            from bk_amd.hip import DeflationOperator, newton_deflated_native
            x1 = newton_deflated_native(prob, DeflationOperator(2, 1.0, [B.bp.x0]), prd["x1"], prd["p"], ls, tol=tol,
                                        max_iterations=50, norm_inf=True)["u"].numpy()
        ob = N.continuation_two_points(oprob, zero, B.bp.p, x1, prd["p"], ls=bordered.default_ls, bls=obls, ds=ds, dsmin=ds, dsmax=ds,
                                       theta=0.5, p_min=B.bp.p - 0.2, p_max=B.bp.p + 0.2, max_steps=3, tol=tol, max_iterations=20,
                                       normC=palc.norminf)
        assert len(ob.param) == len(nb.param)
        for i in range(1, 4):
            lam = abs(spla.eigsh(op.J(ob.sol[i], ob.param[i], NU).tocsc(), k=1, sigma=0.0, which="LM", return_eigenvectors=False)[0])
            probe(f"nf1d.e2e_branch_x.defl{int(defl)}.{i}", np.abs(nb.sol[i].numpy() - ob.sol[i]).max(), 10 * tol / lam, lam=lam)
            probe(f"nf1d.e2e_branch_p.defl{int(defl)}.{i}", abs(nb.param[i] - ob.param[i]), 10 * tol / lam)
        runs[defl] = nb
    # without the normal form (:148-152): x1 = x0 + ampfactor zeta at p + delta_p, and both directions from the two points
    B2 = N1.continuation_from_branch_point(br, ib[0], prob, alg, cps, eig=eig, use_normal_form=False, ampfactor=2.0, delta_p=-ds,
                                           bothside=True, normC=Cn.norminf, save_sol=True)
    s2 = [float(np.dot(v.numpy(), B2.bp.zeta.numpy())) for v in B2.branch.sol]
    print("second branch without the normal form: p", B2.branch.param, "s", s2, "| backward p", B2.backward.param)
    assert B2.branch.param[0] == B2.bp.p and B2.branch.ds[0] == -ds and len(B2.branch.param) > 1 and abs(s2[-1]) > 1e-2
    assert all(p_ < B2.bp.p for p_ in B2.branch.param[1:])
    assert B2.backward is not None and B2.backward.param[0] == B2.bp.p - ds and B2.backward.ds[0] == -ds
    # the deflated start moves the second point along the branch, so the two runs step to different points of the SAME branch
    # (measured: p differs by 2e-5 after three steps); each was compared with the restatement from its own start above
    assert all(a != b for a, b in zip(runs[True].param[1:], runs[False].param[1:]))


# ------------------------------------------------------------------------------------------ 7: errors and flags
def test_errors_flags_and_the_matrix_free_bordered_solver():
    """A cGL problem: the fold-formulation error from every new entry.  <zeta, zeta*> = 0.5: the normalisation error, native and
    mirror.  maxiter = 1: converged is False, no error, and the counter equals the number of solves (three with BorderingBLS, two
    with MatrixFreeBLS, native and mirror alike)."""
    codim2, hip, N1 = _lib()
    from bk_amd import _lib as L
    ctx = hip.Context(0)
    cgl = hip.CGL2d(ctx, (8, 8), (1.0, 1.0))
    x = cgl.vec(np.zeros(cgl.nglobal))
    pv = cgl._pvec(0.5)
    ls0 = hip.GMRESIterativeSolvers(reltol=1e-8, restart=10, maxiter=10, Pl=None)
    for call in (lambda: N1.d3F(cgl, x, pv, x, x, x), lambda: N1.nf1d_dots(cgl, x, pv, 0, x, x),
                 lambda: N1.nf1d_rhs(cgl, x, pv, 0, x, 0.0, 0.0), lambda: N1.nf1d_contract(cgl, x, pv, 0, x, x, x, x),
                 lambda: N1.normal_form1d_native(cgl, x, 0.5, x, x, ls0)):
        with pytest.raises(L.BkHipError, match="fold formulation"):
            call()
    g = N.sh_trivial_closed_form((16, 12), (7.0, 5.0), (2, 3), 1.2)
    dims, box, nu = (16, 12), (7.0, 5.0), 1.2
    n = dims[0] * dims[1]
    op = operators.SwiftHohenberg(dims, box)
    rng = np.random.default_rng(3)
    xs = 1e-3 * rng.standard_normal(n)
    p = g["lstar"] + 1e-6
    w, V = np.linalg.eigh(op.J(xs, p, nu).toarray())
    z = V[:, np.argmin(np.abs(w))]
    prob = hip.SwiftHohenberg(ctx, dims, box, l=p, nu=nu)
    X, Z, half = prob.vec(xs), prob.vec(z), prob.vec(0.5 * z)
    ls = hip.GMRESKrylovKit(dim=40, rtol=RELTOL, atol=1e-13, maxiter=50, Pl=hip.DCTPreconditioner(prob, 1.0))
    with pytest.raises(L.BkHipError, match="normalization"):
        N1.normal_form1d_native(prob, X, p, Z, half, ls)
    with pytest.raises(ValueError, match="normalization"):
        N1.normal_form1d(prob, X, p, Z, half, ls)
    with pytest.raises(L.BkHipError, match="aliases an input"):
        import ctypes as C                                                       # the wrapper allocates its outputs: call the entry
        one = (C.c_double * 1)(0.0)
        ctx.check(ctx.lib.bk_nf1d_predict(ctx.h, n, X.t.data_ptr(), Z.t.data_ptr(), None, None, 1, one, one, one,
                                          (C.c_void_p * 1)(X.t.data_ptr())), "bk_nf1d_predict")
    with pytest.raises(L.BkHipError, match="NULL vector"):
        N1.nf1d_predict(X, Z, None, None, [(1.0, 0.5, 0.0)])
    ls1 = hip.GMRESIterativeSolvers(reltol=1e-13, restart=2, maxiter=1, Pl=None)
    b3 = N1.normal_form1d_native(prob, X, p, Z, Z, ls1)
    assert b3.converged is False and b3.unconverged_solves == 3, (b3.converged, b3.unconverged_solves, b3.itlinear)
    b2 = N1.normal_form1d_native(prob, X, p, Z, Z, ls1, bls=hip.MatrixFreeBLS(ls1))
    assert b2.converged is False and b2.unconverged_solves == 2 and b2.itlinear[2] == 0, (b2.unconverged_solves, b2.itlinear)
    assert np.isfinite([b3.nf.a01, b3.nf.a02, b3.nf.b11, b3.nf.b20, b3.nf.b30, b2.nf.b30]).all()
    m3 = N1.normal_form1d(prob, X, p, Z, Z, ls1)                                       # the mirror: the same three solves
    assert m3.converged is False and m3.itlinear == b3.itlinear and m3.type == b3.type, (m3.itlinear, b3.itlinear)
    m2 = N1.normal_form1d(prob, X, p, Z, Z, ls1, bls=hip.MatrixFreeBLS(ls1))           # ... and the same two
    assert m2.converged is False and m2.itlinear == b2.itlinear and m2.type == b2.type, (m2.itlinear, b2.itlinear)
    ctx.close()


# ------------------------------------------------------------------------------------------ 8: the non-temporal load path
def test_passes_at_a_size_that_takes_the_non_temporal_loads(ctx):
    """n = 2048^2 = 2^22: every pass takes its non-temporal 16-byte instantiation.  Sums against exact sums within 4 n eps sum |terms|,
    the writing passes bit for bit against NumPy (the bounds of test 3)."""
    codim2, hip, N1 = _lib()
    prob = hip.SwiftHohenberg(ctx, (2048, 2048), (np.pi, np.pi), l=-0.2, nu=1.3)
    n, pars = prob.nlocal, [-0.2, 1.3]
    assert n == 1 << 22
    rng = np.random.default_rng(22)
    u, z, zs, p, q = (rng.standard_normal(n) for _ in range(5))
    U, Z, ZS, P, Q = (prob.vec(a) for a in (u, z, zs, p, q))
    for ip in (0, 1):
        for g, t in zip(N1.nf1d_dots(prob, U, pars, ip, Z, ZS), _dots_terms("sh", pars[1], ip, u, z, zs)):
            probe("nf1d.nt_dots_rel", abs(g - math.fsum(t)) / (4 * n * EPS * np.abs(t).sum()), 1.0)
        for g, t in zip(N1.nf1d_contract(prob, U, pars, ip, Z, ZS, P, Q), _contract_terms("sh", pars[1], ip, u, z, zs, p, q)):
            probe("nf1d.nt_contract_rel", abs(g - math.fsum(t)) / (4 * n * EPS * np.abs(t).sum()), 1.0)
        h, g_, d3, f = _polys("sh", pars[1], ip)
        r1, r2 = N1.nf1d_rhs(prob, U, pars, ip, Z, 0.37, -1.9)
        e1, e2 = 0.37 * z - R.horner(f, u), -1.9 * z - (R.horner(h, u) * z) * z
        b1 = 8 * EPS * (np.abs(0.37 * z) + np.abs(R.horner(np.abs(f), np.abs(u))))
        b2 = 10 * EPS * (np.abs(1.9 * z) + np.abs(R.horner(np.abs(h), np.abs(u)) * z * z))
        probe("nf1d.nt_rhs_r1", (np.abs(r1.numpy() - e1) / b1).max(), 1.0, tight=0.0)
        probe("nf1d.nt_rhs_r2", (np.abs(r2.numpy() - e2) / b2).max(), 1.0, tight=0.0)
    coefs = [(0.7, -0.3, 1.1), (-0.7, 0.3, 0.0)]
    for (a, b, c), o in zip(coefs, N1.nf1d_predict(U, Z, P, Q, coefs)):
        bound = 6 * EPS * (np.abs(u) + np.abs(a * z) + np.abs(b * p) + np.abs(c * q))
        probe("nf1d.nt_predict", (np.abs(o.numpy() - (((u + a * z) + b * p) + c * q)) / bound).max(), 1.0, tight=0.0)


# ------------------------------------------------------------------------------------------ 9: the library's predictors
def test_library_predictors_match_the_restatement(ctx):
    """normal_form1d.predictor on hand-built records of type Transcritical (tau off and along zeta) and BranchPoint against the
    restatement's predictor on the same numbers: the scalars to a few ulp (the BranchPoint angle to the bisection's 1e-12), the
    vectors within the 6 eps bound of the fused pass."""
    codim2, hip, N1 = _lib()
    n = 4099
    prob = hip.SwiftHohenberg1D(ctx, n, 6.0, lam=-0.7, nu=2.0)
    rng = np.random.default_rng(9)
    x0, z, P01 = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
    z /= np.linalg.norm(z)
    off = rng.standard_normal(n)
    taus = {"off": (off / np.linalg.norm(off), 0.3), "along": ((z + 0.05 * off / np.linalg.norm(off)) * 0.8, 0.6)}

    def record(kind, coef, tau):
        Zv = prob.vec(z)
        return N1.SimpleBranchPoint(x0=prob.vec(x0), tau=hip.BorderedArray(prob.vec(tau[0]), tau[1]), p=0.25, params=[0.25, 2.0],
                                    lens="lam", zeta=Zv, zeta_star=Zv, nf=N1.BranchPointNF(*coef, prob.vec(P01), None), type=kind)

    def check(name, got, ref, tau, ds, slack=0.0):
        """Scalars to 1e-12; vectors within 8 eps of the magnitudes that enter them (the fused pass rounds three products and three
        sums, NumPy orders them differently), plus ``slack`` |zeta| for the angle of the BranchPoint bisection."""
        for k in ("p", "amp", "dsfactor"):
            assert abs(got[k] - ref[k]) <= 1e-12 * max(1.0, abs(ref[k])), (name, k, got[k], ref[k])
        scale = np.abs(x0) + np.abs(ref["amp"] * z) + np.abs(got["p"] - 0.25) * np.abs(z) + np.abs(ds * P01) + np.abs(ds / tau[1] * tau[0])
        for k in ("x0", "x1", "xm1"):
            if k in ref:
                probe(f"nf1d.predictor_{name}_{k}", (np.abs(got[k].numpy() - ref[k]) / (8 * EPS * scale + slack * np.abs(z))).max(), 1.0)

    coef = (0.0, 0.1, 3.23, -2.24, 1.4)
    for tname, tau in taus.items():
        for ds in (0.1, -0.05):
            nf = dict(type="Transcritical", a01=coef[0], a02=coef[1], b11=coef[2], b20=coef[3], b30=coef[4], Psi01=P01)
            ref = N.predictor(nf, x0, 0.25, z, tau, ds, ampfactor=1.5)
            got = N1.predictor(record("Transcritical", coef, tau), ds, ampfactor=1.5)
            assert got["pm1"] == ref["pm1"] and got["p0"] == 0.25
            check(f"transcritical_{tname}", got, ref, tau, ds)
    along = abs(np.dot(z, taus["along"][0])) >= 0.9 * np.linalg.norm(taus["along"][0])
    assert along and abs(np.dot(z, taus["off"][0])) < 0.9                       # both cases of :410 were taken
    coefb = (0.0, 1.0, 0.0, -1.3, 0.4)
    nf = dict(type="BranchPoint", a01=0.0, a02=1.0, b11=0.0, b20=-1.3, b30=0.4, Psi01=P01)
    for tname, tau in taus.items():
        ref = N.predictor(nf, x0, 0.25, z, tau, 0.1)
        got = N1.predictor(record("BranchPoint", coefb, tau), 0.1)
        assert abs(got["dp"] - ref["dp"]) <= 1e-12
        check(f"branchpoint_{tname}", got, ref, tau, 0.1, slack=1e-12)
    assert N1.predictor(record("Fold", coef, taus["off"]), 0.1) is None


# ------------------------------------------------------------------------------------------ 10: check_precision
def test_check_precision_corrections_native_and_mirror():
    """BorderingBLS(check_precision = True, k = 2): the residual check and the corrections of src/LinearBorderSolver.jl:146-166 with
    the shared J \\ zeta*, native and mirror on fresh contexts, at a point off the trivial state (16 x 12, a random state of size
    1e-3, l = l* + 1e-6).  Against the restatement: 10 x its spread plus the rounding of the sums, as everywhere; against each
    other a few ulp; and at least one correction solve was taken (more GMRES iterations than without the check)."""
    codim2, hip, N1 = _lib()
    dims, box, nu = (16, 12), (7.0, 5.0), 1.2
    n = dims[0] * dims[1]
    op = operators.SwiftHohenberg(dims, box)
    xs = 1e-3 * np.random.default_rng(3).standard_normal(n)
    p = N.sh_trivial_closed_form(dims, box, (2, 3), nu)["lstar"] + 1e-6
    w, V = np.linalg.eigh(op.J(xs, p, nu).toarray())
    z = V[:, np.argmin(np.abs(w))]
    model = R.sh_model(op, "sh", dict(l=p, nu=nu), "l")
    d3F = N.sh_d3F("sh", ["l", "nu"])
    lu = N.normal_form1d(model, d3F, xs, model.at(p), "l", z, z)
    allowed = _spread(model, d3F, op, xs, model.at(p), "l", z, lu, operators.dct_preconditioner(dims, box, 1.0))
    rnd = _sum_rounding("sh", nu, 0, xs, z, lu)
    allowed = {c: allowed[c] + rnd[c] for c in allowed}
    out = {}
    for kind in ("native", "mirror", "plain"):
        ctx = hip.Context(0)
        prob = hip.SwiftHohenberg(ctx, dims, box, l=p, nu=nu)
        ls = hip.GMRESKrylovKit(dim=40, rtol=RELTOL, atol=1e-13, maxiter=50, Pl=hip.DCTPreconditioner(prob, 1.0))
        bls = hip.BorderingBLS(ls, tol=1e-12, check_precision=kind != "plain", k=2)
        f = N1.normal_form1d if kind == "mirror" else N1.normal_form1d_native
        Z = prob.vec(z)
        out[kind] = bp = f(prob, prob.vec(xs), p, Z, Z, ls, bls=bls)
        print(f"check_precision {kind}: b11 {bp.nf.b11:.15g} b30 {bp.nf.b30:.15g} converged {bp.converged} itlinear {bp.itlinear}")
        for c in ("a01", "a02", "b11", "b20", "b30"):
            probe(f"nf1d.check_precision_{c}.{kind}", abs(getattr(bp.nf, c) - lu[c]), allowed[c])
        for name, got in (("Psi01", bp.nf.Psi01.numpy()), ("Psi20", bp.nf.Psi20.numpy())):
            probe(f"nf1d.check_precision_{name}.{kind}", np.abs(got - lu[name]).max(), allowed[name])
        ctx.close()
    assert out["native"].itlinear == out["mirror"].itlinear, (out["native"].itlinear, out["mirror"].itlinear)
    assert sum(out["native"].itlinear[:2]) > sum(out["plain"].itlinear[:2]), (out["native"].itlinear, out["plain"].itlinear)
    for c in ("a01", "a02", "b11", "b20", "b30"):
        _few_ulp(f"nf1d.check_precision_native_vs_mirror_{c}", getattr(out["native"].nf, c), getattr(out["mirror"].nf, c))
