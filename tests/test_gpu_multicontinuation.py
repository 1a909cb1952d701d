"""GPU tests of multicontinuation from branch points with 2-d and 3-d kernels of the Swift-Hohenberg problems: the fused
deflation pass (bk_deflation_dots) against extended-precision sums, hip.DeflationOperator(autodiff=True) against the long-double
formula and the finite-difference operator, bk_newton_deflated_exact against its call-by-call mirror and the dense restatement
(tests/multicontinuation_ref.py), the first-points search on the trivial branch in 2-D and 3-D, and detect -> normal form ->
predictor -> first points -> eight branches end to end.  Every bound is logged next to its measured value by ``probe``."""
import ctypes as C
import math
import warnings
from dataclasses import replace

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import multicontinuation_ref as MC
import normal_form1d_ref as N1R
import normal_form_nd_ref as M
from conftest import probe
from oracle import bordered, palc

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
RELTOL = 1e-10
TOL = 1e-10
LD = np.longdouble


def _lib():
    from bk_amd import hip
    from bk_amd import normal_form_nd as ND
    return hip, ND


def _guarded(hip, ctx, a, off):
    """A device vector holding ``a`` between NaN guards, ``off`` doubles (2: 16-byte aligned, 1: one double off) into a fresh buffer."""
    import torch
    n = a.shape[0]
    t = torch.full((n + 4,), float("nan"), dtype=torch.float64, device=ctx.torch_device)
    t[off:off + n] = torch.from_numpy(np.ascontiguousarray(a)).to(ctx.torch_device)
    v = type("GuardedVec", (hip.HipVec,), {})(ctx, t[off:off + n], n)
    assert v.t.data_ptr() % 16 == (0 if off == 2 else 8)
    v._whole, v._off = t, off
    return v


def _guards_intact(v):
    w = v._whole.cpu().numpy()
    return bool(np.isnan(w[:v._off]).all() and np.isnan(w[v._off + v.n:]).all())


def _ld(t):
    return float(np.sum(t.astype(LD))), float(np.abs(t).sum())


# ------------------------------------------------------------------------------------------ 1: the pass alone
LENGTHS = [2, 3, 255, 256, 257, 4097, 1 << 22]
NROOTS = [1, 2, 7, 8, 9, 17]


@pytest.mark.parametrize("n", LENGTHS)
def test_deflation_dots_match_extended_precision_sums(ctx, n):
    """Every d_i = sum (u - r_i)^2 and e_i = sum (u - r_i) h of bk_deflation_dots within 4 n eps sum |terms| of the NumPy
    longdouble sum of the fp64 terms, for 1, 2, 7, 8, 9 and 17 roots (one launch; 8 + 1; 8 + 8 + 1), with and without h, every
    stream 16-byte aligned and again with root 0 one double off (the element path); n = 2^22 aligned takes the non-temporal
    instantiation.  The sums of root i do not depend on how many roots follow it, so the 17 references are computed once and
    shared by all counts and both alignments; without h the d_i are the same bits as with it.  Operands sit between NaN guards."""
    hip, _ = _lib()
    rng = np.random.default_rng(100 + n % 9973)
    u, h = rng.random(n) - 0.5, rng.random(n) - 0.5
    roots = [rng.random(n) - 0.5 for _ in range(max(NROOTS))]
    rd, re_ = [], []
    for r in roots:                                                                 # one root at a time: 2^22 x 17 x 2 terms
        (td,), (te,) = MC.sum_terms(u, [r], h)
        rd.append(_ld(td))
        re_.append(_ld(te))
    for mis in (False, True):
        U, H = _guarded(hip, ctx, u, 2), _guarded(hip, ctx, h, 2)
        Rv = [_guarded(hip, ctx, r, 1 if (mis and i == 0) else 2) for i, r in enumerate(roots)]
        tag = f"n{n}.{'off8' if mis else 'aligned'}"
        for k in NROOTS:
            op = hip.DeflationOperator(2, 1.0, Rv[:k], autodiff=True)
            d0, e0 = op.dots(U)
            d1, e1 = op.dots(U, H)
            assert e0 is None and len(d0) == len(d1) == len(e1) == k
            assert d0 == d1, (tag, k)                                               # the same sums in the same order
            for i in range(k):
                probe(f"multicont.dots_d.{tag}", abs(d1[i] - rd[i][0]) / (4 * n * EPS * rd[i][1] + 1e-300), 1.0, k=k)
                probe(f"multicont.dots_e.{tag}", abs(e1[i] - re_[i][0]) / (4 * n * EPS * re_[i][1] + 1e-300), 1.0, k=k)
        assert all(_guards_intact(v) for v in [U, H] + Rv)


@pytest.mark.parametrize("n", [3, 257, 4097])
def test_a_root_equal_to_u_gives_zero_exactly(ctx, n):
    """A root that holds u's values (its own buffer): d = 0 and e = 0 exactly, the other roots unaffected; M is infinite and
    neither the operator nor its derivative raises."""
    hip, _ = _lib()
    rng = np.random.default_rng(n)
    u, h = rng.standard_normal(n), rng.standard_normal(n)
    roots = [rng.standard_normal(n) for _ in range(9)]
    roots[3] = u.copy()
    V = lambda a: _guarded(hip, ctx, a, 2)
    op = hip.DeflationOperator(2, 1.0, [V(r) for r in roots], autodiff=True)
    U, H = V(u), V(h)
    d, e = op.dots(U, H)
    assert d[3] == 0.0 and e[3] == 0.0 and all(x > 0 for i, x in enumerate(d) if i != 3)
    assert math.isinf(op(U)) and not math.isfinite(op.dM(U, H))
    assert all(_guards_intact(v) for v in [U, H] + op.roots)


# ------------------------------------------------------------------------------------------ 2: M and dM
@pytest.mark.parametrize("acc", ["prod", "mean"])
@pytest.mark.parametrize("k", [1, 3, 9])
def test_operator_matches_the_long_double_formula_and_the_finite_difference(ctx, acc, k):
    """DeflationOperator(autodiff=True) against the restatement's formula on longdouble sums, to the rounding of its sums: d_i
    carries a relative error of 4 n eps at most (its terms are positive) and e_i an absolute one of 4 n eps sum |t_i h|, so with
    c_i = dM / de_i:  |dM - exact| <= sum_i |c_i| (((p + 1) + p (k - 1)) 4 n eps |e_i| + 8 k eps |e_i| + 4 n eps sum |t_i h|) and
    |M - exact| <= (4 n p k + 4 k) eps M, p the power.  Against the finite-difference operator (autodiff=False, delta = 1e-8) on
    the same device data: the relative difference at most 10 x the one between the restatement's two formulas (with roots 0.3
    away the truncation of the quotient dominates its rounding, so that difference is a property of the data)."""
    hip, _ = _lib()
    n, p = 256, 2
    rng = np.random.default_rng(7 * k)
    u = 0.4 * rng.standard_normal(n)
    unit = lambda v: v / np.linalg.norm(v)
    roots = [u + (0.3 + 0.05 * i) * unit(rng.standard_normal(n)) for i in range(k)]
    h = unit(rng.standard_normal(n))
    kw = dict(mean=acc == "mean")
    V = lambda a: _guarded(hip, ctx, a, 2)
    U, H, Rv = V(u), V(h), [V(r) for r in roots]
    ad = hip.DeflationOperator(p, 1.0, Rv, accumulator=acc, autodiff=True)
    fd = hip.DeflationOperator(p, 1.0, Rv, accumulator=acc)
    Mx, dMx = MC.combine(*MC.sums(u, roots, h, LD), **kw)
    Mx, dMx = float(Mx), float(dMx)
    dl, el = MC.sums(u, roots, h, LD)
    _, te = MC.sum_terms(u, roots, h)
    ci = [abs(float(MC.combine(dl, [LD(1) if j == i else LD(0) for j in range(k)], **kw)[1])) for i in range(k)]
    bound = sum(c * ((((p + 1) + p * (k - 1)) * 4 * n + 8 * k) * EPS * abs(float(e)) + 4 * n * EPS * float(np.abs(t).sum()))
                for c, e, t in zip(ci, el, te))
    probe(f"multicont.M.{acc}.k{k}", abs(ad(U) - Mx), (4 * n * p * k + 4 * k) * EPS * abs(Mx))
    probe(f"multicont.dM.{acc}.k{k}", abs(ad.dM(U, H) - dMx), bound, relative=abs(ad.dM(U, H) - dMx) / abs(dMx))
    cpu = abs(MC.dM_exact(u, h, roots, **kw) - MC.dM_fd(u, h, roots, **kw)) / abs(MC.dM_exact(u, h, roots, **kw))
    gpu = abs(ad.dM(U, H) - fd.dM(U, H)) / abs(ad.dM(U, H))
    probe(f"multicont.dM_vs_fd.{acc}.k{k}", gpu, 10 * cpu, cpu=cpu)
    assert abs(ad(U) - fd(U)) <= 8 * n * p * k * EPS * abs(Mx)                       # M itself: the same quantity twice
    assert all(_guards_intact(v) for v in [U, H] + Rv)


# ------------------------------------------------------------------------------------------ 3: bk_newton_deflated_exact
def _solver(hip, prob, maxiter=50):
    return hip.GMRESKrylovKit(dim=40, rtol=RELTOL, atol=1e-13, maxiter=maxiter, Pl=hip.DCTPreconditioner(prob, 1.0))


class _CountingLS:
    """The linear solver with a count of its calls."""

    def __init__(self, ls):
        self.ls, self.calls = ls, 0

    def __call__(self, J, rhs):
        self.calls += 1
        return self.ls(J, rhs)


def test_exact_deflated_newton_native_mirror_and_restatement(ctx):
    """16 x 16, dp = 0.008: from the predicted state of a square with the trivial state and three of the restatement's rolls
    deflated.  Native and call-by-call mirror agree to 8 ulp (the same kernels and solves in the same order) with equal counts;
    one linear solve per Newton step (the mirror's solver is called itnewton times and the counts agree); the state is within
    10 tol / |smallest eigenvalue of J| of the restatement's -- as far as two points with |F| < tol can be apart -- with the
    Newton count within one.  Under the reference's rule native and mirror agree in the same way, converged or not, and end on
    the same state.  Then the error paths: x aliasing a root is refused with a message, a root on x is a
    flag, no roots is bk_newton, and each is followed by a call that works."""
    hip, ND = _lib()
    from bk_amd import _lib as L
    c = MC.sh_case(2, 0.0)
    dp = 0.008
    fp = MC.sh_first_points(2, 0.0, dp)
    rolls = [x for x in fp["after"][1:] if MC.mode_class(c["Q"], x) == 1][:3]
    zsq = next(z for z in fp["zeros"]["after"][1:] if np.abs(z).min() > 1e-3 * np.abs(z).max())
    start = c["Z"] @ zsq
    p = c["p"] + dp
    held = [np.zeros(c["op"].N)] + rolls
    prob = hip.SwiftHohenberg(ctx, c["dims"], c["ls"], l=p, nu=c["nu"])
    ls = _solver(hip, prob)
    op = hip.DeflationOperator(2, 1.0, [prob.vec(r) for r in held], autodiff=True)
    X0 = prob.vec(start)
    for plain in (True, False):
        cpu = MC.deflated_newton(lambda x: c["F"](x, p), lambda x: c["J"](x, p), held, start, TOL, 50, stop_plain=plain)
        na = hip.newton_deflated_native(prob, op, X0, p, ls, tol=TOL, max_iterations=50, norm_inf=True, stop_plain=plain)
        cl = _CountingLS(ls)
        mi = hip.newton_deflated(prob, op, X0, p, cl, tol=TOL, max_iterations=50, norm_inf=True, stop_plain=plain)
        print(f"stop_plain = {plain}: native {na['itnewton']} / {na['itlineartot']} residuals {na['residuals']}; cpu {cpu['itnewton']} {cpu['residuals']}")
        assert na["itnewton"] == mi["itnewton"] == cl.calls and na["itlineartot"] == mi["itlineartot"] >= na["itnewton"]
        assert na["converged"] == mi["converged"] and len(na["residuals"]) == len(mi["residuals"]) == na["itnewton"] + 1
        un, um = na["u"].numpy(), mi["u"].numpy()
        probe(f"multicont.newton_native_vs_mirror.plain{int(plain)}", np.abs(un - um).max(), 8 * EPS * np.abs(un).max(), tight=0.0)
        probe(f"multicont.newton_M_native_vs_mirror.plain{int(plain)}", abs(na["M"] - mi["M"]), 8 * 4 * len(held) * EPS * abs(na["M"]))
        assert abs(na["min_dist"] - mi["min_dist"]) <= 8 * EPS * na["min_dist"]
        if not plain:
            # the reference's rule on the device: |M| |F| stalls where |F| meets its rounding floor (M ~ 1e4 here), and whether
            # that lies under tol is not a property of the state -- the restatement's F rounds lower and converges.  What the
            # rule leaves behind is a zero by the plain rule, the same one:
            probe("multicont.newton_reference_rule_plain_residual", na["residuals"][-1] / abs(na["M"]), TOL, deflated=na["residuals"][-1])
            assert np.abs(un - found_plain).max() <= 10 * TOL / lam
            continue
        assert cpu["converged"] and na["converged"] and na["residuals"][-1] < TOL
        found_plain = un
        lam = float(np.abs(np.linalg.eigvalsh(c["J"](cpu["u"], p).toarray())).min())
        probe(f"multicont.newton_vs_restatement.plain{int(plain)}", np.abs(un - cpu["u"]).max(), 10 * TOL / lam, lam=lam)
        assert abs(na["itnewton"] - cpu["itnewton"]) <= 1
        probe(f"multicont.newton_min_dist.plain{int(plain)}", abs(na["min_dist"] - cpu["min_dist"]), 10 * TOL / lam * math.sqrt(un.size))
        assert MC.mode_class(c["Q"], un) == 2                                        # a square
    # --- error paths
    ctxh, lo, no = prob.ctx, ls._opts(), hip.newton_opts(TOL, 50, True)
    pv = prob._pvec(p)
    arr = (C.c_double * len(pv))(*pv)

    def raw(x, roots):
        res = L.DeflatedResult()
        rp = (C.c_void_p * max(len(roots), 1))(*[r.t.data_ptr() for r in roots])
        ctxh.check(ctxh.lib.bk_newton_deflated_exact(ctxh.h, prob.h, x.t.data_ptr(), arr, len(pv), rp, len(roots), 2.0, 1.0, 0, 1,
                                                     C.byref(no), C.byref(lo), ls._pl(), C.byref(res)), "bk_newton_deflated_exact")
        return res

    works = lambda: hip.newton_deflated_native(prob, op, X0, p, ls, tol=TOL, max_iterations=50, norm_inf=True, stop_plain=True)
    x = X0.copy()
    with pytest.raises(L.BkHipError, match="aliases root 1"):
        raw(x, [op.roots[0], x])
    assert np.array_equal(x.numpy(), start) and works()["converged"]
    on = hip.DeflationOperator(2, 1.0, [op.roots[0], X0.copy()], autodiff=True)
    for plain in (True, False):
        s = hip.newton_deflated_native(prob, on, X0, p, ls, tol=TOL, max_iterations=50, norm_inf=True, stop_plain=plain)
        assert s["converged"] is False and s["itnewton"] == 0 and math.isinf(s["M"]) and s["min_dist"] == 0.0
        assert np.array_equal(s["u"].numpy(), start)
    assert works()["converged"]
    none = hip.DeflationOperator(2, 1.0, [], autodiff=True)
    s = hip.newton_deflated_native(prob, none, X0, p, ls, tol=TOL, max_iterations=50, norm_inf=True, stop_plain=False)
    s0 = hip.newton_native(prob, X0, p, ls, tol=TOL, max_iterations=50, norm_inf=True)
    assert s["converged"] and s["itnewton"] == s0["itnewton"] and s["itlineartot"] == s0["itlineartot"] and s["M"] == 1.0
    assert np.array_equal(s["u"].numpy(), s0["u"].numpy()) and s["residuals"] == s0["residuals"] and math.isinf(s["min_dist"])
    with pytest.raises(ValueError, match="autodiff"):
        hip.newton_deflated_native(prob, hip.DeflationOperator(2, 1.0, [op.roots[0]]), X0, p, ls, stop_plain=True)
    assert works()["converged"]


# ------------------------------------------------------------------------------------------ 4: first points
@pytest.mark.parametrize("N,dp", [(2, 0.008), (2, 0.002), (3, 1e-4)], ids=["16x16-0.008", "16x16-0.002", "8x8x8-1e-4"])
def test_first_points_on_the_trivial_branch(N, dp):
    """The normal form at u = 0, p = l* in the axis basis (bk_normal_form_nd) -> predictor -> get_first_points_on_branch with
    GMRESKrylovKit(40), reltol 1e-10 and Pl = (L1 + I)^-1: 8 states after and none before (N = 2), 26 before and none after
    (N = 3), none lost; pairwise at least half the restatement's smallest distance apart; every state a zero of the oracle's F to
    10 tol; 4 rolls + 4 squares, 6 + 12 + 8 by mode coordinates."""
    hip, ND = _lib()
    from bk_amd import continuation as Cn
    c = MC.sh_case(N, 0.0)
    ref = MC.sh_first_points(N, 0.0, dp)
    side, other = ("after", "before") if N == 2 else ("before", "after")
    want = 8 if N == 2 else 26
    ctx = hip.Context(0)
    prob = hip.SwiftHohenberg(ctx, c["dims"], c["ls"], l=c["p"], nu=c["nu"])
    ls = _solver(hip, prob)
    bp = ND.normal_form_nd_native(prob, prob.vec(np.zeros(c["op"].N)), c["p"], [prob.vec(z) for z in c["Z"].T], ls)
    assert bp.converged and bp.type == f"{N}-d"
    zeros = ND.predictor(bp, dp)
    assert len(zeros[side]) == want + 1 and len(zeros[other]) == 1
    nopt = Cn.NewtonPar(tol=TOL, max_iterations=20, linsolver=ls)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                                # a lost zero would warn
        fp = ND.get_first_points_on_branch(bp, zeros, prob, ls, nopt, dp, normC=Cn.norminf)
    print([(r["side"], r["status"], r["itnewton"], r["residual"], r["min_dist"]) for r in fp.records])
    assert fp.count(side, "found") == want and fp.count(other, "found") == 0
    assert all(r["status"] in ("found", "trivial") for r in fp.records) and fp.count(side, "trivial") == 1
    held = getattr(fp, side)
    assert len(held) == want + 1 and len(getattr(fp, other)) == 1
    assert (fp.bpp, fp.bpm) == (c["p"] + dp, c["p"] - dp)
    states = [r.numpy() for r in held.roots]
    probe(f"multicont.first_points_distance.N{N}.dp{dp}", 0.5 * MC.smallest_pairwise_distance(ref[side]),
          MC.smallest_pairwise_distance(states))
    pside = fp.bpp if N == 2 else fp.bpm
    for x in states[1:]:
        probe(f"multicont.first_points_residual.N{N}.dp{dp}", np.abs(c["F"](x, pside)).max(), 10 * TOL)
    assert MC.class_counts(c["Q"], states[1:]) == ({1: 4, 2: 4} if N == 2 else {1: 6, 2: 12, 3: 8})
    assert np.abs(states[0]).max() == 0.0 and held.roots[0] is not bp.x0
    ctx.close()


# ------------------------------------------------------------------------------------------ 5: end to end
def test_nd_point_to_eight_branches_end_to_end(ctx):
    """continuation_native along u = 0 of 16 x 16 SH through l* with bisection records a point of type "nd" -> multicontinuation
    (normal form -> predictor -> first points at dp = 0.008 -> one PALC run of three steps per state) returns 8 branches.  On each
    p moves monotonically away from bp.p, |u|_inf grows, every saved point is a zero of the oracle's F to 10 tol, and the
    (p, |u|_inf) pairs agree with the oracle's PALC restatement started from the same two points to 1e-8 (the branch tolerance
    of test_gpu_parity).  continuation_from_branch_point on the same point still raises."""
    hip, ND = _lib()
    from bk_amd import continuation as Cn
    from bk_amd import normal_form1d as N1
    c = MC.sh_case(2, 0.0)
    dims, ls, nu, lstar, op = c["dims"], c["ls"], c["nu"], c["p"], c["op"]
    n = op.N
    prob = hip.SwiftHohenberg(ctx, dims, ls, l=lstar - 0.03, nu=nu)
    Pd = hip.DCTPreconditioner(prob, 1.0)
    ls_ = hip.GMRESKrylovKit(dim=40, rtol=RELTOL, atol=1e-13, maxiter=50, Pl=Pd)
    els = hip.KrylovLSSymmetric("minres", rtol=1e-10, atol=1e-13, itmax=4000, Pl=Pd)
    eig = hip.ShiftInvert(0.3, els, tol=1e-10, maxiter=20, krylovdim=40, hermitian=True, save_vectors=True)
    nopt = Cn.NewtonPar(tol=TOL, max_iterations=20, linsolver=ls_, eigsolver=eig)
    cp = Cn.ContinuationPar(ds=0.02, dsmin=1e-4, dsmax=0.03, p_min=-0.1, p_max=0.1, max_steps=60, nev=8, newton_options=nopt,
                            n_inversion=16, max_bisection_steps=60, dsmin_bisection=1e-12)
    alg = Cn.PALC(tangent="secant", theta=0.5, bls=hip.BorderingBLS(None, check_precision=False))
    br = Cn.continuation_native(prob, prob.vec(np.zeros(n)), lstar - 0.03, alg, cp, normC=Cn.norminf, bisection=True, save_sol=True)
    ib = [i for i, sp in enumerate(br.specialpoint) if sp.get("type") == "nd"]
    assert ib, br.specialpoint
    dp, ds = 0.008, 0.01
    cps = replace(cp, ds=ds, dsmin=ds, dsmax=ds, max_steps=3, detect_bifurcation=0, p_min=lstar - 0.2, p_max=lstar + 0.2)
    branches, fp = ND.multicontinuation(br, ib[0], prob, alg, cps, delta_p=dp, normC=Cn.norminf, save_sol=True)
    assert len(branches) == 8 and fp.count("after", "found") == 8 and fp.count("after", "lost") == 0 and len(fp.before) == 1
    bp = branches[0].bp
    assert isinstance(bp, ND.NdBranchPoint) and all(isinstance(B, N1.Branch) and B.bp is bp for B in branches)
    oprob = palc.Problem(c["F"], c["J"], dparam_factor=lambda x_, p_: x_)
    obls = lambda *a, **k_: bordered.bordering_bls(bordered.default_ls, *a, check_precision=False, **k_)
    for k, B in enumerate(branches):
        nb = B.branch
        amp = [float(np.abs(v.numpy()).max()) for v in nb.sol]
        print(f"branch {k}: p {nb.param} |u|_inf {amp} itnewton {nb.itnewton}")
        assert len(nb.param) == 4 and nb.param[0] == bp.p and nb.ds[0] == ds
        assert np.all(np.diff(nb.param) > 0) and amp[0] == 0.0 and np.all(np.diff(amp) > 0)
        for v, p_ in zip(nb.sol[1:], nb.param[1:]):
            probe("multicont.e2e_residual", np.abs(c["F"](v.numpy(), p_)).max(), 10 * TOL)
        x1 = fp.after.roots[1 + k].numpy()
        ob = N1R.continuation_two_points(oprob, np.zeros(n), bp.p, x1, fp.bpp, ls=bordered.default_ls, bls=obls, ds=ds, dsmin=ds,
                                         dsmax=ds, theta=0.5, p_min=lstar - 0.2, p_max=lstar + 0.2, max_steps=3, tol=TOL,
                                         max_iterations=20, normC=palc.norminf)
        assert len(ob.param) == 4
        for i in range(4):
            probe(f"multicont.e2e_branch_p.{i}", abs(nb.param[i] - ob.param[i]), 1e-8, branch=k)
            probe(f"multicont.e2e_branch_amp.{i}", abs(amp[i] - float(np.abs(ob.sol[i]).max())), 1e-8, branch=k)
    assert MC.class_counts(c["Q"], [B.branch.sol[-1].numpy() for B in branches]) == {1: 4, 2: 4}
    # the stages decoupled: the same branches from the record and the first points computed above
    again, fp2 = ND.multicontinuation(br, bp, prob, alg, cps, delta_p=dp, first_points=fp, normC=Cn.norminf)
    assert fp2 is fp and [B.branch.param for B in again] == [B.branch.param for B in branches]
    with pytest.raises(NotImplementedError, match="multicontinuation"):
        N1.continuation_from_branch_point(br, ib[0], prob, alg, cps, eig=eig, normC=Cn.norminf)
