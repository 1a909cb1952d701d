"""GPU tests of the normal form at branch points with 2-d and 3-d kernels of the Swift-Hohenberg problems (bk_nfnd_dots,
bk_nfnd_rhs, bk_nfnd_contract, bk_normal_form_nd; bk_amd.normal_form_nd): the fused passes against NumPy bit for bit and against
extended-precision sums, the normal form -- native against the call-by-call mirror, closed forms and the dense restatement
(tests/normal_form_nd_ref.py) -- on the trivial branch and at generic states, and detect -> normal form -> predictor -> Newton on
the predicted states end to end.

Tolerances of the solver-dependent comparisons follow DESIGN sections 9e / 9g: the yardstick is the restatement's own spread at the
same point, its direct bordered solve against SciPy GMRES on the same (n + N) system, left-preconditioned by the exact
(L1 + I)^-1 and stopped on the preconditioned residual at the test's reltol; 10 x that spread is allowed, plus the rounding
4 n eps sum |terms| of a coefficient's fixed-order sum and, on the trivial branch, 10 x the restatement's own distance from the
closed form (the two CPU solvers share one rounded J; the closed form does not).  Every bound is logged next to its measured
value by ``probe``."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import minaug_fold_ref as R
import normal_form1d_ref as N1R
import normal_form_nd_ref as M
from conftest import probe
from oracle import operators

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
RELTOL = 1e-10
LD = np.longdouble


def _lib():
    from bk_amd import hip
    from bk_amd import normal_form_nd as ND
    return hip, ND


def _guarded(hip, ctx, a, off, fill=None):
    """A device vector of len(a) doubles between NaN guards, ``off`` doubles (2: 16-byte aligned, 1: one double off) into a fresh
    buffer; ``fill`` None copies a, else the vector starts as that value (outputs: NaN)."""
    import torch
    n = a if isinstance(a, int) else a.shape[0]
    t = torch.full((n + 4,), float("nan"), dtype=torch.float64, device=ctx.torch_device)
    if fill is None:
        t[off:off + n] = torch.from_numpy(np.ascontiguousarray(a)).to(ctx.torch_device)
    v = type("GuardedVec", (hip.HipVec,), {})(ctx, t[off:off + n], n)            # a subclass: room for the whole buffer
    assert v.t.data_ptr() % 16 == (0 if off == 2 else 8)
    v._whole = t
    return v


def _guards_intact(v):
    w = v._whole.cpu().numpy()
    n = v.n
    off = (v.t.data_ptr() - v._whole.data_ptr()) // 8
    return bool(np.isnan(w[:off]).all() and np.isnan(w[off + n:]).all())


def _problem(hip, ctx, kind, n):
    if kind == "sh1d":
        return hip.SwiftHohenberg1D(ctx, n, 6.0, lam=-0.7, nu=2.0), [-0.7, 2.0]
    a = next(d for d in range(int(math.isqrt(n)), 1, -1) if n % d == 0)
    return hip.SwiftHohenberg(ctx, (n // a, a), (np.pi, np.pi), l=-0.2, nu=1.3), [-0.2, 1.3]


def _ld(t):
    """(extended-precision sum, sum of absolute values) of a vector of terms: the reference of one device sum, computed once."""
    return float(np.sum(t.astype(LD))), float(np.abs(t).sum())


def _check_sum(name, got, ref, n):
    """|device sum - extended-precision sum| <= 4 n eps sum |terms|, the bound of the reducing passes of section 9e."""
    probe(name, abs(got - ref[0]) / (4 * n * EPS * ref[1] + 1e-300), 1.0)


def _rhs_raw(ND, prob, X, pars, ip, Z, a01, b20p, outs):
    from bk_amd.codim2 import _carr, _vptrs
    from bk_amd.hip import _ptr
    ctx = prob.ctx
    ctx.check(ctx.lib.bk_nfnd_rhs(prob.h, _ptr(X.t), _carr(pars), len(pars), ip, len(Z), _vptrs(Z),
                                  _carr([float(v) for v in np.ravel(a01)]), _carr([float(v) for v in np.ravel(b20p)]), _vptrs(outs)),
              "bk_nfnd_rhs")


# lengths of the issue; a 2-D grid needs two factors >= 2, so the SH polynomials run at the lengths that have them, and at
# 66177 = 387 x 171 in place of the primes 257 and 65537: odd (the last-element path) and more than one block
LENGTHS = [2, 3, 255, 256, 257, 4097, 65537, 1 << 22]
SH_LENGTHS = [255, 256, 4097, 66177, 1 << 22]
PASS_CASES = [(k, N, n) for k in ("sh1d", "sh") for N in (2, 3) for n in (LENGTHS if k == "sh1d" else SH_LENGTHS)]


# ------------------------------------------------------------------------------------------ 1: the passes alone
@pytest.mark.parametrize("kind,N,n", PASS_CASES, ids=lambda v: str(v))
def test_passes_match_numpy(ctx, kind, N, n):
    """bk_nfnd_rhs bit for bit against NumPy in the kernel's operation order; every sum of bk_nfnd_dots / bk_nfnd_contract within
    4 n eps sum |terms| of the NumPy longdouble sum.  Both parameters; every stream 16-byte aligned, and one stream (a different
    one per pass) one double off, which takes the element path; odd n takes the last-element path; n = 2^22 aligned the
    non-temporal instantiations, and one double off the only length at which a thread of the element path strides the grid a
    second time (more than 1024 x 256 elements for the sums, 4096 x 256 for the writes).  Operands sit between NaN guards,
    outputs start as NaN.  The zeta are random and distinct, so a wrong pair or triple index shows against NumPy directly.  The
    NumPy references are computed once per parameter and shared by the two alignments."""
    hip, ND = _lib()
    prob, pars = _problem(hip, ctx, kind, n)
    assert prob.nlocal == n
    rng = np.random.default_rng(1000 * N + n % 9973)
    P = len(M.pairs(N))
    u = rng.standard_normal(n)
    zs = [rng.standard_normal(n) for _ in range(N)]
    p01 = rng.standard_normal(n)
    qs = [rng.standard_normal(n) for _ in range(P)]
    a01c, b20c = rng.standard_normal(N), rng.standard_normal((N, P))
    ref = {}
    for ip in (0, 1):
        ta01, tb20, tg = M.dots_terms(kind, pars[1], ip, u, zs)
        dots = ([_ld(t) for t in ta01], [[_ld(t) for t in row] for row in tb20], [[_ld(t) for t in row] for row in tg])
        del ta01, tb20, tg
        tb11, ta02, tb30 = M.contract_terms(kind, pars[1], ip, u, zs, p01, qs)
        con = ([[_ld(t) for t in row] for row in tb11], [_ld(t) for t in ta02], [[_ld(t) for t in row] for row in tb30])
        del tb11, ta02, tb30
        ref[ip] = (dots, con, M.rhs_exact(kind, pars[1], ip, u, zs, a01c, b20c))
    for mis in (None, 1):
        off = lambda j: 1 if mis is not None and j == mis else 2
        U = _guarded(hip, ctx, u, 2)
        Z = [_guarded(hip, ctx, z, off(j)) for j, z in enumerate(zs)]                       # dots / rhs: zeta_1 off
        P01 = _guarded(hip, ctx, p01, 2)
        Q = [_guarded(hip, ctx, q, off(j + 1)) for j, q in enumerate(qs)]                   # contract: zeta_1 and Psi_00 off
        tag = f"{kind}.N{N}.n{n}.{'aligned' if mis is None else 'off8'}"
        for ip in (0, 1):
            (ra01, rb20, rg), (rb11, ra02, rb30), rhs = ref[ip]
            a01, b20p, gram = ND.nfnd_dots(prob, U, pars, ip, Z)
            for i in range(N):
                _check_sum(f"nfnd.dots_a01.{tag}", a01[i], ra01[i], n)
                for k in range(P):
                    _check_sum(f"nfnd.dots_b20.{tag}", b20p[i, k], rb20[i][k], n)
                for j in range(N):
                    _check_sum(f"nfnd.dots_gram.{tag}", gram[i, j], rg[i][j], n)
            outs = [_guarded(hip, ctx, n, 2 if mis is None else (1 if j == 0 else 2), fill="nan") for j in range(1 + P)]
            _rhs_raw(ND, prob, U, pars, ip, Z, a01c, b20c, outs)
            for o, e in zip(outs, rhs):
                assert np.array_equal(o.numpy(), e), (tag, ip, np.abs(o.numpy() - e).max())
                assert _guards_intact(o)
            b11, a02, b30p = ND.nfnd_contract(prob, U, pars, ip, Z, P01, Q)
            for i in range(N):
                _check_sum(f"nfnd.contract_a02.{tag}", a02[i], ra02[i], n)
                for j in range(N):
                    _check_sum(f"nfnd.contract_b11.{tag}", b11[i, j], rb11[i][j], n)
                for k in range(len(M.triples(N))):
                    _check_sum(f"nfnd.contract_b30.{tag}", b30p[i, k], rb30[i][k], n)
        assert all(_guards_intact(v) for v in [U, P01] + Z + Q)


@pytest.mark.parametrize("N", [2, 3])
def test_swapped_kernel_vectors_give_the_permuted_outputs(ctx, N):
    """zeta_1 and zeta_2 (0-based: the last two) swapped: every output moves to the permuted index, pairs and triples re-sorted.
    The two calls order the products of an element differently, so they agree to the sum bound of both, 8 n eps sum |terms|."""
    hip, ND = _lib()
    n = 257
    prob, pars = _problem(hip, ctx, "sh1d", n)
    rng = np.random.default_rng(77 + N)
    u, p01 = rng.standard_normal(n), rng.standard_normal(n)
    zs = [rng.standard_normal(n) for _ in range(N)]
    pr, tr = M.pairs(N), M.triples(N)
    qs = [rng.standard_normal(n) for _ in pr]
    perm = list(range(N))
    perm[-1], perm[-2] = perm[-2], perm[-1]
    sp = lambda *I: tuple(sorted(perm[i] for i in I))
    zs2 = [zs[perm[i]] for i in range(N)]
    qs2 = [qs[pr.index(sp(j, k))] for j, k in pr]                                      # Psi'_jk = Psi_{perm j, perm k}
    V = prob.vec
    for ip in (0, 1):
        a, b, g = ND.nfnd_dots(prob, V(u), pars, ip, [V(z) for z in zs])
        a2, b2, g2 = ND.nfnd_dots(prob, V(u), pars, ip, [V(z) for z in zs2])
        ta, tb, tg = M.dots_terms("sh1d", pars[1], ip, u, zs)
        bound = lambda t: 8 * n * EPS * float(np.abs(t).sum())
        for i in range(N):
            probe("nfnd.swap_a01", abs(a2[i] - a[perm[i]]) / bound(ta[perm[i]]), 1.0)
            for k, (j, l) in enumerate(pr):
                k0 = pr.index(sp(j, l))
                probe("nfnd.swap_b20", abs(b2[i, k] - b[perm[i], k0]) / bound(tb[perm[i]][k0]), 1.0)
            for j in range(N):
                probe("nfnd.swap_gram", abs(g2[i, j] - g[perm[i], perm[j]]) / bound(tg[perm[i]][perm[j]]), 1.0)
        c = ND.nfnd_contract(prob, V(u), pars, ip, [V(z) for z in zs], V(p01), [V(q) for q in qs])
        c2 = ND.nfnd_contract(prob, V(u), pars, ip, [V(z) for z in zs2], V(p01), [V(q) for q in qs2])
        t11, t02, t30 = M.contract_terms("sh1d", pars[1], ip, u, zs, p01, qs)
        for i in range(N):
            probe("nfnd.swap_a02", abs(c2[1][i] - c[1][perm[i]]) / bound(t02[perm[i]]), 1.0)
            for j in range(N):
                probe("nfnd.swap_b11", abs(c2[0][i, j] - c[0][perm[i], perm[j]]) / bound(t11[perm[i]][perm[j]]), 1.0)
            for k, t in enumerate(tr):
                k0 = tr.index(sp(*t))
                probe("nfnd.swap_b30", abs(c2[2][i, k] - c[2][perm[i], k0]) / bound(t30[perm[i]][k0]), 1.0)
        # the data tell the indices apart: without the permutation the outputs differ by far more than the bound
        assert abs(c2[2][0, 1] - c[2][0, 1]) > 1e3 * bound(t30[0][1])


# ------------------------------------------------------------------------------------------ 2: whole call, shared pieces
def _solver(hip, prob, maxiter=50):
    return hip.GMRESKrylovKit(dim=40, rtol=RELTOL, atol=1e-13, maxiter=maxiter, Pl=hip.DCTPreconditioner(prob, 1.0))


def _names(N):
    return ["a01", "a02", "b11", "b20", "b30"]


def _spread(model, d3F, x, q, lens, zs, lu, Pl):
    """10 x |SciPy GMRES on the preconditioned (n + N) system at RELTOL - direct bordered solve| of the restatement, per array
    (the largest entry) and per Psi vector (the largest over all of them)."""
    gm = M.normal_form_nd(model, d3F, x, q, lens, zs, solver="gmres", reltol=RELTOL, Pl=Pl)
    al = {k: 10 * float(np.abs(gm[k] - lu[k]).max()) for k in _names(0)}
    al["Psi"] = 10 * max([np.abs(gm["Psi01"] - lu["Psi01"]).max()] + [np.abs(gm["Psi2"][jk] - lu["Psi2"][jk]).max() for jk in lu["Psi2"]])
    return al


def _sum_rounding(kind, nu, ip, x, zs, lu):
    """4 n eps sum |terms| of the fixed-order sums, the largest over the entries of each array, on the restatement's vectors."""
    n, N = x.shape[0], len(zs)
    ta01, tb20, _ = M.dots_terms(kind, nu, ip, x, zs)
    t11, t02, t30 = M.contract_terms(kind, nu, ip, x, zs, lu["Psi01"], [lu["Psi2"][jk] for jk in M.pairs(N)])
    mx = lambda ts: 4 * n * EPS * max(float(np.abs(t).sum()) for t in ts)
    flat = lambda rows: [t for row in rows for t in row]
    return dict(a01=mx(ta01), b20=mx(flat(tb20)), b11=mx(flat(t11)), a02=mx(t02), b30=mx(flat(t30)), Psi=0.0)


def _device_arrays(bp):
    nf = bp.nf
    return dict(a01=nf.a01, a02=nf.a02, b11=nf.b11, b20=nf.b20, b30=nf.b30)


def _compare(tag, bp, lu, allowed):
    got = _device_arrays(bp)
    for k in _names(0):
        d = float(np.abs(got[k] - lu[k]).max())
        probe(f"nfnd.{tag}_{k}", d, allowed[k], relative=d / max(float(np.abs(lu[k]).max()), 1e-300))
    N = bp.N
    psis = [(bp.nf.Psi01, lu["Psi01"])] + [(bp.nf.Psi2[jk], lu["Psi2"][jk]) for jk in M.pairs(N)]
    probe(f"nfnd.{tag}_Psi", max(float(np.abs(g.numpy() - e).max()) for g, e in psis), allowed["Psi"])


def _few_ulp(tag, na, mi):
    """Native against mirror: the same kernels and solves in the same order (the native call only shares Pl^-1 zeta_j), 8 ulp."""
    a, b = _device_arrays(na), _device_arrays(mi)
    for k in _names(0):
        scale = float(np.abs(a[k]).max())
        probe(f"nfnd.{tag}_native_vs_mirror_{k}", float(np.abs(a[k] - b[k]).max()), 8 * EPS * max(scale, 1e-300) + 0.0, tight=0.0)
    assert na.itlinear == mi.itlinear and na.type == mi.type, (na.itlinear, mi.itlinear)


TRIVIAL = {
    2: dict(dims=(16, 16), ls=(np.pi, np.pi), modes=[(1, 2), (2, 1)], nu=1.3),
    3: dict(dims=(8, 8, 8), ls=(2.5, 2.5, 2.5), modes=[(2, 0, 0), (0, 2, 0), (0, 0, 2)], nu=0.9),
}


def _rotation(N, th=0.3):
    c, s = math.cos(th), math.sin(th)
    Rm = np.eye(N)
    Rm[:2, :2] = [[c, s], [-s, c]]
    if N == 3:                                                   # a second plane, so every vector of the basis moves
        R2 = np.eye(3)
        R2[1:, 1:] = [[math.cos(0.5), math.sin(0.5)], [-math.sin(0.5), math.cos(0.5)]]
        Rm = R2 @ Rm
    return Rm


# ------------------------------------------------------------------------------------------ 3: the trivial branch
@pytest.mark.parametrize("N", [2, 3])
@pytest.mark.parametrize("basis", ["axis", "rotated"])
def test_normal_form_on_the_trivial_branch(N, basis):
    """u = 0 at p = l* exactly (the bordered matrix is regular there): 16 x 16, modes (1, 2), (2, 1), nu = 1.3 (N = 2) and
    8 x 8 x 8, half-lengths 2.5, modes (2,0,0), (0,2,0), (0,0,2), nu = 0.9 (N = 3), in the axis basis and in a rotated one.  Native
    and mirror on fresh contexts against the restatement -- and in the axis basis the diagonal of b30 against the closed form --
    and against each other to 8 ulp.  All 1 + P solves converge and the counter stays 0."""
    hip, ND = _lib()
    c = TRIVIAL[N]
    dims, ls, nu = c["dims"], c["ls"], c["nu"]
    lz = [M.sh_cos_mode(dims, ls, m) for m in c["modes"]]
    p = lz[0][0]
    assert all(l == p for l, _ in lz)
    zs = [z for _, z in lz]
    Rm = _rotation(N) if basis == "rotated" else np.eye(N)
    zr = [sum(Rm[i, a] * zs[a] for a in range(N)) for i in range(N)] if basis == "rotated" else zs
    op = operators.SwiftHohenberg(dims, ls)
    n = op.N
    model = R.sh_model(op, "sh", dict(l=p, nu=nu), "l")
    d3F = N1R.sh_d3F("sh", ["l", "nu"])
    zero = np.zeros(n)
    lu = M.normal_form_nd(model, d3F, zero, model.at(p), "l", zr)
    allowed = _spread(model, d3F, zero, model.at(p), "l", zr, lu, operators.dct_preconditioner(dims, ls, 1.0))
    # the restatement's distance from the closed form, measured in the axis basis on the diagonal of b30 and carried to the
    # rotated basis index by index: at most (|c| + |s|)^4 per plane rotation
    lu0 = lu if basis == "axis" else M.normal_form_nd(model, d3F, zero, model.at(p), "l", zs)
    cf = [M.sh_cos_closed_form_diag(dims, ls, m, nu) for m in c["modes"]]
    acf = 10 * max(abs(lu0["b30"][i, i, i, i] - cf[i]) for i in range(N)) * float(np.abs(Rm).sum(axis=1).max()) ** 4
    rnd = _sum_rounding("sh", nu, 0, zero, zr, lu)
    allowed = {k: allowed[k] + rnd[k] + (acf if k == "b30" else 0.0) for k in allowed}
    print(f"N = {N} {basis}: l* = {p:.16g}, closed-form b30 diagonal {cf}, allowed {allowed}")
    out = {}
    for kind in ("native", "mirror"):
        ctx = hip.Context(0)
        prob = hip.SwiftHohenberg(ctx, dims, ls, l=p, nu=nu)
        ls_ = _solver(hip, prob)
        Z = [prob.vec(z) for z in zr]
        f = ND.normal_form_nd_native if kind == "native" else ND.normal_form_nd
        out[kind] = bp = f(prob, prob.vec(zero), p, Z, ls_)
        print(f"{kind}: b11 diag {np.diag(bp.nf.b11)} b30 diag {[bp.nf.b30[i, i, i, i] for i in range(N)]} type {bp.type} "
              f"converged {bp.converged} itlinear {bp.itlinear}")
        assert bp.type == f"{N}-d" and bp.converged is True and len(bp.itlinear) == 1 + len(M.pairs(N))
        _compare(f"trivial{N}_{basis}.{kind}", bp, lu, allowed)
        if basis == "axis":
            for i in range(N):
                probe(f"nfnd.trivial{N}_closed_form_b30.{kind}", abs(bp.nf.b30[i, i, i, i] - cf[i]), allowed["b30"])
        if kind == "native":
            assert bp.unconverged_solves == 0 and ctx.get_option("nfnd_unconverged_solves") == 0.0
        assert bp.p == p and bp.lens == "l" and bp.params == [p, nu] and bp.zeta_star == bp.zeta
        ctx.close()
    _few_ulp(f"trivial{N}_{basis}", out["native"], out["mirror"])


# ------------------------------------------------------------------------------------------ 4: a generic state
@pytest.mark.parametrize("dims,ls,N", [((16, 12), (7.0, 5.0), 2), ((8, 8, 8), (2.5, 2.5, 2.5), 3)], ids=["16x12", "8x8x8"])
@pytest.mark.parametrize("lens", ["l", "nu"])
def test_normal_form_at_a_generic_state(dims, ls, N, lens):
    """u = 0.3 x random, zeta random and orthonormalised, both parameters: every coefficient is alive (a01, a02, b20 != 0).  Native
    and mirror against the restatement's direct solve: 10 x its spread plus the rounding of the sums."""
    hip, ND = _lib()
    nu, l = 1.2, 0.05
    op = operators.SwiftHohenberg(dims, ls)
    n = op.N
    rng = np.random.default_rng(31 + N)
    x = 0.3 * rng.standard_normal(n)
    zs = list(np.linalg.qr(rng.standard_normal((n, N)))[0].T)
    model = R.sh_model(op, "sh", dict(l=l, nu=nu), lens)
    p = l if lens == "l" else nu
    q = model.at(p)
    d3F = N1R.sh_d3F("sh", ["l", "nu"])
    lu = M.normal_form_nd(model, d3F, x, q, lens, zs)
    allowed = _spread(model, d3F, x, q, lens, zs, lu, operators.dct_preconditioner(dims, ls, 1.0))
    rnd = _sum_rounding("sh", nu, 0 if lens == "l" else 1, x, zs, lu)
    allowed = {k: allowed[k] + rnd[k] for k in allowed}
    assert min(float(np.abs(lu[k]).min()) for k in _names(0)) > 1e-6                           # all alive
    print(f"{dims} in {lens}: allowed {allowed}")
    out = {}
    for kind in ("native", "mirror"):
        ctx = hip.Context(0)
        prob = hip.SwiftHohenberg(ctx, dims, ls, l=l, nu=nu, lens=lens)
        ls_ = _solver(hip, prob, maxiter=200)
        f = ND.normal_form_nd_native if kind == "native" else ND.normal_form_nd
        out[kind] = bp = f(prob, prob.vec(x), p, [prob.vec(z) for z in zs], ls_)
        print(f"{kind}: a01 {bp.nf.a01} a02 {bp.nf.a02} converged {bp.converged} itlinear {bp.itlinear}")
        assert bp.type == lu["type"] and bp.converged is True
        _compare(f"generic{N}_{lens}.{kind}", bp, lu, allowed)
        ctx.close()
    _few_ulp(f"generic{N}_{lens}", out["native"], out["mirror"])


# ------------------------------------------------------------------------------------------ 5: end to end
DP_ROLL, DP_SQUARE = 0.05, 0.008


def _ratio(newton, Z, bp_like, predict, dp, pick):
    """|<x, zeta_i> - root|_inf of the Newton solution from the predicted state ``pick`` at dp and at dp / 2, and the two solutions."""
    out = []
    for d in (dp, dp / 2):
        r = pick(predict(d))
        x = newton(r, d)
        out.append((float(np.abs(Z.T @ x - r).max()), x, r))
    return out[0][0] / out[1][0], out


def test_nd_point_to_normal_form_predictor_and_newton_end_to_end(ctx):
    """continuation_native along u = 0 of 16 x 16 SH through l* with bisection records a point of type "nd" with |delta n_unstable| = 2
    -> get_normal_form_nd: zeta span the two cosine modes, b30 equals the restatement evaluated with the device's zeta at the
    device's p -> predictor: 1 zero before, 9 after -> bk_newton from the predicted roll and square states converges to two
    distinct non-zero solutions, and the distance between <x, zeta_i> and the predicted zero falls by at least 3 when dp is halved.

    That last ratio tends to 2^(3/2) = 2.83 as dp -> 0 (the amplitude is sqrt(dp) (c0 + c1 dp + ...), the predictor keeps c0), so it
    exceeds 3 only in a window of dp, measured with the restatement on the CPU (dense Newton): rolls 2.96 at dp = 0.04, 3.07 at 0.05,
    3.49 at 0.07 and 2.83 below 0.01; squares 3.55 at dp = 0.008, 3.07 at 0.004, 2.93 at 0.002, and Newton leaves the square branch
    above 0.012.  Each state is therefore checked at its own dp, 0.05 for the roll and 0.008 for the square; the restatement does the
    same first with the device's zeta and coefficients."""
    hip, ND = _lib()
    import scipy.sparse.linalg as spla

    from bk_amd import continuation as Cn
    c = TRIVIAL[2]
    dims, ls, nu = c["dims"], c["ls"], c["nu"]
    n = dims[0] * dims[1]
    (lstar, z1), (_, z2) = (M.sh_cos_mode(dims, ls, m) for m in c["modes"])
    tol = 1e-10
    prob = hip.SwiftHohenberg(ctx, dims, ls, l=lstar - 0.03, nu=nu)
    Pd = hip.DCTPreconditioner(prob, 1.0)
    ls_ = hip.GMRESKrylovKit(dim=40, rtol=RELTOL, atol=1e-13, maxiter=50, Pl=Pd)
    els = hip.KrylovLSSymmetric("minres", rtol=1e-10, atol=1e-13, itmax=4000, Pl=Pd)
    eig = hip.ShiftInvert(0.3, els, tol=1e-10, maxiter=20, krylovdim=40, hermitian=True, save_vectors=True)     # J - 0.3 < 0 for l < 0.3
    nopt = Cn.NewtonPar(tol=tol, max_iterations=20, linsolver=ls_, eigsolver=eig)
    cp = Cn.ContinuationPar(ds=0.02, dsmin=1e-4, dsmax=0.03, p_min=-0.1, p_max=0.1, max_steps=60, nev=8, newton_options=nopt,
                            n_inversion=16, max_bisection_steps=60, dsmin_bisection=1e-12)
    alg = Cn.PALC(tangent="secant", theta=0.5, bls=hip.BorderingBLS(None, check_precision=False))
    br = Cn.continuation_native(prob, prob.vec(np.zeros(n)), lstar - 0.03, alg, cp, normC=Cn.norminf, bisection=True, save_sol=True)
    ib = [i for i, sp in enumerate(br.specialpoint) if sp.get("type") == "nd"]
    print("special points:", br.specialpoint, "l* =", lstar)
    assert ib, br.specialpoint
    sp = br.specialpoint[ib[0]]
    assert abs(sp["n_unstable"][0] - sp["n_unstable"][1]) == 2
    assert sp["interval"][0] - 1e-9 <= lstar <= sp["interval"][1] + 1e-9
    bp = ND.get_normal_form_nd(br, ib[0], prob, ls_, eig=eig)
    assert isinstance(bp, ND.NdBranchPoint) and bp.N == 2 and bp.type == "2-d" and bp.lens == "l" and bp.converged
    assert bp.p == sp["param"] and np.abs(bp.x0.numpy()).max() == 0.0 and bp.unconverged_solves == 0
    Z = np.stack([z.numpy() for z in bp.zeta], axis=1)
    probe("nfnd.e2e_gram", np.abs(Z.T @ Z - np.eye(2)).max(), 1e-12)
    # principal angles between span(zeta) and the two cosine modes: the sines are the singular values of (I - Q Q') Z
    Q = np.stack([z1, z2], axis=1)
    probe("nfnd.e2e_zeta_vs_modes", np.linalg.svd(Z - Q @ (Q.T @ Z), compute_uv=False).max(), 1e-6)
    op = operators.SwiftHohenberg(dims, ls)
    model = R.sh_model(op, "sh", dict(l=bp.p, nu=nu), "l")
    d3F = N1R.sh_d3F("sh", ["l", "nu"])
    zero = np.zeros(n)
    zs = [Z[:, 0], Z[:, 1]]
    lu = M.normal_form_nd(model, d3F, zero, model.at(bp.p), "l", zs)
    allowed = _spread(model, d3F, zero, model.at(bp.p), "l", zs, lu, operators.dct_preconditioner(dims, ls, 1.0))
    rnd = _sum_rounding("sh", nu, 0, zero, zs, lu)
    allowed = {k: allowed[k] + rnd[k] for k in allowed}
    print("e2e: device b30", bp.nf.b30.ravel(), "restatement", lu["b30"].ravel(), "allowed", allowed, "itlinear", bp.itlinear)
    _compare("e2e", bp, lu, allowed)
    # predictor with its defaults: counts on both sides at both steps
    pred = lambda d: ND.predictor(bp, d)
    for d in (DP_ROLL, DP_SQUARE):
        pr = pred(d)
        assert len(pr["before"]) == 1 and len(pr["after"]) == 9, (d, len(pr["before"]), len(pr["after"]))
    # the basis the eigensolver returns is rotated against the modes by an arbitrary angle: in the device's coordinates a roll is a
    # zero on the line through a mode, a square one on a diagonal between them
    A = Q.T @ Z                                                                           # mode coordinates of a zero x: A x

    def pick(kind):
        def f(pr):
            best = None
            for r in pr["after"][1:]:
                m = A @ r
                is_roll = min(abs(m)) <= 1e-6 * max(abs(m))
                if (kind == "roll") == is_roll and m[0] > 0 and (is_roll or m[1] > 0):
                    best = r
            assert best is not None, (kind, [A @ r for r in pr["after"]])
            return best
        return f

    def cpu_newton(r, d):
        x = Z @ r
        for _ in range(30):
            f = op.F(x, bp.p + d, nu)
            if np.abs(f).max() < 1e-12:
                return x
            x = x - spla.spsolve(op.J(x, bp.p + d, nu).tocsc(), f)
        raise AssertionError("dense Newton did not converge")

    nfd = dict(a01=lu["a01"], a02=lu["a02"], b11=lu["b11"], b20=lu["b20"], b30=lu["b30"])
    cpu_pred = lambda d: M.predictor(nfd, d)

    def gpu_newton(r, d):
        (x0,) = ND.predicted_states(bp, [r])
        assert np.abs(x0.numpy() - Z @ r).max() <= 6 * EPS * np.abs(Z @ r).max() + 1e-300
        s = hip.newton_native(prob, x0, bp.p + d, ls_, tol=tol, max_iterations=30, norm_inf=True)
        assert s["converged"], s["residuals"]
        return s["u"].numpy()

    sols = {}
    for kind, d in (("roll", DP_ROLL), ("square", DP_SQUARE)):
        rc, _ = _ratio(cpu_newton, Z, None, cpu_pred, d, pick(kind))
        probe(f"nfnd.e2e_ratio_cpu_{kind}", 3.0, rc, dp=d)
        rg, pts = _ratio(gpu_newton, Z, None, pred, d, pick(kind))
        probe(f"nfnd.e2e_ratio_gpu_{kind}", 3.0, rg, dp=d, distance=pts[0][0], distance_half=pts[1][0])
        sols[kind] = pts[0][1]
        assert np.abs(pts[0][1]).max() > 1e-2                                           # non-zero
    # two distinct solutions: one lives on a mode, the other on both
    mr, ms = Q.T @ sols["roll"], Q.T @ sols["square"]
    assert abs(mr[1]) <= 1e-6 * abs(mr[0]) and abs(abs(ms[0]) - abs(ms[1])) <= 1e-6 * abs(ms[0]) and abs(ms[1]) > 1e-2, (mr, ms)
    # the record as a callable: x0 + sum x_i zeta_i
    r = np.array([0.25, -0.5])
    assert np.abs(bp(r, 0.0).numpy() - Z @ r).max() <= 6 * EPS * np.abs(Z @ r).max()


# ------------------------------------------------------------------------------------------ 6: errors
def test_errors_are_refused_with_a_message_and_leave_the_library_usable():
    """N = 1 or 4; a cGL problem; a missing pl; zeta with Gram defect 1e-6; aliased outputs: each refused with a message, and an
    unrelated call afterwards still works.  maxiter = 1: converged is False, no error, the counter counts the 1 + P solves."""
    hip, ND = _lib()
    from bk_amd import _lib as L
    from bk_amd.codim2 import _carr, _vptrs
    from bk_amd.hip import _ptr
    ctx = hip.Context(0)
    dims, ls, nu, l = (16, 12), (7.0, 5.0), 1.2, 0.05
    n = dims[0] * dims[1]
    prob = hip.SwiftHohenberg(ctx, dims, ls, l=l, nu=nu)
    rng = np.random.default_rng(3)
    x = 0.3 * rng.standard_normal(n)
    q4 = np.linalg.qr(rng.standard_normal((n, 4)))[0]
    X, Z4 = prob.vec(x), [prob.vec(q4[:, i]) for i in range(4)]
    lsg = _solver(hip, prob, maxiter=200)

    def still_works():
        assert abs(Z4[0].inner(Z4[0]) - 1) <= 1e-14 and abs(Z4[0].inner(Z4[1])) <= 1e-14

    for N in (1, 4):
        with pytest.raises(L.BkHipError, match="dimension 2 and 3 only"):
            ND.normal_form_nd_native(prob, X, l, Z4[:N], lsg)
        with pytest.raises(L.BkHipError, match="dimension 2 and 3 only"):
            ND.nfnd_dots(prob, X, [l, nu], 0, Z4[:N])
        with pytest.raises(NotImplementedError):
            ND.normal_form_nd(prob, X, l, Z4[:N], lsg)
        still_works()
    cgl = hip.CGL2d(ctx, (8, 8), (1.0, 1.0))
    xc = cgl.vec(np.zeros(cgl.nglobal))
    pv = cgl._pvec(0.5)
    ls0 = hip.GMRESIterativeSolvers(reltol=1e-8, restart=10, maxiter=10, Pl=None)
    for call in (lambda: ND.nfnd_dots(cgl, xc, pv, 0, [xc, xc]), lambda: ND.nfnd_rhs(cgl, xc, pv, 0, [xc, xc], [0, 0], np.zeros((2, 3))),
                 lambda: ND.nfnd_contract(cgl, xc, pv, 0, [xc, xc], xc, [xc, xc, xc]),
                 lambda: ND.normal_form_nd_native(cgl, xc, 0.5, [xc, xc], ls0)):
        with pytest.raises(L.BkHipError, match="fold formulation"):
            call()
    still_works()
    nopl = hip.GMRESKrylovKit(dim=40, rtol=RELTOL, atol=1e-13, maxiter=50, Pl=None)
    with pytest.raises(L.BkHipError, match="left preconditioner"):
        ND.normal_form_nd_native(prob, X, l, Z4[:2], nopl)
    with pytest.raises(TypeError, match="left preconditioner"):
        ND.normal_form_nd(prob, X, l, Z4[:2], nopl)
    still_works()
    bad = prob.vec(q4[:, 1] + 1e-6 * q4[:, 0])
    with pytest.raises(L.BkHipError, match="not orthonormal"):
        ND.normal_form_nd_native(prob, X, l, [Z4[0], bad], lsg)
    with pytest.raises(ValueError, match="not orthonormal"):
        ND.normal_form_nd(prob, X, l, [Z4[0], bad], lsg)
    still_works()
    # aliased outputs: the wrappers allocate theirs, so call the entries
    lo = lsg._opts()
    o = [X.similar() for _ in range(4)]
    coef, cv, it = (C.c_double * 22)(), C.c_int(), (C.c_int * 4)()
    for psi01, psi2 in ((Z4[0], o[1:]), (o[0], [o[1], o[1], o[2]]), (o[0], [o[1], X, o[2]])):
        with pytest.raises(L.BkHipError, match="aliases an input|must be distinct"):
            ctx.check(ctx.lib.bk_normal_form_nd(ctx.h, prob.h, _ptr(X.t), _carr([l, nu]), 2, 0, 2, _vptrs(Z4[:2]), C.byref(lo), lsg._pl(),
                                                _ptr(psi01.t), _vptrs(psi2), coef, C.byref(cv), it), "bk_normal_form_nd")
    with pytest.raises(L.BkHipError, match="aliases an input"):
        ctx.check(ctx.lib.bk_nfnd_rhs(prob.h, _ptr(X.t), _carr([l, nu]), 2, 0, 2, _vptrs(Z4[:2]), _carr([0.0, 0.0]), _carr([0.0] * 6),
                                      _vptrs([o[0], o[1], Z4[1], o[2]])), "bk_nfnd_rhs")
    still_works()
    ok = ND.normal_form_nd_native(prob, X, l, Z4[:2], lsg)                                 # the unrelated call: the real thing
    assert ok.converged and ok.unconverged_solves == 0
    ls1 = hip.GMRESKrylovKit(dim=3, rtol=1e-13, atol=0.0, maxiter=1, Pl=hip.DCTPreconditioner(prob, 1.0))
    for N in (2, 3):
        b = ND.normal_form_nd_native(prob, X, l, Z4[:N], ls1)
        nsolve = 1 + len(M.pairs(N))
        assert b.converged is False and b.unconverged_solves == nsolve and len(b.itlinear) == nsolve, (b.converged, b.unconverged_solves)
        assert all(np.isfinite(v).all() for v in _device_arrays(b).values())
        m = ND.normal_form_nd(prob, X, l, Z4[:N], ls1)
        assert m.converged is False and m.itlinear == b.itlinear
    ctx.close()
