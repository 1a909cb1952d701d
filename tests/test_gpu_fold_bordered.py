"""GPU tests of the preconditioned MatrixFreeBLS (csrc/bordered.hip: bk_bordered_tail, bk_bls_matrixfree_pl,
bk_bls_block_matrixfree_pl) and of the fold formulation on it (bk_fold_border, context option fold_bordered; bk_amd.codim2 with
bls = MatrixFreeBLS(ls, use_pl=True)).

The two streaming passes are compared bitwise with host loops on data where rounding cannot occur (integers, dyadic parameters,
every partial sum below 2^53: the rule of tests/stencil_ref.py::exact).  The solver-dependent comparisons follow the yardstick
rule of DESIGN 9d-9f: the restatement (tests/minaug_bordered_ref.py) with direct solves against the restatement with SciPy GMRES at
the device's tolerance and preconditioning gives a spread, measured where the test runs; the device is allowed 10 x that spread.
Vector and scalars are each held to 10 x their OWN spread.  Both solvers of that spread apply the same assembled matrix, whose
L1 = A A is rounded entry by entry; near a singular J that rounding moves the border scalar by more than the two solves differ
(64 x 64, l - l* = 1e-9: 1.6e-10 against 2.3e-11).  So, as DESIGN 9e does on the trivial branch, a second measured yardstick is
added where one exists: the direct solve's own distance from the solve in the DCT basis, where J(0, l) is an exact diagonal
(minaug_bordered_ref.spectral_block); at the hexagon fold, which has no closed form, the direct restatement's own distance from
its Newton limit (two more iterations).  The device is allowed 10 x the sum of the two, per component.
Counts: within 2 Arnoldi steps of SciPy's per solve.  The KrylovKit flavor reports operator applications, numops = 1
(x0) + Arnoldi steps + 1 (explicit residual) per cycle; its solves here take one cycle, so steps = count - 2."""
import ctypes as C

import numpy as np
import pytest
import torch

import minaug_bordered_ref as B
import minaug_fold_ref as R
from conftest import probe
from oracle import operators

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
G = 64                                   # guard doubles before and after every operand
NS = [2, 3, 127, 128, 4099, 4100, 65537]
BIG = (1 << 22) + 1                      # just above the non-temporal threshold of stream.h (nt_hint), odd


def _lib():
    from bk_amd import codim2, hip
    return codim2, hip


class Guarded:
    """A device operand between NaN guards, `off` doubles past a 16-byte boundary."""

    def __init__(self, a, off=0):
        self.n, self.off = int(a.size), off
        self.t = torch.full((2 * G + off + self.n,), float("nan"), dtype=torch.float64, device="cuda")
        self.set(a)

    def set(self, a):
        self.t[G + self.off:G + self.off + self.n] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda")

    @property
    def ptr(self):
        return self.t.data_ptr() + 8 * (G + self.off)

    def get(self):
        torch.cuda.synchronize()
        return self.t[G + self.off:G + self.off + self.n].cpu().numpy()

    def guards_intact(self):
        torch.cuda.synchronize()
        h = self.t.cpu().numpy()
        return bool(np.isnan(h[:G + self.off]).all() and np.isnan(h[G + self.off + self.n:]).all())


def _tail_case(ctx, n, M, mis=None, seed=0):
    """One bk_bordered_tail call on integer data, run twice; operands y, x, atil_0.., b_0.. with operand `mis` one double off."""
    rng = np.random.default_rng(1000 * M + seed + n % 997)
    y = rng.integers(-1000, 1001, n).astype(np.float64)
    x = rng.integers(-32, 128, n).astype(np.float64)
    at = [rng.integers(-32, 128, n).astype(np.float64) for _ in range(M)]
    b = [rng.integers(-32, 128, n).astype(np.float64) for _ in range(M)]
    coef = [float(c) for c in rng.integers(-4, 5, M)]
    coef = [c or float(2 + j) for j, c in enumerate(coef)]                # (no zero coefficient: every column must show)
    ops = [Guarded(a, 1 if mis == k else 0) for k, a in enumerate([y, x] + at + b)]
    if mis is not None:
        assert ops[mis].ptr % 16 == 8
    # host loop: each product and each sum on its own, in j order; integers below 2^53, so every order gives these values
    yref = y.copy()
    for j in range(M):
        yref = yref + coef[j] * at[j]
    dref = [int(np.dot(b[j].astype(np.int64), x.astype(np.int64))) for j in range(M)]
    assert np.abs(yref).max() < 2.0 ** 53 and max(int(np.dot(np.abs(b[j]).astype(np.int64), np.abs(x).astype(np.int64)))
                                                   for j in range(M)) < 2 ** 53
    VP = C.c_void_p
    outs = []
    for run in range(2):
        ops[0].set(y)
        dots = (C.c_double * M)()
        ctx.check(ctx.lib.bk_bordered_tail(ctx.h, n, M, VP(ops[0].ptr), VP(ops[1].ptr), (VP * M)(*[o.ptr for o in ops[2:2 + M]]),
                                           (VP * M)(*[o.ptr for o in ops[2 + M:]]), (C.c_double * M)(*coef), dots),
                  "bk_bordered_tail")
        ctx.sync()
        outs.append((ops[0].get(), [dots[j] for j in range(M)]))
    yo, do = outs[0]
    assert np.array_equal(yo, yref), (n, M, mis, np.flatnonzero(yo != yref)[:8])
    assert np.array_equal(np.array(do), np.array(dref, dtype=np.float64)), (n, M, mis, do, dref)
    assert outs[1][0].tobytes() == yo.tobytes() and np.array(outs[1][1]).tobytes() == np.array(do).tobytes()
    assert all(o.guards_intact() for o in ops), (n, M, mis)
    for k, a in enumerate([None, x] + at + b):                               # the read-only operands are untouched
        if a is not None:
            assert np.array_equal(ops[k].get(), a)


@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("n", NS)
def test_bordered_tail_is_exact_on_integer_data(ctx, n, M):
    _tail_case(ctx, n, M)


@pytest.mark.parametrize("M", [3, 8])
def test_bordered_tail_wide_borders_take_one_item_per_lane(ctx, M):
    """M >= 3 keeps one 16-byte item per lane in flight (another grid size): odd and even lengths, more than one workgroup, one
    operand off a 16-byte boundary."""
    for n in (3, 4099, 65537):
        _tail_case(ctx, n, M)
    _tail_case(ctx, 4100, M, mis=2 + M)


@pytest.mark.parametrize("M", [1, 2])
def test_bordered_tail_each_operand_once_off_a_16_byte_boundary(ctx, M):
    for n in (4099, 4100):
        for mis in range(2 + 2 * M):
            _tail_case(ctx, n, M, mis=mis, seed=mis)


def test_bordered_tail_above_the_non_temporal_threshold(ctx):
    _tail_case(ctx, BIG, 1)
    _tail_case(ctx, BIG, 2)


def test_bordered_tail_rejects_aliases_and_counts(ctx):
    from bk_amd import _lib as L
    a = Guarded(np.ones(8))
    VP = C.c_void_p
    d = (C.c_double * 1)()
    one = (C.c_double * 1)(1.0)
    with pytest.raises(L.BkHipError, match="alias"):
        ctx.check(ctx.lib.bk_bordered_tail(ctx.h, 8, 1, VP(a.ptr), VP(a.ptr), (VP * 1)(a.ptr), (VP * 1)(a.ptr), one, d), "t")
    with pytest.raises(L.BkHipError, match="<= m <="):
        ctx.check(ctx.lib.bk_bordered_tail(ctx.h, 8, 9, VP(a.ptr), VP(a.ptr), (VP * 1)(a.ptr), (VP * 1)(a.ptr), one, d), "t")


# ------------------------------------------------------------------------------------------ bk_fold_border
def _border_problem(hip, ctx, kind, n):
    """A problem of `kind` whose vectors have n (sh1d) or 2 n / 3 n (sh: a 2-D grid needs two axes; three rows keep an odd n odd)
    entries, with dyadic nu so that h(u) is an integer for integer u: sh 2 nu - 6 u = 3 - 6 u, sh1d 6 nu u - 20 u^3 = 3 u - 20 u^3."""
    if kind == "sh":
        return hip.SwiftHohenberg(ctx, (n, 3 if n & 1 else 2), (np.pi, np.pi), l=-0.25, nu=1.5), [-0.25, 1.5]
    return hip.SwiftHohenberg1D(ctx, n, 6.0, lam=-0.75, nu=0.5), [-0.75, 0.5]


def _border_case(ctx, kind, n, mis=None):
    codim2, hip = _lib()
    prob, pars = _border_problem(hip, ctx, kind, n)
    nn = prob.nlocal
    rng = np.random.default_rng(n + (7 if kind == "sh" else 0))
    u = rng.integers(-8, 9, nn).astype(np.float64)
    v = rng.integers(-32, 128, nn).astype(np.float64)
    w = rng.integers(-32, 128, nn).astype(np.float64)
    ops = [Guarded(a, 1 if mis == k else 0) for k, a in enumerate([u, v, w, np.full(nn, np.nan)])]
    h, g = R.sh_polys(kind, pars[1], 0)
    ref = -((w * R.horner(h, u)) * v)
    assert np.abs(ref).max() < 2.0 ** 53
    sp = C.c_double()
    VP = C.c_void_p
    ctx.check(ctx.lib.bk_fold_border(prob.h, VP(ops[0].ptr), (C.c_double * 2)(*pars), 2, 0, VP(ops[1].ptr), VP(ops[2].ptr),
                                     VP(ops[3].ptr), C.byref(sp)), "bk_fold_border")
    ctx.sync()
    got = ops[3].get()
    assert np.array_equal(got, ref), (kind, n, mis, np.flatnonzero(got != ref)[:8])
    assert sp.value == -float(np.dot(w.astype(np.int64), v.astype(np.int64)))           # g_l = 1: sigma_p = -<w, v>, exact
    assert all(o.guards_intact() for o in ops)


@pytest.mark.parametrize("kind", ["sh", "sh1d"])
@pytest.mark.parametrize("n", NS)
def test_fold_border_is_exact_on_integer_data(ctx, kind, n):
    _border_case(ctx, kind, n)


@pytest.mark.parametrize("kind", ["sh", "sh1d"])
def test_fold_border_each_operand_once_off_a_16_byte_boundary(ctx, kind):
    for mis in range(4):
        _border_case(ctx, kind, 4099, mis=mis)
        _border_case(ctx, kind, 4100, mis=mis)


# ------------------------------------------------------------------------------------------ bk_bls_matrixfree_pl
DISTANCES = [5e-3, 1e-9, 0.0]
SHIFT = 0.25
GM = dict(restart=40, maxiter=50, rtol=1e-10, atol=1e-13)
_REF = {}


def _reference(dims, d, shift):
    """Per (grid, distance, shift): the case and the restatement's two solutions of [J + shift, a; a' 0][v; s] = [0; 1] -- direct,
    and SciPy GMRES at the device's tolerance and preconditioning -- with their spread.  Computed once, never changed."""
    key = (dims, d, shift)
    if key not in _REF:
        op, lstar, a = B.trivial_case(dims)
        n = a.size
        J = op.J(np.zeros(n), lstar + d, 1.3)
        pl = operators.dct_preconditioner(op.dims, op.ls, 1.0)
        zero = np.zeros(n)
        xd, pd = B.direct_bordered(J, a, a, 0.0, zero, 1.0, shift=shift)
        xg, pg, info, it = B.bordered_gmres(J, a, a, 0.0, zero, 1.0, pl, shift=shift, **GM)
        assert info == 0
        A1 = a.reshape(-1, 1)
        xs, ps = B.spectral_block(dims, op.ls, lstar + d, a, a, 0.0, zero, 1.0, shift=shift)
        _REF[key] = dict(op=op, lstar=lstar, a=a, J=J, xd=xd, pd=pd, it=it,
                         yard_x=float(np.linalg.norm(xd - xg) + np.linalg.norm(xd - xs)), yard_p=float(abs(pd - pg) + abs(pd - ps[0])),
                         res_g=B.block_residual(J, A1, A1, [[0.0]], zero, 1.0, xg, pg, shift=shift))
    return _REF[key]


def _solvers(hip, Pl):
    return [("krylovkit", hip.GMRESKrylovKit(dim=40, rtol=1e-10, atol=1e-13, maxiter=50, Pl=Pl), 2),
            ("iterativesolvers", hip.GMRESIterativeSolvers(reltol=1e-10, abstol=1e-13, restart=40, maxiter=2000, Pl=Pl), 0),
            ("krylovjl", hip.KrylovLS(atol=1e-13, rtol=1e-10, memory=40, restart=True, itmax=2000, Pl=Pl), 0)]


def _check_pl_solves(ctx, dims, tag):
    codim2, hip = _lib()
    for d in DISTANCES:
        for shift in (None, SHIFT):
            ref = _reference(dims, d, 0.0 if shift is None else shift)
            n = ref["a"].size
            prob = hip.SwiftHohenberg(ctx, dims, ref["op"].ls, l=ref["lstar"] + d, nu=1.3)
            Pl = hip.DCTPreconditioner(prob, 1.0)
            Jd = prob.jacobian(prob.vec(np.zeros(n)), ref["lstar"] + d)
            A, zero = prob.vec(ref["a"]), prob.vec(np.zeros(n))
            A1 = ref["a"].reshape(-1, 1)
            for name, ls, offset in _solvers(hip, Pl):
                v, sg, cv, it = hip.MatrixFreeBLS(ls, use_pl=True)(Jd, A, A, 0.0, zero, 1.0, shift=shift)
                vn = v.numpy()
                what = f"{tag}.{name}.d{d:g}.{'shift' if shift else 'noshift'}"
                assert cv, what
                probe(f"foldb.pl.count_vs_scipy.{what}", abs((it - offset) - ref["it"]), 2, device=it, scipy=ref["it"])
                probe(f"foldb.pl.x_vs_direct.{what}", np.linalg.norm(vn - ref["xd"]), 10 * ref["yard_x"])
                probe(f"foldb.pl.p_vs_direct.{what}", abs(sg - ref["pd"]), 10 * ref["yard_p"])
                res = B.block_residual(ref["J"], A1, A1, [[0.0]], np.zeros(n), 1.0, vn, sg, shift=shift or 0.0)
                probe(f"foldb.pl.true_residual.{what}", res, 10 * ref["res_g"])


@pytest.mark.parametrize("dims", [(16, 8), (32, 32), (64, 64)])
def test_bls_matrixfree_pl_on_the_trivial_singular_case(ctx, dims):
    """[J + shift, a; a' 0][v; s] = [0; 1] at l - l* in {5e-3, 1e-9, 0}: 16 x 8 (per-output transforms), 32 x 32 and 64 x 64 (fused LDS
    passes, stencil-free by default), three GMRES flavors, with and without a shift."""
    _check_pl_solves(ctx, dims, f"{dims[0]}x{dims[1]}")


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_bls_matrixfree_pl_in_every_stencil_free_mode(ctx, mode):
    ctx.set_option("gmres_stencil_free", mode)
    try:
        _check_pl_solves(ctx, (64, 64), f"64x64.sf{mode}")
    finally:
        ctx.set_option("gmres_stencil_free", 1)


def test_bls_block_matrixfree_pl_two_column_border(ctx):
    codim2, hip = _lib()
    dims = (64, 64)
    op, lstar, a = B.trivial_case(dims)
    n = a.size
    rng = np.random.default_rng(11)
    Am = np.column_stack([a, rng.standard_normal(n) / np.sqrt(n)])
    Bm = np.column_stack([a + 0.1 * rng.standard_normal(n) / np.sqrt(n), rng.standard_normal(n) / np.sqrt(n)])
    Cm = np.array([[0.0, 0.3], [-0.2, 1.1]])
    rhst, rhsb = rng.standard_normal(n) / np.sqrt(n), np.array([1.0, -0.5])
    J = op.J(np.zeros(n), lstar, 1.3)
    pl = operators.dct_preconditioner(op.dims, op.ls, 1.0)
    ud, pd = B.direct_block(J, Am, Bm, Cm, rhst, rhsb)
    ug, pg, info, itg = B.block_gmres(J, Am, Bm, Cm, rhst, rhsb, pl, **GM)
    assert info == 0
    prob = hip.SwiftHohenberg(ctx, dims, op.ls, l=lstar, nu=1.3)
    Pl = hip.DCTPreconditioner(prob, 1.0)
    Jd = prob.jacobian(prob.vec(np.zeros(n)), lstar)
    ls = hip.GMRESKrylovKit(dim=40, rtol=1e-10, atol=1e-13, maxiter=50, Pl=Pl)
    u1, u2, cv, it = hip.MatrixFreeBLS(ls, use_pl=True).solve_block(Jd, [prob.vec(Am[:, j]) for j in range(2)],
                                                                    [prob.vec(Bm[:, j]) for j in range(2)], Cm, prob.vec(rhst), rhsb)
    assert cv
    probe("foldb.block.count_vs_scipy", abs((it - 2) - itg), 2, device=it, scipy=itg)
    us, ps = B.spectral_block(dims, op.ls, lstar, Am, Bm, Cm, rhst, rhsb)
    probe("foldb.block.u1_vs_direct", np.linalg.norm(u1.numpy() - ud), 10 * (np.linalg.norm(ud - ug) + np.linalg.norm(ud - us)))
    probe("foldb.block.u2_vs_direct", np.abs(u2 - pd).max(), 10 * (np.abs(pd - pg).max() + np.abs(pd - ps).max()))
    probe("foldb.block.true_residual", B.block_residual(J, Am, Bm, Cm, rhst, rhsb, u1.numpy(), u2),
          10 * B.block_residual(J, Am, Bm, Cm, rhst, rhsb, ug, pg))


def test_use_pl_refusals(ctx):
    codim2, hip = _lib()
    from bk_amd import _lib as L
    op, lstar, a = B.trivial_case((16, 8))
    prob = hip.SwiftHohenberg(ctx, (16, 8), op.ls, l=lstar, nu=1.3)
    Pl = hip.DCTPreconditioner(prob, 1.0)
    J = prob.jacobian(prob.vec(np.zeros(a.size)), lstar)
    A, zero = prob.vec(a), prob.vec(np.zeros(a.size))
    with pytest.raises(TypeError, match="left preconditioner"):
        hip.MatrixFreeBLS(hip.GMRESKrylovKit(dim=40), use_pl=True)(J, A, A, 0.0, zero, 1.0)
    with pytest.raises(L.BkHipError, match="not symmetric"):
        hip.MatrixFreeBLS(hip.KrylovLSSymmetric(Pl=Pl), use_pl=True)(J, A, A, 0.0, zero, 1.0)
    with pytest.raises(L.BkHipError, match="right preconditioner"):
        hip.MatrixFreeBLS(hip.GMRESIterativeSolvers(restart=40, Pl=Pl, Pr=Pl), use_pl=True)(J, A, A, 0.0, zero, 1.0)
    with pytest.raises(TypeError, match="use_pl=True"):
        codim2.newton_fold(prob, zero, lstar, A, A, hip.GMRESKrylovKit(dim=40, Pl=Pl), bls=hip.MatrixFreeBLS(hip.GMRESKrylovKit(dim=40, Pl=Pl)))


# ------------------------------------------------------------------------------------------ newton_fold on the bordered path
KW_TRIVIAL = dict(tol=1e-10, max_iterations=20, norm_inf=True)


def _trivial_device(hip, dstart=0.005):
    c = hip.Context(0)
    op, lstar, a = B.trivial_case()
    prob = hip.SwiftHohenberg(c, (64, 64), op.ls, l=lstar + dstart, nu=1.3)
    ls = hip.GMRESKrylovKit(dim=40, rtol=1e-10, atol=1e-13, maxiter=50, Pl=hip.DCTPreconditioner(prob, 1.0))
    return c, op, lstar, a, prob, ls


def test_newton_fold_bordered_native_and_mirror_on_the_trivial_singular_point():
    """Native and mirror each on a fresh context (equal solver states); the same Newton solve on today's path (option 0) in the same
    test: both GMRES totals recorded, and the bordered one is the smaller."""
    codim2, hip = _lib()
    out = {}
    for name, fn in (("native", codim2.newton_fold_native), ("mirror", codim2.newton_fold), ("today", codim2.newton_fold_native)):
        c, op, lstar, a, prob, ls = _trivial_device(hip)
        A = prob.vec(a)
        bls = None if name == "today" else hip.MatrixFreeBLS(ls, use_pl=True)
        out[name] = fn(prob, prob.vec(np.zeros(a.size)), lstar + 0.005, A, A, ls, bls=bls, **KW_TRIVIAL)
        out[name]["x"] = out[name]["u"].u.numpy()
        c.close()
    sn, sm, st = out["native"], out["mirror"], out["today"]
    print("trivial fold, bordered: itnewton", sn["itnewton"], "itlinear", sn["itlineartot"], "residuals", sn["residuals"],
          "| today's path: itnewton", st["itnewton"], "itlinear", st["itlineartot"], "unconverged", st["unconverged_solves"])
    assert sn["converged"] and sm["converged"], (sn["residuals"], sm["residuals"])
    assert sn["itnewton"] == sm["itnewton"]
    probe("foldb.newton.native_vs_mirror_p", abs(sn["u"].p - sm["u"].p), 1e-12)
    probe("foldb.newton.native_vs_mirror_x", np.abs(sn["x"] - sm["x"]).max(), 1e-12)
    probe("foldb.newton.p_vs_exact", abs(sn["u"].p - lstar), 1e-10)
    assert sn["unconverged_solves"] == 0 and sm["unconverged_solves"] == 0
    probe("foldb.newton.itlinear_bordered_vs_today", sn["itlineartot"], st["itlineartot"] - 1, today=st["itlineartot"],
          today_unconverged=st["unconverged_solves"])


def _hex_device(hip, hb):
    c = hip.Context(0)
    x0, p0, z0 = B.hex_fold_guess(hb)
    prob = hip.SwiftHohenberg(c, hb["dims"], hb["ls"], l=p0, nu=B.NU_HEX)
    ls = hip.GMRESKrylovKit(dim=40, rtol=1e-10, atol=1e-13, maxiter=200, Pl=hip.DCTPreconditioner(prob, 1.0))
    return c, prob, ls, x0, p0, z0


def test_newton_fold_bordered_refines_the_hexagon_fold():
    """64 x 64, nu = 1.2.  Yardsticks: the restatement on the bordered path with direct solves against the same with SciPy GMRES(40),
    rtol 1e-10, Pl = (L1 + I)^-1, and against its own next two Newton iterates (it stops at a residual of 1e-11, where the iterate
    still moves).  The same Newton solve on today's path (option 0, a fresh context, one second) gives the other GMRES total: both
    are recorded, and the bordered one is the smaller."""
    codim2, hip = _lib()
    hb = B.hex_fold_case()
    c, prob, ls, x0, p0, z0 = _hex_device(hip, hb)
    model = R.sh_model(hb["op"], "sh", dict(l=p0, nu=B.NU_HEX), "l")
    kw = dict(tol=1e-9, max_iterations=15, normN=lambda z: np.abs(z).max())
    rd = B.newton_fold(model, x0, p0, z0, z0, "sh", **kw)
    rg = B.newton_fold(model, x0, p0, z0, z0, "sh", pl=operators.dct_preconditioner(hb["dims"], hb["ls"], 1.0), gm=GM, **kw)
    assert rd["converged"] and rg["converged"] and all(rg["flags"])
    r2 = B.newton_fold(model, x0, p0, z0, z0, "sh", tol=0.0, max_iterations=rd["itnewton"] + 2, normN=kw["normN"])
    Z = prob.vec(z0)
    sn = codim2.newton_fold_native(prob, prob.vec(x0), p0, Z, Z, ls, bls=hip.MatrixFreeBLS(ls, use_pl=True), tol=1e-9,
                                   max_iterations=15, norm_inf=True)
    x = sn["u"].u.numpy()
    print("hexagon fold, bordered: itnewton", sn["itnewton"], "itlinear", sn["itlineartot"], "residuals", sn["residuals"],
          "| restatement with SciPy GMRES: itnewton", rg["itnewton"], "inner iterations", rg["itlinear"])
    assert sn["converged"], sn["residuals"]
    assert sn["unconverged_solves"] == 0
    assert np.abs(x).max() > 0.5
    probe("foldb.hex.p_vs_restatement", abs(sn["u"].p - rd["p"]), 10 * (abs(rd["p"] - rg["p"]) + abs(rd["p"] - r2["p"])),
          itlinear=sn["itlineartot"])
    probe("foldb.hex.x_vs_restatement", np.abs(x - rd["u"]).max(),
          10 * (np.abs(rd["u"] - rg["u"]).max() + np.abs(rd["u"] - r2["u"]).max()))
    c.close()
    c, prob, ls, x0, p0, z0 = _hex_device(hip, hb)
    Z = prob.vec(z0)
    st = codim2.newton_fold_native(prob, prob.vec(x0), p0, Z, Z, ls, tol=1e-9, max_iterations=15, norm_inf=True)
    c.close()
    print("hexagon fold, today's path: itnewton", st["itnewton"], "itlinear", st["itlineartot"], "unconverged solves",
          st["unconverged_solves"])
    probe("foldb.hex.itlinear_bordered_vs_today", sn["itlineartot"], st["itlineartot"] - 1, today=st["itlineartot"],
          today_unconverged=st["unconverged_solves"])


def test_continuation_fold_with_the_bordered_solver_follows_the_exact_curve(ctx):
    """The three fixed steps of test_gpu_fold.py::test_continuation_fold_follows_the_exact_fold_curve_and_the_restatement, with that
    test's own bounds."""
    codim2, hip = _lib()
    from bk_amd import continuation as Cn
    op, lstar, a = B.trivial_case()
    n = a.size
    prob = hip.SwiftHohenberg(ctx, (64, 64), op.ls, l=lstar + 0.005, nu=1.3)
    ls = hip.GMRESKrylovKit(dim=40, rtol=1e-10, atol=1e-13, maxiter=50, Pl=hip.DCTPreconditioner(prob, 1.0))
    A = prob.vec(a)
    cp = Cn.ContinuationPar(ds=0.01, dsmax=0.05, p_min=0.5, p_max=2.0, max_steps=3,
                            newton_options=Cn.NewtonPar(tol=1e-10, max_iterations=10))
    dss = [0.01, 0.01, 0.02]
    br = codim2.continuation_fold(prob, hip.BorderedArray(prob.vec(np.zeros(n)), lstar + 1e-4), 1.3, "nu", A, A, ls, cp,
                                  ds_sequence=dss, bls=hip.MatrixFreeBLS(ls, use_pl=True))
    print("continuation_fold (bordered): p1", br.p1, "p2", br.p2, "itnewton", br.itnewton, "itlinear", br.itlinear)
    assert len(br.p2) == len(dss) + 1 and all(np.diff(br.p2) > 0)
    probe("foldb.curve_p1_vs_exact", max(abs(p - lstar) for p in br.p1), 1e-10, itlinear=float(sum(br.itlinear)))
    model = R.sh_model(op, "sh", dict(l=lstar + 0.005, nu=1.3), "l", "nu")
    rr = R.continuation_fold(model, np.zeros(n), lstar + 1e-4, 1.3, a, a, ds=0.01, max_steps=3, tol=1e-10, max_iterations=10,
                             ds_sequence=dss)
    probe("foldb.curve_vs_restatement_p1", max(abs(p - q) for p, q in zip(br.p1, rr["p1"])), 1e-8)
    probe("foldb.curve_vs_restatement_p2", max(abs(p - q) for p, q in zip(br.p2, rr["p2"])), 1e-8)


# ------------------------------------------------------------------------------------------ the default path is untouched
def test_default_path_is_bitwise_the_same_with_the_option_unset_and_at_zero():
    codim2, hip = _lib()
    from bk_amd import _lib as L
    out = []
    for set_zero in (False, True):
        c, op, lstar, a, prob, ls = _trivial_device(hip)
        if set_zero:
            c.set_option("fold_bordered", 0.0)
        else:
            with pytest.raises(L.BkHipError):
                c.get_option("fold_bordered")                    # never set on a fresh context
        A = prob.vec(a)
        s = codim2.newton_fold_native(prob, prob.vec(np.zeros(a.size)), lstar + 0.005, A, A, ls, **KW_TRIVIAL)
        out.append((s["u"].p, s["u"].u.numpy().tobytes(), tuple(s["residuals"]), s["itnewton"], s["itlineartot"],
                    s["unconverged_solves"]))
        c.close()
    assert out[0] == out[1]


def test_matrixfreebls_without_use_pl_issues_the_unpreconditioned_entry_point(ctx, monkeypatch):
    codim2, hip = _lib()
    op, lstar, a = B.trivial_case((16, 8))
    prob = hip.SwiftHohenberg(ctx, (16, 8), op.ls, l=lstar + 0.5, nu=1.3)
    Pl = hip.DCTPreconditioner(prob, 1.0)
    J = prob.jacobian(prob.vec(np.zeros(a.size)), lstar + 0.5)
    A, zero = prob.vec(a), prob.vec(np.zeros(a.size))
    ls = hip.GMRESKrylovKit(dim=63, rtol=1e-8, atol=1e-13, maxiter=5, Pl=Pl)
    calls = []

    class Spy:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            f = getattr(self._lib, name)
            if name.startswith("bk_bls_"):
                calls.append(name)
            return f
    monkeypatch.setattr(ctx, "lib", Spy(ctx.lib))
    assert hip.MatrixFreeBLS(ls).use_pl is False
    hip.MatrixFreeBLS(ls)(J, A, A, 0.0, zero, 1.0)
    hip.MatrixFreeBLS(ls, use_pl=True)(J, A, A, 0.0, zero, 1.0)
    assert calls == ["bk_bls_matrixfree", "bk_bls_matrixfree_pl"], calls
