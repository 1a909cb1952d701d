"""GPU tests of the complex preconditioned MatrixFreeBLS (csrc/bordered.hip: bk_cbordered_tail, bk_bls_matrixfree_pl_cshift) and of
the Hopf formulation on it (context option hopf_bordered; bk_amd.codim2 with bls = MatrixFreeBLS(ls, use_pl=True)).

The streaming pass is compared bitwise with a host loop on data where rounding cannot occur (integers, every partial sum below
2^53: the rule of tests/stencil_ref.py::exact).  The solver-dependent comparisons follow the yardstick rule of DESIGN 9d-9f, as
tests/test_gpu_fold_bordered.py does: the restatement (tests/minaug_hopf_bordered_ref.py) with direct solves against the restatement
with SciPy GMRES at the device's tolerance and preconditioning gives a spread, measured where the test runs; on the trivial state
the direct solve's own distance from the solve in the DST basis, where J(0) is exactly block-diagonal, is added (the sparse direct
solve works on a Laplacian rounded entry by entry).  v, w and sigma are each held to 10 x their OWN yardstick.  Off the trivial
state there is no exact basis; the second term there is named in the test that needs one.
Counts: within 2 Arnoldi steps of SciPy's per solve.  The KrylovKit flavor reports operator applications, 1 (x0) +
Arnoldi steps + 1 (explicit residual) per cycle; its solves here take one cycle, so steps = count - 2."""
import ctypes as C

import numpy as np
import pytest
import torch

import bautin_ref as BR
import minaug_hopf_bordered_ref as H
import minaug_hopf_ref as R
from conftest import probe
from oracle import operators

pytestmark = pytest.mark.gpu

G = 64                                   # guard doubles before and after every operand
NS = [2, 3, 127, 128, 4099, 4100, 65537]
BIG = (1 << 22) + 1                      # just above the non-temporal threshold of stream.h (nt_hint), odd
DIMS, LS = (41, 21), (np.pi, np.pi / 2)  # the grid of examples/cGL2d.jl
PARS = H.PARS
NU = PARS["nu"]
VP = C.c_void_p


def _lib():
    from bk_amd import codim2, hip
    return codim2, hip


def _pair(prob, z):
    return prob.vec(np.ascontiguousarray(z.real)), prob.vec(np.ascontiguousarray(z.imag))


def _num(pair):
    return pair[0].numpy() + 1j * pair[1].numpy()


# ------------------------------------------------------------------------------------------ bk_cbordered_tail
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


OPERANDS = ("yr", "yi", "xr", "xi", "atr", "ati", "br", "bi")         # the eight device vectors: ten streams, yr and yi both ways


def _ctail(ctx, ops, n, coef):
    dots = (C.c_double * 2)()
    ctx.check(ctx.lib.bk_cbordered_tail(ctx.h, n, *[VP(o.ptr) for o in ops], (C.c_double * 2)(*coef), dots), "bk_cbordered_tail")
    ctx.sync()
    return [dots[0], dots[1]]


def _ctail_case(ctx, n, mis=None, seed=0):
    """One bk_cbordered_tail call on integer data, run twice, with operand `mis` one double off a 16-byte boundary."""
    rng = np.random.default_rng(7000 + seed + n % 997)
    yr, yi = (rng.integers(-1000, 1001, n).astype(np.float64) for _ in range(2))
    xr, xi, atr, ati, br, bi = (rng.integers(-32, 128, n).astype(np.float64) for _ in range(6))
    cr, ci = 3.0, -2.0
    host = [yr, yi, xr, xi, atr, ati, br, bi]
    ops = [Guarded(a, 1 if mis == k else 0) for k, a in enumerate(host)]
    if mis is not None:
        assert ops[mis].ptr % 16 == 8
    # host loop in the kernel's order; integers below 2^53, so every product and sum is exact in any order
    ref_r = (yr + cr * atr) - ci * ati
    ref_i = (yi + cr * ati) + ci * atr
    I = lambda a: a.astype(np.int64)
    sums = [int(np.dot(I(br), I(xr))), int(np.dot(I(bi), I(xi))), int(np.dot(I(br), I(xi))), int(np.dot(I(bi), I(xr)))]
    assert max(int(np.dot(np.abs(I(p)), np.abs(I(q)))) for p in (br, bi) for q in (xr, xi)) < 2 ** 52
    dref = [float(sums[0] + sums[1]), float(sums[2] - sums[3])]
    outs = []
    for run in range(2):
        ops[0].set(yr)
        ops[1].set(yi)
        d = _ctail(ctx, ops, n, (cr, ci))
        outs.append((ops[0].get(), ops[1].get(), d))
    gr, gi, d = outs[0]
    assert np.array_equal(gr, ref_r), (n, mis, np.flatnonzero(gr != ref_r)[:8])
    assert np.array_equal(gi, ref_i), (n, mis, np.flatnonzero(gi != ref_i)[:8])
    assert d == dref, (n, mis, d, dref)
    assert outs[1][0].tobytes() == gr.tobytes() and outs[1][1].tobytes() == gi.tobytes() and outs[1][2] == d
    assert all(o.guards_intact() for o in ops), (n, mis)
    for k in range(2, 8):                                                  # the read-only operands are untouched
        assert np.array_equal(ops[k].get(), host[k]), OPERANDS[k]


@pytest.mark.parametrize("n", NS)
def test_cbordered_tail_is_exact_on_integer_data(ctx, n):
    _ctail_case(ctx, n)


@pytest.mark.parametrize("n", [4099, 4100])
def test_cbordered_tail_each_operand_once_off_a_16_byte_boundary(ctx, n):
    """The scalar path: each of the eight device vectors -- the ten streams, yr and yi are read and written -- once 8 bytes off."""
    for mis in range(8):
        _ctail_case(ctx, n, mis=mis, seed=mis)


def test_cbordered_tail_above_the_non_temporal_threshold(ctx):
    _ctail_case(ctx, BIG)


def test_cbordered_tail_rounds_every_product_and_sum_on_its_own(ctx):
    """Non-integer data: bitwise the host expression (yr + cr atr) - ci ati, (yi + cr ati) + ci atr in IEEE double without
    contraction, on the vector and on the scalar path; the dots within the summation bound 4 n eps sum |terms|."""
    rng = np.random.default_rng(5)
    n = 4101
    host = [rng.standard_normal(n) for _ in range(8)]
    yr, yi, xr, xi, atr, ati, br, bi = host
    cr, ci = 0.7310585786300049, -1.2345678901234567
    for mis in (None, 4):
        ops = [Guarded(a, 1 if mis == k else 0) for k, a in enumerate(host)]
        d = _ctail(ctx, ops, n, (cr, ci))
        assert np.array_equal(ops[0].get(), (yr + cr * atr) - ci * ati)
        assert np.array_equal(ops[1].get(), (yi + cr * ati) + ci * atr)
        ref = np.vdot(br + 1j * bi, xr + 1j * xi)
        eps = np.finfo(float).eps
        bound = 4 * n * eps * (np.abs(br) + np.abs(bi)) @ (np.abs(xr) + np.abs(xi))
        assert abs(d[0] - ref.real) <= bound and abs(d[1] - ref.imag) <= bound


def test_cbordered_tail_rejects_aliases_and_nulls(ctx):
    from bk_amd import _lib as L
    ops = [Guarded(np.ones(8)) for _ in range(8)]
    coef, d = (C.c_double * 2)(1.0, 0.0), (C.c_double * 2)()
    ptrs = [VP(o.ptr) for o in ops]
    for y in (0, 1):
        for other in range(8):
            if other == y:
                continue
            p = list(ptrs)
            p[other] = ptrs[y]
            with pytest.raises(L.BkHipError, match="alias"):
                ctx.check(ctx.lib.bk_cbordered_tail(ctx.h, 8, *p, coef, d), "t")
    for k in range(8):
        p = list(ptrs)
        p[k] = None
        assert ctx.lib.bk_cbordered_tail(ctx.h, 8, *p, coef, d) == -1
    assert ctx.lib.bk_cbordered_tail(ctx.h, 8, *ptrs, None, d) == -1 and ctx.lib.bk_cbordered_tail(ctx.h, 8, *ptrs, coef, None) == -1
    assert all(np.array_equal(o.get(), np.ones(8)) for o in ops)               # nothing ran
    d[0] = d[1] = 5.0
    ctx.check(ctx.lib.bk_cbordered_tail(ctx.h, 0, *ptrs, coef, d), "t")         # n = 0: empty sums, nothing touched
    assert (d[0], d[1]) == (0.0, 0.0)


# ------------------------------------------------------------------------------------------ bk_bls_matrixfree_pl_cshift
DISTANCES = [2e-2, 1e-9, 0.0]
GM = dict(restart=60, maxiter=10, rtol=1e-12)
_REF = {}


def _reference(dims, d, adjoint):
    """Per (grid, distance, system): the restatement's solutions of [J - i nu, a; b^H, 0][v; s] = [0; 1] (adjoint: [J' + i nu, b;
    a^H, 0]) at u = 0 -- sparse direct, SciPy GMRES at the device's tolerance and preconditioning, and the DST basis -- with their
    spreads.  Computed once, never changed."""
    key = (dims, d, adjoint)
    if key not in _REF:
        op, rstar, a, b = H.trivial_case(dims, LS)
        n = a.size
        J = op.J(np.zeros(n), **dict(PARS, r=rstar + d))
        if adjoint:
            J, a, b, shift = J.T.tocsr(), b, a, 1j * NU
        else:
            shift = -1j * NU
        pl = operators.dst_block_preconditioner_cgl(dims, LS, rstar + 0.02, 0.95 * NU)
        zero = np.zeros(n)
        xd, pd = H.direct_cbordered(J, a, b, 0.0, zero, 1.0, shift=shift)
        xg, pg, info, it, _ = H.cbordered_gmres(J, a, b, 0.0, zero, 1.0, pl, shift=shift, **GM)
        assert info == 0
        xs, ps = H.spectral_cbordered(dims, LS, rstar + d, NU, a, b, 0.0, zero, 1.0, shift=shift, adjoint=adjoint)
        _REF[key] = dict(rstar=rstar, a=a, b=b, J=J, shift=shift, xd=xd, pd=pd, it=it,
                         yard_x=float(np.linalg.norm(xd - xg) + np.linalg.norm(xd - xs)), yard_p=float(abs(pd - pg) + abs(pd - ps)),
                         res_g=H.cresidual(J, a, b, 0.0, zero, 1.0, xg, pg, shift=shift))
    return _REF[key]


def _solvers(hip, Pl, restart=60, rtol=1e-12):
    return [("krylovkit", hip.GMRESKrylovKit(dim=restart, rtol=rtol, atol=0.0, maxiter=10, Pl=Pl), 2),
            ("iterativesolvers", hip.GMRESIterativeSolvers(reltol=rtol, abstol=0.0, restart=restart, maxiter=600, Pl=Pl), 0),
            ("krylovjl", hip.KrylovLS(atol=0.0, rtol=rtol, memory=restart, restart=True, itmax=600, Pl=Pl), 0)]


@pytest.mark.parametrize("dims", [(41, 21), (16, 8)])
def test_bls_matrixfree_pl_cshift_at_every_distance_to_the_hopf_point(ctx, dims):
    """u = 0, r - r* in {2e-2, 1e-9, 0}, the system and its adjoint (the same, untransposed Pl), three GMRES flavors."""
    codim2, hip = _lib()
    for d in DISTANCES:
        for adjoint in (False, True):
            ref = _reference(dims, d, adjoint)
            n = ref["a"].size
            r = ref["rstar"] + d
            prob = hip.CGL2d(ctx, dims, LS, **dict(PARS, r=r))
            Pl = hip.CGLBlockPreconditioner(prob, ref["rstar"] + 0.02, 0.95 * NU)
            x0 = prob.vec(np.zeros(n))
            Jd = prob.jacobian_adjoint(x0, r) if adjoint else prob.jacobian(x0, r)
            A, B, zero = _pair(prob, ref["a"]), _pair(prob, ref["b"]), prob.vec(np.zeros(n))
            for name, ls, offset in _solvers(hip, Pl):
                v, sg, cv, it = hip.MatrixFreeBLS(ls, use_pl=True).solve_complex(Jd, A, B, 0.0, (zero, None), 1.0, shift=ref["shift"])
                vn = _num(v)
                what = f"{dims[0]}x{dims[1]}.{'adjoint' if adjoint else 'system'}.{name}.d{d:g}"
                assert cv, what
                assert it[1] == 0
                probe(f"hopfb.pl.count_vs_scipy.{what}", abs((it[0] - offset) - ref["it"]), 2, device=it[0], scipy=ref["it"])
                probe(f"hopfb.pl.x_vs_direct.{what}", np.linalg.norm(vn - ref["xd"]), 10 * ref["yard_x"])
                probe(f"hopfb.pl.sigma_vs_direct.{what}", abs(sg - ref["pd"]), 10 * ref["yard_p"])
                res = H.cresidual(ref["J"], ref["a"], ref["b"], 0.0, np.zeros(n), 1.0, vn, sg, shift=ref["shift"])
                probe(f"hopfb.pl.true_residual.{what}", res, 10 * ref["res_g"])


def test_bls_matrixfree_pl_cshift_general_case(ctx):
    """16 x 8, u != 0, a general complex shift, non-zero complex R, dzp and n, xiu, xip and dotscale off 1, three flavors.  Off the
    trivial state there is no exact basis: the second term of the yardstick is the sparse direct solve's distance from a dense LU
    solve of the same matrix, the direct solve's own rounding."""
    codim2, hip = _lib()
    dims = (16, 8)
    op = operators.CGL2d(dims, LS)
    rng = np.random.default_rng(17)
    n = 2 * op.n
    cvec = lambda: (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2 * n)
    u = 0.3 * rng.standard_normal(n)
    pars = dict(PARS, r=1.0, gamma=0.1)
    a, b, Rv = cvec(), cvec(), cvec()
    dzp, nn, xiu, xip, dotscale, shift = 0.7 - 0.2j, 0.6 + 0.3j, 0.8, 1.25, 0.5, 0.37 - 1.1j
    J = op.J(u, **pars)
    c, kappa = dzp * xip, xiu * dotscale
    pl = operators.dst_block_preconditioner_cgl(dims, LS, 1.0, NU)
    xd, pd = H.direct_cbordered(J, a, b, c, Rv, nn, kappa, shift)
    xg, pg, info, itg, _ = H.cbordered_gmres(J, a, b, c, Rv, nn, pl, kappa=kappa, shift=shift, **GM)
    assert info == 0
    y = np.linalg.solve(H.complex_matrix(J, a, b, c, kappa, shift).toarray(), np.append(Rv, nn))
    yard_x = float(np.linalg.norm(xd - xg) + np.linalg.norm(xd - y[:-1]))
    yard_p = float(abs(pd - pg) + abs(pd - y[-1]))
    res_g = H.cresidual(J, a, b, c, Rv, nn, xg, pg, kappa, shift)
    prob = hip.CGL2d(ctx, dims, LS, **pars)
    Pl = hip.CGLBlockPreconditioner(prob, 1.0, NU)
    Jd = prob.jacobian(prob.vec(u), pars["r"])
    for name, ls, offset in _solvers(hip, Pl):
        X, dl, cv, it = hip.MatrixFreeBLS(ls, use_pl=True).solve_complex(Jd, _pair(prob, a), _pair(prob, b), dzp, _pair(prob, Rv), nn,
                                                                         xiu, xip, shift=shift, dotscale=dotscale)
        assert cv, name
        xn = _num(X)
        probe(f"hopfb.general.count_vs_scipy.{name}", abs((it[0] - offset) - itg), 2, device=it[0], scipy=itg)
        probe(f"hopfb.general.x_vs_direct.{name}", np.linalg.norm(xn - xd), 10 * yard_x)
        probe(f"hopfb.general.dl_vs_direct.{name}", abs(dl - pd), 10 * yard_p)
        probe(f"hopfb.general.true_residual.{name}", H.cresidual(J, a, b, c, Rv, nn, xn, dl, kappa, shift), 10 * res_g)


def test_use_pl_refusals_of_the_complex_solve(ctx):
    codim2, hip = _lib()
    from bk_amd import _lib as L
    op, rstar, a, b = H.trivial_case((16, 8), LS)
    prob = hip.CGL2d(ctx, (16, 8), LS, **dict(PARS, r=rstar))
    Pl = hip.CGLBlockPreconditioner(prob, rstar + 0.02, NU)
    x0 = prob.vec(np.zeros(a.size))
    J = prob.jacobian(x0, rstar)
    A, B = _pair(prob, a), _pair(prob, b)
    args = (J, A, B, 0.0, (x0, None), 1.0)
    with pytest.raises(TypeError, match="left preconditioner"):
        hip.MatrixFreeBLS(hip.GMRESKrylovKit(dim=40), use_pl=True).solve_complex(*args, shift=-1j)
    with pytest.raises(TypeError, match="use_pl=True"):
        hip.MatrixFreeBLS(hip.GMRESKrylovKit(dim=40, Pl=Pl)).solve_complex(*args, shift=-1j)
    with pytest.raises(L.BkHipError, match="not symmetric"):
        hip.MatrixFreeBLS(hip.KrylovLSSymmetric(Pl=Pl), use_pl=True).solve_complex(*args, shift=-1j)
    with pytest.raises(L.BkHipError, match="right preconditioner"):
        hip.MatrixFreeBLS(hip.GMRESIterativeSolvers(restart=40, Pl=Pl, Pr=Pl), use_pl=True).solve_complex(*args, shift=-1j)
    ls = hip.GMRESIterativeSolvers(reltol=1e-10, restart=40, maxiter=100, Pl=Pl)
    X0 = codim2.HopfVec(x0, [rstar + 0.02, 0.95 * NU])
    with pytest.raises(TypeError, match="use_pl=True"):
        codim2.newton_hopf(prob, X0, A, B, ls, bls=hip.MatrixFreeBLS(ls))
    with pytest.raises(TypeError, match="use_pl=True"):
        codim2.newton_hopf_native(prob, X0, A, B, ls, bls=hip.MatrixFreeBLS(ls))
    nopl = hip.GMRESIterativeSolvers(reltol=1e-10, restart=40, maxiter=100)
    with pytest.raises(L.BkHipError, match="needs the left preconditioner"):
        codim2.newton_hopf_native(prob, X0, A, B, nopl, bls=hip.MatrixFreeBLS(nopl, use_pl=True))
    assert ctx.get_option("hopf_bordered") == 0.0                      # put back after the failed call


# ------------------------------------------------------------------------------------------ newton_hopf on the bordered path
def _solver(hip, prob, r0, reltol=1e-13):
    return hip.GMRESIterativeSolvers(reltol=reltol, restart=60, maxiter=600, Pl=hip.CGLBlockPreconditioner(prob, r0, NU))


def _newton_three_ways(make, a, b, X0, kw):
    """native and mirror on the bordered path, native on the elimination path; each on a fresh context (equal solver states)."""
    codim2, hip = _lib()
    out = {}
    for name in ("native", "mirror", "elimination"):
        c = hip.Context(0)
        prob, ls = make(hip, c)
        bls = None if name == "elimination" else hip.MatrixFreeBLS(ls, use_pl=True)
        f = codim2.newton_hopf if name == "mirror" else codim2.newton_hopf_native
        out[name] = s = f(prob, codim2.HopfVec(prob.vec(X0[0]), [X0[1], X0[2]]), _pair(prob, a), _pair(prob, b), ls, bls=bls, **kw)
        s["x"] = s["u"].u.numpy()
        s["vw"] = (_num(s["v"]), _num(s["w"]))
        print(f"{name}: itnewton {s['itnewton']}, GMRES {s['itlineartot']}, unconverged {s['unconverged_solves']}, residuals "
              f"{s['residuals']}")
        c.close()
    return out


def _bit_equal(sn, sm):
    assert sn["itnewton"] == sm["itnewton"] and sn["itlineartot"] == sm["itlineartot"]
    assert tuple(sn["u"].p) == tuple(sm["u"].p), (sn["u"].p, sm["u"].p)
    assert sn["x"].tobytes() == sm["x"].tobytes()
    assert sn["residuals"] == sm["residuals"], (sn["residuals"], sm["residuals"])
    assert sn["sigma"] == sm["sigma"]
    assert sn["vw"][0].tobytes() == sm["vw"][0].tobytes() and sn["vw"][1].tobytes() == sm["vw"][1].tobytes()


def test_newton_hopf_bordered_native_and_mirror_on_the_closed_form_hopf_point():
    """41 x 21, u = 0, gamma = 0, from (r* + 0.02, 0.95 nu) with the start vectors and solver of
    test_gpu_hopf.py::test_newton_hopf_native_mirror_and_restatement_land_on_the_closed_form_hopf_point and that test's bound
    (1e-11 relative).  The elimination path (option 0) runs in the same test: it reports unconverged solves, the bordered path
    none.  Both GMRES totals are recorded; no ratio is asserted."""
    op = operators.CGL2d(DIMS, LS)
    n = 2 * op.n
    rstar = float(-H.dirichlet_eigenvalues(DIMS, LS).max())
    model = R.cgl_model(op, dict(PARS), "r")
    x0 = np.zeros(n)
    a, b = R.start_vectors(model, x0, model.at(rstar + 0.02), 0.95 * NU, seed=3)
    kw = dict(tol=1e-12, max_iterations=15)
    ref = R.newton_hopf(model, x0, rstar + 0.02, 0.95 * NU, a, b, **kw)
    assert ref["converged"], ref["residuals"]

    def make(hip, c):
        prob = hip.CGL2d(c, DIMS, LS, **dict(PARS, r=rstar + 0.02))
        return prob, _solver(hip, prob, rstar + 0.02)
    out = _newton_three_ways(make, a, b, (x0, rstar + 0.02, 0.95 * NU), kw)
    sn, sm, se = out["native"], out["mirror"], out["elimination"]
    assert sn["converged"] and sm["converged"], (sn["residuals"], sm["residuals"])
    _bit_equal(sn, sm)
    assert sn["itnewton"] == ref["itnewton"], (sn["residuals"], ref["residuals"])
    assert sn["unconverged_solves"] == 0 and sm["unconverged_solves"] == 0
    assert se["unconverged_solves"] >= 1, se
    assert np.abs(sn["x"]).max() == 0.0
    p, om = sn["u"].p
    probe("hopfb.newton.closed_form_r", abs(p - rstar) / abs(rstar), 1e-11, itlinear_bordered=sn["itlineartot"],
          itlinear_elimination=se["itlineartot"], unconverged_elimination=se["unconverged_solves"])
    probe("hopfb.newton.closed_form_omega", abs(om - NU) / NU, 1e-11)


def test_newton_hopf_bordered_at_the_hopf_point_off_the_trivial_state():
    """gamma = 0.1, u != 0: Newton in mu from 0.3 away at the Hopf point
    test_gpu_hopf.py::test_newton_hopf_in_a_hessian_coefficient_matches_mirror_and_restatement refines, with that test's bounds
    (1e-11 in mu and omega, 1e-10 in the state)."""
    op = operators.CGL2d(DIMS, LS)
    rstar = float(-H.dirichlet_eigenvalues(DIMS, LS).max())
    z = H.hopf_mode(DIMS)
    base = R.newton_hopf(R.cgl_model(op, dict(PARS, gamma=0.1), "r"), np.zeros(2 * op.n), rstar, NU, z, z, tol=1e-12, max_iterations=20)
    assert base["converged"] and np.abs(base["u"]).max() > 0.1, base["residuals"]
    pars = dict(PARS, gamma=0.1, r=base["p"])
    p0 = PARS["mu"] + 0.3
    a, b = base["w"] / np.linalg.norm(base["w"]), base["v"] / np.linalg.norm(base["v"])
    kw = dict(tol=1e-12, max_iterations=15)
    ref = R.newton_hopf(R.cgl_model(op, pars, "mu"), base["u"], p0, base["omega"], a, b, **kw)
    assert ref["converged"] and abs(ref["p"] - PARS["mu"]) <= 1e-11, ref["residuals"]

    def make(hip, c):
        prob = hip.CGL2d(c, DIMS, LS, lens="mu", **dict(pars, mu=p0))
        return prob, _solver(hip, prob, base["p"])
    out = _newton_three_ways(make, a, b, (base["u"], p0, base["omega"]), kw)
    sn, sm, se = out["native"], out["mirror"], out["elimination"]
    assert sn["converged"] and sm["converged"], (sn["residuals"], sm["residuals"])
    _bit_equal(sn, sm)
    assert sn["itnewton"] == ref["itnewton"], (sn["residuals"], ref["residuals"])
    assert sn["unconverged_solves"] == 0 and sm["unconverged_solves"] == 0
    assert se["unconverged_solves"] >= 1, se
    p, om = sn["u"].p
    probe("hopfb.newton.offtrivial_mu", abs(p - ref["p"]), 1e-11, itlinear_bordered=sn["itlineartot"],
          itlinear_elimination=se["itlineartot"], unconverged_elimination=se["unconverged_solves"])
    probe("hopfb.newton.offtrivial_omega", abs(om - ref["omega"]), 1e-11)
    probe("hopfb.newton.offtrivial_x", np.abs(sn["x"] - ref["u"]).max(), 1e-10)


def test_hopf_curve_with_the_bordered_solver_matches_the_restatement():
    """Three fixed steps of ds = 0.01 in gamma from the closed-form Hopf point (the curve of
    test_gpu_hopf.py::test_hopf_curve_in_gamma_leaves_the_trivial_state_and_matches_the_restatement).  Yardstick per recorded
    quantity: the restatement with direct solves against the restatement with every solve by SciPy GMRES at the device's reltol and
    preconditioning (H.krylov_solves), plus -- the state is off u = 0, there is no exact basis -- the direct restatement's distance
    from its own Newton limit (tol 1e-13 instead of 1e-10: what the Newton tolerance leaves free), plus one ulp of the quantity."""
    codim2, hip = _lib()
    from bk_amd import continuation as Cn
    op = operators.CGL2d(DIMS, LS)
    n = 2 * op.n
    rstar = float(-H.dirichlet_eigenvalues(DIMS, LS).max())
    tol = 1e-10
    model = R.cgl_model(op, dict(PARS), "r", "gamma")
    z = H.hopf_mode(DIMS)
    dss = [0.01] * 3
    kw = dict(ds=0.01, dsmax=0.01, max_iterations=10, ds_sequence=dss)
    rd = R.continuation_hopf(model, np.zeros(n), rstar, NU, 0.0, z, z, tol=tol, **kw)
    rl = R.continuation_hopf(model, np.zeros(n), rstar, NU, 0.0, z, z, tol=1e-13, **kw)
    with H.krylov_solves(operators.dst_block_preconditioner_cgl(DIMS, LS, rstar, NU), restart=60, maxiter=10, rtol=1e-13) as log:
        rg = R.continuation_hopf(model, np.zeros(n), rstar, NU, 0.0, z, z, tol=tol, **kw)
    assert all(info == 0 for info, _ in log)
    c = hip.Context(0)
    prob = hip.CGL2d(c, DIMS, LS, **dict(PARS, r=rstar))
    ls = _solver(hip, prob, rstar)
    Z = _pair(prob, z)
    cp = Cn.ContinuationPar(ds=0.01, dsmin=1e-4, dsmax=0.01, p_min=-1.0, p_max=1.0, max_steps=3,
                            newton_options=Cn.NewtonPar(tol=tol, max_iterations=10))
    bad0 = c.get_option("hopf_unconverged_solves")
    br = codim2.continuation_hopf(prob, codim2.HopfVec(prob.vec(np.zeros(n)), [rstar, NU]), 0.0, "gamma", Z, Z, ls, cp,
                                  ds_sequence=dss, bls=hip.MatrixFreeBLS(ls, use_pl=True))
    print("continuation_hopf (bordered): p1", br.p1, "p2", br.p2, "omega", br.omega, "itnewton", br.itnewton, "itlinear", br.itlinear,
          "| restatement with SciPy GMRES: inner iterations", sum(it for _, it in log))
    assert len(br.p2) == len(rd["p2"]) == 4 and all(np.diff(br.p2) > 0)
    assert br.itnewton == rd["itnewton"], (br.itnewton, rd["itnewton"])
    for key, got in (("p1", br.p1), ("p2", br.p2), ("omega", br.omega)):
        d, g, l = (np.array(r_[key]) for r_ in (rd, rg, rl))
        # ... and one unit in the last place of the quantity: the restatement's two runs can agree to the last bit (omega does),
        # and two correctly rounded evaluations of the same formula in another order still differ by that much
        yard = float(np.abs(d - g).max() + np.abs(d - l).max() + np.spacing(np.abs(d).max()))
        probe(f"hopfb.curve_{key}_vs_restatement", float(np.abs(np.array(got) - d).max()), 10 * yard, yardstick=yard,
              itlinear=float(sum(br.itlinear)))
    c.close()


def test_bautin_l2_with_the_bordered_h21_solve():
    """The Bautin point of tests/test_gpu_bautin.py (gamma = 0.1, c3 = -0.1024) with hopf_bordered = 1: native and mirror against the
    dense restatement within that file's ``allowed`` (bautin_ref.cgl_bautin_yardstick).  J - i omega is singular there; with the
    bordered solve H21 converges, so the whole normal form reports convergence (on the elimination path that is recorded, not
    required)."""
    codim2, hip = _lib()
    y = BR.cgl_bautin_yardstick()
    lu, allowed, loc = y["lu"], y["allowed"], y["loc"]
    pars = dict(y["par"])
    out, h21 = {}, {}
    for kind in ("native", "mirror"):
        c = hip.Context(0)
        prob = hip.CGL2d(c, DIMS, LS, **pars)
        ls = _solver(hip, prob, loc["p1"], reltol=BR.RELTOL)
        X = codim2.HopfVec(prob.vec(loc["u"]), [loc["p1"], loc["omega"]])
        hp = codim2.hopf_normal_form_native(prob, X, _pair(prob, y["zeta"]), _pair(prob, y["zeta_star"]), ls)
        assert hp.converged, hp.itlinear
        f = codim2.bautin_normal_form_native if kind == "native" else codim2.bautin_normal_form
        out[kind] = bt = f(prob, hp, ls, lens2="c3", bls=hip.MatrixFreeBLS(ls, use_pl=True))
        print(f"{kind}: G21 = {bt.nf.G21:.12g}, G32 = {bt.nf.G32:.12g}, l2 = {bt.nf.l2:.12g} (restatement {lu['l2']:.12g}), type "
              f"{bt.type}, converged {bt.converged}, itlinear {bt.itlinear}, unconverged {bt.unconverged_solves}")
        assert bt.converged and bt.type == lu["type"] == "Supercritical"
        for k in ("G21", "G32", "l2"):
            d = abs(complex(getattr(bt.nf, k)) - lu[k])
            probe(f"hopfb.bautin_{k}.{kind}", d, allowed[k], relative=d / abs(lu[k]))
        d = np.abs(_num(bt.nf.H21) - lu["H21"]).max()
        probe(f"hopfb.bautin_H21.{kind}", d, allowed["H21"], relative=d / np.abs(lu["H21"]).max())
        if kind == "native":
            assert c.get_option("hopf_bordered") == 0.0            # put back after the call
        h21[kind] = _num(bt.nf.H21)
        c.close()
    na, mi = out["native"], out["mirror"]
    assert na.unconverged_solves == 0
    assert na.itlinear == mi.itlinear, (na.itlinear, mi.itlinear)
    assert h21["native"].tobytes() == h21["mirror"].tobytes()


# ------------------------------------------------------------------------------------------ the default path is untouched
def test_default_path_is_bitwise_the_same_with_the_option_unset_and_at_zero():
    codim2, hip = _lib()
    from bk_amd import _lib as L
    op, rstar, a, b = H.trivial_case()
    out = []
    for set_zero in (False, True):
        c = hip.Context(0)
        prob = hip.CGL2d(c, DIMS, LS, **dict(PARS, r=rstar + 0.02))
        ls = _solver(hip, prob, rstar + 0.02)
        if set_zero:
            c.set_option("hopf_bordered", 0.0)
        else:
            with pytest.raises(L.BkHipError):
                c.get_option("hopf_bordered")                    # never set on a fresh context
        X0 = codim2.HopfVec(prob.vec(np.zeros(a.size)), [rstar + 0.02, 0.95 * NU])
        s = codim2.newton_hopf_native(prob, X0, _pair(prob, a), _pair(prob, b), ls, tol=1e-12, max_iterations=15)
        if not set_zero:
            with pytest.raises(L.BkHipError):
                c.get_option("hopf_bordered")                    # bls = None touches no option
        out.append((tuple(s["u"].p), s["u"].u.numpy().tobytes(), tuple(s["residuals"]), s["itnewton"], s["itlineartot"],
                    s["unconverged_solves"], _num(s["v"]).tobytes(), _num(s["w"]).tobytes()))
        c.close()
    assert out[0] == out[1]
