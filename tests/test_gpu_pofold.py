"""GPU tests of the adjoint layer of the trapezoid periodic orbits of cGL (csrc/pofold.hip, bk_amd.periodic_orbit): the adjoint
marching kernel against the restatement in extended precision (tests/pofold_ref.py, pinned by test_pofold_reference.py), its
duality with the forward kernel, chunk independence, the transposed space-time preconditioner against sparse LU of A0^T, the
adjoint preconditioned solve and the doubly bordered solve against SciPy GMRES on the same systems, the border row of the fold
system against extended precision, the fold refinement (native and mirror) and three steps of the fold curve in c5 against the
restatement's, the cross-check of the refined point with the Floquet multipliers, and the refusals.

Shapes, those of the orbit tests: (12, 9) M = 7; (23, 17) M = 9 -- a partial tile, odd extents, the second field of every slice
8-byte misaligned --; (16, 12) M = 12; (12, 9) M = 3, the smallest cycle (K = 2)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import scipy.sparse.linalg as spla
import torch

import pofold_ref as F
import potrap_ref as R
from conftest import probe
from test_gpu_hopf import LS, PARS

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
LD = np.longdouble
CASES = [((12, 9), 7), ((23, 17), 9), ((16, 12), 12), ((12, 9), 3)]
GUARD = 64                      # doubles of NaN on both sides of every output


def _mods():
    from bk_amd import hip, periodic_orbit
    return hip, periodic_orbit


def _pv(pars):
    return [pars[k] for k in R.PNAMES]


@functools.lru_cache(maxsize=None)
def _model(dims):
    return R.Model(dims, LS)


@functools.lru_cache(maxsize=None)
def _inputs(dims, M):
    m = _model(dims)
    rng = np.random.default_rng(2000 * dims[0] + M)
    d = dict(U=0.6 * rng.standard_normal((M, m.N)), W=rng.standard_normal((M, m.N)), X=rng.standard_normal((M, m.N)),
             phi=rng.standard_normal((M, m.N)), T=5.0 + rng.random(), tau=rng.standard_normal(), dT=rng.standard_normal())
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _adjoint(ctx, po, U, T, pv, W, tau):
    """bk_potrap_jvp_adjoint into a NaN-guarded buffer -> (out (M, N), tail); the guard bands stay NaN."""
    from bk_amd.hip import _ptr
    from bk_amd.periodic_orbit import _parr
    full = torch.full((po.n + 2 * GUARD,), float("nan"), dtype=torch.float64, device=ctx.torch_device)
    out = full[GUARD:GUARD + po.n]
    tail = C.c_double()
    ctx.check(ctx.lib.bk_potrap_jvp_adjoint(po.h, _ptr(U.t), float(T), _parr(pv), len(pv), _ptr(W.t), float(tau), _ptr(out),
                                            C.byref(tail)), "jvp_adjoint")
    ctx.sync()
    a = full.cpu().numpy()
    assert np.isnan(a[:GUARD]).all() and np.isnan(a[GUARD + po.n:]).all()
    return a[GUARD:GUARD + po.n].reshape(po.M, -1).copy(), tail.value


def _setup(ctx, dims, M):
    hip, po_ = _mods()
    d = _inputs(dims, M)
    pars = dict(PARS, r=0.3, gamma=0.2)
    prob = hip.CGL2d(ctx, dims, LS, **pars)
    po = po_.PeriodicOrbitTrap(prob, M)
    po.set_section(po.vec(d["phi"]), po.vec(np.zeros_like(d["phi"])))
    return d, pars, po


# ------------------------------------------------------------------------------------------ the adjoint march
@pytest.mark.parametrize("dims,M", CASES)
def test_adjoint_march_matches_extended_precision_and_is_dual_to_the_forward_march(ctx, dims, M):
    """Random slices, w, T, tau, gamma != 0 against the long-double restatement in units of eps * (sum of the moduli of the terms):
    a monomial passes through at most ~13 roundings of eps / 2 on the device (6 in the quintic term of the Jacobian block, s_j, the
    product with it, 2 in the sums of q, the product with h / 2, the difference, the closure and the section terms), so 7 units is
    the worst case and 16 the bound the two forward marching kernels are held to.  The tail within the summation bound of the phase
    dot of test_gpu_potrap.py, 4 n eps sum |terms|.  <dG x, y> = <x, dG^T y> between the two native applications: both sides are
    summed in long double on the host from the device's outputs, whose entries are within 16 eps units and whose tails within
    4 n eps units (above; test_gpu_potrap.py for the forward one), so the two sides differ by at most the summation bound
    4 n eps (sum unit_fwd |y| + sum unit_adj |x|), tails included."""
    hip, po_ = _mods()
    m = _model(dims)
    d, pars, po = _setup(ctx, dims, M)
    U, W, X = po.vec(d["U"]), po.vec(d["W"]), po.vec(d["X"])
    n = po.n
    got, tail = _adjoint(ctx, po, U, d["T"], _pv(pars), W, d["tau"])
    ref, rtail = F.jvp_adjoint(m, d["U"].astype(LD), d["T"], pars, d["W"].astype(LD), d["tau"], d["phi"].astype(LD))
    unit, utail = F.jvp_adjoint(m, d["U"], d["T"], pars, d["W"], d["tau"], d["phi"], mod=True)
    probe(f"pofold.adjoint_ulps.{dims}.{M}", float((np.abs(got - ref) / (EPS * unit)).max()), 16.0, tight=4.0)
    probe(f"pofold.adjoint_tail.{dims}.{M}", abs(tail - float(rtail)) / (4 * n * EPS * utail), 1.0)
    # the operator handle is the same pass, and its adjoint is the forward one
    J = po.jacobian(U, d["T"], _pv(pars))
    JT = J.adjoint()
    o = JT(hip.BorderedArray(W, d["tau"]))
    assert JT.is_adjoint and np.array_equal(o.u.numpy().reshape(M, -1), got) and o.p == tail
    fx = J(hip.BorderedArray(X, d["dT"]))
    fb = JT.adjoint()(hip.BorderedArray(X, d["dT"]))
    assert not JT.adjoint().is_adjoint and np.array_equal(fb.u.numpy(), fx.u.numpy()) and fb.p == fx.p
    fxu = fx.u.numpy().reshape(M, -1)
    lhs = np.sum(fxu.astype(LD) * d["W"].astype(LD)) + LD(fx.p) * LD(d["tau"])
    rhs = np.sum(d["X"].astype(LD) * got.astype(LD)) + LD(d["dT"]) * LD(tail)
    funit, futail = R.jvp(m, d["U"], d["T"], pars, d["X"], d["dT"], d["phi"], mod=True)
    scale = (np.sum(funit * np.abs(d["W"])) + futail * abs(d["tau"])) + (np.sum(unit * np.abs(d["X"])) + utail * abs(d["dT"]))
    probe(f"pofold.duality.{dims}.{M}", abs(float(lhs - rhs)) / (4 * n * EPS * scale), 1.0)


def test_adjoint_rows_have_the_same_bits_for_every_chunking_and_aliasing_is_refused(ctx):
    """Context option potrap_chunks = 1, 2, 4, 11 and the default at 16 x 12, M = 12 (K = 11: 2 chunks are C = 6 with a last chunk
    of 5 rows, 4 chunks C = 3 / 2 rows, 11 chunks one row each): every chunking gives the rows of the single chunk bit for bit;
    only the tail, reduced over another set of workgroups, may differ, within its summation bound.  out aliasing u, w or the
    section is refused."""
    hip, po_ = _mods()
    from bk_amd._lib import BkHipError
    from bk_amd.hip import _ptr
    from bk_amd.periodic_orbit import _parr
    dims, M = (16, 12), 12
    m = _model(dims)
    d, pars, po = _setup(ctx, dims, M)
    U, W = po.vec(d["U"]), po.vec(d["W"])
    res = {}
    try:
        for k in (1.0, 2.0, 4.0, 11.0, 0.0):
            ctx.set_option("potrap_chunks", k)
            res[k] = _adjoint(ctx, po, U, d["T"], _pv(pars), W, d["tau"])
    finally:
        ctx.set_option("potrap_chunks", 0.0)
    _, utail = F.jvp_adjoint(m, d["U"], d["T"], pars, d["W"], d["tau"], d["phi"], mod=True)
    for k in res:
        assert np.array_equal(res[k][0], res[1.0][0]), k
        # two tails, each within the summation bound 4 n eps sum |terms| of the exact sum, differ by at most twice that
        assert abs(res[k][1] - res[1.0][1]) <= 8 * po.n * EPS * utail
    again = _adjoint(ctx, po, U, d["T"], _pv(pars), W, d["tau"])
    assert again[1] == res[0.0][1]
    pv, tail = _pv(pars), C.c_double()
    phi, _ = po.get_section()
    for out in (U, W):
        with pytest.raises(BkHipError, match="must not alias"):
            ctx.check(ctx.lib.bk_potrap_jvp_adjoint(po.h, _ptr(U.t), 6.0, _parr(pv), 6, _ptr(W.t), 0.5, _ptr(out.t), C.byref(tail)),
                      "alias")
    po2 = po_.PeriodicOrbitTrap(po.prob, M)
    with pytest.raises(BkHipError, match="no section set"):
        po2.jvp_adjoint(U, 6.0, pv, W, 0.5)
    with pytest.raises(BkHipError, match="no section set"):
        po_.PoTrapJacobian(po2, U, 6.0, pv, adjoint=True)
    with pytest.raises(BkHipError, match="params = "):
        po.jvp_adjoint(U, 6.0, pv[:5], W, 0.5)


def test_fold_border_rows_have_the_same_bits_for_every_chunking(ctx):
    """bk_potrap_fold_border, lens r, under potrap_chunks = 1, 2, 4, 11 and the default at 16 x 12, M = 12 (K = 11: C = 11, 6 / 5,
    3 / 3 / 3 / 2, 1): every chunking gives sigx of the single chunk bit for bit; (sigma_x)_T and sigma_p, reduced over another set
    of workgroups, stay within the summation bound 4 n eps sum |terms| of the long-double restatement, the bound of
    test_fold_border_matches_extended_precision."""
    hip, po_ = _mods()
    dims, M = (16, 12), 12
    m = _model(dims)
    d, pars, po = _setup(ctx, dims, M)
    U, W, V = po.vec(d["U"]), po.vec(d["W"]), po.vec(d["X"])
    vT = d["dT"]
    res = {}
    try:
        for k in (1.0, 2.0, 4.0, 11.0, 0.0):
            ctx.set_option("potrap_chunks", k)
            sx, sp = po.fold_border(U, d["T"], _pv(pars), R.PNAMES.index("r"), hip.BorderedArray(V, vT), W)
            res[k] = (sx.u.numpy(), sx.p, sp)
    finally:
        ctx.set_option("potrap_chunks", 0.0)
    L = lambda a: a.astype(LD)
    _, rT, rp = F.fold_border(m, L(d["U"]), d["T"], pars, "r", L(d["X"]), vT, L(d["W"]))
    _, uT, up = F.fold_border(m, d["U"], d["T"], pars, "r", d["X"], vT, d["W"], mod=True)
    for k, (sx, sT, sp) in res.items():
        assert np.array_equal(sx, res[1.0][0]), k
        probe(f"pofold.border_chunks_T.{int(k)}", abs(sT - float(rT)) / (4 * po.n * EPS * uT), 1.0)
        probe(f"pofold.border_chunks_p.{int(k)}", abs(sp - float(rp)) / (4 * po.n * EPS * up), 1.0)


# ------------------------------------------------------------------------------------------ the adjoint preconditioner
@functools.lru_cache(maxsize=None)
def _precond_reference(dims, M):
    m = _model(dims)
    a, b, T = -m.lam.max() - 0.05, PARS["nu"], 2 * math.pi
    f = np.random.default_rng(3 + M).standard_normal((M, m.N))
    lu = spla.splu(R.A0_sparse(m, M, T, a, b).T.tocsc()).solve(f.reshape(-1)).reshape(M, -1)
    md = F.modal_solve_adjoint(m, M, T, a, b, f)
    return a, b, T, f, lu, float(np.abs(md - lu).max())


@pytest.mark.parametrize("dims,M", CASES)
def test_adjoint_preconditioner_matches_sparse_lu_of_A0_transposed(ctx, dims, M):
    """bk_precond_apply of the transposed space-time preconditioner against sparse LU of the assembled A0^T.  Bound: 10 x
    max(the restatement's own modal-versus-LU difference at the same case, 8 eps |solution|) -- the project's margin; the floor
    because the restatement's difference can fall under the rounding of the solution's own entries."""
    hip, po_ = _mods()
    a, b, T, f, lu, yard = _precond_reference(dims, M)
    prob = hip.CGL2d(ctx, dims, LS, **PARS)
    po = po_.PeriodicOrbitTrap(prob, M)
    P = po_.PoTrapPreconditioner(po, a, b, adjoint=True).set_period(T)
    got = P.ldiv(po.vec(f)).numpy().reshape(M, -1)
    err = float(np.abs(got - lu).max())
    print(f"adjoint preconditioner {dims} M={M}: GPU vs LU {err:.3e}, restatement vs LU {yard:.3e}")
    probe(f"pofold.precond_vs_lu.{dims}.{M}", err, 10 * max(yard, 8 * EPS * float(np.abs(lu).max())))
    # not the forward one: the two differ by far more than the bound
    fwd = po_.PoTrapPreconditioner(po, a, b).set_period(T).ldiv(po.vec(f)).numpy().reshape(M, -1)
    assert np.abs(fwd - lu).max() > 1e-3 * np.abs(lu).max()


def test_adjoint_preconditioner_transform_paths_and_period_guard(ctx):
    """41 x 21, M = 3: the matrix-core transform pass along x and the one-thread-per-output kernel (option dct_gemm = 0) give the
    same bits, and each is within the yardstick; the plan records which ran.  The period guard refuses the Hopf-critical
    (a, b, T) as for the forward preconditioner (the moduli are equal)."""
    hip, po_ = _mods()
    from bk_amd._lib import BkHipError
    dims, M = (41, 21), 3
    a, b, T, f, lu, yard = _precond_reference(dims, M)
    prob = hip.CGL2d(ctx, dims, LS, **PARS)
    po = po_.PeriodicOrbitTrap(prob, M)
    P = po_.PoTrapPreconditioner(po, a, b, adjoint=True).set_period(T)
    assert P.transform_paths() == (-1, -1)
    out = {}
    try:
        for g in (1.0, 0.0):
            ctx.set_option("dct_gemm", g)
            out[g] = P.ldiv(po.vec(f)).numpy().reshape(M, -1)
            probe(f"pofold.precond_vs_lu.gemm{int(g)}", float(np.abs(out[g] - lu).max()),
                  10 * max(yard, 8 * EPS * float(np.abs(lu).max())))
            assert P.transform_paths() == ((1, 0) if g else (0, 0))
    finally:
        ctx.set_option("dct_gemm", 1.0)
    assert np.array_equal(out[1.0], out[0.0])
    dims, M = (16, 12), 12
    m = _model(dims)
    po = po_.PeriodicOrbitTrap(hip.CGL2d(ctx, dims, LS, **PARS), M)
    P = po_.PoTrapPreconditioner(po, -m.lam.max(), PARS["nu"], adjoint=True)
    with pytest.raises(BkHipError, match=r"rho\^K.*sine mode \(1, 1\).*move a"):
        P.set_period((2 * M / PARS["nu"]) * math.tan(math.pi / (M - 1)))
    with pytest.raises(BkHipError, match="no period set"):
        P.ldiv(po.vec(np.zeros(po.n)))
    P.set_period(2 * math.pi)


# ------------------------------------------------------------------------------------------ the adjoint solve
@functools.lru_cache(maxsize=None)
def _orbit_like(dims, M):
    """A smooth orbit-like state (the first sine mode turning once), its section by updatesection!, a random right-hand side."""
    m = _model(dims)
    pars = dict(PARS, r=-m.lam.max() - 0.1)
    x, y = np.meshgrid(np.arange(1, m.nx + 1) / (m.nx + 1), np.arange(1, m.ny + 1) / (m.ny + 1))
    mode = (np.sin(np.pi * x) * np.sin(np.pi * y)).reshape(-1)
    th = 2 * math.pi * np.arange(M) / (M - 1)
    U = 0.6 * np.stack([np.concatenate([math.cos(t) * mode, math.sin(t) * mode]) for t in th])
    T = 2 * math.pi * M / (M - 1)
    phi, xpi = R.update_section(m, U, pars)
    rhs = np.random.default_rng(5).standard_normal(M * m.N + 1)
    return pars, U, T, phi, xpi, rhs


def test_adjoint_solve_matches_preconditioned_scipy_gmres_and_a_mixed_pair_is_refused(ctx):
    """One adjoint solve at 16 x 12, M = 12, rtol 1e-9, IterativeSolvers flavor, against the restatement's preconditioned SciPy
    GMRES on the same transposed system: the iteration count within 4 of SciPy's (the margin of test_gpu_potrap.py), the error
    against the exact solution (sparse LU of the assembled transpose) within 10 x the restatement's.  A forward operator with an
    adjoint preconditioner, and the reverse, are refused."""
    hip, po_ = _mods()
    from bk_amd._lib import BkHipError
    dims, M = (16, 12), 12
    m = _model(dims)
    pars, U0, T, phi, xpi, rhs = _orbit_like(dims, M)
    a, b = pars["r"], pars["nu"]
    exact = spla.splu(R.jacobian_sparse(m, U0, T, pars, phi).T.tocsc()).solve(rhs)
    xc, itc = F.gmres_solve_adjoint(m, U0, T, pars, phi, rhs, a, b, T, 1e-9)
    prob = hip.CGL2d(ctx, dims, LS, **pars)
    po = po_.PeriodicOrbitTrap(prob, M, po_.HipVec.from_numpy(ctx, phi.reshape(-1)), po_.HipVec.from_numpy(ctx, xpi.reshape(-1)))
    U = po.vec(U0)
    J = po.jacobian(U, T, _pv(pars))
    JT = J.adjoint()
    P = po_.PoTrapPreconditioner(po, a, b).set_period(T)
    PT = po_.PoTrapPreconditioner(po, a, b, adjoint=True).set_period(T)
    ls = hip.GMRESIterativeSolvers(reltol=1e-9, restart=60, maxiter=200)
    b_ = hip.BorderedArray(po.vec(rhs[:-1]), float(rhs[-1]))
    x, cv, it = po_.po_solve(JT, PT, b_, ls)
    xg = R.pack(x.u.numpy().reshape(M, -1), x.p)
    print(f"adjoint solve: iterations GPU {it}, SciPy {itc}; |x - exact| GPU {np.abs(xg - exact).max():.3e}, "
          f"SciPy {np.abs(xc - exact).max():.3e}")
    assert cv
    probe("pofold.adjoint_solve_error", float(np.abs(xg - exact).max()), 10 * float(np.abs(xc - exact).max()))
    probe("pofold.adjoint_solve_count", abs(it - itc), 4, gpu=it, scipy=itc)
    with pytest.raises(BkHipError, match="a forward operator with an adjoint preconditioner"):
        po_.po_solve(J, PT, b_, ls)
    with pytest.raises(BkHipError, match="an adjoint operator with a forward preconditioner"):
        po_.po_solve(JT, P, b_, ls)


# ------------------------------------------------------------------------------------------ the doubly bordered solve
@pytest.mark.parametrize("adjoint", [False, True])
def test_doubly_bordered_solve_matches_scipy_and_sparse_lu(ctx, adjoint):
    """[A a; b' c][x; s] = [rhs; rhs_s] at 16 x 12, M = 12 with A = dG (and dG^T) on the orbit-like state, random a, b with T
    entries, c = 0.3: ONE GMRES at rtol 1e-9 left-preconditioned by diag(A0^-1, 1, 1) against the restatement's SciPy GMRES on the
    same system -- the iteration count within 4 --, and the error against sparse LU of the assembled bordered matrix within 10 x
    the restatement's.  The refusals are those of bk_potrap_solve."""
    hip, po_ = _mods()
    from bk_amd._lib import BkHipError
    dims, M = (16, 12), 12
    m = _model(dims)
    pars, U0, T, phi, xpi, _ = _orbit_like(dims, M)
    pa, pb = pars["r"], pars["nu"]
    rng = np.random.default_rng(77)
    nt = M * m.N + 1
    a, b, rhs, c = rng.standard_normal(nt), rng.standard_normal(nt), rng.standard_normal(nt + 1), 0.3
    exact, _ = F.bordered_solve_lu(m, U0, T, pars, phi, a, b, c, rhs, adjoint)
    xc, itc = F.bordered_solve_gmres(m, U0, T, pars, phi, a, b, c, rhs, pa, pb, T, 1e-9, adjoint)
    prob = hip.CGL2d(ctx, dims, LS, **pars)
    po = po_.PeriodicOrbitTrap(prob, M, po_.HipVec.from_numpy(ctx, phi.reshape(-1)), po_.HipVec.from_numpy(ctx, xpi.reshape(-1)))
    J = po_.PoTrapJacobian(po, po.vec(U0), T, _pv(pars), adjoint=adjoint)
    P = po_.PoTrapPreconditioner(po, pa, pb, adjoint=adjoint).set_period(T)
    ls = hip.GMRESIterativeSolvers(reltol=1e-9, restart=60, maxiter=200)
    B = lambda v: hip.BorderedArray(po.vec(v[:-1]), float(v[-1]))
    x, s, cv, it = po_.po_bordered_solve(J, P, B(a), B(b), c, B(rhs[:-1]), float(rhs[-1]), ls)
    xg = np.concatenate([x.u.numpy(), [x.p, s]])
    print(f"bordered solve adjoint={adjoint}: iterations GPU {it}, SciPy {itc}; |x - exact| GPU {np.abs(xg - exact).max():.3e}, "
          f"SciPy {np.abs(xc - exact).max():.3e}")
    assert cv
    probe(f"pofold.bordered_solve_error.{adjoint}", float(np.abs(xg - exact).max()), 10 * float(np.abs(xc - exact).max()))
    probe(f"pofold.bordered_solve_count.{adjoint}", abs(it - itc), 4, gpu=it, scipy=itc)
    Pw = po_.PoTrapPreconditioner(po, pa, pb, adjoint=not adjoint).set_period(T)
    with pytest.raises(BkHipError, match="operator with a.* preconditioner"):
        po_.po_bordered_solve(J, Pw, B(a), B(b), c, B(rhs[:-1]), float(rhs[-1]), ls)
    from bk_amd import _lib
    from bk_amd.hip import _ptr
    Ba, Bb, r_ = B(a), B(b), B(rhs[:-1])
    res, o, xt, xb = _lib.SolveResult(), ls._opts(), C.c_double(), C.c_double()
    with pytest.raises(BkHipError, match="must not alias"):
        ctx.check(ctx.lib.bk_potrap_bordered_solve(ctx.h, J.h, P.h, _ptr(Ba.u.t), 0.0, _ptr(Bb.u.t), 0.0, c, _ptr(r_.u.t), 0.0, 1.0,
                                                   _ptr(r_.u.t), C.byref(xt), C.byref(xb), C.byref(o), C.byref(res)), "alias")


# ------------------------------------------------------------------------------------------ the fold border
@pytest.mark.parametrize("name", ["r", "c5"])
@pytest.mark.parametrize("dims,M", CASES)
def test_fold_border_matches_extended_precision(ctx, dims, M, name):
    """bk_potrap_fold_border on random u, v, w for the lenses r and c5 against the long-double restatement: the vector within 16
    units of eps * (sum of the moduli of the terms) -- a monomial passes through ~11 roundings of eps / 2 (4 in the quintic term of
    the Hessian, its sum, the products with v and s and their sums, the product with h / 2, the final sum) --, the two sums within
    the summation bound 4 n eps sum |terms|.  The closure row is zero."""
    hip, po_ = _mods()
    m = _model(dims)
    d, pars, po = _setup(ctx, dims, M)
    U, W, V = po.vec(d["U"]), po.vec(d["W"]), po.vec(d["X"])
    vT = d["dT"]
    sx, sp = po.fold_border(U, d["T"], _pv(pars), R.PNAMES.index(name), hip.BorderedArray(V, vT), W)
    got = sx.u.numpy().reshape(M, -1)
    L = lambda a: a.astype(LD)
    ref, rT, rp = F.fold_border(m, L(d["U"]), d["T"], pars, name, L(d["X"]), vT, L(d["W"]))
    unit, uT, up = F.fold_border(m, d["U"], d["T"], pars, name, d["X"], vT, d["W"], mod=True)
    assert np.all(got[M - 1] == 0.0)
    safe = np.where(unit > 0, unit, 1.0)
    probe(f"pofold.border_ulps.{dims}.{M}.{name}", float((np.abs(got - ref) / (EPS * safe)).max()), 16.0, tight=4.0)
    probe(f"pofold.border_T.{dims}.{M}.{name}", abs(sx.p - float(rT)) / (4 * po.n * EPS * uT), 1.0)
    probe(f"pofold.border_p.{dims}.{M}.{name}", abs(sp - float(rp)) / (4 * po.n * EPS * up), 1.0)


def test_fold_border_refusals(ctx):
    hip, po_ = _mods()
    from bk_amd._lib import BkHipError
    from bk_amd.hip import _ptr
    from bk_amd.periodic_orbit import _parr
    d, pars, po = _setup(ctx, (12, 9), 7)
    U, W, V = po.vec(d["U"]), po.vec(d["W"]), po.vec(d["X"])
    pv, a, b = _pv(pars), C.c_double(), C.c_double()
    for out in (U, V, W):
        with pytest.raises(BkHipError, match="must not alias"):
            ctx.check(ctx.lib.bk_potrap_fold_border(po.h, _ptr(U.t), 6.0, _parr(pv), 6, 0, _ptr(V.t), 0.1, _ptr(W.t), _ptr(out.t),
                                                    C.byref(a), C.byref(b)), "alias")
    with pytest.raises(BkHipError, match="bad parameter index"):
        po.fold_border(U, 6.0, pv, 7, hip.BorderedArray(V, 0.1), W)
    with pytest.raises(BkHipError, match="params = "):
        po.fold_border(U, 6.0, pv[:5], 0, hip.BorderedArray(V, 0.1), W)


# ------------------------------------------------------------------------------------------ fold refinement
def _fold_branch(ctx, save_sol=None, steps=None):
    """continuation_po_trap over the fold run of test_gpu_floquet.py (16 x 12, M = 12, dr = 0.15) -> (prob, po, guess, pars, br)."""
    from bk_amd import continuation as Cn
    from test_gpu_floquet import FOLD, RTOL, TOL_EIG
    from test_gpu_potrap import _guess
    hip, po_ = _mods()
    dims, M, dr, nsteps, tol, cpd = (FOLD[k] for k in ("dims", "M", "dr", "steps", "tol_stability", "cp"))
    prob, po, g, pars, _ = _guess(ctx, dims, M, dr)
    cp = Cn.ContinuationPar(ds=cpd["ds"], dsmin=cpd["dsmin"], dsmax=cpd["dsmax"], a=cpd["a"], eta=cpd["eta"], p_min=-10.0, p_max=10.0,
                            max_steps=nsteps if steps is None else steps, detect_bifurcation=0,
                            newton_options=Cn.NewtonPar(tol=1e-10, max_iterations=10))
    ls = hip.GMRESIterativeSolvers(reltol=RTOL, restart=60, maxiter=200)
    eig = hip.EigKrylovKit(tol=TOL_EIG, maxiter=20, krylovdim=20)
    kw = {} if save_sol is None else dict(save_sol=save_sol)
    br = po_.continuation_po_trap(po, g["orbit"], g["T"], _pv(pars), "r", cp, ls, nev=2, detect_bifurcation=2, tol_stability=tol,
                                  eig=eig, **kw)
    return prob, po, g, pars, br, ls


_REF = {}


def _fold_reference(m, g, pars, M):
    """The restatement's fold run from the GPU's Hopf guess, computed once and shared by the refinement and the fold-curve test:
    PALC with sparse LU to the point after the fold, the fold Newton with sparse LU and with preconditioned SciPy GMRES, and three
    PALC steps of the fold curve in c5 (FOLD_CP) with both."""
    if not _REF:
        from test_gpu_floquet import FOLD
        U0, T0 = g["orbit"].numpy().reshape(M, -1), g["T"]
        phi, xpi = g["phi"].numpy().reshape(M, -1), g["xpi"].numpy().reshape(M, -1)
        pars_of = lambda p: dict(pars, r=p)
        st = F.fold_start(m, U0, T0, pars, "r", phi, xpi, R.lu_solver(m, pars_of), FOLD["cp"], FOLD["steps"])
        pp = dict(pars, r=st["p"])
        solvers = dict(lu=F.lu_bsolver(m), gm=F.gmres_bsolver(m, pp["r"], pp["nu"], st["T"], 1e-9))
        _REF.update(st=st, pp=pp)
        for k, bs in solvers.items():
            _REF[k] = F.newton_fold(m, st["U"], st["T"], pp, "r", st["phi"], st["xpi"], st["tau"], st["tau"], bs)
        # each curve starts from the fold its own solver refined (as the device's starts from the device's), with the
        # preconditioner of the refinement (a = r of the guess, its period)
        for k, bs in solvers.items():
            ppf = dict(pp, r=_REF[k]["p"])
            _REF["curve_" + k] = F.palc_fold(m, _REF[k]["U"], _REF[k]["T"], ppf, "r", "c5", st["phi"], st["xpi"], st["tau"],
                                             st["tau"], bs, FOLD_CP, 3)
    return _REF


# the fold curve: optcontfold of cGL2d.jl:381 (ds = 0.01, dsmin = 1e-3, dsmax = 0.05) with the Newton settings of the orbit tests
FOLD_CP = dict(ds=0.01, dsmin=1e-3, dsmax=0.05, a=0.5, eta=150.0, tol=1e-10, max_iterations=10)


def test_fold_refinement_native_and_mirror_match_the_restatement(ctx):
    """continuation_po_trap(..., save_sol=True, nev=2, detect_bifurcation=2) over the fold run, po_fold_point, then
    newton_fold_po_native and newton_fold_po (GMRES rtol 1e-9, a = r, b = nu at the guess, period of the guess).  The restatement
    runs the same from the same Hopf guess: PALC with sparse LU, the fold Newton with sparse LU and with preconditioned SciPy GMRES.
    p, T and amplitude within 10 x |restatement-LU - restatement-GMRES| of the restatement's LU values, floored at 8 eps of the
    quantity -- and since the two start points (GPU branch, LU branch) differ by the branch's own GMRES-versus-LU difference, which
    Newton contracts quadratically, no term is added for it; the residual histories are as long as the restatement's; native and
    mirror agree within the same bound; the GMRES count of every bordered solve is within 4 of SciPy's."""
    from test_gpu_floquet import FOLD
    hip, po_ = _mods()
    dims, M = FOLD["dims"], FOLD["M"]
    m = _model(dims)
    prob, po, g, pars, br, ls = _fold_branch(ctx, save_sol=True)
    (sp,) = br["specialpoints"]
    assert sp["type"] == "bp" and sp["param"] == br["p"][sp["step"]] and sp["x"].p == br["T"][sp["step"]]
    ref_ = _fold_reference(m, g, pars, M)
    st, pp, lu, gm = ref_["st"], ref_["pp"], ref_["lu"], ref_["gm"]
    assert lu["converged"] and gm["converged"]
    fp = po_.po_fold_point(br, 0, po, _pv(pars), "r")
    tau = np.concatenate([fp["a"].u.numpy(), [fp["a"].p]])
    assert abs(np.linalg.norm(tau) - 1) <= 1e-14 and np.abs(tau - st["tau"]).max() <= 1e-6
    pv = _pv(dict(pars, r=fp["p"]))
    nat = po_.newton_fold_po_native(po, fp["orbit"], fp["T"], pv, "r", fp["a"], fp["b"], ls)
    mir = po_.newton_fold_po(po, fp["orbit"], fp["T"], pv, "r", fp["a"], fp["b"], ls)
    ref = dict(p=lu["p"], T=lu["T"], amplitude=float(np.abs(lu["U"]).max()))
    yard = dict(p=abs(lu["p"] - gm["p"]), T=abs(lu["T"] - gm["T"]),
                amplitude=abs(float(np.abs(lu["U"]).max()) - float(np.abs(gm["U"]).max())))
    print(f"fold refinement: native residuals {nat['residuals']}, mirror {mir['residuals']}, restatement {lu['residuals']}; "
          f"GMRES counts native {nat['itlinear']} {nat['last_terms_its']}, SciPy {gm['itlinear']} {gm['last_terms_its']}; yard {yard}")
    for name, s in (("native", nat), ("mirror", mir)):
        assert s["converged"] and len(s["residuals"]) == len(lu["residuals"]), (name, s["residuals"], lu["residuals"])
        got = dict(p=s["p"], T=s["T"], amplitude=po_.amplitude(s["u"]))
        for k in ref:
            probe(f"pofold.refine_{k}.{name}", abs(got[k] - ref[k]), 10 * max(yard[k], 8 * EPS * abs(ref[k])), got=got[k], ref=ref[k])
        counts = [c for t in s["itlinear"] for c in t] + list(s["last_terms_its"])
        scipy_counts = [c for t in gm["itlinear"] for c in t] + list(gm["last_terms_its"])
        assert len(counts) == len(scipy_counts)
        probe(f"pofold.refine_counts.{name}", max(abs(a - b) for a, b in zip(counts, scipy_counts)), 4)
    for k, a, b in (("p", nat["p"], mir["p"]), ("T", nat["T"], mir["T"]),
                    ("amplitude", po_.amplitude(nat["u"]), po_.amplitude(mir["u"]))):
        probe(f"pofold.native_vs_mirror_{k}", abs(a - b), 10 * max(yard[k], 8 * EPS * abs(ref[k])))
    assert abs(nat["sigma"]) <= 1e-10 and abs(mir["sigma"]) <= 1e-10
    assert nat["itlineartot"] == mir["itlineartot"] == sum(sum(t) for t in nat["itlinear"]) + sum(nat["last_terms_its"])
    # Cross-check with the Floquet layer, which shares nothing with the fold system: at the refined point both leading
    # multipliers sit at 1.  The bound of 9l for a simple multiplier is 10 kappa (delta + tol_eig); at the fold the multiplier 1 is
    # double and DEFECTIVE (the trivial one and the fold's share one eigenvector), so a perturbation of size e of the monodromy --
    # its GMRES error delta, the eigensolver's tolerance -- moves the pair by the order of sqrt(e), and the allowed distance is
    # the square root of that bound.  kappa of a defective eigenvalue is infinite; the kappa used is the larger of the two
    # leading multipliers' at the nearest regular point the restatement has, the branch point the Newton started from (dense
    # monodromy, multipliers 1 and 0.887), delta the recorded one of floquet_ref.DELTA at this grid and M.
    import floquet_ref as Fq
    from test_gpu_floquet import TOL_EIG
    wd, _, kap = Fq.leading_multipliers(Fq.dense_monodromy(m, st["U"], st["T"], pp), 2)
    bound = math.sqrt(10 * float(kap.max()) * (Fq.DELTA[(dims, M, 0.1)] + TOL_EIG))
    pvf = _pv(dict(pars, r=nat["p"]))
    fl = po_.floquet_multipliers(po, nat["u"], nat["T"], pvf, 2, ls, eig=hip.EigKrylovKit(tol=TOL_EIG, maxiter=20, krylovdim=20))
    dist = np.abs(np.asarray(fl["multipliers"])[:2] - 1.0)
    print(f"multipliers at the refined fold {fl['multipliers']}, |mu - 1| {dist}, bound {bound:.3e} (kappa {kap}, dense multipliers "
          f"at the start point {wd})")
    assert len(dist) == 2
    for k in range(2):
        probe(f"pofold.fold_multiplier.{k}", float(dist[k]) if dist[k] == dist[k] else float("inf"), bound)


def test_fold_curve_three_steps_in_c5_match_the_restatement(ctx):
    """continuation_fold_po for three steps in c5 from the refined point (ds = 0.01, dsmax = 0.05: the natural steps reach
    c5 = 1.014, 1.032, 1.057), a, b renewed after every point: (p1, p2, T) and the amplitude per step against the restatement's
    PALC of the fold curve with sparse LU, within 10 x |restatement-LU - restatement-GMRES|, floored at 8 eps of the quantity;
    the Newton counts are the restatement's, the GMRES counts per step within 4 per solve of SciPy's.  Sanity: along a fold curve
    of the quintic normal form r_fold - r_hopf ~ -c3^2 / (4 c5) x const, so (p1 - r_hopf) c5 stays near -0.2005; it is asserted
    within three times the spread the restatement shows."""
    from bk_amd import continuation as Cn
    from test_gpu_floquet import FOLD
    hip, po_ = _mods()
    dims, M = FOLD["dims"], FOLD["M"]
    m = _model(dims)
    prob, po, g, pars, br, ls = _fold_branch(ctx, save_sol=True)
    ref_ = _fold_reference(m, g, pars, M)
    lu, gm = ref_["curve_lu"], ref_["curve_gm"]
    fp = po_.po_fold_point(br, 0, po, _pv(pars), "r")
    pv = _pv(dict(pars, r=fp["p"]))
    nat = po_.newton_fold_po_native(po, fp["orbit"], fp["T"], pv, "r", fp["a"], fp["b"], ls)
    assert nat["converged"]
    c = FOLD_CP
    cp = Cn.ContinuationPar(ds=c["ds"], dsmin=c["dsmin"], dsmax=c["dsmax"], a=c["a"], eta=c["eta"], p_min=-10.0, p_max=40.1, max_steps=3,
                            detect_bifurcation=0, newton_options=Cn.NewtonPar(tol=c["tol"], max_iterations=c["max_iterations"]))
    B = hip.BorderedArray
    guess = B(B(nat["u"], nat["T"]), nat["p"])
    pl = po_.PoTrapPreconditioner(po, fp["p"], pars["nu"]).set_period(fp["T"])       # the refinement's: a = r and T of the guess
    plT = po_.PoTrapPreconditioner(po, fp["p"], pars["nu"], adjoint=True).set_period(fp["T"])
    fb = po_.continuation_fold_po(po, guess, pars["c5"], "c5", fp["a"], fp["b"], ls, cp, params=_pv(dict(pars, r=nat["p"])), pl=pl,
                                  pl_adjoint=plT)
    rh = -m.lam.max()
    print(f"fold curve: p1 - r_hopf {[p - rh for p in fb.p1]} (restatement {[p - rh for p in lu['p1']]}), p2 {fb.p2} ({lu['p2']}), "
          f"T {fb.T} ({lu['T']}), newton {fb.itnewton} ({lu['itnewton']}), gmres {fb.itlinear} (SciPy {gm['itlinear']})")
    assert len(fb.p1) == 4 and fb.itnewton[1:] == lu["itnewton"][1:]
    got = dict(p1=fb.p1, p2=fb.p2, T=fb.T, amplitude=fb.amplitude)
    for key in got:
        for k in range(4):
            yard = max(abs(lu[key][k] - gm[key][k]), 8 * EPS * abs(lu[key][k]))
            probe(f"pofold.curve_{key}.{k}", abs(got[key][k] - lu[key][k]), 10 * yard, got=got[key][k], ref=lu[key][k])
    for k in range(1, 4):
        # per step 2 bordered vectors per point and 2 fold solves per Newton step: (itnewton + 1) 2 + 2 itnewton solves
        nsolves = 2 * (lu["itnewton"][k] + 1) + 2 * lu["itnewton"][k]
        probe(f"pofold.curve_counts.{k}", abs(fb.itlinear[k] - gm["itlinear"][k]), 4 * nsolves, gpu=fb.itlinear[k], scipy=gm["itlinear"][k])
    prod_ref = [(a - rh) * b for a, b in zip(lu["p1"], lu["p2"])]
    spread = max(prod_ref) - min(prod_ref)
    prod = [(a - rh) * b for a, b in zip(fb.p1, fb.p2)]
    assert all(abs(q - prod_ref[0]) <= 3 * spread for q in prod), (prod, prod_ref)
    assert fb.p2[3] > fb.p2[0] and all(abs(x) <= 1.0 for x in fb.ab)


def test_continuation_po_trap_with_save_sol_false_gives_the_default_records(ctx):
    """save_sol=False, no keyword and save_sol=True give the same records key by key over the fold run (the runs are bitwise
    repeatable); save_sol=True only adds x, tau and param to the special point."""
    runs = {k: _fold_branch(ctx, save_sol=k)[4] for k in (None, False, True)}
    base = runs[None]
    for k in (False, True):
        br = runs[k]
        assert set(br) == set(base)
        for key in base:
            if key == "orbit":
                assert np.array_equal(br[key].u.numpy(), base[key].u.numpy()) and br[key].p == base[key].p
            elif key == "floquet":
                assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(br[key], base[key]))
            elif key == "specialpoints":
                assert len(br[key]) == len(base[key]) == 1
                extra = set(br[key][0]) - set(base[key][0])
                assert extra == ({"x", "tau", "param"} if k else set())
                assert all(br[key][0][q] == base[key][0][q] for q in base[key][0])
            else:
                assert br[key] == base[key], key
