"""GPU tests of the trapezoid periodic orbits of cGL (csrc/potrap.hip, bk_amd.periodic_orbit): the marching residual / JVP kernels
against the restatement in extended precision (tests/potrap_ref.py, pinned by test_potrap_reference.py), the space-time
preconditioner against sparse LU of its matrix, the preconditioned solve against SciPy GMRES on the same system, Newton from the
Hopf predictor and three PALC steps against the restatement's, and the refusals.

Shapes: (12, 9) M = 7; (16, 12) M = 12; (23, 17) M = 9 -- an odd point count, the second field of every slice is 8-byte
misaligned --; M = 3, the smallest cycle (K = 2); M = 33, past any bound at 32, and with a chunk count that does not divide."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import scipy.sparse.linalg as spla
import torch

import potrap_ref as R
from conftest import probe
from test_gpu_hopf import LS, PARS, _hopf_mode, _pair, _solver

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
LD = np.longdouble
CASES = [((12, 9), 7), ((16, 12), 12), ((23, 17), 9), ((12, 9), 3), ((12, 9), 33)]
GUARD = 64                      # doubles of NaN on both sides of every output


def _mods():
    from bk_amd import codim2, hip, periodic_orbit
    return codim2, hip, periodic_orbit


def _pv(pars):
    return [pars[k] for k in R.PNAMES]


@functools.lru_cache(maxsize=None)
def _model(dims):
    return R.Model(dims, LS)


@functools.lru_cache(maxsize=None)
def _inputs(dims, M):
    m = _model(dims)
    rng = np.random.default_rng(1000 * dims[0] + M)
    d = dict(U=0.6 * rng.standard_normal((M, m.N)), dU=rng.standard_normal((M, m.N)), phi=rng.standard_normal((M, m.N)),
             xpi=rng.standard_normal((M, m.N)), T=5.0 + rng.random(), dT=rng.standard_normal())
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _guarded(ctx, n):
    t = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float64, device=ctx.torch_device)
    return t, t[GUARD:GUARD + n]


def _march(ctx, po, hip, U, T, pv, dU=None, dT=0.0):
    """bk_potrap_residual / bk_potrap_jvp into a NaN-guarded buffer -> (out (M, N), tail); the guard bands stay NaN."""
    from bk_amd.hip import _ptr
    from bk_amd.periodic_orbit import _parr
    full, out = _guarded(ctx, po.n)
    tail = C.c_double()
    if dU is None:
        ctx.check(ctx.lib.bk_potrap_residual(po.h, _ptr(U.t), float(T), _parr(pv), len(pv), _ptr(out), C.byref(tail)), "residual")
    else:
        ctx.check(ctx.lib.bk_potrap_jvp(po.h, _ptr(U.t), float(T), _parr(pv), len(pv), _ptr(dU.t), float(dT), _ptr(out),
                                        C.byref(tail)), "jvp")
    ctx.sync()
    a = full.cpu().numpy()
    assert np.isnan(a[:GUARD]).all() and np.isnan(a[GUARD + po.n:]).all()
    return a[GUARD:GUARD + po.n].reshape(po.M, -1).copy(), tail.value


# ------------------------------------------------------------------------------------------ residual and JVP
@pytest.mark.parametrize("dims,M", CASES)
def test_potrap_residual_and_jvp_match_extended_precision(ctx, dims, M):
    """Random slices, T, dT, gamma != 0 against the long-double restatement in units of eps * (sum of the moduli of the terms):
    a monomial passes through at most ~11 roundings of eps / 2 on the device (5 in the quintic term, 2 in the sums of NL and the
    Laplacian, F + F_prev, the product with h / 2, the final difference), so 6 units is the worst case and 16 the bound -- the
    factor of test_gpu_hopf_normal_form's pointwise passes.  The phase sums within the summation bound 4 n eps sum |terms|."""
    _, hip, po_ = _mods()
    m, d = _model(dims), _inputs(dims, M)
    pars = dict(PARS, r=0.3, gamma=0.2)
    prob = hip.CGL2d(ctx, dims, LS, **pars)
    po = po_.PeriodicOrbitTrap(prob, M)
    po.set_section(po.vec(d["phi"]), po.vec(d["xpi"]))
    U, dU = po.vec(d["U"]), po.vec(d["dU"])
    n = po.n
    got, tail = _march(ctx, po, hip, U, d["T"], _pv(pars))
    ref, rtail = R.residual(m, d["U"].astype(LD), d["T"], pars, d["phi"].astype(LD), d["xpi"].astype(LD))
    unit, utail = R.residual(m, d["U"], d["T"], pars, d["phi"], d["xpi"], mod=True)
    probe(f"potrap.residual_ulps.{dims}.{M}", float((np.abs(got - ref) / (EPS * unit)).max()), 16.0, tight=4.0)
    probe(f"potrap.residual_tail.{dims}.{M}", abs(tail - float(rtail)) / (4 * n * EPS * utail), 1.0)
    got, tail = _march(ctx, po, hip, U, d["T"], _pv(pars), dU, d["dT"])
    ref, rtail = R.jvp(m, d["U"].astype(LD), d["T"], pars, d["dU"].astype(LD), d["dT"], d["phi"].astype(LD))
    unit, utail = R.jvp(m, d["U"], d["T"], pars, d["dU"], d["dT"], d["phi"], mod=True)
    probe(f"potrap.jvp_ulps.{dims}.{M}", float((np.abs(got - ref) / (EPS * unit)).max()), 16.0, tight=4.0)
    probe(f"potrap.jvp_tail.{dims}.{M}", abs(tail - float(rtail)) / (4 * n * EPS * utail), 1.0)
    # the operator handle is the same pass
    J = po.jacobian(U, d["T"], _pv(pars))
    o = J(hip.BorderedArray(dU, d["dT"]))
    assert np.array_equal(o.u.numpy().reshape(M, -1), got) and o.p == tail


def _chunking(K, want):
    """(C, nchunks) of potrap_chunking for a wanted chunk count."""
    want = min(max(int(want), 1), K)
    C = -(-K // want)
    return C, -(-K // C)


@pytest.mark.parametrize("dims,M,forced", [((12, 9), 33, (5, 3, 7)), ((16, 12), 12, (4, 2)), ((160, 128), 12, ())])
def test_potrap_rows_have_the_same_bits_for_every_chunking(ctx, dims, M, forced):
    """Context option potrap_chunks: 1 = a single time chunk (C = K), a huge value = one chunk per row (C = 1), and forced counts
    that do not divide K, so that chunks start at r0 > 0, carry their registers over several rows, and the last chunk is short
    and writes the closure row: K = 32 in 5 chunks is C = 7 with a last chunk of 4 rows, in 3 chunks C = 11 / 10 rows, in 7
    chunks C = 5 / 2 rows; K = 11 in 4 chunks is C = 3 / 2 rows, in 2 chunks C = 6 / 5 rows.  At 160 x 128 (80 tiles) the default
    rule itself picks 1 < C < K with a ragged end (asserted from the device's compute-unit count).  Every chunking gives the rows
    of the single chunk bit for bit -- those are within 16 units of the long-double restatement, checked here once more -- and
    only the phase sum, reduced over another set of workgroups, may differ, within its summation bound."""
    _, hip, po_ = _mods()
    K = M - 1
    for k in forced:
        C, nch = _chunking(K, k)
        assert 1 < C < K and K % C != 0 and nch == k, (k, C, nch)
    if not forced:
        cus = torch.cuda.get_device_properties(ctx.torch_device).multi_processor_count
        tiles = -(-dims[0] * dims[1] // 256)
        C, nch = _chunking(K, -(-2 * cus // tiles))
        assert 1 < C < K and K % C != 0, (cus, tiles, C, nch)
    m, d = _model(dims), _inputs(dims, M)
    pars = dict(PARS, r=0.3, gamma=0.2)
    prob = hip.CGL2d(ctx, dims, LS, **pars)
    po = po_.PeriodicOrbitTrap(prob, M, po_.HipVec.from_numpy(ctx, d["phi"].reshape(-1)), po_.HipVec.from_numpy(ctx, d["xpi"].reshape(-1)))
    U, dU = po.vec(d["U"]), po.vec(d["dU"])
    res = {}
    try:
        for k in (1.0, 1e9, 0.0) + tuple(float(f) for f in forced):
            ctx.set_option("potrap_chunks", k)
            res[k] = (_march(ctx, po, hip, U, d["T"], _pv(pars)), _march(ctx, po, hip, U, d["T"], _pv(pars), dU, d["dT"]))
    finally:
        ctx.set_option("potrap_chunks", 0.0)
    uu, ut = R.residual(m, d["U"], d["T"], pars, d["phi"], d["xpi"], mod=True)
    ju, jt = R.jvp(m, d["U"], d["T"], pars, d["dU"], d["dT"], d["phi"], mod=True)
    rr, _ = R.residual(m, d["U"].astype(LD), d["T"], pars, d["phi"].astype(LD), d["xpi"].astype(LD))
    jr, _ = R.jvp(m, d["U"].astype(LD), d["T"], pars, d["dU"].astype(LD), d["dT"], d["phi"].astype(LD))
    probe(f"potrap.chunk1_residual_ulps.{dims}.{M}", float((np.abs(res[1.0][0][0] - rr) / (EPS * uu)).max()), 16.0)
    probe(f"potrap.chunk1_jvp_ulps.{dims}.{M}", float((np.abs(res[1.0][1][0] - jr) / (EPS * ju)).max()), 16.0)
    for k in res:
        for w, unit in ((0, ut), (1, jt)):
            assert np.array_equal(res[k][w][0], res[1.0][w][0]), (k, w)
            assert abs(res[k][w][1] - res[1.0][w][1]) <= 8 * po.n * EPS * unit
    # run to run the phase sum has the same bits too
    again = _march(ctx, po, hip, U, d["T"], _pv(pars), dU, d["dT"])
    assert again[1] == res[0.0][1][1]


def test_potrap_update_section_and_dparam_match_the_restatement(ctx):
    _, hip, po_ = _mods()
    dims, M = (23, 17), 9
    m, d = _model(dims), _inputs(dims, M)
    pars = dict(PARS, r=0.3, gamma=0.2)
    prob = hip.CGL2d(ctx, dims, LS, **pars)
    po = po_.PeriodicOrbitTrap(prob, M)
    U = po.vec(d["U"])
    po.update_section(U, d["T"], _pv(pars))
    phi, xpi = R.update_section(m, d["U"].astype(LD), pars)
    # <u - xpi, phi> = 0 at u = xpi, up to the rounding of the two sums
    r = po.residual(U, d["T"], _pv(pars))
    unit = np.sum(np.abs(d["U"] * phi.astype(float)))
    assert abs(r.p) <= 8 * po.n * EPS * unit
    # the section itself, read back, entry by entry: xpi is u, phi_i is F(u_i) / M within 16 units of eps * (moduli of F's terms)
    # / M, the bound of the pointwise passes (the device multiplies by 1 / M, one rounding more than the division)
    gphi, gxpi = (v.numpy().reshape(M, -1) for v in po.get_section())
    assert np.array_equal(gxpi, d["U"])
    unit_phi = np.stack([m.F_abs(d["U"][i], pars) / M for i in range(M)])
    probe("potrap.update_section_phi_ulps", float((np.abs(gphi - phi) / (EPS * unit_phi)).max()), 16.0, tight=4.0)
    # ... and a set_section round trip returns what was set
    po.set_section(po.vec(d["phi"]), po.vec(d["xpi"]))
    sphi, sxpi = (v.numpy().reshape(M, -1) for v in po.get_section())
    assert np.array_equal(sphi, d["phi"]) and np.array_equal(sxpi, d["xpi"])
    po.update_section(U, d["T"], _pv(pars))
    got = po.jvp(U, d["T"], _pv(pars), po.vec(d["dU"]), 0.0).p
    ref = float(np.sum(d["dU"].astype(LD) * phi))
    assert abs(got - ref) <= 8 * po.n * EPS * float(np.sum(np.abs(d["dU"] * phi.astype(float))))
    for name in ("r", "mu", "c5"):
        g = po.dparam(U, d["T"], _pv(pars), R.PNAMES.index(name)).numpy().reshape(M, -1)
        ref = R.dparam(m, d["U"].astype(LD), d["T"], pars, name).astype(float)
        assert np.abs(g - ref).max() <= 16 * EPS * np.abs(ref).max(), name
        assert np.all(g[M - 1] == 0.0)


# ------------------------------------------------------------------------------------------ the preconditioner
@functools.lru_cache(maxsize=None)
def _precond_reference(dims, M):
    m = _model(dims)
    a, b, T = -m.lam.max() - 0.05, PARS["nu"], 2 * math.pi
    f = np.random.default_rng(3 + M).standard_normal((M, m.N))
    lu = spla.splu(R.A0_sparse(m, M, T, a, b)).solve(f.reshape(-1)).reshape(M, -1)
    md = R.modal_solve(m, M, T, a, b, f)
    return a, b, T, f, lu, float(np.abs(md - lu).max())


@pytest.mark.parametrize("dims,M", CASES)
def test_potrap_preconditioner_matches_sparse_lu_of_A0(ctx, dims, M):
    """bk_precond_apply of the space-time preconditioner (batched DST-I, time solve, DST-I) against sparse LU of the assembled A0.
    The yardstick is the restatement's own modal-versus-LU difference at the same case (test_potrap_reference pins it, DESIGN 9k
    lists it); the GPU gets 10 x it."""
    _, hip, po_ = _mods()
    a, b, T, f, lu, yard = _precond_reference(dims, M)
    prob = hip.CGL2d(ctx, dims, LS, **PARS)
    po = po_.PeriodicOrbitTrap(prob, M)
    P = po_.PoTrapPreconditioner(po, a, b).set_period(T)
    got = P.ldiv(po.vec(f)).numpy().reshape(M, -1)
    err = float(np.abs(got - lu).max())
    print(f"potrap preconditioner {dims} M={M}: GPU vs LU {err:.3e}, restatement vs LU {yard:.3e}")
    probe(f"potrap.precond_vs_lu.{dims}.{M}", err, 10 * yard)


def test_potrap_preconditioner_matrix_core_and_direct_transform_paths(ctx):
    """41 points along x run the transform pass as the matrix-core product (>= 32), 21 along y as the one-thread-per-output
    kernel; option dct_gemm = 0 forces the latter on both axes.  Which kernel a pass dispatched to is recorded in the plan by
    the dispatch itself and read back (bk_precond_potrap_transform_paths: per axis 1 = matrix cores, 0 = one thread per output,
    -1 before the first application); both give the preconditioner within the yardstick.  (Both kernels accumulate along the
    transformed index in the same order, so the bits cannot tell them apart.)"""
    _, hip, po_ = _mods()
    dims, M = (41, 21), 3
    a, b, T, f, lu, yard = _precond_reference(dims, M)
    prob = hip.CGL2d(ctx, dims, LS, **PARS)
    po = po_.PeriodicOrbitTrap(prob, M)
    P = po_.PoTrapPreconditioner(po, a, b).set_period(T)
    assert P.transform_paths() == (-1, -1)
    out = {}
    try:
        for g in (1.0, 0.0):
            ctx.set_option("dct_gemm", g)
            out[g] = P.ldiv(po.vec(f)).numpy().reshape(M, -1)
            probe(f"potrap.precond_vs_lu.gemm{int(g)}", float(np.abs(out[g] - lu).max()), 10 * yard)
            assert P.transform_paths() == ((1, 0) if g else (0, 0))
    finally:
        ctx.set_option("dct_gemm", 1.0)
    # a shape of the other tests takes no matrix-core pass at all
    po2 = po_.PeriodicOrbitTrap(hip.CGL2d(ctx, (16, 12), LS, **PARS), 3)
    P2 = po_.PoTrapPreconditioner(po2, 0.3, 1.0).set_period(6.0)
    P2.ldiv(po2.vec(np.ones(po2.n)))
    assert P2.transform_paths() == (0, 0)


def test_potrap_preconditioner_refuses_a_hopf_critical_mode(ctx):
    _, hip, po_ = _mods()
    from bk_amd._lib import BkHipError
    dims, M = (16, 12), 12
    m = _model(dims)
    prob = hip.CGL2d(ctx, dims, LS, **PARS)
    po = po_.PeriodicOrbitTrap(prob, M)
    P = po_.PoTrapPreconditioner(po, -m.lam.max(), PARS["nu"])
    with pytest.raises(BkHipError, match=r"rho\^K.*sine mode \(1, 1\).*move a"):
        P.set_period((2 * M / PARS["nu"]) * math.tan(math.pi / (M - 1)))
    with pytest.raises(BkHipError, match="no period set"):
        P.ldiv(po.vec(np.zeros(po.n)))
    P.set_period(2 * math.pi)                                 # away from the critical period the same (a, b) is fine


# ------------------------------------------------------------------------------------------ the solve
def _hopf_record(ctx, dims):
    """The Hopf point of the trivial state in closed form (r* = -lam_11, omega = nu, zeta = zeta* = the first sine mode) through
    hopf_normal_form_native -- what get_normal_form ends with, without the continuation run and bisection that lead there."""
    codim2, hip, _ = _mods()
    m = _model(dims)
    rstar = -m.lam.max()
    prob = hip.CGL2d(ctx, dims, LS, **dict(PARS, r=rstar))
    zr, zi = _hopf_mode(dims)
    Z = _pair(prob, zr, zi)
    X = codim2.HopfVec(prob.vec(np.zeros(prob.nlocal)), [rstar, PARS["nu"]])
    hp = codim2.hopf_normal_form_native(prob, X, Z, Z, _solver(hip, prob, rstar))
    assert hp.converged and hp.type == "SubCritical"
    return prob, hp, rstar


def _guess(ctx, dims, M, dr):
    codim2, hip, po_ = _mods()
    prob, hp, rstar = _hopf_record(ctx, dims)
    pred = codim2.predictor(hp, dr)
    assert pred["dsfactor"] == -1 and abs(pred["p"] - (rstar - dr)) <= 1e-14
    g = po_.po_guess_from_hopf(pred, M, prob)
    pars = dict(PARS, r=g["p"])
    po = po_.PeriodicOrbitTrap(prob, M, g["phi"], g["xpi"])
    return prob, po, g, pars, pred


@pytest.mark.parametrize("rtol", [1e-3, 1e-9])
def test_potrap_solve_matches_preconditioned_scipy_gmres(ctx, rtol):
    """The first Newton system of the 16 x 12, M = 12 orbit (guess of the Hopf predictor, right-hand side = the functional there),
    IterativeSolvers flavor, against the restatement's preconditioned SciPy GMRES with the same rule |r| <= rtol |r0|:
      * the true preconditioned residual, through the restatement's Jacobian and modal solve, meets the rule (1e-6 relative slack
        for the difference between the Arnoldi estimate and the residual itself);
      * the error against the exact solution (sparse LU of the assembled Jacobian) is within 10 x SciPy's own;
      * the iteration count is SciPy's within 4, the longest block the block Arnoldi may speculate past convergence (an
        operator with a tail takes single steps, so the counts are expected equal)."""
    _, hip, po_ = _mods()
    dims, M, dr = (16, 12), 12, 0.1
    m = _model(dims)
    prob, po, g, pars, _ = _guess(ctx, dims, M, dr)
    U0, T0 = g["orbit"].numpy().reshape(M, -1), g["T"]
    phi = g["phi"].numpy().reshape(M, -1)
    a, b = pars["r"], pars["nu"]
    G = po.residual(g["orbit"], T0, _pv(pars))
    rhs = R.pack(G.u.numpy().reshape(M, -1), G.p)
    xc, itc = R.gmres_solve(m, U0, T0, pars, phi, rhs, a, b, T0, rtol)
    exact = spla.splu(R.jacobian_sparse(m, U0, T0, pars, phi)).solve(rhs)
    P = po_.PoTrapPreconditioner(po, a, b).set_period(T0)
    ls = hip.GMRESIterativeSolvers(reltol=rtol, restart=60, maxiter=200)
    x, cv, it = po_.po_solve(po.jacobian(g["orbit"], T0, _pv(pars)), P, G, ls)
    xg = R.pack(x.u.numpy().reshape(M, -1), x.p)
    prec = lambda v: np.concatenate([R.modal_solve(m, M, T0, a, b, v[:-1].reshape(M, -1)).reshape(-1), v[-1:]])
    o, t = R.jvp(m, U0, T0, pars, *R.unpack(m, xg), phi)
    pb = prec(rhs)
    true = np.linalg.norm(pb - prec(R.pack(o, t)))
    print(f"potrap solve rtol {rtol:g}: iterations GPU {it}, SciPy {itc}; |x - exact| GPU {np.abs(xg - exact).max():.3e}, "
          f"SciPy {np.abs(xc - exact).max():.3e}; true residual {true / np.linalg.norm(pb):.3e}")
    assert cv
    probe(f"potrap.solve_true_residual.{rtol:g}", true, rtol * np.linalg.norm(pb) * (1 + 1e-6) + 1e-13 * np.linalg.norm(pb))
    probe(f"potrap.solve_error.{rtol:g}", float(np.abs(xg - exact).max()), 10 * float(np.abs(xc - exact).max()))
    probe(f"potrap.solve_count.{rtol:g}", abs(it - itc), 4, gpu=it, scipy=itc)


# ------------------------------------------------------------------------------------------ Newton and continuation
# the restatement's LU-versus-GMRES difference of the converged orbit and T at 41 x 21, M = 30, dr = 0.01, measured once on the CPU
# by scripts/potrap_yardstick_41x21.py (sparse LU of the 51 661-unknown Jacobian takes minutes there, so no test of the suite
# reproduces the figures; the script does): 2.44e-15 in the orbit, 8.9e-16 in T, the values DESIGN 9k records
YARD_41x21 = (2.44e-15, 8.9e-16)


@pytest.mark.parametrize("dims,M,dr", [((16, 12), 12, 0.1), ((41, 21), 30, 0.01)])
def test_newton_po_trap_from_the_hopf_predictor(ctx, dims, M, dr):
    """hopf normal form -> predictor -> po_guess_from_hopf -> newton_po_trap (GMRES rtol 1e-9, a = r, b = nu) converges to 1e-10
    in the sup norm, to the orbit and not to the trivial state (amplitude above half the predictor's).  Orbit and T against the
    restatement's Newton from the same guess: with sparse LU at 16 x 12 -- the yardstick is the restatement's own LU-versus-GMRES
    difference, floored at 8 eps of the magnitude (two results cannot be asked to agree below the rounding of the last update),
    margin 10 x -- and at 41 x 21, where LU takes minutes, with the restatement's GMRES and the yardstick measured once.
    (M = 12 starts from dr = 0.1: from dr = 0.01 the reference's guess, M slices on the whole circle, sends Newton to the trivial
    state in the restatement too -- test_potrap_reference.py::test_newton_from_the_m12_guess_at_dr_001_lands_on_the_trivial_state.)"""
    _, hip, po_ = _mods()
    m = _model(dims)
    prob, po, g, pars, pred = _guess(ctx, dims, M, dr)
    U0, T0 = g["orbit"].numpy().reshape(M, -1), g["T"]
    phi, xpi = g["phi"].numpy().reshape(M, -1), g["xpi"].numpy().reshape(M, -1)
    ref_phi, _ = R.section_from_guess(m, U0, pars)
    assert np.abs(phi - ref_phi).max() <= 64 * EPS * np.abs(ref_phi).max()
    pars_of = lambda p: dict(pars, r=p)
    gm = R.newton(m, U0, T0, pars["r"], pars_of, phi, xpi, R.gmres_solver(m, pars_of, pars["r"], pars["nu"], T0, 1e-9), 1e-10, 10)
    if m.n <= 200:
        lu = R.newton(m, U0, T0, pars["r"], pars_of, phi, xpi, R.lu_solver(m, pars_of), 1e-10, 10)
        yard = (float(np.abs(lu["U"] - gm["U"]).max()), abs(lu["T"] - gm["T"]))
        ref = lu
    else:
        yard, ref = YARD_41x21, gm
    assert ref["converged"]
    ls = hip.GMRESIterativeSolvers(reltol=1e-9, restart=60, maxiter=200)
    s = po_.newton_po_trap(po, g["orbit"], T0, _pv(pars), ls, tol=1e-10, max_iterations=10, norm_inf=True)
    U = s["u"].numpy().reshape(M, -1)
    print(f"newton_po_trap {dims} M={M}: residuals {s['residuals']}, gmres {s['itlinear']} (restatement {gm['itlinear']}), "
          f"T {s['T']:.15g} (ref {ref['T']:.15g}), |dU| {np.abs(U - ref['U']).max():.3e}, yardstick {yard}")
    assert s["converged"] and s["residuals"][-1] < 1e-10, s["residuals"]
    assert np.abs(U).max() > 0.5 * np.abs(U0).max()
    assert len(s["itlinear"]) == s["itnewton"]
    probe(f"potrap.newton_orbit.{dims}.{M}", float(np.abs(U - ref["U"]).max()), 10 * max(yard[0], 8 * EPS * np.abs(ref["U"]).max()))
    probe(f"potrap.newton_T.{dims}.{M}", abs(s["T"] - ref["T"]), 10 * max(yard[1], 8 * EPS * ref["T"]))
    times, sl = po_.get_periodic_orbit(po, s["u"], s["T"])
    assert sl.shape == (M, m.N) and np.array_equal(sl, U) and abs(times[-1] - s["T"]) <= 4 * EPS * s["T"] and len(times) == M


def test_continuation_po_trap_three_steps_match_the_restatement(ctx):
    """Three PALC steps at 16 x 12, M = 12 from the converged orbit at r_hopf - 0.1 towards smaller r: p, T and amplitude per step
    against the restatement's three steps with sparse LU; the yardstick is the restatement's own LU-versus-GMRES difference per
    quantity, floored at 8 eps of the magnitude, margin 10 x."""
    _, hip, po_ = _mods()
    from bk_amd import continuation as Cn
    dims, M, dr = (16, 12), 12, 0.1
    m = _model(dims)
    prob, po, g, pars, _ = _guess(ctx, dims, M, dr)
    U0, T0 = g["orbit"].numpy().reshape(M, -1), g["T"]
    phi, xpi = g["phi"].numpy().reshape(M, -1), g["xpi"].numpy().reshape(M, -1)
    cpd = dict(ds=-0.01, dsmin=1e-4, dsmax=0.03, a=0.5, eta=150.0, tol=1e-10, max_iterations=10)
    pars_of = lambda p: dict(pars, r=p)
    lu = R.palc(m, U0, T0, pars, "r", phi, xpi, R.lu_solver(m, pars_of), cpd, 3)
    box = [T0]
    gm = R.palc(m, U0, T0, pars, "r", phi, xpi, R.gmres_solver(m, pars_of, pars["r"], pars["nu"], lambda: box[0], 1e-9), cpd, 3, Tp_box=box)
    cp = Cn.ContinuationPar(ds=cpd["ds"], dsmin=cpd["dsmin"], dsmax=cpd["dsmax"], a=cpd["a"], eta=cpd["eta"], p_min=-10.0, p_max=10.0,
                            max_steps=3, detect_bifurcation=0, newton_options=Cn.NewtonPar(tol=1e-10, max_iterations=10))
    ls = hip.GMRESIterativeSolvers(reltol=1e-9, restart=60, maxiter=200)
    br = po_.continuation_po_trap(po, g["orbit"], T0, _pv(pars), "r", cp, ls)
    print(f"continuation_po_trap: p {br['p']}, T {br['T']}, amplitude {br['amplitude']}, newton {br['itnewton']}, gmres {br['itlinear']}")
    assert len(br["p"]) == 4 and all(br["converged"]) and br["itnewton"][1:] == lu["itnewton"][1:]
    for key in ("p", "T", "amplitude"):
        for k in range(4):
            yard = max(abs(lu[key][k] - gm[key][k]), 8 * EPS * abs(lu[key][k]))
            probe(f"potrap.palc_{key}.{k}", abs(br[key][k] - lu[key][k]), 10 * yard)
    assert br["p"][3] < br["p"][0] and br["amplitude"][3] > br["amplitude"][0]


# ------------------------------------------------------------------------------------------ refusals
def test_potrap_refusals(ctx):
    _, hip, po_ = _mods()
    from bk_amd._lib import BkHipError
    from bk_amd.hip import _ptr
    from bk_amd.periodic_orbit import _parr
    sh = hip.SwiftHohenberg(ctx, (16, 16), (np.pi, np.pi))
    with pytest.raises(BkHipError, match="BK_PDE_CGL2D only"):
        po_.PeriodicOrbitTrap(sh, 5)
    prob = hip.CGL2d(ctx, (12, 9), LS, **PARS)
    with pytest.raises(BkHipError, match="M >= 3"):
        po_.PeriodicOrbitTrap(prob, 2)
    po = po_.PeriodicOrbitTrap(prob, 5)
    U = po.vec(np.ones(po.n))
    pv = _pv(PARS)
    with pytest.raises(BkHipError, match="no section set"):
        po.residual(U, 6.0, pv)
    with pytest.raises(BkHipError, match="no section set"):
        po.jacobian(U, 6.0, pv)
    po.set_section(po.vec(np.ones(po.n)))
    tail = C.c_double()
    for call in (lambda: ctx.lib.bk_potrap_residual(po.h, _ptr(U.t), 6.0, _parr(pv), 6, _ptr(U.t), C.byref(tail)),
                 lambda: ctx.lib.bk_potrap_jvp(po.h, _ptr(U.t), 6.0, _parr(pv), 6, _ptr(U.t), 0.0, _ptr(U.t), C.byref(tail))):
        with pytest.raises(BkHipError, match="must not alias"):
            ctx.check(call(), "alias")
    with pytest.raises(BkHipError, match="params = "):
        po.residual(U, 6.0, pv[:5])
    # a preconditioner of another kind, and one of another orbit length
    J = po.jacobian(U, 6.0, pv)
    rhs = hip.BorderedArray(po.vec(np.ones(po.n)), 1.0)
    ls = hip.GMRESIterativeSolvers(reltol=1e-6, restart=30, maxiter=60)
    with pytest.raises(BkHipError, match="not a preconditioner of bk_precond_potrap_create"):
        po_.po_solve(J, hip.CGLBlockPreconditioner(prob, 0.5, 1.0), rhs, ls)
    other = po_.PoTrapPreconditioner(po_.PeriodicOrbitTrap(prob, 7), 0.5, 1.0).set_period(6.0)
    with pytest.raises(BkHipError, match="for this orbit"):
        po_.po_solve(J, other, rhs, ls)
    blk = hip.CGLBlockPreconditioner(prob, 0.5, 1.0)          # named: the handle must outlive the call
    with pytest.raises(BkHipError, match="not a preconditioner of bk_precond_potrap_create"):
        ctx.check(ctx.lib.bk_precond_potrap_set_period(blk.h, 6.0), "set_period")
