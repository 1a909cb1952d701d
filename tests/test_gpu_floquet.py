"""GPU tests of the Floquet multipliers of the trapezoid orbits of cGL (csrc/floquet.hip, bk_amd.periodic_orbit): the marching
kernel of the initial-value operator against the long-double restatement (tests/floquet_ref.py, pinned by
test_floquet_reference.py), its preconditioner against sparse LU, one application of the monodromy against the dense monodromy, SciPy
GMRES on the same system and the sequential mirror, the leading multipliers against dense eigenvalues, and the stability record of
continuation_po_trap across the fold of limit cycles.

Shapes: (12, 9) M = 7; (23, 17) M = 9 -- two tiles, the second partial, odd extents, the second field 8-byte misaligned --;
(16, 12) M = 12; (12, 9) M = 3 -- K = 2, the smallest case with a predecessor row and the smallest M bk_potrap_create accepts."""
import functools
import math
import warnings

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import floquet_ref as Fq
import potrap_ref as R
from conftest import probe
from test_gpu_hopf import LS, PARS
from test_gpu_potrap import GUARD, _guarded, _guess, _model, _mods, _pv

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
LD = np.longdouble
CASES = [((12, 9), 7), ((23, 17), 9), ((16, 12), 12), ((12, 9), 3)]
RTOL = 1e-9
TOL_EIG = 1e-8


@functools.lru_cache(maxsize=None)
def _inputs(dims, M):
    m = _model(dims)
    rng = np.random.default_rng(2000 * dims[0] + M)
    d = dict(U=0.6 * rng.standard_normal((M, m.N)), Y=rng.standard_normal((M - 1, m.N)), T=5.0 + rng.random())
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _march(ctx, po, U, T, pv, Y):
    """bk_potrap_ivp_march into a NaN-guarded buffer -> out (K, N); the guard bands stay NaN."""
    from bk_amd.hip import _ptr
    from bk_amd.periodic_orbit import _parr
    n = po.N * (po.M - 1)
    full, out = _guarded(ctx, n)
    ctx.check(ctx.lib.bk_potrap_ivp_march(po.h, _ptr(U.t), float(T), _parr(pv), len(pv), _ptr(Y.t), _ptr(out)), "ivp_march")
    ctx.sync()
    a = full.cpu().numpy()
    assert np.isnan(a[:GUARD]).all() and np.isnan(a[GUARD + n:]).all()
    return a[GUARD:GUARD + n].reshape(po.M - 1, -1).copy()


# ------------------------------------------------------------------------------------------ 1. the marching operator
@pytest.mark.parametrize("dims,M", CASES)
def test_ivp_march_matches_extended_precision(ctx, dims, M):
    """Random orbit slices and y, gamma != 0, against the long-double restatement in units of eps * (sum of the moduli of the
    terms): 16 units, the bound of test_gpu_potrap.py for the cyclic kernel (a monomial passes through ~11 roundings of eps / 2).
    The NaN guard bands around out stay NaN (_march)."""
    _, hip, po_ = _mods()
    m, d = _model(dims), _inputs(dims, M)
    pars = dict(PARS, r=0.3, gamma=0.2)
    prob = hip.CGL2d(ctx, dims, LS, **pars)
    po = po_.PeriodicOrbitTrap(prob, M)
    got = _march(ctx, po, po.vec(d["U"]), d["T"], _pv(pars), po.vec(d["Y"]))
    ref = Fq.ivp_apply(m, d["U"].astype(LD), d["T"], pars, d["Y"].astype(LD))
    unit = Fq.ivp_apply(m, d["U"], d["T"], pars, d["Y"], mod=True)
    ulps = float((np.abs(got - ref) / (EPS * unit)).max())
    print(f"ivp march {dims} M={M}: {ulps:.3f} units")
    probe(f"floquet.march_ulps.{dims}.{M}", ulps, 16.0, tight=4.0)


def test_ivp_march_rows_have_the_same_bits_for_every_chunking_and_aliasing_is_refused(ctx):
    """16 x 12, M = 12 (K = 11): potrap_chunks = 1 (one chunk from exact zeros), 2 (C = 6 / 5), 4 (C = 3 / 2), 11 (one row per
    chunk, every row's predecessor re-evaluated) and the default give bitwise equal outputs."""
    _, hip, po_ = _mods()
    from bk_amd._lib import BkHipError
    from bk_amd.hip import _ptr
    from bk_amd.periodic_orbit import _parr
    dims, M = (16, 12), 12
    d = _inputs(dims, M)
    pars = dict(PARS, r=0.3, gamma=0.2)
    prob = hip.CGL2d(ctx, dims, LS, **pars)
    po = po_.PeriodicOrbitTrap(prob, M)
    U, Y = po.vec(d["U"]), po.vec(d["Y"])
    res = {}
    try:
        for k in (1.0, 2.0, 4.0, 11.0, 0.0):
            ctx.set_option("potrap_chunks", k)
            res[k] = _march(ctx, po, U, d["T"], _pv(pars), Y)
    finally:
        ctx.set_option("potrap_chunks", 0.0)
    for k in res:
        assert np.array_equal(res[k], res[1.0]), k
    pv = _pv(pars)
    with pytest.raises(BkHipError, match="must not alias"):
        ctx.check(ctx.lib.bk_potrap_ivp_march(po.h, _ptr(U.t), d["T"], _parr(pv), 6, _ptr(Y.t), _ptr(Y.t)), "alias")
    sh = hip.SwiftHohenberg(ctx, (16, 16), (np.pi, np.pi))
    with pytest.raises(BkHipError, match="BK_PDE_CGL2D only"):
        po_.PeriodicOrbitTrap(sh, 5)


# ------------------------------------------------------------------------------------------ 2. the preconditioner
@functools.lru_cache(maxsize=None)
def _precond_reference(dims, M):
    m = _model(dims)
    a, b, T = -m.lam.max() - 0.05, PARS["nu"], 2 * math.pi
    f = np.random.default_rng(3 + M).standard_normal((M - 1, m.N))
    lu = spla.splu(Fq.A0_ivp_sparse(m, M, T, a, b)).solve(f.reshape(-1)).reshape(M - 1, -1)
    md = Fq.modal_solve_ivp(m, M, T, a, b, f)
    return a, b, T, f, lu, max(float(np.abs(md - lu).max()), 8 * EPS * float(np.abs(lu).max()))


@pytest.mark.parametrize("dims,M", CASES)
def test_ivp_preconditioner_matches_sparse_lu_of_A0(ctx, dims, M):
    """bk_precond_apply of the initial-value preconditioner (batched DST-I of 2 K fields, time solve, DST-I) against sparse LU of
    the assembled A0, a = r_hopf - 0.05, b = nu, T = 2 pi.  Yardstick: the restatement's own modal-versus-LU difference at the same
    case (test_floquet_reference prints it; DESIGN 9l lists it), floored at 8 eps of the solution's magnitude; the GPU gets 10 x."""
    _, hip, po_ = _mods()
    a, b, T, f, lu, yard = _precond_reference(dims, M)
    prob = hip.CGL2d(ctx, dims, LS, **PARS)
    po = po_.PeriodicOrbitTrap(prob, M)
    P = po_.PoTrapIvpPreconditioner(po, a, b, T)
    got = P.ldiv(po.vec(f)).numpy().reshape(M - 1, -1)
    err = float(np.abs(got - lu).max())
    print(f"ivp preconditioner {dims} M={M}: GPU vs LU {err:.3e}, yardstick {yard:.3e}")
    probe(f"floquet.precond_vs_lu.{dims}.{M}", err, 10 * yard)


def test_ivp_preconditioner_transform_paths_and_guard(ctx):
    """41 x 21, M = 3: as for the orbit preconditioner the 41 points along x run the transform pass as the matrix-core
    product, the 21 along y one thread per output, and option dct_gemm = 0 forces the latter on both; the dispatch records which
    ran.  Both within the yardstick, and their bits are equal (both accumulate along the transformed index in the same order).
    Guard: alpha = 1 - hh (a + lam + i b) can vanish only for b = 0; a = 1 / hh - lam_11 puts the (1, 1) mode below 1e-8."""
    _, hip, po_ = _mods()
    from bk_amd._lib import BkHipError
    dims, M = (41, 21), 3
    a, b, T, f, lu, yard = _precond_reference(dims, M)
    prob = hip.CGL2d(ctx, dims, LS, **PARS)
    po = po_.PeriodicOrbitTrap(prob, M)
    P = po_.PoTrapIvpPreconditioner(po, a, b, T)
    assert P.transform_paths() == (-1, -1)
    out = {}
    try:
        for g in (1.0, 0.0):
            ctx.set_option("dct_gemm", g)
            out[g] = P.ldiv(po.vec(f)).numpy().reshape(M - 1, -1)
            probe(f"floquet.precond_vs_lu.gemm{int(g)}", float(np.abs(out[g] - lu).max()), 10 * yard)
            assert P.transform_paths() == ((1, 0) if g else (0, 0))
    finally:
        ctx.set_option("dct_gemm", 1.0)
    assert np.array_equal(out[1.0], out[0.0])
    m = _model((16, 12))
    po2 = po_.PeriodicOrbitTrap(hip.CGL2d(ctx, (16, 12), LS, **PARS), 12)
    hh = R._hh(T, 12, float)
    with pytest.raises(BkHipError, match=r"alpha.*below 1e-08 at sine mode \(1, 1\).*move a"):
        po_.PoTrapIvpPreconditioner(po2, 1 / hh - m.lam.max(), 0.0, T)
    po_.PoTrapIvpPreconditioner(po2, 1 / hh - m.lam.max(), PARS["nu"], T)          # b != 0: |alpha| >= hh b


# ------------------------------------------------------------------------------------------ orbits shared by 3. and 4.
_ORBITS = {}


def _orbit(ctx, dims, M, dr):
    """The orbit of newton_po_trap (guess helper of test_gpu_potrap.py), downloaded, and the restatement's dense monodromy of it."""
    key = (dims, M, dr)
    if key not in _ORBITS:
        _, hip, po_ = _mods()
        prob, po, g, pars, _ = _guess(ctx, dims, M, dr)
        ls = hip.GMRESIterativeSolvers(reltol=RTOL, restart=60, maxiter=200)
        s = po_.newton_po_trap(po, g["orbit"], g["T"], _pv(pars), ls, tol=1e-10, max_iterations=10, norm_inf=True)
        assert s["converged"], s["residuals"]
        U = s["u"].numpy().reshape(M, -1)
        _ORBITS[key] = dict(prob=prob, po=po, pars=pars, u=s["u"], T=s["T"], U=U, ls=ls,
                            dense=Fq.dense_monodromy(_model(dims), U, s["T"], pars))
    return _ORBITS[key]


ORBIT_CASES = [((16, 12), 12, 0.1), ((16, 12), 30, 0.01)]


# ------------------------------------------------------------------------------------------ 3. one application
@pytest.mark.parametrize("dims,M,dr", ORBIT_CASES)
def test_one_monodromy_application(ctx, dims, M, dr):
    """x a random unit vector, rtol 1e-9, IterativeSolvers flavor, preconditioner a = r, b = nu.
      * iterations within 4 of SciPy GMRES on the same system (the rule of test_gpu_potrap.py; CPU: 9 and 5);
      * the last slice within 10 x the restatement's own error against the dense monodromy, taken from the restatement here;
      * the K slices of solve() satisfy the initial-value rows to the solve tolerance: the true preconditioned residual, through the
        restatement's operator and modal solve, meets |r| <= rtol |r0| (1e-6 relative slack for the Arnoldi estimate);
      * native and monodromy_sequential agree within the sum of their bounds, the sequential one's being 10 x the error of the
        restatement's sequential form with SciPy GMRES at the same rtol;
      * stats() counts one solve, no failure, and the solve's iterations."""
    _, hip, po_ = _mods()
    o = _orbit(ctx, dims, M, dr)
    m, po, pars, U, T = _model(dims), o["po"], o["pars"], o["U"], o["T"]
    pv, K = _pv(pars), M - 1
    x = np.random.default_rng(5).standard_normal(m.N)
    x /= np.linalg.norm(x)
    exact = o["dense"] @ x
    Yr, it_ref = Fq.spacetime_solve(m, U, T, pars, x, pars["r"], pars["nu"], RTOL)
    yard = float(np.abs(Yr[-1] - exact).max())
    mono = po_.PoTrapMonodromy(po, o["u"], T, pv, o["ls"])
    xv = po.prob.vec(x)
    y_all, cv, it = mono.solve(xv)
    st = mono.stats()
    assert cv and st["solves"] == 1 and st["failed"] == 0 and st["inner_its"] == it and st["paths"] == (0, 0)
    Y = y_all.numpy().reshape(K, -1)
    err = float(np.abs(Y[-1] - exact).max())
    P = lambda v: Fq.modal_solve_ivp(m, M, T, pars["r"], pars["nu"], v)
    pf = P(Fq.ivp_rhs(m, U, T, pars, x))
    true = float(np.linalg.norm(pf - P(Fq.ivp_apply(m, U, T, pars, Y))))
    (ys, its_ref_seq) = Fq.monodromy_sequential(m, U, T, pars, x, rtol=RTOL)
    yard_seq = float(np.abs(ys[-1] - exact).max())
    seq, its_seq, ok = po_.monodromy_sequential(po, o["u"], T, pv, xv, o["ls"])
    sq = seq.numpy()
    print(f"monodromy {dims} M={M}: iterations GPU {it}, SciPy {it_ref}; |y - dense| GPU {err:.3e}, restatement {yard:.3e}; true "
          f"residual {true / np.linalg.norm(pf):.3e}; sequential: iterations GPU {its_seq}, SciPy {its_ref_seq}, |seq - dense| GPU "
          f"{np.abs(sq - exact).max():.3e}, restatement {yard_seq:.3e}; |native - seq| {np.abs(sq - Y[-1]).max():.3e}")
    probe(f"floquet.apply_count.{M}", abs(it - it_ref), 4, gpu=it, scipy=it_ref)
    probe(f"floquet.apply_error.{M}", err, 10 * yard)
    probe(f"floquet.apply_true_residual.{M}", true, RTOL * np.linalg.norm(pf) * (1 + 1e-6) + 1e-13 * np.linalg.norm(pf))
    assert ok
    probe(f"floquet.native_vs_sequential.{M}", float(np.abs(sq - Y[-1]).max()), 10 * yard + 10 * yard_seq)
    # the operator handle: a0 x + a1 y_{K-1} of one more solve of the same system
    got = mono(xv, 2.0, 3.0).numpy()
    assert np.abs(got - (2.0 * x + 3.0 * Y[-1])).max() <= 16 * EPS * (2 + 3 * np.abs(Y[-1]).max())
    assert mono.stats()["solves"] == 2


# ------------------------------------------------------------------------------------------ 4. multipliers
@pytest.mark.parametrize("dims,M,dr,nev,expect", [((16, 12), 12, 0.1, 2, (2.7594, 1.0)),
                                                  ((16, 12), 30, 0.01, 4, (1.1315, 1.0, 0.01754, 0.01652))])
def test_floquet_multipliers_match_dense_eigenvalues(ctx, dims, M, dr, nev, expect):
    """floquet_multipliers against the dense eigenvalues of the restatement's monodromy of the same (downloaded) orbit.  Per simple
    eigenvalue the bound is 10 kappa (delta + tol_eig): kappa = 1 / |y^H x| from the dense left and right eigenvectors, delta =
    |M_gmres - M_dense|_2 of the restatement's column-by-column space-time GMRES at the same rtol (floquet_ref.DELTA, pinned by
    test_floquet_reference), tol_eig = 1e-8 the Krylov-Schur tolerance.  nev = 2 at M = 12: behind 2.7594 and 1 sits a cluster at
    modulus 0.406.  The trivial multiplier is within its bound of 1, exponents come sorted by decreasing real part, and the
    eigenfunction's last slice is mu zeta within the same bound."""
    _, hip, po_ = _mods()
    o = _orbit(ctx, dims, M, dr)
    m, po, pars, T = _model(dims), o["po"], o["pars"], o["T"]
    w, _, kap = Fq.leading_multipliers(o["dense"], nev)
    assert np.abs(w.imag).max() == 0 and np.allclose(w.real, expect, rtol=2e-4)
    delta = Fq.DELTA[(dims, M, dr)]
    bound = 10 * kap * (delta + TOL_EIG)
    eig = hip.EigKrylovKit(tol=TOL_EIG, maxiter=20, krylovdim=20)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                   # no NaN / infinite multiplier
        fl = po_.floquet_multipliers(po, o["u"], T, _pv(pars), nev, o["ls"], eig=eig)
    mu, sig = fl["multipliers"], fl["exponents"]
    print(f"floquet {dims} M={M}: multipliers {mu}, dense {w}, |diff| {np.abs(mu[:nev] - w)}, bounds {bound}, kappa {kap}, delta "
          f"{delta:.3e}; exponents {sig}; applications {fl['numops']}, GMRES iterations {fl['inner_its']}")
    assert fl["converged"] and len(mu) == nev and fl["numops"] >= nev and fl["inner_its"] > 0
    for k in range(nev):
        probe(f"floquet.multiplier.{M}.{k}", abs(mu[k] - w[k]), bound[k], gpu=[mu[k].real, mu[k].imag], dense=float(w[k].real))
    probe(f"floquet.trivial_multiplier.{M}", abs(mu[1] - 1.0), bound[1])
    assert np.all(np.diff(sig.real) <= 0) and np.allclose(np.exp(sig), mu, rtol=1e-14)
    mono = fl["monodromy"]
    for k in range(nev):
        zr, zi = fl["vectors"][k]
        nz = zr.norm()                                                   # the real part of an eigenvector of a real multiplier is one
        Y = po_.floquet_eigenfunction(mono, zr).numpy().reshape(M - 1, -1)
        probe(f"floquet.eigenfunction.{M}.{k}", float(np.abs(Y[-1] - mu[k].real * zr.numpy()).max()), bound[k] * nz)
        # ... and its slices solve the homogeneous rows: slice i of the reference's list is the sequential form's step i
        if k == 0:
            ys = Fq.monodromy_sequential(m, o["U"], T, pars, zr.numpy())
            assert np.abs(Y - ys).max() <= 10 * Fq.DELTA[(dims, M, dr)] * max(1.0, np.abs(ys).max())


# ------------------------------------------------------------------------------------------ 5. stability along the branch
def test_continuation_defaults_leave_the_records_unchanged(ctx):
    """Three steps of the M = 12 case of test_gpu_potrap.py: the new keywords at their defaults give the records of a call without
    them, value for value, and no stability record."""
    _, hip, po_ = _mods()
    from bk_amd import continuation as Cn
    dims, M, dr = (16, 12), 12, 0.1
    prob, po, g, pars, _ = _guess(ctx, dims, M, dr)
    cp = Cn.ContinuationPar(ds=-0.01, dsmin=1e-4, dsmax=0.03, a=0.5, eta=150.0, p_min=-10.0, p_max=10.0, max_steps=3,
                            detect_bifurcation=0, newton_options=Cn.NewtonPar(tol=1e-10, max_iterations=10))
    ls = hip.GMRESIterativeSolvers(reltol=RTOL, restart=60, maxiter=200)
    runs = []
    for kw in ({}, dict(nev=0, detect_bifurcation=0, tol_stability=1e-10, eig=None)):
        po.set_section(g["phi"], g["xpi"])
        runs.append(po_.continuation_po_trap(po, g["orbit"], g["T"], _pv(pars), "r", cp, ls, **kw))
    a, b = runs
    assert set(a) == set(b) == {"p", "T", "amplitude", "itnewton", "itlinear", "ds", "converged", "orbit"}
    for key in a:
        if key != "orbit":
            assert a[key] == b[key], key
    assert np.array_equal(a["orbit"].u.numpy(), b["orbit"].u.numpy()) and a["orbit"].p == b["orbit"].p


# the fold run: 16 x 12, M = 12 from dr = 0.15, ds = -0.02, dsmax = 0.04 -- chosen on the CPU: the restatement's branch (sparse LU)
# has p - r_hopf = -0.150, -0.168, -0.189, -0.200 with dense multipliers (3.41, 1), (3.22, 1), (2.39, 1), (1, 0.887): the fold of
# limit cycles is crossed between points 2 and 3, the third accepted step.  tol_stability = 1e-5: the trivial exponent measures
# 3e-10 at most on the restatement's points and is bounded by ~1.3e-7 (10 kappa (delta + tol_eig)) on the GPU; the nearest other
# exponent is -0.119.
FOLD = dict(dims=(16, 12), M=12, dr=0.15, steps=3, tol_stability=1e-5,
            cp=dict(ds=-0.02, dsmin=1e-4, dsmax=0.04, a=0.5, eta=150.0, tol=1e-10, max_iterations=10))


def test_stability_along_the_branch_across_the_fold_of_limit_cycles(ctx):
    """continuation_po_trap with nev = 2, detect_bifurcation = 2 over the run above: n_unstable at every recorded point equals the
    restatement's count from the dense multipliers at the restatement's own branch points (1, 1, 1, 0; the exponents of both are
    printed side by side), and exactly one special point is recorded: type bp,
    delta = (-1, 0), in the step interval where the restatement's count changes.  (The closed-form fold of the one-mode reduction
    is near r_hopf - 0.25; this grid's is at r_hopf - 0.200.)"""
    _, hip, po_ = _mods()
    from bk_amd import continuation as Cn
    dims, M, dr, steps, tol, cpd = (FOLD[k] for k in ("dims", "M", "dr", "steps", "tol_stability", "cp"))
    m = _model(dims)
    prob, po, g, pars, _ = _guess(ctx, dims, M, dr)
    U0, T0 = g["orbit"].numpy().reshape(M, -1), g["T"]
    phi, xpi = g["phi"].numpy().reshape(M, -1), g["xpi"].numpy().reshape(M, -1)
    pars_of = lambda p: dict(pars, r=p)
    ref = Fq.branch_stability(m, U0, T0, pars, "r", phi, xpi, R.lu_solver(m, pars_of), cpd, steps, 2, tol)
    assert ref["n_unstable"] == [1, 1, 1, 0] and ref["n_imag"] == [0, 0, 0, 0]
    triv = max(float(np.abs(s).min()) for s in ref["exponents"])
    assert triv < 1e-8 < tol
    cp = Cn.ContinuationPar(ds=cpd["ds"], dsmin=cpd["dsmin"], dsmax=cpd["dsmax"], a=cpd["a"], eta=cpd["eta"], p_min=-10.0, p_max=10.0,
                            max_steps=steps, detect_bifurcation=0, newton_options=Cn.NewtonPar(tol=1e-10, max_iterations=10))
    ls = hip.GMRESIterativeSolvers(reltol=RTOL, restart=60, maxiter=200)
    eig = hip.EigKrylovKit(tol=TOL_EIG, maxiter=20, krylovdim=20)
    br = po_.continuation_po_trap(po, g["orbit"], T0, _pv(pars), "r", cp, ls, nev=2, detect_bifurcation=2, tol_stability=tol, eig=eig)
    print(f"fold run: p {br['p']} (restatement {ref['p']}), n_unstable {br['n_unstable']}, exponents {br['floquet']} (dense "
          f"{ref['exponents']}), special points {br['specialpoints']}, trivial exponent of the restatement <= {triv:.2e}")
    assert len(br["p"]) == steps + 1 and all(br["converged"]) and all(br["eig_converged"])
    assert np.allclose(br["p"], ref["p"], rtol=0, atol=1e-7)
    assert br["n_unstable"] == ref["n_unstable"] and br["n_imag"] == ref["n_imag"]
    assert br["stable"] == [False, False, False, True]
    (sp,) = br["specialpoints"]
    kf = ref["n_unstable"].index(0)
    assert sp["type"] == "bp" and sp["delta"] == (-1, 0) and sp["step"] == kf and sp["ind_ev"] == 1
    assert sp["interval"] == (br["p"][kf - 1], br["p"][kf])
