"""GPU tests of the spectral ETDRK2 flow of cGL and the standard-shooting periodic orbits on it (csrc/flow.hip, csrc/shooting.hip,
bk_amd.shooting) against the restatement in extended precision (tests/shooting_ref.py, pinned by test_shooting_reference.py) and
its fixture tests/golden/shooting_cgl.json: the coefficient tables, evolve and the flow's tangent, the functional, its JVP and
section tail, the stored and the recomputed operator, the unpreconditioned solve against SciPy GMRES, Newton on the limit cycle at
r = 1.2 and on the small orbit next to the Hopf point, the Floquet multipliers, three PALC steps, and the refusals.

Shapes: (8, 6), (12, 9) -- no matrix-core transform pass --, (23, 17) -- an odd point count, the second field of every state is
8-byte misaligned --, (41, 21) -- the matrix-core pass along x --, (40, 33) -- on both axes; B, M in {1, 2, 3}; nsteps in {1, 2, 48}."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import potrap_ref as P
import shooting_ref as S
from conftest import probe

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
LD = np.longdouble
GUARD = 64                      # doubles of NaN on both sides of every output
PATHS = {(8, 6): (0, 0), (12, 9): (0, 0), (23, 17): (0, 0), (41, 21): (1, 0), (40, 33): (1, 1)}
# the largest error of the device tables against the long-double ones that was measured, in units of eps max(1, |z|) |value| (the
# device's eigenvalue table carries the rounding of the host's sine, which z = h lam multiplies): E 2.371, h phi1 1.314, h phi2 1.145
# at (12, 9) and (41, 21) over the steps below (profiles/shooting_tolerance_probe.jsonl); the bound in force is 4 x the largest, the margin
# for another expm1
TABLE_MEASURED = 2.371


def _mods():
    from bk_amd import hip, shooting
    return hip, shooting


def _pv(pars):
    return [pars[k] for k in S.PNAMES]


@functools.lru_cache(maxsize=None)
def _fl(dims, dtype=LD):
    return S.Flow(P.Model(dims, S.LS), dtype)


@functools.lru_cache(maxsize=None)
def _states(dims, B):
    """B different states near the limit cycle at r = 1.2 (0.1 rand after t = 20, 23, 26) and as many tangents."""
    fl = _fl(dims, float)
    x = [fl.march(S.cycle_start(fl.m), 20.0, 200, S.PARS)["u"]]
    for _ in range(1, B):
        x.append(fl.march(x[-1], 3.0, 30, S.PARS)["u"])
    X = np.stack(x)
    dX = np.random.default_rng(7 + dims[0]).standard_normal(X.shape)
    X.setflags(write=False)
    dX.setflags(write=False)
    return X, dX


def _guarded(ctx, n):
    t = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float64, device=ctx.torch_device)
    return t, t[GUARD:GUARD + n]


def _unguard(full, n):
    a = full.cpu().numpy()
    assert np.isnan(a[:GUARD]).all() and np.isnan(a[GUARD + n:]).all()
    assert not np.isnan(a[GUARD:GUARD + n]).any()
    return a[GUARD:GUARD + n].copy()


def _evolve(ctx, flow, X, tau, nsteps, pv, dX=None):
    """bk_flow_evolve / bk_flow_jvp into NaN-guarded buffers -> (out, dout or None), shaped as X."""
    from bk_amd.hip import HipVec, _ptr
    from bk_amd.periodic_orbit import _parr
    x = HipVec.from_numpy(ctx, X.reshape(-1))
    fo, o = _guarded(ctx, X.size)
    if dX is None:
        ctx.check(ctx.lib.bk_flow_evolve(flow.h, _ptr(x.t), float(tau), int(nsteps), _parr(pv), len(pv), _ptr(o)), "evolve")
        ctx.sync()
        return _unguard(fo, X.size).reshape(X.shape), None
    dx = HipVec.from_numpy(ctx, dX.reshape(-1))
    fd, d = _guarded(ctx, X.size)
    ctx.check(ctx.lib.bk_flow_jvp(flow.h, _ptr(x.t), _ptr(dx.t), float(tau), int(nsteps), _parr(pv), len(pv), _ptr(o), _ptr(d)), "jvp")
    ctx.sync()
    return _unguard(fo, X.size).reshape(X.shape), _unguard(fd, X.size).reshape(X.shape)


# ------------------------------------------------------------------------------------------ the tables
@pytest.mark.parametrize("dims", [(12, 9), (41, 21)])
def test_flow_tables_match_the_long_double_tables(ctx, dims):
    """bk_flow_coefficients for steps that put z = h lam across the series switch at |z| = 1 (h = 1e-9: every |z| tiny; 6.3 / 64:
    the steps of the tests; 0.5: most |z| > 1) against the long-double tables at the same z.  Unit: eps max(1, |z|) |value| -- the
    device's eigenvalues carry the last-place rounding of the host's sine, and e^z turns that into |z| eps.  No bound is given;
    the largest value measured is recorded above and 4 x it asserted.  A step that puts the stiffest mode at z = -800 gives E = 0
    and finite tables."""
    hip, sh_ = _mods()
    fl = _fl(dims)
    flow = sh_.Flow(hip.CGL2d(ctx, dims, S.LS, **S.PARS), 1)
    worst = 0.0
    for h in (1e-9, 6.3 / 64, 6.3 / 3 / 48, 0.5):
        got = flow.coefficients(h)
        z = np.abs(float(h) * fl.lam).reshape(-1)
        for name, g, r in zip(("E", "P1", "P2"), got, fl.tables(h)):
            r = r.reshape(-1)
            assert np.all(np.isfinite(g)), name
            err = float((np.abs(g.astype(LD) - r) / (EPS * np.maximum(1.0, z) * np.abs(r))).max())
            print(f"flow tables {dims} h={h:g} {name}: {err:.3f} units")
            worst = max(worst, err)
    probe(f"shooting.tables.{dims}", worst, 4 * TABLE_MEASURED, tight=TABLE_MEASURED)
    h800 = -800.0 / float(fl.lam.min())
    E, P1, P2 = flow.coefficients(h800)
    assert np.all(np.isfinite(E)) and np.all(np.isfinite(P1)) and np.all(np.isfinite(P2))
    k = int(np.argmin(fl.lam.reshape(-1)))
    assert E[k] == 0.0 and abs(P1[k] - h800 / 800.0) <= 4 * EPS * h800 / 800.0 and P2[k] > 0.0


# ------------------------------------------------------------------------------------------ evolve and the flow's tangent
@pytest.mark.parametrize("dims,B,nsteps", [((8, 6), 1, 1), ((12, 9), 3, 2), ((23, 17), 2, 48), ((41, 21), 3, 48), ((40, 33), 1, 2),
                                            ((12, 9), 2, 48), ((41, 21), 1, 1)])
def test_flow_evolve_and_jvp_match_the_restatement(ctx, dims, B, nsteps):
    """Phi(x, tau) and dPhi(x, tau) dx for B states against the long-double restatement within 4 nsteps (nx + ny) eps unit, unit =
    the restatement's largest |state| (|tangent|) over the steps: the worst-case accumulation of four length-nx / ny transforms per
    step.  The state of bk_flow_jvp has the bits of bk_flow_evolve.  The route of the transforms is asserted."""
    hip, sh_ = _mods()
    fl = _fl(dims)
    X, dX = _states(dims, B)
    pars = dict(S.PARS, gamma=0.05)
    tau = 0.1 * nsteps
    flow = sh_.Flow(hip.CGL2d(ctx, dims, S.LS, **pars), B)
    assert flow.transform_paths() == (-1, -1)
    ref = fl.march(X.astype(LD), tau, nsteps, pars, dX.astype(LD))
    out, _ = _evolve(ctx, flow, X, tau, nsteps, _pv(pars))
    assert flow.transform_paths() == PATHS[dims]
    out2, dout = _evolve(ctx, flow, X, tau, nsteps, _pv(pars), dX)
    assert np.array_equal(out, out2)
    bound = 4 * nsteps * (dims[0] + dims[1]) * EPS
    probe(f"shooting.evolve.{dims}.{B}.{nsteps}", float(np.abs(out - ref["u"]).max()), bound * ref["umax"], tight=64 * EPS * ref["umax"])
    probe(f"shooting.flow_jvp.{dims}.{B}.{nsteps}", float(np.abs(dout - ref["du"]).max()), bound * ref["dumax"], tight=64 * EPS * ref["dumax"])
    assert flow.stats()["base_marches"] == 2


@pytest.mark.parametrize("dims", [(12, 9), (41, 21)])
def test_flow_batch_of_three_has_the_bits_of_three_single_calls(ctx, dims):
    hip, sh_ = _mods()
    X, dX = _states(dims, 3)
    prob = hip.CGL2d(ctx, dims, S.LS, **S.PARS)
    f3, f1 = sh_.Flow(prob, 3), sh_.Flow(prob, 1)
    o3, d3 = _evolve(ctx, f3, X, 0.7, 5, _pv(S.PARS), dX)
    for b in range(3):
        o1, d1 = _evolve(ctx, f1, X[b:b + 1], 0.7, 5, _pv(S.PARS), dX[b:b + 1])
        assert np.array_equal(o1[0], o3[b]) and np.array_equal(d1[0], d3[b]), b
    try:
        ctx.set_option("dct_gemm", 0.0)                    # the direct transform kernel on every axis: the same bits
        o0, d0 = _evolve(ctx, f3, X, 0.7, 5, _pv(S.PARS), dX)
        assert f3.transform_paths() == (0, 0)
    finally:
        ctx.set_option("dct_gemm", 1.0)
    assert np.array_equal(o0, o3) and np.array_equal(d0, d3)


# ------------------------------------------------------------------------------------------ the functional
def _functional(ctx, dims, M, nsteps, pars):
    hip, sh_ = _mods()
    prob = hip.CGL2d(ctx, dims, S.LS, **pars)
    sh = sh_.ShootingProblem(prob, M, nsteps)
    X, dX = _states(dims, M)
    rng = np.random.default_rng(11)
    normal, center = rng.standard_normal(prob.nlocal), 0.3 * rng.standard_normal(prob.nlocal)
    sh.section = (prob.vec(normal), prob.vec(center))
    return prob, sh, X, dX, normal, center


def _call(ctx, sh, X, T, pv, dX=None, dT=0.0):
    """bk_shooting_residual / bk_shooting_jvp into a NaN-guarded buffer -> (out (M, N), tail)."""
    from bk_amd.hip import _ptr
    from bk_amd.periodic_orbit import _parr
    x = sh.vec(X)
    full, out = _guarded(ctx, sh.n)
    tail = C.c_double()
    if dX is None:
        ctx.check(ctx.lib.bk_shooting_residual(sh.h, _ptr(x.t), float(T), _parr(pv), len(pv), _ptr(out), C.byref(tail)), "residual")
    else:
        dx = sh.vec(dX)
        ctx.check(ctx.lib.bk_shooting_jvp(sh.h, _ptr(x.t), float(T), _parr(pv), len(pv), _ptr(dx.t), float(dT), _ptr(out),
                                          C.byref(tail)), "jvp")
    ctx.sync()
    return _unguard(full, sh.n).reshape(sh.M, -1), tail.value


@pytest.mark.parametrize("dims,M,nsteps", [((8, 6), 2, 2), ((12, 9), 3, 48), ((23, 17), 1, 1), ((41, 21), 2, 48), ((40, 33), 3, 2)])
def test_shooting_residual_jvp_and_tail_match_the_restatement(ctx, dims, M, nsteps):
    """G and dG (dX, dT) against the long-double restatement with the yardstick of the flow, 4 nsteps (nx + ny) eps unit; the period
    column adds |F(Phi)| |dT| / M to the unit of the JVP.  The tails within the summation bound 4 N eps sum |terms|.  The period
    column alone (dX = 0, dT = 1) is F(Phi_i) / M of the restatement."""
    prob, sh, X, dX, normal, center = _functional(ctx, dims, M, nsteps, dict(S.PARS, gamma=0.05))
    pars = dict(S.PARS, gamma=0.05)
    fl = _fl(dims)
    T, dT = 0.1 * nsteps * M, 0.37
    N = prob.nlocal
    bound = 4 * nsteps * (dims[0] + dims[1]) * EPS
    got, tail = _call(ctx, sh, X, T, _pv(pars))
    assert sh.transform_paths() == PATHS[dims]
    ref, rtail = S.residual(fl, X.astype(LD), T, pars, nsteps, normal.astype(LD), center.astype(LD))
    umax = fl.march(X.astype(LD), S.seg_tau(LD, M, T), nsteps, pars)["umax"]
    probe(f"shooting.residual.{dims}.{M}.{nsteps}", float(np.abs(got - ref).max()), bound * umax, tight=64 * EPS * umax)
    utail = (np.sum(np.abs(X[0] * normal)) + np.sum(np.abs(center * normal))) * T
    probe(f"shooting.residual_tail.{dims}.{M}.{nsteps}", abs(tail - float(rtail)) / (4 * N * EPS * utail), 1.0)
    got, tail = _call(ctx, sh, X, T, _pv(pars), dX, dT)
    ref, rtail, parts = S.jvp(fl, X.astype(LD), T, pars, nsteps, dX.astype(LD), dT, normal.astype(LD), center.astype(LD), parts=True)
    unit = parts["dumax"] + float(np.abs(parts["FPhi"]).max()) * abs(dT) / M
    probe(f"shooting.jvp.{dims}.{M}.{nsteps}", float(np.abs(got - ref).max()), bound * unit, tight=64 * EPS * unit)
    utail = utail / T * abs(dT) + np.sum(np.abs(dX[0] * normal)) * T
    probe(f"shooting.jvp_tail.{dims}.{M}.{nsteps}", abs(tail - float(rtail)) / (4 * N * EPS * utail), 1.0)
    col, ctail = _call(ctx, sh, X, T, _pv(pars), np.zeros_like(dX), 1.0)
    fu = np.stack([fl.m.F_abs(np.asarray(parts["Phi"][i], dtype=float), pars) for i in range(M)]) / M
    fbound = 16 * EPS * fu + bound * parts["umax"] * (4 * (fl.m.ax + fl.m.ay) + 8.0) / M       # rounding of F + F's Lipschitz constant x the error of Phi
    assert np.all(np.abs(col - parts["FPhi"] / M) <= fbound)
    assert abs(ctail - float(np.sum(X[0] * normal) - np.sum(center * normal))) <= 4 * N * EPS * utail


def test_shooting_jvp_matches_central_differences_of_the_device_residual(ctx):
    """dT = 0 against central differences of bk_shooting_residual, step 1e-6, at (12, 9), M = 2, 48 steps.  The bound is the
    difference quotient's own error as the restatement shows it for the same step -- its float64 quotient against its long-double
    JVP -- times 10."""
    dims, M, nsteps = (12, 9), 2, 48
    prob, sh, X, dX, normal, center = _functional(ctx, dims, M, nsteps, S.PARS)
    T, h = 6.3, 1e-6
    fl, f64 = _fl(dims), _fl(dims, float)
    jref, tref = S.jvp(fl, X.astype(LD), T, S.PARS, nsteps, dX.astype(LD), 0.0, normal.astype(LD), center.astype(LD))
    q = [S.residual(f64, X + s * h * dX, T, S.PARS, nsteps, normal, center) for s in (1, -1)]
    yard = float(np.abs((q[0][0] - q[1][0]) / (2 * h) - jref).max())
    yard_t = abs((q[0][1] - q[1][1]) / (2 * h) - float(tref))
    g = [_call(ctx, sh, X + s * h * dX, T, _pv(S.PARS)) for s in (1, -1)]
    J, Jt = _call(ctx, sh, X, T, _pv(S.PARS), dX, 0.0)
    probe("shooting.jvp_vs_differences", float(np.abs((g[0][0] - g[1][0]) / (2 * h) - J).max()), 10 * yard, yard=yard)
    probe("shooting.jvp_tail_vs_differences", abs((g[0][1] - g[1][1]) / (2 * h) - Jt), 10 * yard_t, yard=yard_t)


# ------------------------------------------------------------------------------------------ the operator: stored and recomputed
@pytest.mark.parametrize("dims,M,nsteps", [((12, 9), 3, 48), ((41, 21), 2, 2), ((23, 17), 1, 1)])
def test_shooting_operator_stored_and_recomputed_have_the_same_bits(ctx, dims, M, nsteps):
    """Three applications with distinct vectors through the operator that keeps the base trajectory (one base march, at creation)
    and through the one that marches state and tangent together every time (option shooting_store = 0: one base march per
    application, none at creation; the same for a store budget of one double): the same bits, vector and tail, and those of
    bk_shooting_jvp."""
    hip, sh_ = _mods()
    prob, sh, X, dX, normal, center = _functional(ctx, dims, M, nsteps, S.PARS)
    x, T, pv = sh.vec(X), 0.1 * nsteps * M, _pv(S.PARS)
    rng = np.random.default_rng(2)
    vs = [(rng.standard_normal(X.size), float(rng.standard_normal())) for _ in range(3)]
    res = {}
    try:
        for key, opts in (("stored", {}), ("recomputed", {"shooting_store": 0.0}), ("budget", {"shooting_store_max": 1.0})):
            for k, v in opts.items():
                ctx.set_option(k, v)
            J = sh.jacobian(x, T, pv)
            st0 = J.stats()
            outs = [J(hip.BorderedArray(sh.vec(v), t)) for v, t in vs]
            res[key] = ([(o.u.numpy(), o.p) for o in outs], st0, J.stats())
            ctx.set_option("shooting_store", 1.0)
            ctx.set_option("shooting_store_max", 268435456.0)
    finally:
        ctx.set_option("shooting_store", 1.0)
        ctx.set_option("shooting_store_max", 268435456.0)
    assert res["stored"][1] == dict(stored=True, base_marches=1, applications=0)
    assert res["stored"][2] == dict(stored=True, base_marches=1, applications=3)
    for key in ("recomputed", "budget"):
        assert res[key][1] == dict(stored=False, base_marches=0, applications=0)
        assert res[key][2] == dict(stored=False, base_marches=3, applications=3)
        for (a, at), (b, bt) in zip(res["stored"][0], res[key][0]):
            assert np.array_equal(a, b) and at == bt, key
    direct = sh.jvp(x, T, pv, sh.vec(vs[0][0]), vs[0][1])
    assert np.array_equal(direct.u.numpy(), res["stored"][0][0][0]) and direct.p == res["stored"][0][0][1]


# ------------------------------------------------------------------------------------------ the solve
@functools.lru_cache(maxsize=None)
def _cycle(k):
    """The restatement's side of cycle case k: (record of the fixture, Newton result, (model, flow, guess, normal, center))."""
    rec = S.load_fixture()["cycle"][k]
    got, s, aux = S.cycle_case(*S.CYCLE_CASES[k], with_multipliers=False)
    return rec, s, aux


@pytest.mark.parametrize("rtol", [1e-4, 1e-9])
def test_shooting_solve_matches_scipy_gmres(ctx, rtol):
    """The first Newton system of the (12, 9), M = 3 cycle case (the guess of the restatement, right-hand side = the functional
    there), IterativeSolvers flavor, unpreconditioned, against SciPy GMRES with the same rule |r| <= rtol |rhs|: the true residual
    through the restatement's JVP meets the rule (the slack of test_gpu_potrap's solve test), and the application count is SciPy's
    within 4, what that test allows."""
    hip, sh_ = _mods()
    dims, M, nsteps = S.CYCLE_CASES[1]
    _, _, (m, fl, X0, normal, center) = _cycle(1)
    T0 = 6.3
    prob = hip.CGL2d(ctx, dims, S.LS, **S.PARS)
    sh = sh_.ShootingProblem(prob, M, nsteps)
    sh.section = (prob.vec(normal), prob.vec(center))
    x = sh.vec(X0)
    G = sh.residual(x, T0, _pv(S.PARS))
    rhs = S.pack(G.u.numpy().reshape(M, -1), G.p)
    xc, itc = S.gmres_solve(fl, X0, T0, S.PARS, nsteps, normal, center, rhs, rtol, restart=50, maxiter=200)
    ls = hip.GMRESIterativeSolvers(reltol=rtol, restart=50, maxiter=200)
    sol, cv, it = sh_.shooting_solve(sh.jacobian(x, T0, _pv(S.PARS)), G, ls)
    o, t = S.jvp(fl, X0, T0, S.PARS, nsteps, sol.u.numpy().reshape(M, -1), sol.p, normal, center)
    true = float(np.linalg.norm(rhs - S.pack(o, t)))
    nb = float(np.linalg.norm(rhs))
    print(f"shooting solve rtol {rtol:g}: applications GPU {it}, SciPy {itc}; true residual {true / nb:.3e}")
    assert cv
    probe(f"shooting.solve_true_residual.{rtol:g}", true, rtol * nb * (1 + 1e-6) + 1e-13 * nb)
    probe(f"shooting.solve_count.{rtol:g}", abs(it - itc), 4, gpu=it, scipy=itc)


# ------------------------------------------------------------------------------------------ Newton and Floquet
def _newton_checks(name, s, rec, ref):
    print(f"newton_po_shooting {name}: residuals {s['residuals']}, gmres {s['itlinear']} (restatement {ref['itlinear']}), "
          f"T {s['T']:.12g} (fixture {rec['T']:.12g})")
    assert s["converged"] and s["residuals"][-1] < 1e-9, s["residuals"]
    assert s["itnewton"] <= ref["itnewton"] + 2 and len(s["itlinear"]) == s["itnewton"]
    probe(f"shooting.newton_T.{name}", abs(s["T"] - rec["T"]) / rec["T"], 1e-8)
    probe(f"shooting.newton_amplitude.{name}", abs(s["u"].norminf() - rec["amplitude"]) / rec["amplitude"], 1e-6)


def _polish(sh_, sh, s, pv, ls):
    """The orbit converged on to the residual the fixture's multipliers were taken at (shooting_ref.POLISH_TOL): the multipliers of
    two orbits known to 1e-9 differ by 1e-9 |(I - M)^-1|, 1e-8 next to the Hopf point, which is the size of the Krylov-Schur bound."""
    p = sh_.newton_po_shooting(sh, s["u"], s["T"], pv, ls, tol=S.POLISH_TOL, max_iterations=6)
    assert p["converged"], p["residuals"]
    return p


def _floquet_checks(name, fl_, rec, tol):
    mu = fl_["multipliers"]
    want = np.array([complex(*v) for v in rec["multipliers"]])
    print(f"floquet {name}: {mu[:5]} (fixture {want})")
    assert fl_["converged"]
    for w in want:
        k = int(np.argmin(np.abs(mu - w)))
        probe(f"shooting.multiplier.{name}.{w.real:.4f}", abs(mu[k] - w), max(tol, np.sqrt(EPS) * abs(w)))
    # the trivial multiplier: within the fixture's own distance of 1, the distance its recorded Newton run (stopped at 1e-9) left; the
    # tangent is the exact derivative of the discrete map, so the distance measures how far Newton went, and the orbit here went on
    # to 1e-11
    probe(f"shooting.trivial_multiplier.{name}", float(np.min(np.abs(mu - 1.0))), rec["trivial_distance"])
    return mu


@pytest.mark.parametrize("k", range(len(S.CYCLE_CASES)))
def test_newton_po_shooting_on_the_limit_cycle_and_its_multipliers(ctx, k):
    """shooting_guess_from_flow (t = 120 in 1200 steps from the restatement's 0.1 rand, T = 6.3) -> newton_po_shooting with the
    example's GMRES (rtol 1e-4, restart 50): below 1e-9 within the restatement's step count + 2, T within 1e-8 of the fixture
    (both sides stop at 1e-9 and |(I - M)^-1| on the section is O(1): the yardstick is the residual).  Then the five leading
    Floquet multipliers -- of the orbit converged on to 1e-11, as the fixture's are -- against the fixture's dense eigenvalues within
    Krylov-Schur's max(tol, sqrt(eps) |mu|), the trivial one as close to 1 as the fixture's, all inside the unit circle."""
    hip, sh_ = _mods()
    dims, M, nsteps = S.CYCLE_CASES[k]
    rec, ref, (m, fl, X0, normal, center) = _cycle(k)
    prob = hip.CGL2d(ctx, dims, S.LS, **S.PARS)
    sh = sh_.ShootingProblem(prob, M, nsteps)
    pv = _pv(S.PARS)
    g = sh_.shooting_guess_from_flow(prob, prob.vec(S.cycle_start(m)), 120.0, 1200, 6.3, M, pv, sh)
    gnorm, gcen = sh.section
    assert np.array_equal(gcen.numpy(), g["orbit"].numpy()[:m.N]) and abs(gnorm.norm() - 1.0) <= 8 * EPS
    ls = hip.GMRESIterativeSolvers(reltol=1e-4, restart=50, maxiter=50)
    s = sh_.newton_po_shooting(sh, g["orbit"], g["T"], pv, ls, tol=1e-9, max_iterations=25)
    _newton_checks(f"{dims}.{M}", s, rec, ref)
    s = _polish(sh_, sh, s, pv, ls)
    eig = hip.EigKrylovKit(tol=1e-8, maxiter=20, krylovdim=20)
    mu = _floquet_checks(f"{dims}.{M}", sh_.floquet_multipliers_shooting(sh, s["u"], s["T"], pv, 5, eig=eig), rec, eig.tol)
    assert np.max(np.abs(mu)) <= 1.0 + 1e-6
    times, states = sh_.get_periodic_orbit_shooting(sh, s["u"], s["T"], pv, nout=4)
    assert states.shape == (4, m.N) and np.array_equal(states[0], s["u"].numpy()[:m.N]) and abs(times[1] - s["T"] / 4) <= 4 * EPS * s["T"]


@pytest.mark.parametrize("k", range(len(S.HOPF_CASES)))
def test_newton_po_shooting_from_the_hopf_predictor_and_its_multipliers(ctx, k):
    """hopf normal form -> predictor -> shooting_guess_from_hopf -> newton_po_shooting at r_H - dr: the small unstable orbit of the
    fixture, with exactly one multiplier outside the unit circle."""
    from test_gpu_potrap import _hopf_record
    from bk_amd import codim2
    hip, sh_ = _mods()
    dims, M, nsteps, dr = S.HOPF_CASES[k]
    rec = S.load_fixture()["hopf"][k]
    _, ref, _ = S.hopf_case(dims, M, nsteps, dr, with_multipliers=False)
    prob, hp, rstar = _hopf_record(ctx, dims)
    pred = codim2.predictor(hp, dr)
    pars = dict(S.PARS, r=pred["p"])
    assert abs(pars["r"] - rec["r"]) <= 1e-13
    sh = sh_.ShootingProblem(prob, M, nsteps)
    g = sh_.shooting_guess_from_hopf(pred, M, prob, sh=sh, params=_pv(pars))
    ls = hip.GMRESIterativeSolvers(reltol=1e-4, restart=50, maxiter=50)
    s = sh_.newton_po_shooting(sh, g["orbit"], g["T"], _pv(pars), ls, tol=1e-9, max_iterations=25)
    _newton_checks(f"hopf.{dims}.{dr}", s, rec, ref)
    s = _polish(sh_, sh, s, _pv(pars), ls)
    eig = hip.EigKrylovKit(tol=1e-8, maxiter=20, krylovdim=20)
    mu = _floquet_checks(f"hopf.{dims}.{dr}", sh_.floquet_multipliers_shooting(sh, s["u"], s["T"], _pv(pars), 5, eig=eig), rec, eig.tol)
    assert int(np.sum(np.abs(mu) > 1.0 + 1e-6)) == 1


# ------------------------------------------------------------------------------------------ continuation
def test_continuation_po_shooting_three_steps_match_the_restatement(ctx):
    """Three PALC steps at (12, 9), M = 2, 48 steps per segment, from the r = 1.2 orbit with ds = -0.01 against three steps of the
    restatement driven by the same continuation.py engine on NumPy vectors: p, T and the step sizes agree to 1e-7 -- the linear
    solves stop at 1e-4 and Newton's tol = 1e-9 sets the agreement -- and the Newton counts are equal."""
    from bk_amd import continuation as Cn
    hip, sh_ = _mods()
    dims, M, nsteps = (12, 9), 2, 48
    fl = _fl(dims, float)
    m = fl.m
    X0 = S.guess_from_flow(fl, S.cycle_start(m), 120.0, 1200, 6.3, M, nsteps, S.PARS)
    normal, center = S.update_section(fl, X0, S.PARS)
    cp = Cn.ContinuationPar(ds=-0.01, dsmin=1e-4, dsmax=0.03, a=0.5, eta=150.0, p_min=-10.0, p_max=10.0, max_steps=3,
                            detect_bifurcation=0, newton_options=Cn.NewtonPar(tol=1e-9, max_iterations=25))
    ref = S.palc(fl, X0, 6.3, S.PARS, "r", nsteps, normal, center, cp, 3)
    prob = hip.CGL2d(ctx, dims, S.LS, **S.PARS)
    sh = sh_.ShootingProblem(prob, M, nsteps)
    sh.section = (prob.vec(normal), prob.vec(center))
    ls = hip.GMRESIterativeSolvers(reltol=1e-4, restart=50, maxiter=50)
    br = sh_.continuation_po_shooting(sh, sh.vec(X0), 6.3, _pv(S.PARS), "r", cp, ls)
    print(f"continuation_po_shooting: p {br['p']}, T {br['T']}, ds {br['ds']}, newton {br['itnewton']} (restatement {ref['itnewton']}), "
          f"gmres {br['itlinear']} (restatement {ref['itlinear']})")
    assert len(br["p"]) == 4 and all(br["converged"]) and len(ref["p"]) == 4
    assert br["itnewton"] == ref["itnewton"]
    for key in ("p", "T", "ds"):
        for k in range(4):
            probe(f"shooting.palc_{key}.{k}", abs(br[key][k] - ref[key][k]), 1e-7 * max(1.0, abs(ref[key][k])))
    assert br["p"][3] < br["p"][0]


# ------------------------------------------------------------------------------------------ refusals
def test_shooting_refusals(ctx):
    hip, sh_ = _mods()
    from bk_amd._lib import BkHipError
    from bk_amd.hip import _ptr
    from bk_amd.periodic_orbit import _parr
    swift = hip.SwiftHohenberg(ctx, (16, 16), (np.pi, np.pi))
    with pytest.raises(BkHipError, match="BK_PDE_CGL2D only"):
        sh_.ShootingProblem(swift, 2, 8)
    with pytest.raises(BkHipError, match="BK_PDE_CGL2D only"):
        sh_.Flow(swift, 1)
    prob = hip.CGL2d(ctx, (12, 9), S.LS, **S.PARS)
    with pytest.raises(BkHipError, match="M >= 1"):
        sh_.ShootingProblem(prob, 0, 8)
    with pytest.raises(BkHipError, match="nsteps >= 1"):
        sh_.ShootingProblem(prob, 2, 0)
    sh = sh_.ShootingProblem(prob, 2, 4)
    X = sh.vec(np.ones(sh.n))
    pv = _pv(S.PARS)
    with pytest.raises(BkHipError, match="no section set"):
        sh.residual(X, 6.0, pv)
    with pytest.raises(BkHipError, match="no section set"):
        sh.jacobian(X, 6.0, pv)
    sh.section = (prob.vec(np.ones(prob.nlocal)), prob.vec(np.zeros(prob.nlocal)))
    tail = C.c_double()
    flow = sh_.Flow(prob, 2)
    Y = sh.vec(np.ones(sh.n))
    for call in (lambda: ctx.lib.bk_shooting_residual(sh.h, _ptr(X.t), 6.0, _parr(pv), 6, _ptr(X.t), C.byref(tail)),
                 lambda: ctx.lib.bk_shooting_jvp(sh.h, _ptr(X.t), 6.0, _parr(pv), 6, _ptr(Y.t), 0.0, _ptr(Y.t), C.byref(tail)),
                 lambda: ctx.lib.bk_flow_evolve(flow.h, _ptr(X.t), 1.0, 4, _parr(pv), 6, _ptr(X.t)),
                 lambda: ctx.lib.bk_flow_jvp(flow.h, _ptr(X.t), _ptr(Y.t), 1.0, 4, _parr(pv), 6, _ptr(Y.t), _ptr(X.t)),
                 lambda: ctx.lib.bk_flow_jvp(flow.h, _ptr(X.t), _ptr(Y.t), 1.0, 4, _parr(pv), 6, _ptr(sh.vec(np.ones(sh.n)).t), _ptr(X.t))):
        with pytest.raises(BkHipError, match="must not alias"):
            ctx.check(call(), "alias")
    with pytest.raises(BkHipError, match="nsteps >= 1"):
        flow.evolve(X, 1.0, 0, pv)
    with pytest.raises(BkHipError, match="tau must be finite"):
        flow.evolve(X, float("inf"), 4, pv)
    with pytest.raises(BkHipError, match="params = "):
        sh.residual(X, 6.0, pv[:5])
    J = sh.jacobian(X, 6.0, pv)
    rhs = hip.BorderedArray(sh.vec(np.ones(sh.n)), 1.0)
    minres = hip.GMRESIterativeSolvers(reltol=1e-6, restart=30, maxiter=60)
    minres.flavor = 3                                          # BK_KRYLOV_MINRES
    with pytest.raises(BkHipError, match="use a GMRES flavor"):
        sh_.shooting_solve(J, rhs, minres)
    # the context is still usable
    r = sh.residual(X, 6.0, pv)
    assert np.isfinite(r.u.norminf()) and np.isfinite(r.p)
