"""GPU tests of the corrector without its entry copy (csrc/solver.hip: bk_newton_palc_from, option palc_entry_copy) and of whole
GMRES solves with the six-slot projection launch (csrc/block_dots_wide.hip, option block_dots_wide).

Neither change touches a sum: the first Newton update reads the predictor where it read a copy of it, and the wide launch gives
every accumulator the fma sequence of the launches it replaces.  So everything a corrector or a solve returns must agree in every
BIT between the settings, and with the parent's own sequence -- a copy of the predictor handed to bk_newton_palc, which runs in
place.  That the copy really is gone (equal bits are trivial where it is still made) is read off the profiling scope "entry_copy";
that the wide launch really ran, off the solve's block log.

Grids: the bench's cell, and 256 x 128 x 128 = 2^22 points, where every streaming kernel takes its non-temporal path.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import operators  # noqa: E402

NU, LAM = 1.2, -0.7          # l = -0.7: the Jacobian is definite on the perturbed state and every solve converges (test_gpu_solve_edges)
DS, THETA = -0.001, 0.5
CELL = ((64, 32, 32), (2.0 * np.pi, 2.0 * np.pi / np.sqrt(3.0), np.pi))     # the bench's cell
GNT = ((256, 128, 128), (25.0, 12.5, 12.5))                                  # 2^22 points
G64 = ((64, 64, 64), (6.0, 6.5, 7.0))
GRIDS = [CELL, GNT]
_SETUP = {}


def _hip():
    from bk_amd import hip
    return hip


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def _setup(ctx, dims, ls):
    """Problem, preconditioner, last point, tangent and predictor of one grid, made once; the predictor's bits on the host."""
    if dims not in _SETUP:
        hip = _hip()
        sh = operators.SwiftHohenberg(dims, ls)
        prob = hip.SwiftHohenberg(ctx, dims, ls, l=LAM, nu=NU)
        rng = np.random.default_rng(5)
        u0 = sh.guess() + 0.05 * rng.standard_normal(sh.N)
        B = hip.BorderedArray
        z0 = B(prob.vec(u0), LAM)
        tau = B(prob.vec(0.01 * rng.standard_normal(sh.N)), -1.0)
        zp = z0.copy().add_(tau, DS)
        _SETUP[dims] = dict(prob=prob, P=hip.DCTPreconditioner(prob, 1.0), z0=z0, tau=tau, zp=zp, zp_bits=_bits(zp.u.numpy()).copy(),
                            u0=u0, rhs=rng.standard_normal(sh.N))
    return _SETUP[dims]


def _bls(S, kind):
    hip = _hip()
    if kind == "matrixfree":                 # one unpreconditioned GMRES on the (N + 1) operator: a short one, converged or not
        return hip.MatrixFreeBLS(hip.GMRESKrylovKit(dim=10, rtol=1e-9, atol=1e-12, maxiter=2))
    gm = hip.GMRESKrylovKit(dim=30, rtol=1e-9, atol=1e-12, maxiter=150, Pl=S["P"])       # the bench's solver
    return hip.BorderingBLS(gm, check_precision=(kind == "check_precision"))


def _result(u, p, res):
    return (u.numpy(), float(p), tuple(res.residuals[i] for i in range(res.itnewton + 1)), bool(res.converged), res.itlinear,
            res.itnewton)


def _native(S, bls, tol, max_iterations, linesearch=False):
    s = _hip().newton_palc_native(S["prob"], S["z0"], S["tau"], S["zp"], DS, THETA, bls, tol=tol, max_iterations=max_iterations,
                                  norm_inf=True, linesearch=linesearch)
    return (s["u"].u.numpy(), float(s["u"].p), tuple(s["residuals"]), bool(s["converged"]), s["itlineartot"], s["itnewton"])


def _parent(S, bls, tol, max_iterations, linesearch=False):
    """The sequence before bk_newton_palc_from existed: copy the predictor, then bk_newton_palc in place on the copy."""
    hip = _hip()
    from bk_amd import _lib as LB
    prob, z0, tau, zp = S["prob"], S["z0"], S["tau"], S["zp"]
    ctx = prob.ctx
    x = zp.u.copy()
    p = C.c_double(zp.p)
    pv = prob._pvec(zp.p)
    arr = (C.c_double * len(pv))(*pv)
    no = hip.newton_opts(tol, max_iterations, True, linesearch, 1.0, 1e-3, None)
    if isinstance(bls, hip.MatrixFreeBLS):
        bo = LB.BorderingOpts(0.0, 0, 1, 1)
    else:
        bo = LB.BorderingOpts(bls.tol, 1 if bls.check_precision else 0, bls.k, 0)
    lo = bls.solver._opts()
    res = LB.NewtonResult()
    ptr = lambda v: C.c_void_p(v.t.data_ptr())
    ctx.check(ctx.lib.bk_newton_palc(ctx.h, prob.h, ptr(x), C.byref(p), ptr(z0.u), float(z0.p), ptr(tau.u), float(tau.p), DS, THETA,
                                     arr, len(pv), prob.ipar, -1.7e308, 1.7e308, C.byref(no), C.byref(bo), C.byref(lo),
                                     bls.solver._pl(), C.byref(res)), "bk_newton_palc")
    return _result(x, p.value, res)


def _same(a, b):
    return (np.array_equal(_bits(a[0]), _bits(b[0])) and _bits(a[1]) == _bits(b[1]) and np.array_equal(_bits(a[2]), _bits(b[2]))
            and a[3:] == b[3:])


def _counted(ctx, fn):
    """(fn(), launches of the "entry_copy" scope)"""
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        r = fn()
        ctx.sync()
        return r, ctx.prof_get("entry_copy")["calls"]
    finally:
        ctx.prof_enable(False)
        ctx.prof_reset()


@pytest.mark.parametrize("max_iterations,tol", [(1, 0.0), (3, 0.0), (3, 1e300)], ids=["one", "three", "none"])
@pytest.mark.parametrize("dims,ls", GRIDS, ids=["cell", "nt"])
def test_corrector_without_the_entry_copy(ctx, dims, ls, max_iterations, tol):
    """u, p, residuals, the flag, itlineartot and itnewton bitwise equal with palc_entry_copy at 0 and at 1 and on the parent's
    sequence; the predictor is untouched after every call; no copy with the option at 0 unless no iteration ran, where the copy IS
    the result."""
    S = _setup(ctx, dims, ls)
    bls = _bls(S, "bordering")
    out = {}
    try:
        ref = _parent(S, bls, tol, max_iterations)
        assert np.array_equal(_bits(S["zp"].u.numpy()), S["zp_bits"])
        for opt in (0, 1):
            ctx.set_option("palc_entry_copy", opt)
            out[opt] = _counted(ctx, lambda: _native(S, bls, tol, max_iterations))
            assert np.array_equal(_bits(S["zp"].u.numpy()), S["zp_bits"]), opt
    finally:
        ctx.set_option("palc_entry_copy", 0)
    (r0, c0), (r1, c1) = out[0], out[1]
    print(f"corrector_edges dims={dims} max_iterations={max_iterations} tol={tol}: itnewton={r0[5]} itlinear={r0[4]} "
          f"residuals={r0[2]} entry copies {c0} / {c1}")
    assert _same(r0, r1), (r0[1:], r1[1:])
    assert _same(ref, r0), (ref[1:], r0[1:])
    assert np.isfinite(r0[0]).all() and np.isfinite(r0[2]).all()
    if tol == 0.0:
        assert r0[5] == max_iterations and c0 == 0 and c1 == 1, (r0[5], c0, c1)
    else:
        assert r0[5] == 0 and r0[4] == 0 and c0 == 1 and c1 == 1, (r0[4:], c0, c1)
        assert np.array_equal(_bits(r0[0]), S["zp_bits"]) and _bits(r0[1]) == _bits(S["zp"].p)


@pytest.mark.parametrize("kind,linesearch", [("bordering", True), ("check_precision", False), ("matrixfree", False)],
                         ids=["linesearch", "check_precision", "matrixfree"])
@pytest.mark.parametrize("dims,ls", GRIDS, ids=["cell", "nt"])
def test_in_place_paths_copy_first(ctx, dims, ls, kind, linesearch):
    """The line search, check_precision and MatrixFreeBLS run in place: one entry copy whatever the option says, and the bits of the
    parent's sequence."""
    S = _setup(ctx, dims, ls)
    bls = _bls(S, kind)
    iters = 1 if kind == "matrixfree" else 2
    out = {}
    try:
        ref = _parent(S, bls, 0.0, iters, linesearch)
        for opt in (0, 1):
            ctx.set_option("palc_entry_copy", opt)
            out[opt] = _counted(ctx, lambda: _native(S, bls, 0.0, iters, linesearch))
            assert np.array_equal(_bits(S["zp"].u.numpy()), S["zp_bits"]), opt
    finally:
        ctx.set_option("palc_entry_copy", 0)
    (r0, c0), (r1, c1) = out[0], out[1]
    print(f"corrector_edges dims={dims} {kind} linesearch={linesearch}: itnewton={r0[5]} itlinear={r0[4]} entry copies {c0} / {c1}")
    assert _same(ref, r0) and _same(ref, r1), (ref[1:], r0[1:], r1[1:])
    assert c0 == 1 and c1 == 1 and r0[5] >= 1, (c0, c1, r0[5])


def _wide_blocks(log):
    """(measured basis vectors, right-hand vectors) of every Arnoldi block of the log that follows another block of its cycle: the
    block that starts at column j after one that started at j' measures j' + 1 vectors against the j - j' the earlier block made
    plus its own steps (solver.hip: arnoldi_block)."""
    out = []
    for a, b in zip(log[:-1], log[1:]):
        if a["solve"] == b["solve"] and b["j"] > a["j"] and a["got"] == a["steps"]:
            out.append((int(a["j"]) + 1, int(b["j"] - a["j"] + b["steps"])))
    return out


@pytest.mark.parametrize("dims,ls", [G64, GNT], ids=["g64", "nt"])
def test_solve_with_the_wide_projection(ctx, dims, ls):
    """One cycle of GMRES(13) with a tolerance it cannot reach: the blocks run 3, 4, 4, 2 steps, so the last one measures 8 basis
    vectors against 4 + 2 right-hand vectors (asserted from the block log).  x, numops and the residual norm bitwise equal with
    block_dots_wide at 0 and at 1."""
    hip = _hip()
    S = _setup(ctx, dims, ls)
    prob = S["prob"]
    J = prob.jacobian(prob.vec(S["u0"]), LAM)
    rd = prob.vec(S["rhs"])
    gm = hip.GMRESKrylovKit(dim=13, rtol=1e-30, atol=0.0, maxiter=1, Pl=S["P"])
    out = {}
    try:
        ctx.set_option("gmres_block_log", 1)
        for opt in (0, 1):
            ctx.set_option("block_dots_wide", opt)
            ctx.solver_block_log(reset=True)
            x, ok, it = gm(J, rd, 0.0, 1.0)
            out[opt] = (x.numpy(), ok, it, gm.last_resnorm, ctx.solver_block_log(reset=True))
    finally:
        ctx.set_option("gmres_block_log", 0)
        ctx.set_option("block_dots_wide", 1)
    r0, r1 = out[0], out[1]
    shapes = _wide_blocks(r1[4])
    print(f"corrector_edges solve dims={dims}: numops={r1[2]} resnorm={r1[3]!r} blocks (measured, right-hand)={shapes}")
    assert any(5 <= k <= 8 and nr == 6 for k, nr in shapes), shapes
    assert shapes == _wide_blocks(r0[4])
    assert np.array_equal(_bits(r0[0]), _bits(r1[0]))
    assert r0[1:3] == r1[1:3] and _bits(r0[3]) == _bits(r1[3]), (r0[1:4], r1[1:4])
    assert np.isfinite(r1[0]).all() and r1[2] >= 13
