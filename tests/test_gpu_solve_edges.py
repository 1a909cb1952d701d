"""GPU tests of the three passes taken out around each GMRES solve (options gmres_check_nostore, gmres_fuse_v0, palc_fuse_update;
csrc/dct_fast.hip: dct_fused_kernel FZS without a store array and SRC, csrc/solver.hip: start_cycle / bk_op::arm_v0, palc_update).

All three changes are elementwise: no sum changes its order, so option 0 (the launches as they were) and option 1 must agree in
every BIT of everything a solve or a corrector step returns.  That a fused pass really ran -- equal bits are trivial where it
declines -- is read off the profiling scopes: the check's x-forward pass accounts 24 instead of 32 bytes per point, a fused cycle
start saves one "blas1" launch per cycle, the fused update one per Newton step.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import operators  # noqa: E402

L, NU = 0.1, 1.2
KK, IS = 0, 1
# (flavor, a0, a1) as tests/test_gpu_spectral_check.py: KrylovKit unshifted, shifted (the fold form), IterativeSolvers, KrylovKit a1 != 1
FORMS = [(KK, 0.0, 1.0), (KK, -0.6, 1.0), (IS, 0.3, 1.0), (KK, 0.0, 0.7)]
G64 = ((64, 64, 64), (6.0, 6.5, 7.0))
G3 = ((128, 64, 256), (12.5, 6.0, 25.0))            # three different extents
GNT = ((128, 128, 256), (12.5, 12.5, 25.0))         # 2^22 points: the non-temporal instantiations
OPTS = ("gmres_check_nostore", "gmres_fuse_v0", "palc_fuse_update")


def _hip():
    from bk_amd import hip
    return hip


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _case(dims, ls):
    sh = operators.SwiftHohenberg(dims, ls)
    rng = np.random.default_rng(13)
    u = sh.guess() + 0.2 * rng.standard_normal(sh.N)
    return sh, u, rng.standard_normal(sh.N), rng.standard_normal(sh.N)


def _set(ctx, **kw):
    for k, v in kw.items():
        ctx.set_option(k, v)


def _profiled(ctx, fn):
    """(fn(), launches of the "blas1" scope, bytes of the "dct_pass" scope)"""
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        r = fn()
        ctx.sync()
        return r, ctx.prof_get("blas1")["calls"], ctx.prof_get("dct_pass")["bytes"]
    finally:
        ctx.prof_enable(False)


# ------------------------------------------------------------------------------------------ A: gmres_check_nostore
@pytest.mark.parametrize("dims,ls", [G64, G3, GNT])
def test_check_without_the_stored_sum(ctx, dims, ls):
    """bk_precond_check_norm on the operator forms of the spectral-check tests: value and path flag bitwise equal with the option at 0
    and at 1, and the pass accounts 8 bytes per point less (the sum rhs + c tmp is no longer written)."""
    hip = _hip()
    sh, u, x, rhs = _case(dims, ls)
    prob = hip.SwiftHohenberg(ctx, dims, ls, l=L, nu=NU)
    J = prob.jacobian(prob.vec(u), L)
    P = hip.DCTPreconditioner(prob, 1.0)
    xd, rd = prob.vec(x), prob.vec(rhs)
    try:
        for flavor, a0, a1 in FORMS:
            out = {}
            for opt in (0, 1):
                ctx.set_option("gmres_check_nostore", opt)
                out[opt] = _profiled(ctx, lambda: P.check_norm(J, xd, rd, a0, a1, flavor))
            (v0, s0), _, b0 = out[0]
            (v1, s1), _, b1 = out[1]
            print(f"solve_edges check dims={dims} form={(flavor, a0, a1)} value={v0!r} / {v1!r} dct bytes {b0:.0f} / {b1:.0f}")
            assert s0 and s1, (dims, flavor, a0, s0, s1)                  # the spectral path ran in both
            assert _bits(v0) == _bits(v1), (dims, flavor, a0, v0, v1)
            assert b0 - b1 == 8.0 * sh.N, (dims, flavor, b0, b1)
    finally:
        ctx.set_option("gmres_check_nostore", 1)


# ------------------------------------------------------------------------------------------ B: gmres_fuse_v0
# (name, grid, solver factory, extra options, right-hand side offset by 8 bytes, the fusion is expected to run)
def _kk(**kw):
    return lambda hip, P: hip.GMRESKrylovKit(**dict(dict(dim=30, rtol=1e-9, atol=0.0, maxiter=150, Pl=P), **kw))


SOLVES = [("kk64", G64, _kk(), {}, False, True),
          ("is64", G64, lambda hip, P: hip.GMRESIterativeSolvers(reltol=1e-9, restart=30, maxiter=400, Pl=P), {}, False, True),
          ("kk3", G3, _kk(), {}, False, True),
          ("restart64", G64, _kk(dim=5), {}, False, True),                 # restarts: start_cycle from the residual vector r
          ("nosstep64", G64, _kk(), {"gmres_sstep": 0}, False, False),     # no block cycles: declines
          ("chain64", G64, _kk(), {"gmres_stencil_free": 0}, False, False),   # the literal chain: declines
          # rhs 8 bytes off: the cycle's source is b = Pl \\ rhs (first cycle) or the residual r (restarts), both 16-byte-aligned library
          # scratch, so the fusion RUNS; the alignment guard of start_cycle cannot be reached through the API (no case asserts its decline)
          ("offset64", G64, _kk(), {}, True, True)]


@pytest.mark.parametrize("name,grid,mk,extra,offset,fuses", SOLVES, ids=[s[0] for s in SOLVES])
def test_cycle_start_in_the_first_transform_pass(ctx, name, grid, mk, extra, offset, fuses):
    """GMRES solves with the spectral preconditioner, J taken at l = -0.7 where it is definite (17 applications at dim 30; dim 5
    restarts): x, numops, converged, last_resnorm and the MEASURED orthogonality defect of the basis (option orth_probe: max |V'V - I|
    over the cycles, which reads V[0] as the fused pass stored it) bitwise equal with gmres_fuse_v0 at 0 and at 1.  Whether the fused
    pass ran is asserted in every case from the number of "blas1" launches: one fewer per cycle where it runs (a misaligned caller
    vector included: the solver's own source vectors are aligned scratch), the same number where it declines (no block cycles, the
    literal chain)."""
    import torch
    hip = _hip()
    dims, ls = grid
    sh, u, _, rhs = _case(dims, ls)
    l2 = -0.7
    prob = hip.SwiftHohenberg(ctx, dims, ls, l=l2, nu=NU)
    J = prob.jacobian(prob.vec(u), l2)
    P = hip.DCTPreconditioner(prob, 1.0)
    if offset:
        t = torch.empty(sh.N + 1, dtype=torch.float64, device=ctx.torch_device)
        t[1:] = torch.from_numpy(rhs).to(ctx.torch_device)
        rd = hip.HipVec(ctx, t[1:], sh.N)
        assert rd.t.data_ptr() % 16 == 8
    else:
        rd = prob.vec(rhs)
    gm = mk(hip, P)
    defaults = {k: {"gmres_sstep": -1, "gmres_stencil_free": 1}[k] for k in extra}
    out = {}
    try:
        _set(ctx, orth_probe=1, **extra)
        for opt in (0, 1):
            ctx.set_option("gmres_fuse_v0", opt)

            def solve():
                x, ok, it = gm(J, rd, 0.0, 1.0)
                return x.numpy(), ok, it, gm.last_resnorm, ctx.get_option("gmres_last_orth_defect")
            out[opt] = _profiled(ctx, solve)
    finally:
        _set(ctx, orth_probe=0, gmres_fuse_v0=1, **defaults)
    (r0, c0, _), (r1, c1, _) = out[0], out[1]
    print(f"solve_edges v0 {name}: ok={r1[1]} it={r1[2]} resnorm={r1[3]!r} defect={r1[4]:.3e} blas1 launches {c0} / {c1}")
    assert r0[1] and r1[1], (name, r0[1:], r1[1:])
    assert np.array_equal(_bits(r0[0]), _bits(r1[0])), name
    assert r0[1:3] == r1[1:3] and _bits(r0[3]) == _bits(r1[3]) and _bits(r0[4]) == _bits(r1[4]), (name, r0[1:], r1[1:])
    if name == "restart64":
        assert r1[2] > 2 * 6, (name, r1[2])                  # more applications than two cycles of dim 5 hold
    if fuses:
        assert c1 < c0, (name, c0, c1)                        # one scale pass fewer per cycle
    else:
        assert c1 == c0, (name, c0, c1)


# ------------------------------------------------------------------------------------------ C: palc_fuse_update
def _dev(ctx, a, offset):
    """a on the device, starting `offset` doubles into its allocation"""
    import torch
    t = torch.empty(a.size + offset, dtype=torch.float64, device=ctx.torch_device)
    t[offset:] = torch.from_numpy(a).to(ctx.torch_device)
    return _hip().HipVec(ctx, t[offset:], a.size)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", [1, 2, 255, 256 * 4 * 3 + 1, (1 << 22) + 3])
def test_fused_update_has_the_bits_of_the_two_axpby(ctx, n, offset):
    """bk_palc_update against bk_vec_axpby(-dl, dx, 1, x1) followed by bk_vec_axpby(-1, x1, 1, x) on random data: the ragged end of
    the 16-byte walk, more than one sweep, the non-temporal path (n >= 2^22), pointers aligned and 8 bytes off (element by element);
    dl = 0 (the dx term is skipped as v_axpbyz skips an operand), -0.75, 1e-3.  x1 and dx are left untouched."""
    hip = _hip()
    rng = np.random.default_rng(n + offset)
    dx, x1, x = (rng.standard_normal(n) for _ in range(3))
    x1[0] = -0.0                                              # (0.0 + (-0.0) is +0.0: the skipped operand's sign behaviour)
    x[0] = -0.0
    for dl in (0.0, -0.75, 1e-3):
        Dx, X1, X = _dev(ctx, dx, offset), _dev(ctx, x1, offset), _dev(ctx, x, offset)
        R1, R = _dev(ctx, x1, offset), _dev(ctx, x, offset)
        assert X.t.data_ptr() % 16 == 8 * offset
        R1.add_(Dx, -dl, 1.0)
        R.add_(R1, -1.0, 1.0)
        hip.palc_update(X, X1, Dx, dl)
        got, ref = X.numpy(), R.numpy()
        assert np.array_equal(_bits(got), _bits(ref)), (n, offset, dl, int((_bits(got) != _bits(ref)).sum()))
        assert np.array_equal(_bits(X1.numpy()), _bits(x1)) and np.array_equal(_bits(Dx.numpy()), _bits(dx)), (n, offset, dl)


CELL = ((64, 32, 32), (2.0 * np.pi, 2.0 * np.pi / np.sqrt(3.0), np.pi))     # the bench's cell


def _corrector(ctx, dims, ls, **kw):
    """One PALC corrector run with the bench's settings (GMRESKrylovKit(30), rtol 1e-9, atol 1e-12, 150 cycles, BorderingBLS without
    check_precision, norminf, no line search), two Newton steps from a perturbed state.  Taken at l = -0.7, where the Jacobian is
    definite on such a state and every solve converges (at l = 0.1 restarted GMRES stalls on it and no solve reaches its explicit
    check): each Newton step then runs two solves with one check each, the bordered tail and the update."""
    hip = _hip()
    L = -0.7
    csh = operators.SwiftHohenberg(dims, ls)
    cprob = hip.SwiftHohenberg(ctx, dims, ls, l=L, nu=NU)
    rng = np.random.default_rng(5)
    u0 = csh.guess() + 0.05 * rng.standard_normal(csh.N)
    B = hip.BorderedArray
    CP = hip.DCTPreconditioner(cprob, 1.0)
    bls = hip.BorderingBLS(hip.GMRESKrylovKit(dim=30, rtol=1e-9, atol=1e-12, maxiter=150, Pl=CP),
                           check_precision=kw.pop("check_precision", False))
    z0 = B(cprob.vec(u0), L)
    tau = B(cprob.vec(0.01 * rng.standard_normal(csh.N)), -1.0)
    zp = z0.copy().add_(tau, -0.001)

    def run():
        s = hip.newton_palc_native(cprob, z0, tau, zp, -0.001, 0.5, bls, tol=1e-9, max_iterations=2, norm_inf=True, **kw)
        return (s["u"].u.numpy(), s["u"].p, tuple(s["residuals"]), bool(s["converged"]), s["itlineartot"], s["itnewton"])
    return run


def _same(a, b):
    return (np.array_equal(_bits(a[0]), _bits(b[0])) and _bits(a[1]) == _bits(b[1]) and np.array_equal(_bits(a[2]), _bits(b[2]))
            and a[3:] == b[3:])


@pytest.mark.parametrize("dims,ls", [CELL, G64])
def test_corrector_is_bitwise_untouched(ctx, dims, ls):
    """newton_palc_native (two Newton steps): u, p, the residual history, the flag and the counts bitwise equal with the three options
    all at 0, all at 1 and each one alone at 1; the fused update saves one blas1 launch per Newton step.  With check_precision or the
    line search the fused update must decline: same launches, same bits."""
    run = _corrector(ctx, dims, ls)
    combos = [(0, 0, 0), (1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)]
    res = {}
    try:
        ctx.set_option("two_lanes", 0)                       # (one lane: every launch is accounted on this context's scopes)
        for c in combos:
            _set(ctx, **dict(zip(OPTS, c)))
            res[c] = _profiled(ctx, run)
        base, calls0, _ = res[(0, 0, 0)]
        for c in combos[1:]:
            r, calls, _ = res[c]
            print(f"solve_edges corrector dims={dims} options={c}: itnewton={r[5]} itlinear={r[4]} blas1 launches {calls0} / {calls}")
            assert _same(base, r), (dims, c, base[1:], r[1:])
        assert base[5] >= 1, base[1:]
        assert res[(0, 0, 1)][1] == calls0 - base[5], (calls0, res[(0, 0, 1)][1])      # one pass fewer per Newton step
        assert res[(0, 1, 0)][1] < calls0 and res[(1, 1, 1)][1] < res[(0, 1, 0)][1]
        for kw in ({"check_precision": True}, {"linesearch": True}):
            rk = _corrector(ctx, dims, ls, **kw)
            out = {}
            for c in (0, 1):
                _set(ctx, gmres_check_nostore=1, gmres_fuse_v0=1, palc_fuse_update=c)
                out[c] = _profiled(ctx, rk)
            assert _same(out[0][0], out[1][0]) and out[0][1] == out[1][1], (dims, kw, out[0][1], out[1][1])
    finally:
        _set(ctx, two_lanes=1, **dict(zip(OPTS, (1, 1, 1))))


def test_two_lanes_reproduce_one_lane(ctx):
    """The 64^3 corrector under the new defaults with the two solves of the bordered system on two lanes and on one: equal bits."""
    dims, ls = G64
    run = _corrector(ctx, dims, ls)
    out = {}
    try:
        for tl in (0, 1):
            ctx.set_option("two_lanes", tl)
            out[tl] = run()
    finally:
        ctx.set_option("two_lanes", 1)
    assert _same(out[0], out[1]), (out[0][1:], out[1][1:])
