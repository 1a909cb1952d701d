"""GPU tests of the x turnaround (csrc/dct_fast.hip: dct_fused_kernel TURN, csrc/dct.hip: dct_apply_pw_chain).

Inside a Newton-basis block of GMRES the stencil-free operator is applied s times in a row, p_{i+1} = (T - theta_i) p_i with
T = Pl^-1 diag(g(u) + s).  With option dct_x_turnaround = 1 (the default) the x-inverse pass of application i and the x-forward pass
of application i + 1 run as ONE kernel: the doubles of p_{i+1} are formed and stored exactly as the x-inverse pass stores them and
enter the x-forward transform from registers instead of from memory.  Nothing in the arithmetic changes, so every solve must give
the same BITS with the option at 0 and at 1: solution, residual norm, operator-application count and block log.
"""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import operators  # noqa: E402  (the problem's initial guess only)


def _hip():
    from bk_amd import hip
    return hip


# x extents >= 64 (the fused x-axis kernel runs, so the stencil-free form and the chain do); 64 x 32 x 128 takes the y pass off the
# fused kernel (32 < 64) and has three different extents; 256 x 64 is the 2-D plan (the y round trip is the only middle pass)
GRIDS = [((64, 64, 64), (6.0, 6.5, 7.0)), ((128, 64, 64), (12.5, 6.0, 6.5)), ((64, 32, 128), (6.0, 3.5, 12.0)),
         ((256, 64), (25.0, 6.0))]


def _same_log(a, b):
    if len(a) != len(b):
        return False
    for ra, rb in zip(a, b):
        for k in ra:
            x, y = ra[k], rb[k]
            if not (x == y or (isinstance(x, float) and isinstance(y, float) and math.isnan(x) and math.isnan(y))):
                return False
    return True


def _run_both(ctx, fn):
    """fn() with dct_x_turnaround = 0 and = 1: (result, block log, dct_pass calls) for each"""
    out = {}
    try:
        for opt in (0, 1):
            ctx.set_option("dct_x_turnaround", opt)
            ctx.set_option("gmres_block_log", 1)
            ctx.solver_block_log()
            ctx.prof_enable(True)
            ctx.prof_reset()
            r = fn()
            calls = ctx.prof_get("dct_pass")["calls"]
            ctx.prof_enable(False)
            out[opt] = (r, ctx.solver_block_log(), calls)
    finally:
        ctx.set_option("gmres_block_log", 0)
        ctx.set_option("dct_x_turnaround", 1)
    return out


@pytest.mark.parametrize("shift", [1.0, 0.0])
@pytest.mark.parametrize("dims,ls", GRIDS)
def test_x_turnaround_solves_are_bitwise_those_of_the_five_pass_path(ctx, dims, ls, shift):
    """Every GMRES flavor that takes Pl (KrylovKit, IterativeSolvers, Krylov.jl), shifted and unshifted operators, on the
    stencil-free form: with the turnaround on, the same solution bits, flag, count, residual norm and block log as without, and the
    block logs hold chained blocks of >= 2 steps both in first (unshifted, theta0 = NaN) and -- shift-1 pairing -- in Newton-shifted
    blocks, with fewer transform passes than the five-pass path."""
    hip = _hip()
    sh = operators.SwiftHohenberg(dims, ls)
    prob = hip.SwiftHohenberg(ctx, dims, ls)
    rng = np.random.default_rng(11)
    u = sh.guess() + 0.2 * rng.standard_normal(sh.N)
    J = prob.jacobian(prob.vec(u), 0.1)
    rhs = prob.vec(rng.standard_normal(sh.N))
    P = hip.DCTPreconditioner(prob, shift)
    solvers = [("kk", hip.GMRESKrylovKit(dim=30, rtol=1e-10, atol=0.0, maxiter=40, Pl=P), (-0.7, 1.0)),
               ("is", hip.GMRESIterativeSolvers(reltol=1e-10, restart=30, maxiter=400, Pl=P), (-0.6, 1.0)),
               ("kj", hip.KrylovLS(atol=0.0, rtol=1e-10, memory=20, restart=True, itmax=400, Pl=P), (-0.6, 1.0))]
    if shift == 0.0:
        solvers.append(("kk0", hip.GMRESKrylovKit(dim=30, rtol=1e-9, atol=0.0, maxiter=40, Pl=P), (0.0, 1.0)))
    for name, ls_, (a0, a1) in solvers:
        def solve():
            x, ok, it = ls_(J, rhs, a0, a1)
            return x.numpy(), ok, it, ls_.last_resnorm
        out = _run_both(ctx, solve)
        (r0, log0, c0), (r1, log1, c1) = out[0], out[1]
        tag = (dims, shift, name)
        assert r0[1] == r1[1] and r0[2] == r1[2] and r0[3] == r1[3], (tag, r0[1:], r1[1:])
        assert np.array_equal(r0[0], r1[0]), (tag, np.abs(r0[0] - r1[0]).max())
        assert _same_log(log0, log1), tag
        first = [r for r in log1 if r["j"] == 0 and math.isnan(r["theta0"]) and r["steps"] >= 2]
        shifted = [r for r in log1 if not math.isnan(r["theta0"]) and r["steps"] >= 2]
        # (shift 0: |Pl^-1| ~ 1e4 .. 1e8 and the Newton-shifted blocks shrink to 1-2 steps -- DESIGN 3 -- so chained shifted blocks are
        # asserted on the shift-1 pairing, where every flavor has them)
        assert first and (shifted or shift == 0.0), (tag, [(r["j"], r["steps"], r["theta0"]) for r in log1])
        # one pass fewer per link of every chained block
        assert c1 < c0, (tag, c0, c1)


def test_x_turnaround_corrector_and_two_lanes_are_bitwise_unchanged(ctx):
    """A PALC corrector on a 64^3 grid (BorderingBLS: two GMRES solves per Newton step) with the turnaround on and off: the same
    residual history, counts and bits; and the two-lane bordered solve (each lane chains on its own preconditioner scratch)
    reproduces the sequential one bitwise."""
    hip = _hip()
    dims, ls = (64, 64, 64), (6.0, 6.5, 7.0)
    sh = operators.SwiftHohenberg(dims, ls)
    prob = hip.SwiftHohenberg(ctx, dims, ls, l=0.1, nu=1.2)
    rng = np.random.default_rng(5)
    u0 = sh.guess() + 0.05 * rng.standard_normal(sh.N)
    B = hip.BorderedArray
    P = hip.DCTPreconditioner(prob, 1.0)
    ls_ = hip.GMRESKrylovKit(dim=30, rtol=1e-9, atol=1e-12, maxiter=150, Pl=P)
    bls = hip.BorderingBLS(ls_, check_precision=False)
    z0 = B(prob.vec(u0), 0.1)
    tau = B(prob.vec(0.01 * rng.standard_normal(sh.N)), -1.0)
    zp = z0.copy().add_(tau, -0.001)

    def corrector():
        s = hip.newton_palc_native(prob, z0, tau, zp, -0.001, 0.5, bls, tol=1e-9, max_iterations=4, norm_inf=True)
        return s["u"].u.numpy(), s["u"].p, list(s["residuals"]), s["itlineartot"], s["itnewton"]
    out = _run_both(ctx, corrector)
    (r0, log0, c0), (r1, log1, c1) = out[0], out[1]
    assert r0[1] == r1[1] and r0[2] == r1[2] and r0[3] == r1[3] and r0[4] == r1[4], (r0[1:], r1[1:])
    assert np.array_equal(r0[0], r1[0])
    assert _same_log(log0, log1)
    assert any(r["steps"] >= 2 for r in log1) and c1 < c0, (c0, c1)

    J = prob.jacobian(prob.vec(u0), 0.1)
    n = prob.nglobal
    g = np.random.default_rng(n)
    R, dR, dz = (prob.vec(g.standard_normal(n)) for _ in range(3))
    res = {}
    try:
        for tl in (0, 1):
            ctx.set_option("two_lanes", tl)
            dX, dl, ok, it = bls(J, dR, dz, 0.3, R, 0.7, 0.5, 0.5, dotscale=1.0 / n)
            res[tl] = (dX.numpy(), dl, ok, it)
    finally:
        ctx.set_option("two_lanes", 1)
    a, b = res[0], res[1]
    assert a[2] == b[2] and a[3] == b[3], (a[2:], b[2:])
    assert a[1] == b[1] and np.array_equal(a[0], b[0])
