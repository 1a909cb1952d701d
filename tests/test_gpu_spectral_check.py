"""GPU tests of the spectral residual check (csrc/solver.hip: ShiftPrecOp::check_norm, csrc/dct.hip: ShDctPrecond::apply_nrm2,
csrc/dct_fast.hip: dct_fused_kernel NRM; option gmres_check_spectral).

A GMRES solve that converges on its Arnoldi estimate evaluates |b - Pl^-1 J x| once explicitly.  With the option at 1 (the default)
the value is |Pl^-1 (rhs - J x)| taken from the preconditioner's spectrum -- the chain's stencil pass, rhs - J x formed in the x-forward
transform, the forward transforms, sum_k sym_k^2 |.^_k|^2 in the last one -- instead of the norm of a residual vector built through the whole chain (option
0).  The value is a different summation of the same quantity; everything else a solve returns must keep its BITS.

Measured on MI355X (relative deviation of the check value from the float64 NumPy oracle, random x and rhs, the three operator
forms).  Shift 1.0: chain up to 2.2e-15, spectral up to 1.9e-15 over the grids; shift 0.0 on GRIDS_S0: 6.2e-14 and 5.6e-14.  Shift 0.0 on the four grids of GRIDS: the CHAIN
(option 0, the parent's path) sits 5.2e-12 from the oracle on 64^3, and at five times the lengths (h ~ 1) 1.4e-12 (64^3), 1.1e-11
(128 x 64 x 256), 1.1e-11 (32 x 32 x 512), 2.4e-11 (32 x 256 x 512); the spectral value 2.2e-12 resp. 1.4e-12, 1.1e-11, 1.1e-11,
2.4e-11 -- inside 4 x the chain's deviation.  With shift 0 the norm is carried by the few modes next to the critical sphere, whose
symbol 1 / (1 + sum lam)^2 loses eps |sum lam| / |1 + sum lam| to the rounding of the eigenvalue tables in ANY evaluation; with
2^18 .. 2^22 modes some lie within 1e-4 .. 1e-5 of the sphere whatever the lengths (a search over 300 length triples per grid leaves
a predicted 1.1e-12 .. 1.8e-11), so on these grids the chain itself cannot be held to 1e-12 at shift 0 and they are the wrong grids
for that condition.  It is asserted at shift 0 on GRIDS_S0 instead: the same kernel paths (runtime length, the wide tile at 256
lines, N = 512 at 16 lines per tile) on grids of 2^13 .. 2^16 modes with lengths chosen so that max |sum lam| / |1 + sum lam| <= 600,
i.e. a floor of 4e-16 x 600 = 2.4e-13.  (The non-temporal instantiations need >= 2^22 points and have no such grid; at shift 0 they are
covered by the relative bound on the listed grid.)  On GRIDS at shift 0 the relative bound alone -- spectral within 4 x the chain's
deviation -- is asserted.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from conftest import probe  # noqa: E402
from oracle import operators  # noqa: E402


def _hip():
    from bk_amd import hip
    return hip


# runtime-length kernels; three different extents (256 lines: the wide tile); N = 512 at 16 lines per tile; >= 2^22 points (NTM);
# lengths as in tests/test_gpu_dct_const_len.py (h ~ 0.2)
GRIDS = [((64, 64, 64), (6.0, 6.5, 7.0)),
         ((128, 64, 256), (12.5, 6.0, 25.0)),
         ((32, 32, 512), (3.2, 3.3, 50.0)),
         ((32, 256, 512), (3.2, 25.0, 50.0))]
# shift 0: few modes, h ~ 0.7 .. 1.5, no mode next to the critical sphere (see the module docstring)
GRIDS_S0 = [((16, 8, 64), (7.18, 5.6, 22.74)),
            ((32, 8, 256), (11.42, 4.09, 126.53)),
            ((16, 8, 512), (10.03, 2.85, 197.58))]
# (grid, lengths, shift, whether the absolute 1e-12 condition is asserted)
VALUE_CASES = ([(d, l, 1.0, True) for d, l in GRIDS] + [(d, l, 0.0, True) for d, l in GRIDS_S0] +
               [(d, l, 0.0, False) for d, l in GRIDS])
L, NU = 0.1, 1.2
KK, IS = 0, 1
# (flavor, a0, a1): KrylovKit unshifted, KrylovKit shifted (the fold form), IterativeSolvers; KrylovKit with a1 != 1, where the
# scale c = -a1 of rhs + c J x is not -1 (|v + c w| and |w + c v| differ)
FORMS = [(KK, 0.0, 1.0), (KK, -0.6, 1.0), (IS, 0.3, 1.0), (KK, 0.0, 0.7)]


@functools.lru_cache(maxsize=None)
def _case(dims, ls):
    """The oracle's side of one grid, computed once: state, vectors, J x."""
    sh = operators.SwiftHohenberg(dims, ls)
    rng = np.random.default_rng(13)
    u = sh.guess() + 0.2 * rng.standard_normal(sh.N)
    x = rng.standard_normal(sh.N)
    rhs = rng.standard_normal(sh.N)
    Jx = sh.dF(u, L, NU, x)
    return sh, u, x, rhs, Jx


def _oracle_value(Plo, x, rhs, Jx, flavor, a0, a1):
    if flavor == KK:
        return float(np.linalg.norm(Plo(rhs) - a0 * x - a1 * Plo(Jx)))
    return float(np.linalg.norm(Plo(rhs - (a0 * x + a1 * Jx))))


def _with_option(ctx, fn):
    """fn() with gmres_check_spectral = 0 and = 1"""
    out = {}
    try:
        for opt in (0, 1):
            ctx.set_option("gmres_check_spectral", opt)
            out[opt] = fn()
    finally:
        ctx.set_option("gmres_check_spectral", 1)
    return out[0], out[1]


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("dims,ls,shift,absolute", VALUE_CASES)
def test_check_value_random_vectors(ctx, dims, ls, shift, absolute):
    """O(1) residual: both paths against the NumPy oracle on the three operator forms.  The chain's own deviation is measured; the
    spectral path gets 4 x the largest of those (same number of terms, another summation order) and must stay below 1e-12 -- at
    shift 0 on the grids on which the chain itself can (module docstring)."""
    hip = _hip()
    sh, u, x, rhs, Jx = _case(dims, ls)
    Plo = operators.dct_preconditioner(dims, ls, shift)
    prob = hip.SwiftHohenberg(ctx, dims, ls, l=L, nu=NU)
    J = prob.jacobian(prob.vec(u), L)
    P = hip.DCTPreconditioner(prob, shift)
    xd, rd = prob.vec(x), prob.vec(rhs)
    dev = {0: [], 1: []}
    for flavor, a0, a1 in FORMS:
        ref = _oracle_value(Plo, x, rhs, Jx, flavor, a0, a1)
        (v0, s0), (v1, s1) = _with_option(ctx, lambda: P.check_norm(J, xd, rd, a0, a1, flavor))
        assert (s0, s1) == (False, True), (dims, shift, flavor, a0, s0, s1)
        dev[0].append(abs(v0 - ref) / ref)
        dev[1].append(abs(v1 - ref) / ref)
        # determinism: the same bits from call to call
        for opt in (0, 1):
            ctx.set_option("gmres_check_spectral", opt)
            again = P.check_norm(J, xd, rd, a0, a1, flavor)[0]
            ctx.set_option("gmres_check_spectral", 1)
            assert _bits(again) == _bits((v0, v1)[opt]), (dims, shift, flavor, a0, opt)
    chain = max(dev[0])
    print(f"spectral_check random dims={dims} shift={shift} chain={dev[0]} spectral={dev[1]}")
    if absolute:
        probe("spectral_check/random/chain", chain, 1e-12, dims=list(dims), shift=shift)
    for (flavor, a0, a1), d1 in zip(FORMS, dev[1]):
        probe("spectral_check/random/spectral", d1, min(4.0 * chain, 1e-12) if absolute else 4.0 * chain, dims=list(dims),
              shift=shift, flavor=flavor, a0=a0, chain=chain)


@pytest.mark.parametrize("shift", [1.0, 0.0])
@pytest.mark.parametrize("dims,ls", GRIDS)
def test_check_value_at_a_converged_solution(ctx, dims, ls, shift):
    """The regime of the real check: x from a converged solve (rtol 1e-9) of J x = rhs.  J is taken at l = -0.7, where
    g(u) = l + 2 nu u - 3 u^2 <= l + nu^2 / 3 < 0 makes it definite (at l = 0.1 it is indefinite on these random states and restarted
    GMRES stalls: 60 cycles did not converge on any grid).  The oracle evaluates |Pl^-1 (rhs - J x)|; the chain subtracts two nearly
    equal vectors and is the less accurate of the two: the spectral path gets 4 x the chain's own deviation."""
    hip = _hip()
    sh, u, _, rhs, _ = _case(dims, ls)
    l2 = -0.7
    Plo = operators.dct_preconditioner(dims, ls, shift)
    prob = hip.SwiftHohenberg(ctx, dims, ls, l=l2, nu=NU)
    J = prob.jacobian(prob.vec(u), l2)
    P = hip.DCTPreconditioner(prob, shift)
    rd = prob.vec(rhs)
    # (the solve itself always runs with the shift-1 preconditioner -- 17 applications on every grid; with shift 0, |Pl^-1| ~ 1e8,
    # restarted GMRES does not converge on the 2^22-point grid within 24000 applications -- the CHECK is the one of `shift`)
    gm = hip.GMRESKrylovKit(dim=30, rtol=1e-9, atol=0.0, maxiter=150, Pl=hip.DCTPreconditioner(prob, 1.0))
    xd, ok, it = gm(J, rd, 0.0, 1.0)
    print(f"spectral_check converged dims={dims} shift={shift} ok={ok} numops={it} last_resnorm={gm.last_resnorm:.6e}")
    assert ok, (dims, shift, it, gm.last_resnorm)
    x = xd.numpy()
    ref = float(np.linalg.norm(Plo(rhs - sh.dF(u, l2, NU, x))))
    (v0, s0), (v1, s1) = _with_option(ctx, lambda: P.check_norm(J, xd, rd, 0.0, 1.0, KK))
    assert (s0, s1) == (False, True)
    d0, d1 = abs(v0 - ref) / ref, abs(v1 - ref) / ref
    print(f"spectral_check converged dims={dims} shift={shift} ref={ref:.6e} chain={d0:.3e} spectral={d1:.3e}")
    probe("spectral_check/converged/spectral", d1, 4.0 * d0, dims=list(dims), shift=shift, chain=d0, check_value=ref)
    again = P.check_norm(J, xd, rd, 0.0, 1.0, KK)[0]
    assert _bits(again) == _bits(v1)


def _solve_pair(ctx, fn):
    r0, r1 = _with_option(ctx, fn)
    return r0, r1


@pytest.mark.parametrize("two_lanes", [1, 0])
@pytest.mark.parametrize("shift", [1.0, 0.0])
def test_solves_are_bitwise_untouched(ctx, shift, two_lanes):
    """A KrylovKit solve (the fold form), an IterativeSolvers solve and one PALC corrector step with BorderingBLS -- on the bench's
    cell and on a grid whose check runs the spectral path: x / u, p, the Newton residual history, flags and counts bitwise equal with
    the option at 0 and at 1; last_resnorm (the check's value) within the bound of the converged-solution test."""
    hip = _hip()
    dims, ls = GRIDS[0]
    sh, u, _, rhs, _ = _case(dims, ls)
    prob = hip.SwiftHohenberg(ctx, dims, ls, l=L, nu=NU)
    J = prob.jacobian(prob.vec(u), L)
    P = hip.DCTPreconditioner(prob, shift)
    rd = prob.vec(rhs)
    Plo = operators.dct_preconditioner(dims, ls, shift)
    try:
        ctx.set_option("two_lanes", two_lanes)
        for name, gm, (a0, a1) in [("kk", hip.GMRESKrylovKit(dim=20, rtol=1e-10, atol=0.0, maxiter=3, Pl=P), (-0.6, 1.0)),
                                   ("is", hip.GMRESIterativeSolvers(reltol=1e-10, restart=30, maxiter=400, Pl=P), (-0.6, 1.0))]:
            def solve():
                x, ok, it = gm(J, rd, a0, a1)
                return x.numpy(), ok, it, gm.last_resnorm
            r0, r1 = _solve_pair(ctx, solve)
            assert np.array_equal(_bits(r0[0]), _bits(r1[0])) and r0[1] == r1[1] and r0[2] == r1[2], (name, shift, r0[1:], r1[1:])
            # shift 1: both solves converge, i.e. their check ran and passed.  Shift 0 (|Pl^-1| ~ 1e4): the IterativeSolvers solve
            # converges (49 iterations: its check ran and passed); the KrylovKit solve ends unconverged after its three cycles
            # (GMRES(30) with 300 cycles does not converge on this state either) WITHOUT reaching a check -- that comparison only
            # says that the option changes nothing else.  The shift-0 check of the KrylovKit flavor is covered by the value tests.
            print(f"spectral_check solve {name} shift={shift} ok={r0[1]} it={r0[2]} resnorm={r0[3]:.3e} / {r1[3]:.3e}")
            assert r0[1] == (shift == 1.0 or name == "is"), (name, shift, r0[1:])
            if name == "kk" and r0[1]:
                # the reported norm IS the check's value: both within 4 x the chain's deviation from the oracle
                x = r0[0]
                ref = float(np.linalg.norm(Plo(rhs) - a0 * x - a1 * Plo(sh.dF(u, L, NU, x))))
                d0 = abs(r0[3] - ref) / ref
                probe("spectral_check/solve/last_resnorm", abs(r1[3] - ref) / ref, 4.0 * d0, shift=shift, chain=d0)
            else:
                assert r0[3] == r1[3], (name, r0[3], r1[3])       # (the estimate, resp. a failed check's chain value)

        for cdims, cls in [((64, 32, 32), (2.0 * np.pi, 2.0 * np.pi / np.sqrt(3.0), np.pi)), (dims, ls)]:
            csh = operators.SwiftHohenberg(cdims, cls)
            cprob = hip.SwiftHohenberg(ctx, cdims, cls, l=L, nu=NU)
            rng = np.random.default_rng(5)
            u0 = csh.guess() + 0.05 * rng.standard_normal(csh.N)
            B = hip.BorderedArray
            CP = hip.DCTPreconditioner(cprob, shift)
            bls = hip.BorderingBLS(hip.GMRESKrylovKit(dim=30, rtol=1e-9, atol=1e-12, maxiter=20, Pl=CP), check_precision=False)
            z0 = B(cprob.vec(u0), L)
            tau = B(cprob.vec(0.01 * rng.standard_normal(csh.N)), -1.0)
            zp = z0.copy().add_(tau, -0.001)

            def corrector():
                s = hip.newton_palc_native(cprob, z0, tau, zp, -0.001, 0.5, bls, tol=1e-9, max_iterations=1, norm_inf=True)
                return (s["u"].u.numpy(), s["u"].p, tuple(s["residuals"]), bool(s["converged"]), s["itlineartot"], s["itnewton"])
            c0, c1 = _solve_pair(ctx, corrector)
            assert np.array_equal(_bits(c0[0]), _bits(c1[0])), cdims
            assert _bits(c0[1]) == _bits(c1[1]) and np.array_equal(_bits(c0[2]), _bits(c1[2])) and c0[3:] == c1[3:], (cdims, c0[1:], c1[1:])
    finally:
        ctx.set_option("two_lanes", 1)
    # (the 64^3 grid does run the spectral path)
    assert P.check_norm(J, rd, rd, 0.0, 1.0, KK)[1]


def _trace(ctx, capfd, fn):
    """(fn(), (axis, mode) of every fused transform pass it launches) -- option dct_trace: one stderr line per fused pass"""
    capfd.readouterr()
    ctx.set_option("dct_trace", 1)
    try:
        r = fn()
    finally:
        ctx.set_option("dct_trace", 0)
    out = []
    for ln in capfd.readouterr().err.splitlines():
        if ln.startswith("dct_trace axis="):
            f = dict(kv.split("=", 1) for kv in ln.split() if "=" in kv and not kv.startswith("phases"))
            out.append((int(f["axis"]), int(f["mode"])))
    return r, out


FIVE = [(0, 0), (1, 0), (2, 2), (1, 1), (0, 1)]


def test_failing_check_falls_back(ctx, capfd):
    """A tolerance the true residual cannot reach (rtol 1e-15; 64^3, shift 1): the Arnoldi estimate passes it, the check fails at
    ~5e-13, and the solve restarts from the residual vector r = b - w of the fall-back (apply_check_resume: the chain continued from
    the stencil result the spectral check already has).  KrylovKit gets six cycles, so that the cycles after the first failed check
    start from that r and everything they produce depends on it: x, numops, the flag AND last_resnorm (the last check fails too: the
    chain's value in both runs) bitwise equal with the option at 0 and at 1, the same number of stencil launches, and the trace of
    option 1 shows norm-only passes (mode 3) each followed by the chain's five.  IterativeSolvers (three cycles): the mismatch
    counter is > 0 and equal.  (With shift 0 the estimate of these solves stalls near 1e-7: no check is reached, nothing to test.)"""
    hip = _hip()
    dims, ls = GRIDS[0]
    sh, u, _, rhs, _ = _case(dims, ls)
    prob = hip.SwiftHohenberg(ctx, dims, ls, l=L, nu=NU)
    J = prob.jacobian(prob.vec(u), L)
    P = hip.DCTPreconditioner(prob, 1.0)
    rd = prob.vec(rhs)
    for name, gm in (("kk", hip.GMRESKrylovKit(dim=30, rtol=1e-15, atol=0.0, maxiter=6, Pl=P)),
                     ("is", hip.GMRESIterativeSolvers(reltol=1e-15, restart=30, maxiter=90, Pl=P))):
        def solve():
            ctx.set_option("gmres_check_mismatch", 0)
            ctx.prof_enable(True)
            ctx.prof_reset()
            (x, ok, it), tr = _trace(ctx, capfd, lambda: gm(J, rd, -0.6, 1.0))
            jv = ctx.prof_get("jvp")["calls"]
            ctx.prof_enable(False)
            return x.numpy(), ok, it, ctx.get_option("gmres_check_mismatch"), gm.last_resnorm, jv, tr
        r0, r1 = _with_option(ctx, solve)
        n3 = [i for i, am in enumerate(r1[6]) if am == (2, 3)]
        print(f"spectral_check failing {name}: ok={r1[1]} it={r1[2]} mismatch={r1[3]} resnorm={r1[4]:.3e} stencil launches {r0[5]} / {r1[5]} "
              f"norm-only passes {len(n3)} of {len(r1[6])}")
        assert np.array_equal(_bits(r0[0]), _bits(r1[0])) and r0[1:4] == r1[1:4], (name, r0[1:6], r1[1:6])
        assert r0[5] == r1[5], (name, r0[5], r1[5])                   # the stencil runs once per check, failed or not
        assert (2, 3) not in r0[6]
        # every failed spectral check is followed by the chain's five passes (from the stencil result in place)
        failed = [i for i in n3 if i + 1 < len(r1[6])]
        assert failed and all(r1[6][i + 1:i + 6] == FIVE for i in failed), (name, n3, len(r1[6]))
        if name == "kk":
            assert len(failed) >= 2 and not r1[1], (name, n3, r1[1])      # (cycles after a failed check ran: x depends on its r)
            assert _bits(r0[4]) == _bits(r1[4]), (r0[4], r1[4])
        else:
            assert r1[3] > 0, r1[3]


def test_which_passes_ran(ctx, capfd):
    """The check of a converged solve on 64^3 (KrylovKit, shift 1): the solve's last passes are x forward, y forward and the norm-only
    pass (mode 3) -- the only one of the solve -- and no inverse pass follows; with the option at 0 it ends on the five passes of the
    chain and shows no mode 3.  The probe entry on the same solution: exactly those three, resp. (it first forms b = Pl \\ rhs) the
    five twice."""
    hip = _hip()
    dims, ls = GRIDS[0]
    sh, u, _, rhs, _ = _case(dims, ls)
    prob = hip.SwiftHohenberg(ctx, dims, ls, l=L, nu=NU)
    J = prob.jacobian(prob.vec(u), L)
    P = hip.DCTPreconditioner(prob, 1.0)
    rd = prob.vec(rhs)
    gm = hip.GMRESKrylovKit(dim=30, rtol=1e-9, atol=0.0, maxiter=40, Pl=P)
    ((x0, ok0, _), t0), ((x1, ok1, _), t1) = _with_option(ctx, lambda: _trace(ctx, capfd, lambda: gm(J, rd, -0.6, 1.0)))
    assert ok0 and ok1
    assert t1[-3:] == [(0, 0), (1, 0), (2, 3)] and t1.count((2, 3)) == 1, t1[-8:]
    assert t0[-5:] == FIVE and (2, 3) not in t0, t0[-8:]
    (_, p0), (_, p1) = _with_option(ctx, lambda: _trace(ctx, capfd, lambda: P.check_norm(J, x1, rd, -0.6, 1.0, KK)))
    assert p1 == [(0, 0), (1, 0), (2, 3)], p1
    assert p0 == FIVE + FIVE, p0


@pytest.mark.parametrize("dims,ls", [((48, 64, 64), (4.5, 6.0, 6.5)), ((48, 64), (4.5, 6.0))])
def test_declined_shapes(ctx, dims, ls):
    """A grid on the dense transforms (48 is no power of two), 3-D and 2-D: the check declines the spectral path, and the value has
    the chain's bits whatever the option says."""
    hip = _hip()
    sh = operators.SwiftHohenberg(dims, ls)
    prob = hip.SwiftHohenberg(ctx, dims, ls, l=L, nu=NU)
    rng = np.random.default_rng(3)
    u = sh.guess() + 0.2 * rng.standard_normal(sh.N)
    J = prob.jacobian(prob.vec(u), L)
    P = hip.DCTPreconditioner(prob, 1.0)
    xd, rd = prob.vec(rng.standard_normal(sh.N)), prob.vec(rng.standard_normal(sh.N))
    for flavor, a0, a1 in FORMS:
        (v0, s0), (v1, s1) = _with_option(ctx, lambda: P.check_norm(J, xd, rd, a0, a1, flavor))
        assert not s0 and not s1 and _bits(v0) == _bits(v1), (dims, flavor, a0, v0, v1)
