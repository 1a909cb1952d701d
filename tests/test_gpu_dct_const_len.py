"""GPU tests of the compile-time-length transform kernels (csrc/dct_fast.hip: dct_fused_kernel<..., CN = 512>, option dct_const_len).

At N = 512 with 16 lines per tile -- the tiling of the 512^3 product path -- the z round trip (with and without the spectral dot, NTM
on and off) runs an instantiation in which the transform length, the tile height and the axis are template constants.  Only the index
arithmetic changes, and every result must have the same BITS with the option at 0 (runtime length) and at 1 (the default).  The file
compiles with FMA contraction on, so this equality rests on the compiler contracting the same products in both instantiations: these
tests are what establishes it.  Every other pass runs the runtime-length kernels under both settings (test_const_len_kernel_choice).

The grids put a 512 line on the z axis and stay small; the one of >= 2^22 points runs the non-temporal (NTM) instantiations.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import operators  # noqa: E402  (the problem's initial guess only)


def _hip():
    from bk_amd import hip
    return hip


# (dims, lengths, which passes run at the compile-time length)
GRIDS = [((32, 32, 512), (3.2, 3.3, 50.0), "z"),          # z round trip, with and without DOT
         ((32, 256, 512), (3.2, 25.0, 50.0), "z NTM")]


def _both(ctx, fn):
    """fn() with dct_const_len = 0 and = 1"""
    out = {}
    try:
        for opt in (0, 1):
            ctx.set_option("dct_const_len", opt)
            out[opt] = fn()
    finally:
        ctx.set_option("dct_const_len", 1)
    return out[0], out[1]


def _same(a, b, tag):
    assert len(a) == len(b), tag
    for x, y in zip(a, b):
        if isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and np.array_equal(x.view(np.uint64), y.view(np.uint64)), (tag, np.abs(x - y).max())
        else:
            assert x == y or (x != x and y != y), (tag, x, y)


@pytest.mark.parametrize("shift", [1.0, 0.0])
@pytest.mark.parametrize("dims,ls,which", GRIDS)
def test_const_len_is_bitwise_the_runtime_length(ctx, dims, ls, which, shift):
    """Pl \\ v, the preconditioned operator a0 v + a1 Pl \\ (J v), a GMRES solve and a MINRES solve (the z round trip with the spectral
    dot): the same bits, counts and residual norms."""
    hip = _hip()
    sh = operators.SwiftHohenberg(dims, ls)
    prob = hip.SwiftHohenberg(ctx, dims, ls)
    rng = np.random.default_rng(7)
    u = sh.guess() + 0.2 * rng.standard_normal(sh.N)
    J = prob.jacobian(prob.vec(u), 0.1)
    v = prob.vec(rng.standard_normal(sh.N))
    P = hip.DCTPreconditioner(prob, shift)
    gm = hip.GMRESKrylovKit(dim=20, rtol=1e-10, atol=0.0, maxiter=3, Pl=P)
    mr = hip.KrylovLSSymmetric(KrylovAlg="minres", atol=0.0, rtol=1e-10, itmax=60, Pl=P)

    def run():
        pv = P.ldiv(v).numpy()
        lv, sf = P.linmap(J, v, -0.7, 1.0)
        x, ok, it = gm(J, v, -0.6, 1.0)
        y, ok2, it2 = mr(J, v, 0.3, 1.0)
        return pv, lv.numpy(), sf, x.numpy(), ok, it, gm.last_resnorm, y.numpy(), ok2, it2, mr.last_resnorm
    r0, r1 = _both(ctx, run)
    _same(r0, r1, (dims, which, shift))
    assert np.isfinite(r1[0]).all() and np.abs(r1[0]).max() > 0


def _trace_const_len(ctx, capfd, prob, P, v):
    """const_len value of every fused pass of one Pl \\ v (option dct_trace: one stderr line per fused pass)"""
    capfd.readouterr()
    ctx.set_option("dct_trace", 1)
    try:
        P.ldiv(v)                      # (the trace path synchronizes the stream after every fused pass)
    finally:
        ctx.set_option("dct_trace", 0)
    err = capfd.readouterr().err
    lines = [ln for ln in err.splitlines() if ln.startswith("dct_trace axis=")]
    out = []
    for ln in lines:
        f = dict(kv.split("=", 1) for kv in ln.split() if "=" in kv and not kv.startswith("phases"))
        out.append((int(f["axis"]), int(f["mode"]), int(f["const_len"])))
    return out


@pytest.mark.parametrize("dims,ls,expect", [
    ((32, 32, 512), (3.2, 3.3, 50.0), {(2, 2): 512}),
    # y and x passes at N = 512: runtime length
    ((32, 512, 16), (3.2, 50.0, 1.7), {(1, 0): 0, (1, 1): 0}),
    ((512, 16, 16), (50.0, 1.6, 1.7), {(0, 0): 0, (0, 1): 0}),
    # 256 lines: the wide tile (LT = 32) and the runtime-length kernels
    ((32, 32, 256), (3.2, 3.3, 25.0), {(2, 2): 0}),
    ((64, 256, 64), (6.0, 25.0, 6.0), {(0, 0): 0, (1, 0): 0, (2, 2): 0, (1, 1): 0, (0, 1): 0}),
    # 512 lines on a tile of fewer than 16 lines (n0 = 8): the runtime-length kernel
    ((8, 8, 512), (0.8, 0.8, 50.0), {})])
def test_const_len_kernel_choice(ctx, capfd, dims, ls, expect):
    """The compile-time-length kernel runs exactly for the z round trip where N = 512 and LT = 16 (and not with the option at 0); every
    other pass takes the runtime-length fallback."""
    hip = _hip()
    prob = hip.SwiftHohenberg(ctx, dims, ls)
    P = hip.DCTPreconditioner(prob, 1.0)
    v = prob.vec(np.random.default_rng(3).standard_normal(int(np.prod(dims))))
    seen = _trace_const_len(ctx, capfd, prob, P, v)
    got = {(a, m): c for a, m, c in seen}
    for key, cl in expect.items():
        assert got.get(key) == cl, (dims, key, seen)
    assert all(c in (0, 512) for _, _, c in seen) and all(c == 0 or (dims[a] == 512 and a == 2) for a, _, c in seen), seen
    try:
        ctx.set_option("dct_const_len", 0)
        seen0 = _trace_const_len(ctx, capfd, prob, P, v)
    finally:
        ctx.set_option("dct_const_len", 1)
    assert [(a, m) for a, m, _ in seen0] == [(a, m) for a, m, _ in seen] and all(c == 0 for _, _, c in seen0), seen0


def test_const_len_gmres_and_corrector_at_512_cubed(ctx):
    """The product shape: the preconditioned operator through bk_precond_op_apply, a 30-step GMRES solve and one PALC corrector step
    (BorderingBLS, two GMRES solves) at 512^3, with the option at 0 and at 1: the same bits."""
    hip = _hip()
    dims = (512, 512, 512)
    ls = (8 * 2 * np.pi / np.sqrt(3.0),) * 3
    prob = hip.SwiftHohenberg(ctx, dims, ls, l=0.1, nu=1.2)
    n = prob.nglobal
    g = np.random.default_rng(2)
    u0 = prob.vec(0.1 * g.standard_normal(n))
    v = prob.vec(g.standard_normal(n))
    J = prob.jacobian(u0, 0.1)
    P = hip.DCTPreconditioner(prob, 1.0)
    gm = hip.GMRESKrylovKit(dim=30, rtol=1e-12, atol=0.0, maxiter=1, Pl=P)
    B = hip.BorderedArray
    bls = hip.BorderingBLS(hip.GMRESKrylovKit(dim=30, rtol=1e-9, atol=1e-12, maxiter=2, Pl=P), check_precision=False)
    z0 = B(u0, 0.1)
    tau = B(prob.vec(0.01 * g.standard_normal(n)), -1.0)
    zp = z0.copy().add_(tau, -0.001)

    def run():
        lv, sf = P.linmap(J, v, -0.7, 1.0)
        x, ok, it = gm(J, v, -0.6, 1.0)
        s = hip.newton_palc_native(prob, z0, tau, zp, -0.001, 0.5, bls, tol=1e-9, max_iterations=1, norm_inf=True)
        return (lv.numpy(), sf, x.numpy(), ok, it, gm.last_resnorm, s["u"].u.numpy(), s["u"].p, tuple(s["residuals"]),
                s["itlineartot"], s["itnewton"])
    r0, r1 = _both(ctx, run)
    _same(r0, r1, "512^3")
    assert r1[1] and r1[4] >= 1
