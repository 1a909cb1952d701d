"""CPU tests of tests/stencil_ref.py, the reference the GPU stencil tests compare with bit for bit: on grids with power-of-two mesh
widths and integer data it must equal the project's oracle (oracle/operators.py: assembled sparse matrices, L1 = A * A as a matrix
product) EXACTLY -- both are then free of rounding, whatever order the sparse products sum in -- and on random real data its
longdouble evaluation must agree with the oracle's float64 to the oracle's own rounding error.
"""
import numpy as np
import pytest

import stencil_ref as R
from oracle import operators as O

EPS = np.finfo(np.float64).eps


def ls_for(dims, hs):
    """Half-lengths l with h = 2 l / N equal to `hs`."""
    return tuple(h * n / 2.0 for n, h in zip(dims, hs))


def ints(rng, shape, m):
    return rng.integers(-m, m + 1, size=shape, dtype=np.int64)


# ------------------------------------------------------------------------------------------------ the exact arithmetic itself
def test_ex_arithmetic_and_bound():
    a = np.array([3, -5, 7], dtype=np.int64)
    e = 0.25 * R.Ex.of(a) - 1.5 + R.Ex.of(a) * R.Ex.of(a)
    assert np.array_equal(e.exact(), 0.25 * a - 1.5 + a * a)
    assert (e.sh, e.bnd) == (2, 7 + 6 + 4 * 49)              # units of 1/4: |0.25 a| <= 7, 1.5 = 6, a^2 <= 49
    assert (-e).bnd == e.bnd and np.array_equal((2.0 - e).exact(), 2.0 - e.exact())
    s = (R.Ex.of(a) * 0.5).sum()
    assert float(s.exact()) == 2.5 and s.bnd == 3 * 7
    with pytest.raises(AssertionError, match="not below 2\\^53"):
        (R.Ex.of(np.array([2 ** 30], dtype=np.int64)) * R.Ex.of(np.array([2 ** 24], dtype=np.int64))).exact()
    with pytest.raises(AssertionError, match="integer data only"):
        R.Ex.of(np.array([0.5]))


def test_data_ranges_of_the_gpu_tests_are_exact_and_need_more_than_fp32():
    """|A|_1 = |c0| + 2 (ax + ay + az) = 4.25 for ainv = (1/4, 1/16, 1): |A^2|_1 <= 18.0625.  With v in [-4096, 4096], u in [-8, 8]
    and quarter coefficients the bound stays far below 2^53 and above 2^24."""
    rng = np.random.default_rng(0)
    v, u = ints(rng, (5, 6, 7), 4096), ints(rng, (5, 6, 7), 8)
    v.flat[0], u.flat[0] = 4096, 8
    for mode in (0, 1):
        e = R.sh_apply(v, u, (0.25, 0.0625, 1.0), 0.25, 0.75, -0.5, 2.0, 0.75, mode)
        e.exact()
        assert 24 < e.bits < 53, e.bits
    A2 = R.sh_A(R.sh_A(R.Ex.of(v), (0.25, 0.0625, 1.0)), (0.25, 0.0625, 1.0))
    assert A2.bnd == int(18.0625 * 256) * 4096 and A2.sh == 8
    # the fused dot: v in [-64, 64], fewer than 2^17 points (the bound is a max-norm: a small grid of extreme values, scaled)
    vv, uu, rr = np.full((4, 4, 4), 64, dtype=np.int64), np.full((4, 4, 4), 8, dtype=np.int64), np.full((4, 4, 4), -64, dtype=np.int64)
    out, dot = R.sh_fused(vv, uu, rr, (0.25, 0.0625, 1.0), 0.25, 0.75, -0.5, 2.0, 0.75)
    assert dot.bnd // 64 * 2 ** 17 < R.LIMIT
    assert float(dot.exact()) == float((vv * out.exact()).sum())


# ------------------------------------------------------------------------------------------------ Swift-Hohenberg 2-D / 3-D
SH_GRIDS = [((5, 4, 3), (2, 4, 1)), ((7, 6, 5), (1, 2, 4)), ((2, 3, 4), (2, 4, 1)), ((3, 2, 2), (4, 1, 2)), ((4, 4, 4), (2, 2, 2)),
            ((6, 5), (2, 4)), ((2, 3), (1, 2)), ((3, 7), (4, 4))]


@pytest.mark.parametrize("dims,hs", SH_GRIDS)
def test_sh_reference_equals_the_oracle_exactly(dims, hs):
    rng = np.random.default_rng(sum(dims))
    sh = O.SwiftHohenberg(dims, ls_for(dims, hs))
    ainv = tuple(1.0 / h ** 2 for h in hs)
    shape = dims[::-1]
    v, u = ints(rng, shape, 4096), ints(rng, shape, 8)
    l, nu = 0.25, 0.75
    F = R.sh_apply(u, None, ainv, l, nu, 0.0, 1.0, mode=1).exact()
    assert np.array_equal(F.ravel(), sh.F(u.ravel().astype(float), l, nu))
    J = R.sh_apply(v, u, ainv, l, nu, 0.0, 1.0, mode=0).exact()
    assert np.array_equal(J.ravel(), sh.dF(u.ravel().astype(float), l, nu, v.ravel().astype(float)))
    # the scalings the kernels fuse: a0, a1 and the separately scaled pointwise part
    a0, a1, ag = -0.5, 2.0, 0.75
    g = l + 2 * nu * u - 3.0 * u * u
    want = a0 * v.ravel() + a1 * -(sh.L1 @ v.ravel().astype(float)) + ag * (g * v).ravel()
    assert np.array_equal(R.sh_apply(v, u, ainv, l, nu, a0, a1, ag, 0).exact().ravel(), want)


@pytest.mark.parametrize("dims", [(7, 5, 4), (9, 6), (2, 3, 2)])
def test_sh_longdouble_evaluation_agrees_with_the_oracle(dims):
    rng = np.random.default_rng(len(dims))
    ls = (np.pi, 2.0, 1.3)[:len(dims)]
    sh = O.SwiftHohenberg(dims, ls)
    ainv = tuple((n / (2.0 * l)) ** 2 for n, l in zip(dims, ls))
    ainv_l = tuple(np.longdouble(a) for a in ainv)
    shape = dims[::-1]
    v, u = rng.standard_normal(shape), rng.standard_normal(shape)
    for mode in (0, 1):
        ref = R.sh_apply(v.astype(np.longdouble), u.astype(np.longdouble), ainv_l, 0.1, 1.2, 0.0, 1.0, mode=mode)
        got = sh.dF(u.ravel(), 0.1, 1.2, v.ravel()) if mode == 0 else sh.F(v.ravel(), 0.1, 1.2)
        bound = 64 * EPS * R.sh_abs(v, u, ainv, 0.1, 1.2, 0.0, 1.0, mode=mode)
        assert np.all(np.abs(got - ref.ravel().astype(np.float64)) <= bound.ravel())
        assert np.abs(got).max() > 1e3 * bound.max()           # the bound is far below the values: it can fail


# ------------------------------------------------------------------------------------------------ Swift-Hohenberg 1-D
@pytest.mark.parametrize("n,h", [(2, 2), (3, 1), (4, 4), (5, 2), (16, 1), (33, 2)])
def test_sh1d_reference_equals_the_oracle_exactly(n, h):
    rng = np.random.default_rng(n)
    o = O.SwiftHohenberg1D(n, h * n / 2.0)
    v, u, w = ints(rng, n, 4096), ints(rng, n, 8), ints(rng, n, 128)
    ax, lam, nu = 1.0 / h ** 2, -0.25, 2.0
    assert np.array_equal(R.sh1d_apply(w, None, ax, lam, nu, 0.0, 1.0, 1).exact(), o.F(w.astype(float), lam, nu))
    assert np.array_equal(R.sh1d_apply(v, u, ax, lam, nu, 0.0, 1.0, 0).exact(), o.dF(u.astype(float), lam, nu, v.astype(float)))


def test_sh1d_longdouble_evaluation_agrees_with_the_oracle():
    rng = np.random.default_rng(1)
    n, l = 41, 6.0
    o = O.SwiftHohenberg1D(n, l)
    ax = (n / (2.0 * l)) ** 2
    v, u = rng.standard_normal(n), rng.standard_normal(n)
    for mode in (0, 1):
        ref = R.sh1d_apply(v.astype(np.longdouble), u.astype(np.longdouble), np.longdouble(ax), -0.1, 2.0, 0.0, 1.0, mode)
        got = o.dF(u, -0.1, 2.0, v) if mode == 0 else o.F(v, -0.1, 2.0)
        assert np.all(np.abs(got - ref.astype(np.float64)) <= 64 * EPS * R.sh1d_abs(v, u, ax, -0.1, 2.0, 0.0, 1.0, mode))


# ------------------------------------------------------------------------------------------------ cGL 2-D
CGL_P = dict(r=0.5, mu=0.25, nu=1.0, c3=-1.0, c5=0.75, gamma=0.25)


@pytest.mark.parametrize("dims,hs", [((2, 2), (2, 1)), ((3, 2), (1, 4)), ((6, 5), (2, 4)), ((5, 7), (1, 2))])
def test_cgl_reference_equals_the_oracle_exactly(dims, hs):
    rng = np.random.default_rng(sum(dims))
    o = O.CGL2d(dims, ls_for(dims, hs))
    ainv = tuple(1.0 / h ** 2 for h in hs)
    shape = (2,) + dims[::-1]
    v, u = ints(rng, shape, 4096), ints(rng, shape, 4)
    p = tuple(CGL_P.values())
    uf, vf = u.ravel().astype(float), v.ravel().astype(float)
    assert np.array_equal(R.cgl_apply(u, None, ainv, *p, 0.0, 1.0, 1).exact().ravel(), o.F(uf, **CGL_P))
    assert np.array_equal(R.cgl_apply(v, u, ainv, *p, 0.0, 1.0, 0).exact().ravel(), o.dF(uf, vf, **CGL_P))
    JT = o.J(uf, **CGL_P).T.tocsr()
    adj = R.cgl_apply(v, u, ainv, *p, 0.0, 1.0, 2).exact().ravel()
    assert np.array_equal(adj, JT @ vf)
    assert not np.array_equal(adj, o.dF(uf, vf, **CGL_P))


def test_cgl_longdouble_evaluation_agrees_with_the_oracle():
    rng = np.random.default_rng(2)
    dims, ls = (9, 7), (np.pi, 2.0)
    o = O.CGL2d(dims, ls)
    ainv = tuple((n / (2.0 * l)) ** 2 for n, l in zip(dims, ls))
    v, u = rng.standard_normal((2, 7, 9)), rng.standard_normal((2, 7, 9))
    p = tuple(CGL_P.values())
    for mode in (0, 1, 2):
        ref = R.cgl_apply(v.astype(np.longdouble), u.astype(np.longdouble), tuple(np.longdouble(a) for a in ainv), *p, 0.0, 1.0, mode)
        got = {0: lambda: o.dF(u.ravel(), v.ravel(), **CGL_P), 1: lambda: o.F(v.ravel(), **CGL_P),
               2: lambda: o.J(u.ravel(), **CGL_P).T @ v.ravel()}[mode]()
        bound = 64 * EPS * R.cgl_abs(v, u, ainv, *p, 0.0, 1.0, mode)
        assert np.all(np.abs(got - ref.ravel().astype(np.float64)) <= bound.ravel())


# ------------------------------------------------------------------------------------------------ dF/dparam
@pytest.mark.parametrize("pde,ipar", R.DPARAM_CASES)
def test_dparam_reference_is_the_parameter_derivative_of_the_oracle(pde, ipar):
    """Every parameter enters the oracle's F linearly: F(p + 1) - F(p) is the derivative, exactly on integer data."""
    rng = np.random.default_rng(10 * pde + ipar)
    if pde == R.PDE_CGL2D:
        dims = (5, 4)
        o = O.CGL2d(dims, ls_for(dims, (2, 1)))
        u = ints(rng, (2, 20), 4)
        names = list(CGL_P)
        p1 = dict(CGL_P, **{names[ipar]: CGL_P[names[ipar]] + 1.0})
        want = o.F(u.ravel().astype(float), **p1) - o.F(u.ravel().astype(float), **CGL_P)
    elif pde == R.PDE_SH:
        o = O.SwiftHohenberg((5, 4), ls_for((5, 4), (2, 1)))
        u = ints(rng, 20, 8)
        p = [0.25, 0.75]
        q = list(p)
        q[ipar] += 1.0
        want = o.F(u.astype(float), *q) - o.F(u.astype(float), *p)
    else:
        o = O.SwiftHohenberg1D(20, 20.0)
        u = ints(rng, 20, 8)
        p = [0.25, 0.75]
        q = list(p)
        q[ipar] += 1.0
        want = o.F(u.astype(float), *q) - o.F(u.astype(float), *p)
    assert np.array_equal(R.dparam(pde, ipar, 0.5, u).exact().ravel(), 0.5 * want)
