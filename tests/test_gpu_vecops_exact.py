"""The Krylov vector kernels of ``csrc/vecops.hip``, called launcher by launcher (``tests/vecops_abi.py``) and compared with plain
host references that do not touch the GPU.

Two kinds of reference:
* integer-exact data (entries in [-32, 127], coefficients in [-4, 4], powers of two as scales): every product and every partial
  sum is an integer below 2^53, so ANY summation order gives the exact value and the assertions are bitwise against int64 numpy.
  The sums reach 10^8 and more (above 2^24): an accumulator that became fp32 is caught as well.
* random real data against np.longdouble (64-bit mantissa), with the bounds derived next to each use.

Every device operand sits between guards of G doubles, and the padding between n and ldv is NaN: a NaN in a result shows an
over-read, a changed guard bit an over-write.  COVERAGE (checked by test_vecops_coverage_host.py) maps every kernel launch
expression of vecops.hip to the tests that reach it.
"""
import contextlib
import ctypes as C
import math

import numpy as np
import pytest
import torch

from vecops_abi import K_MAX_BASIS, SSTEP_KR, SSTEP_KS, SSTEP_KTRI, Launchers, sstep_tri

pytestmark = pytest.mark.gpu

G = 64                                   # guard doubles before and after every operand
NAN_BITS = 0x7FF8000000000000            # torch.full(nan)
BIG = 1 << 22                            # nt_hint threshold (vecops.hip: nt_hint)
U = 2.0 ** -53                           # unit roundoff of fp64
assert np.finfo(np.longdouble).eps < 1e-18, "the longdouble references need a 64-bit mantissa (x86-64)"

# option defaults of the product path (vecops.hip, DESIGN appendix): every test restores them
DEFAULTS = dict(nt_hint=1, krylov_burst=1, dot_burst=0, dot_variant=1, axpy_variant=3, axpy_nt=1, vec_xcd_map=1,
                axpy_stagger=0, block_dots_nr5=1)

# vector lengths: tiny, odd (scalar tail on block 0 / thread 0), the ragged end of stream_loop (n / 2 = j * 256 * U +- 1 for U = 2,
# 4, 8: 3073 = 3 * 1024 + 1 = 6 * 512 + 1 = 2048 + 1025, 4095 = 4 * 1024 - 1), and sums above 2^24 (65537)
N_SMALL = [1, 2, 3, 255, 6146, 8191, 65537]
N_BIG = [BIG - 2, BIG + 1, BIG + 2 * 4097]     # around nt_hint; n / 2 = 2^21 + 4097 splits into uneven eighths (XCD map)
NB_MAX, NB_VEC = BIG + 2 * 4097, 34            # the big basis: 34 vectors of up to NB_MAX entries (1.1 GB)
K_BUCKETS = [1, 4, 5, 8, 9, 16, 17, 24, 25, 32, 33, 48, 49, 63, 64]


# ------------------------------------------------------------------------------------------------ plumbing
@pytest.fixture(scope="module")
def vc():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    from bk_amd import hip
    c = hip.Context(0)
    yield c, Launchers(c.lib)
    c.close()


@contextlib.contextmanager
def options(c, **kv):
    for k, v in kv.items():
        c.set_option(k, v)
    try:
        yield
    finally:
        for k in kv:
            c.set_option(k, DEFAULTS[k])


def hptr(a):
    return C.c_void_p(a.ctypes.data)


def ld_for(n, layout):
    """Leading dimension: even for the 16-byte path, odd (with the base one double off) for the scalar path; >= 1 padding."""
    return n + 2 - (n & 1) if layout == "vec" else n + 1 + (n & 1)


class Dev:
    """nvec device vectors of leading dimension ld, `off` doubles past a 16-byte boundary, NaN guards and NaN padding."""

    def __init__(self, nvec, ld, off=0):
        self.nvec, self.ld, self.off = nvec, ld, off
        self.t = torch.full((2 * G + off + nvec * ld,), float("nan"), dtype=torch.float64, device="cuda")
        self.base = G + off
        self.rows, self.n = 0, 0

    @classmethod
    def of(cls, A, layout="vec", nvec=None, ld=None):
        A = np.atleast_2d(A)
        d = cls(nvec or A.shape[0], ld or ld_for(A.shape[1], layout), 0 if layout == "vec" else 1)
        d.set(torch.from_numpy(np.ascontiguousarray(A)))
        return d

    def body(self):
        return self.t[self.base:self.base + self.nvec * self.ld].view(self.nvec, self.ld)

    def set(self, A):
        """Rows [0, r) x [0, n) = A (any dtype, host or device); everything else NaN."""
        r, n = A.shape
        self.t.fill_(float("nan"))
        self.body()[:r, :n] = A.to("cuda").to(torch.float64)
        self.rows, self.n = r, n

    def p(self, j=0):
        return C.c_void_p(self.t.data_ptr() + 8 * (self.base + j * self.ld))

    def get(self, rows=None):
        torch.cuda.synchronize()
        r = self.rows if rows is None else rows
        return self.body()[:r, :self.n].cpu().numpy()

    def check(self, rows=None):
        """Every double outside rows [0, r) x [0, n) still carries the NaN bits of the fill."""
        torch.cuda.synchronize()
        r = self.rows if rows is None else rows
        bits = self.t.view(torch.int64)
        body = bits[self.base:self.base + self.nvec * self.ld].view(self.nvec, self.ld)
        parts = [bits[:self.base], bits[self.base + self.nvec * self.ld:], body[:, self.n:], body[r:, :self.n]]
        for i, q in enumerate(parts):
            assert bool((q == NAN_BITS).all()), f"guard / padding region {i} was written"


class HostOut:
    """Host output array of m doubles between NaN guards."""

    def __init__(self, m):
        self.a = np.full(2 * G + m, np.nan)
        self.m = m

    def p(self):
        return C.c_void_p(self.a.ctypes.data + 8 * G)

    @property
    def v(self):
        return self.a[G:G + self.m]

    def check(self):
        g = np.concatenate([self.a[:G], self.a[G + self.m:]]).view(np.int64)
        assert np.all(g == np.array(np.nan).view(np.int64)), "host guard written"


def ints(rng, shape, lo=-32, hi=128):
    return rng.integers(lo, hi, size=shape, dtype=np.int64)


def exact(x):
    """int64 (< 2^53) -> the float64 it is exactly."""
    x = np.asarray(x)
    assert np.all(np.abs(x) < 2 ** 53)
    return x.astype(np.float64)


def ok(st, c, what):
    assert st == 0, (what, st)


def red_depth(n, grid_cap=1024):
    """Longest chain of roundings in a stage-1 + stage-2 reduction of n products (vecops.hip): each lane accumulates
    ceil(n / (256 * grid)) products with one fma each (the smallest grid any launcher picks for n is min(ceil(n / 512), 512)),
    then 6 wave-shuffle levels and 2 workgroup levels, then stage 2 (context.hip): ceil(grid / 256) per thread, 6 + 2 levels."""
    g = max(1, min(-(-n // 512), 512))
    return -(-n // (256 * g)) + 8 + -(-grid_cap // 256) + 8


def bound_red(n, absterms):
    """|fl(sum) - sum| <= depth * u * sum |terms| (1 + O(depth u)): each level adds at most u times a partial sum whose
    magnitude is below sum |terms|; factor 2 covers the O(depth u) term and the final conversion."""
    return 2 * red_depth(n) * U * absterms


# ------------------------------------------------------------------------------------------------ BLAS-1, exact
@pytest.mark.parametrize("layout", ["vec", "scalar"])
@pytest.mark.parametrize("n", N_SMALL + N_BIG)
def test_blas1_exact(vc, n, layout):
    c, L = vc
    rng = np.random.default_rng(n + (layout == "vec"))
    X = ints(rng, (4, n))
    x, y, z = X[0], X[1], X[2]
    d = Dev.of(X[:3], layout, nvec=4)
    h = d.p
    out = HostOut(2)
    ok(L.v_dot(c.h, n, h(0), h(1), out.p()), c, "dot")
    assert out.v[0] == exact(x @ y)
    ok(L.v_dot2(c.h, n, h(0), h(1), h(2), out.p()), c, "dot2")
    assert out.v[0] == exact(x @ y) and out.v[1] == exact(x @ z)
    ok(L.v_nrm2(c.h, n, h(0), out.p()), c, "nrm2")
    assert out.v[0] == np.sqrt(exact(x @ x))                 # IEEE sqrt is correctly rounded
    ok(L.v_diff_nrm2(c.h, n, h(0), h(1), out.p()), c, "diff_nrm2")
    assert out.v[0] == np.sqrt(exact((x - y) @ (x - y)))
    ok(L.v_nrminf(c.h, n, h(1), out.p()), c, "nrminf")
    assert out.v[0] == np.abs(y).max()
    out.check()
    d.check(rows=3)
    # z = a x + b y (x, y, z distinct; z == x; z == y; x absent), pointwise scale (z == x)
    ok(L.v_axpbyz(c.h, n, 2.0, h(0), -3.0, h(1), h(3)), c, "axpbyz")
    assert np.array_equal(d.get(4)[3], exact(2 * x - 3 * y))
    d.check(rows=4)
    ok(L.v_axpbyz(c.h, n, 0.5, h(0), 4.0, h(1), h(0)), c, "axpbyz z == x")
    assert np.array_equal(d.get(1)[0], 0.5 * x + 4.0 * y)
    ok(L.v_axpbyz(c.h, n, 0.0, None, -2.0, h(1), h(1)), c, "axpbyz z == y, no x")
    assert np.array_equal(d.get(2)[1], exact(-2 * y))
    ok(L.v_pw_scale(c.h, n, h(2), h(1), 3.0, -2.0, 1.0, h(2)), c, "pw_scale z == x")
    yy = -2 * y
    assert np.array_equal(d.get(3)[2], exact(z * (3 + yy * (-2 + yy))))
    d.check(rows=4)


@pytest.mark.parametrize("has_r", [False, True])
@pytest.mark.parametrize("layout", ["vec", "scalar"])
@pytest.mark.parametrize("n", [1, 3, 255, 5122, 65537, BIG + 1])
def test_axpy_dot_exact(vc, n, layout, has_r):
    c, L = vc
    rng = np.random.default_rng(7 * n)
    r, y, z = ints(rng, (3, n))
    d = Dev.of(np.stack([r, y, z]), layout)
    out = HostOut(1)
    ok(L.v_axpy_dot(c.h, n, -4.0, d.p(0) if has_r else None, d.p(1), d.p(2), out.p()), c, "axpy_dot")
    yn = y - 4 * r if has_r else y
    assert out.v[0] == exact(z @ yn)
    assert np.array_equal(d.get()[1], exact(yn))
    d.check()
    out.check()


@pytest.mark.parametrize("layout", ["vec", "scalar"])
@pytest.mark.parametrize("n", [1, 2, 3, 255, 5122, 65537, BIG - 2, BIG + 1])
def test_minres_updates_exact(vc, n, layout):
    c, L = vc
    rng = np.random.default_rng(11 * n)
    za, zb, m2, m1, x = ints(rng, (5, n))
    cza, c1a, c2a, czb, c1b, c2b, phia, phib = 2.0, -1.0, 3.0, -2.0, 1.0, 0.5, 0.25, -1.0
    wa_ = cza * za + c1a * m2 + c2a * m1
    wb_ = czb * zb + c1b * m1 + c2b * wa_
    x1_ = x + phia * wa_
    x2_ = x1_ + phib * wb_
    # single update: w <- cz z + c1 w1 + c2 w2 ; x <- x + phi w
    d = Dev.of(np.stack([za, m2, m1, x]), layout, nvec=5)
    ok(L.v_minres_update(c.h, n, cza, d.p(0), c1a, d.p(1), c2a, d.p(2), d.p(4), phia, d.p(3)), c, "minres_update")
    g = d.get(5)
    assert np.array_equal(g[4], wa_) and np.array_equal(g[3], x1_)
    d.check(rows=5)
    # the fused pair; wb aliases m2
    d = Dev.of(np.stack([za, zb, m2, m1, x]), layout, nvec=6)
    st = L.v_minres_update2(c.h, n, cza, d.p(0), c1a, c2a, czb, d.p(1), c1b, c2b, d.p(2), d.p(3), d.p(5), d.p(2), phia, phib, d.p(4))
    if n & 1 or layout != "vec":
        assert st == 1                                     # not covered: the caller takes two single updates
        assert np.array_equal(d.get()[2], exact(m2)) and np.array_equal(d.get()[4], exact(x))
        d.check(rows=5)
        return
    assert st == 0
    g = d.get(6)
    assert np.array_equal(g[5], wa_) and np.array_equal(g[2], wb_) and np.array_equal(g[4], x2_)
    d.check(rows=6)


@pytest.mark.parametrize("n", [2, 6146, 65536, BIG + 2])
def test_minres_update2_equals_two_updates(vc, n):
    """On random real data the fused pair performs the fma sequence of two single updates, element for element."""
    c, L = vc
    rng = np.random.default_rng(n)
    Z = rng.standard_normal((5, n))
    s = rng.standard_normal(8)
    a = Dev.of(Z, "vec", nvec=7)        # za zb m2 m1 x | wa wb
    ok(L.v_minres_update(c.h, n, s[0], a.p(0), s[1], a.p(2), s[2], a.p(3), a.p(5), s[6], a.p(4)), c, "u1")
    ok(L.v_minres_update(c.h, n, s[3], a.p(1), s[4], a.p(3), s[5], a.p(5), a.p(6), s[7], a.p(4)), c, "u2")
    b = Dev.of(Z, "vec", nvec=6)        # za zb m2 m1 x | wa ; wb -> m2
    ok(L.v_minres_update2(c.h, n, s[0], b.p(0), s[1], s[2], s[3], b.p(1), s[4], s[5], b.p(2), b.p(3), b.p(5), b.p(2), s[6], s[7], b.p(4)),
       c, "u12")
    ga, gb = a.get(7), b.get(6)
    assert np.array_equal(ga[5], gb[5]) and np.array_equal(ga[6], gb[2]) and np.array_equal(ga[4], gb[4])


# ------------------------------------------------------------------------------------------------ BLAS-1, random real data
@pytest.mark.parametrize("n", [255, 65537, BIG + 1])
def test_blas1_longdouble(vc, n):
    c, L = vc
    rng = np.random.default_rng(3 * n)
    X = rng.standard_normal((3, n))
    x, y, z = X.astype(np.longdouble)
    d = Dev.of(X, "vec")
    out = HostOut(2)
    ok(L.v_dot2(c.h, n, d.p(0), d.p(1), d.p(2), out.p()), c, "dot2")
    assert abs(out.v[0] - np.dot(x, y)) <= bound_red(n, np.dot(abs(x), abs(y)))
    assert abs(out.v[1] - np.dot(x, z)) <= bound_red(n, np.dot(abs(x), abs(z)))
    ok(L.v_nrm2(c.h, n, d.p(0), out.p()), c, "nrm2")
    ref = np.sqrt(np.dot(x, x))                              # sqrt halves the relative error of the sum, plus one rounding
    assert abs(out.v[0] - ref) <= (red_depth(n) + 1) * U * ref
    ok(L.v_diff_nrm2(c.h, n, d.p(0), d.p(1), out.p()), c, "diff_nrm2")
    ref = np.sqrt(np.dot(x - y, x - y))                      # each difference is rounded once: + u relative per term
    assert abs(out.v[0] - ref) <= (red_depth(n) + 2) * U * ref
    # determinism: the same call gives the same bits
    outs = set()
    for _ in range(3):
        ok(L.v_dot(c.h, n, d.p(0), d.p(1), out.p()), c, "dot")
        outs.add(out.v[0].tobytes())
    assert len(outs) == 1


# ------------------------------------------------------------------------------------------------ multidot / multiaxpy, small n
def check_multidot(c, L, Vd, w_d, V, w, k, n):
    out = HostOut(k + 1)
    ok(L.v_multidot(c.h, n, Vd.p(0), Vd.ld, k, w_d.p(0), out.p()), c, "multidot")
    ref = np.array([int(V[j] @ w) for j in range(k)] + [int(w @ w)])
    assert np.array_equal(out.v, exact(ref)), np.nonzero(out.v != exact(ref))
    out.check()


def check_multiaxpy(c, L, Vd, src_d, V, src, k, n, coef, scale, want_norm, alias, dst_d=None):
    """dst = scale * (src + sum_j c_j V_j), |dst|^2: exact.  alias: dst = src."""
    cc = np.array(coef, dtype=np.float64)
    nn = HostOut(1)
    dst = src_d if alias else dst_d
    ok(L.v_multiaxpy(c.h, n, Vd.p(0), Vd.ld, k, hptr(cc), src_d.p(0) if src is not None else None, scale, dst.p(0),
                     nn.p() if want_norm else None), c, "multiaxpy")
    acc = np.zeros(n, dtype=np.int64) if src is None else src.copy()
    for j in range(k):
        acc += int(coef[j]) * V[j]
    ref = exact(acc) * scale
    got = dst.get()[0]
    assert np.array_equal(got, ref), np.nonzero(got != ref)[0][:10]
    if want_norm:
        assert nn.v[0] == exact(int(acc @ acc)) * scale * scale
    else:
        assert np.isnan(nn.v[0])                              # not written
    nn.check()
    dst.check()


@pytest.mark.parametrize("k", K_BUCKETS)
@pytest.mark.parametrize("n,layout", [(1, "vec"), (3, "scalar"), (255, "vec"), (6146, "vec"), (8191, "scalar"), (65537, "vec")])
def test_multidot_multiaxpy_exact(vc, n, layout, k):
    c, L = vc
    rng = np.random.default_rng(100 * k + n)
    V = ints(rng, (k, n))
    w = ints(rng, n)
    coef = rng.integers(-4, 5, k)
    Vd = Dev.of(V, layout)
    wd = Dev.of(w, layout)
    check_multidot(c, L, Vd, wd, V, w, k, n)
    dd = Dev(1, ld_for(n, layout), 0 if layout == "vec" else 1)
    dd.n, dd.rows = n, 1
    check_multiaxpy(c, L, Vd, wd, V, w, k, n, coef, 0.5, True, False, dd)
    check_multiaxpy(c, L, Vd, wd, V, None, k, n, coef, 1.0, False, False, dd)
    if layout == "vec":
        with options(c, axpy_nt=0):
            check_multiaxpy(c, L, Vd, wd, V, w, k, n, coef, 0.25, True, False, dd)
    check_multiaxpy(c, L, Vd, wd, V, w, k, n, coef, 2.0, True, True)         # dst == src (last: overwrites w)
    Vd.check()


def test_multidot_multiaxpy_reject_bad_k(vc):
    c, L = vc
    Vd, wd = Dev.of(np.ones((2, 8)), "vec"), Dev.of(np.ones(8), "vec")
    out = HostOut(K_MAX_BASIS + 2)
    assert L.v_multidot(c.h, 8, Vd.p(0), Vd.ld, K_MAX_BASIS + 1, wd.p(0), out.p()) != 0
    cc = np.zeros(K_MAX_BASIS + 1)
    assert L.v_multiaxpy(c.h, 8, Vd.p(0), Vd.ld, -1, hptr(cc), None, 1.0, wd.p(0), None) != 0


# ------------------------------------------------------------------------------------------------ the big basis (n >= 2^22)
class BigBasis:
    """NB_VEC integer vectors of NB_MAX entries (int8 on host and device, fp64 in a guarded device basis), loaded at prefix n."""

    def __init__(self):
        rng = np.random.default_rng(2024)
        self.h = rng.integers(-32, 128, size=(NB_VEC + 1, NB_MAX), dtype=np.int8)     # last row: w
        self.d8 = torch.from_numpy(self.h).to("cuda")
        self.V = Dev(NB_VEC, NB_MAX + 2)
        self.w = Dev(1, NB_MAX + 2)
        self.dst = Dev(1, NB_MAX + 2)
        self._dots = {}

    def load(self, n, rows):
        self.V.set(self.d8[:rows, :n])
        self.w.set(self.d8[NB_VEC:, :n])
        self.dst.t.fill_(float("nan"))
        self.dst.n, self.dst.rows = n, 1

    def row(self, j, n):
        return self.h[NB_VEC if j == W else j, :n].astype(np.int64)

    def dot(self, i, j, n):
        key = (min(i, j), max(i, j), n)
        if key not in self._dots:
            self._dots[key] = int(self.row(i, n) @ self.row(j, n))
        return self._dots[key]


@pytest.fixture(scope="module")
def big(vc):
    b = BigBasis()
    yield b
    del b
    torch.cuda.empty_cache()


W = -1             # index of w in the dot callbacks of the reference

BIG_CASES = ([(BIG + 1, k, {}) for k in (1, 4, 5, 6, 8, 9, 16, 17, 24, 25, 32, 33)]
             + [(BIG - 2, 12, {}), (NB_MAX, 12, {}), (NB_MAX, 12, dict(vec_xcd_map=2)), (NB_MAX, 12, dict(vec_xcd_map=0))]
             + [(BIG + 1, k, dict(dot_burst=4)) for k in (6, 9, 32)]
             + [(BIG + 1, k, dict(krylov_burst=0)) for k in (4, 12, 32)]
             + [(NB_MAX, 12, dict(krylov_burst=0, vec_xcd_map=2)), (BIG + 1, 12, dict(krylov_burst=0, dot_variant=0)),
                (BIG + 1, 9, dict(nt_hint=0)), (BIG + 1, 33, dict(nt_hint=0))]
             + [(BIG + 1, 9, dict(krylov_burst=0, axpy_variant=v, axpy_nt=t)) for v in range(4) for t in (0, 1)]
             + [(BIG + 1, 9, dict(axpy_stagger=4)), (BIG + 1, 20, dict(axpy_stagger=3, axpy_stagger_map=1))])


@pytest.mark.parametrize("n,k,opts", BIG_CASES, ids=[f"{n}-k{k}-" + ",".join(f"{a}={b}" for a, b in o.items()) for n, k, o in BIG_CASES])
def test_multidot_multiaxpy_big_exact(vc, big, n, k, opts):
    """Every option variant gives the exact result, hence the default's bits."""
    c, L = vc
    big.load(n, k)
    rng = np.random.default_rng(k)
    coef = rng.integers(-4, 5, k)
    with options(c, **{a: b for a, b in opts.items() if a in DEFAULTS}):
        if "axpy_stagger_map" in opts:
            c.set_option("axpy_stagger_map", opts["axpy_stagger_map"])
        out = HostOut(k + 1)
        ok(L.v_multidot(c.h, n, big.V.p(0), big.V.ld, k, big.w.p(0), out.p()), c, "multidot")
        ref = [big.dot(j, W, n) for j in range(k)] + [big.dot(W, W, n)]
        assert np.array_equal(out.v, exact(ref))
        out.check()
        cc = coef.astype(np.float64)
        nn = HostOut(1)
        ok(L.v_multiaxpy(c.h, n, big.V.p(0), big.V.ld, k, hptr(cc), big.w.p(0), 0.5, big.dst.p(0), nn.p()), c, "multiaxpy")
        if "axpy_stagger_map" in opts:
            c.set_option("axpy_stagger_map", 0)
    acc = big.row(W, n)
    for j in range(k):
        acc += int(coef[j]) * big.row(j, n)
    got = big.dst.get()[0]
    assert np.array_equal(got, exact(acc) * 0.5)
    assert nn.v[0] == exact(int(acc @ acc)) * 0.25
    big.dst.check()
    big.V.check()
    big.w.check()


# ------------------------------------------------------------------------------------------------ multidot with the Gram column
def gram_check(c, L, Vd, wd, rowf, dotf, k, n):
    out, gram = HostOut(k + 1), HostOut(k)
    assert L.v_multidot_gram_ok(c.h, n, Vd.p(0), Vd.ld, k, wd.p(0))
    ok(L.v_multidot_gram(c.h, n, Vd.p(0), Vd.ld, k, wd.p(0), out.p(), gram.p()), c, "multidot_gram")
    ref = [dotf(j, W) for j in range(k)] + [dotf(W, W)]
    assert np.array_equal(out.v, exact(ref)), np.nonzero(out.v != exact(ref))
    g = [dotf(j, k - 1) for j in range(k)]
    assert np.array_equal(gram.v, exact(g)), np.nonzero(gram.v != exact(g))
    out.check()
    gram.check()


@pytest.mark.parametrize("k", [1, 2, 4, 5, 6, 8, 9, 16, 17, 24, 25, 32, 33, 45, 64])
@pytest.mark.parametrize("n", [2, 3, 6146, 8191, 65537])
def test_multidot_gram_exact(vc, n, k):
    c, L = vc
    rng = np.random.default_rng(k * 7 + n)
    V = ints(rng, (k, n))
    w = ints(rng, n)
    Vd, wd = Dev.of(V, "vec"), Dev.of(w, "vec")
    A = np.vstack([V, w[None]])                                     # row k = w (W = -1 selects it)
    gram_check(c, L, Vd, wd, None, lambda i, j: int(A[i] @ A[j]), k, n)
    Vd.check()
    wd.check()


@pytest.mark.parametrize("n,k", [(BIG + 1, 1), (BIG + 1, 5), (BIG + 1, 8), (BIG + 1, 16), (BIG - 2, 24), (BIG + 1, 32), (BIG + 1, 33)])
def test_multidot_gram_big_exact(vc, big, n, k):
    c, L = vc
    big.load(n, k)
    gram_check(c, L, big.V, big.w, None, lambda i, j: big.dot(i, j, n), k, n)
    big.V.check()


def test_multidot_gram_contract(vc):
    c, L = vc
    Vd, wd = Dev.of(np.ones((2, 9)), "scalar"), Dev.of(np.ones(9), "vec")
    assert not L.v_multidot_gram_ok(c.h, 9, Vd.p(0), Vd.ld, 2, wd.p(0))       # odd ldv / unaligned
    Vd = Dev.of(np.ones((2, 8)), "vec")
    assert not L.v_multidot_gram_ok(c.h, 8, Vd.p(0), Vd.ld, 65, wd.p(0))
    assert L.v_multidot_gram_ok(c.h, 8, Vd.p(0), Vd.ld, 64, wd.p(0))


# ------------------------------------------------------------------------------------------------ s-step block kernels
def block_dots_check(c, L, V, n, kold, r0, nr, dotf, ldv):
    D, T = HostOut(max(kold, 1) * SSTEP_KR), HostOut(SSTEP_KTRI)
    ok(L.v_block_dots(c.h, n, V.p(0), ldv, kold, r0, nr, D.p(), T.p()), c, "block_dots")
    Dref = np.zeros(kold * SSTEP_KR)
    for i in range(kold):
        for r in range(nr):
            Dref[i * SSTEP_KR + r] = dotf(i, r0 + r)             # exact zeros for r >= nr
    assert np.array_equal(D.v[:kold * SSTEP_KR], Dref), np.nonzero(D.v[:kold * SSTEP_KR] != Dref)
    if kold == 0:
        assert np.all(np.isnan(D.v))                              # nothing written
    Tref = np.zeros(SSTEP_KTRI)
    for r in range(nr):
        for q in range(r, nr):
            Tref[sstep_tri(r, q)] = dotf(r0 + r, r0 + q)
    assert np.array_equal(T.v, Tref), np.nonzero(T.v != Tref)
    D.check()
    T.check()


# block_dots_nr5 = 0 only changes the path where the NR5 launch applies (nr <= 5, kold > 4)
BD_CASES = [(kold, nr, nr5) for kold in (0, 1, 4, 5, 8, 9, 12, 13, 32) for nr in range(1, 9)
            for nr5 in ((1, 0) if nr <= 5 and kold > 4 else (1,))]


@pytest.mark.parametrize("kold,nr,nr5", BD_CASES)
@pytest.mark.parametrize("n", [2, 6147, 65537])
def test_block_dots_exact(vc, n, kold, nr, nr5):
    c, L = vc
    r0 = kold + (1 if kold % 2 else 0)                             # the right-hand vectors from slot r0 (not always kold)
    rows = r0 + nr
    rng = np.random.default_rng(n + 13 * kold + nr)
    V = ints(rng, (rows, n))
    Vd = Dev.of(V, "vec", nvec=rows + 1)
    assert L.v_block_ok(c.h, n, Vd.p(0), Vd.ld)
    with options(c, block_dots_nr5=nr5):
        block_dots_check(c, L, Vd, n, kold, r0, nr, lambda i, j: float(int(V[i] @ V[j])), Vd.ld)
    Vd.check()


@pytest.mark.parametrize("kold,nr,nr5", [(0, 8, 1), (4, 8, 1), (9, 4, 1), (9, 4, 0), (13, 5, 1), (5, 8, 1)])
def test_block_dots_big_exact(vc, big, kold, nr, nr5):
    c, L = vc
    n = BIG + 1
    big.load(n, kold + nr)
    with options(c, block_dots_nr5=nr5):
        block_dots_check(c, L, big.V, n, kold, kold, nr, lambda i, j: float(big.dot(i, j, n)), big.V.ld)
    big.V.check()


def block_axpy_ref(V, k, s, Cm, Tm):
    out = []
    for q in range(s):
        acc = np.zeros(V.shape[1], dtype=np.int64)
        for r in range(q + 1):
            acc += int(Tm[r, q]) * V[k + r]
        for i in range(k):
            acc += int(Cm[i, q]) * V[i]
        out.append(acc)
    return exact(np.array(out))


def block_coefs(rng, k):
    Cm = rng.integers(-4, 5, (k, SSTEP_KS)).astype(np.float64)
    Tm = np.triu(rng.integers(-3, 4, (SSTEP_KS, SSTEP_KS))).astype(np.float64)
    Tm[np.tril_indices(SSTEP_KS, -1)] = np.nan                      # documented upper triangular: never read
    return Cm, Tm


@pytest.mark.parametrize("s", [1, 2, 3, 4])
@pytest.mark.parametrize("k", [1, 8, 9, 16, 17, 32])
@pytest.mark.parametrize("n", [2, 3, 8194, 65537])
def test_block_axpy_exact(vc, n, k, s):
    c, L = vc
    rng = np.random.default_rng(n + 100 * k + s)
    V = ints(rng, (k + s, n))
    Cm, Tm = block_coefs(rng, k)
    Vd = Dev.of(V, "vec", nvec=k + s + 1)                          # slot k + s stays NaN: must not be written
    ok(L.v_block_axpy(c.h, n, Vd.p(0), Vd.ld, k, s, hptr(Cm), hptr(Tm)), c, "block_axpy")
    g = Vd.get()
    assert np.array_equal(g[:k], exact(V[:k]))                     # the old basis is read only
    ref = block_axpy_ref(V, k, s, Cm, Tm)
    assert np.array_equal(g[k:k + s], ref), np.argwhere(g[k:k + s] != ref)[:10]
    Vd.check()


@pytest.mark.parametrize("k,s", [(1, 4), (8, 2), (17, 4), (32, 1)])
def test_block_axpy_big_exact(vc, big, k, s):
    c, L = vc
    n = BIG + 1
    big.load(n, k + s)
    rng = np.random.default_rng(k * 5 + s)
    Cm, Tm = block_coefs(rng, k)
    ok(L.v_block_axpy(c.h, n, big.V.p(0), big.V.ld, k, s, hptr(Cm), hptr(Tm)), c, "block_axpy")
    got = big.V.body()[k:k + s, :n].cpu().numpy()
    for q in range(s):
        acc = np.zeros(n, dtype=np.int64)
        for r in range(q + 1):
            acc += int(Tm[r, q]) * big.row(k + r, n)
        for i in range(k):
            acc += int(Cm[i, q]) * big.row(i, n)
        assert np.array_equal(got[q], exact(acc))
    big.V.check()


def test_block_axpy_rejects_bad_sizes(vc):
    c, L = vc
    Vd = Dev.of(np.ones((2, 8)), "vec", nvec=40)
    Cm, Tm = np.zeros((33, SSTEP_KS)), np.zeros((SSTEP_KS, SSTEP_KS))
    assert L.v_block_axpy(c.h, 8, Vd.p(0), Vd.ld, 33, 1, hptr(Cm), hptr(Tm)) != 0
    assert L.v_block_axpy(c.h, 8, Vd.p(0), Vd.ld, 4, 5, hptr(Cm), hptr(Tm)) != 0
    Vd.check(rows=2)


# ------------------------------------------------------------------------------------------------ basis rotation
@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("m", [1, 16, 17, 32, 33, 48, 49, 64])
@pytest.mark.parametrize("n", [1, 255, 8191])
def test_basis_combine_exact(vc, n, m, inplace):
    c, L = vc
    rng = np.random.default_rng(n + m)
    V = ints(rng, (m, n))
    kout = m if inplace else min(m, 7)
    Q = rng.integers(-4, 5, (m, kout))
    Qh = np.asfortranarray(Q.astype(np.float64))                    # m x kout, column-major
    Vd = Dev.of(V, "vec")
    if inplace:
        dst, ldd = Vd, Vd.ld
    else:
        dst = Dev(kout, ld_for(n, "vec") + 2)                       # lddst != ldv
        dst.n, dst.rows, ldd = n, kout, dst.ld
    ok(L.v_basis_combine(c.h, n, Vd.p(0), Vd.ld, m, C.c_void_p(Qh.ctypes.data), kout, dst.p(0), ldd), c, "combine")
    ref = exact(Q.T @ V)
    assert np.array_equal(dst.get(), ref)
    dst.check()
    if not inplace:
        assert np.array_equal(Vd.get(), exact(V))
        Vd.check()


# ------------------------------------------------------------------------------------------------ device-resident Arnoldi step
def ortho_basis(rng, k, n, L_):
    """k exactly orthonormal vectors: random signs times 2^-log2(sqrt(L_)) on disjoint blocks of L_ = 4^m entries."""
    assert k * L_ <= n
    V = np.zeros((k, n))
    for j in range(k):
        V[j, j * L_:(j + 1) * L_] = rng.choice([-1.0, 1.0], L_) / math.sqrt(L_)
    return V


def w_with_ratio(rng, V, n, k, L_, rho):
    """w = V a + delta r, r unit and exactly orthogonal to V (supported after the blocks): ||w - V a|| / ||w|| = rho."""
    a = rng.standard_normal(k)
    r = np.zeros(n)
    r[k * L_:] = rng.standard_normal(n - k * L_)
    r /= np.linalg.norm(r)
    delta = rho * np.linalg.norm(a) / math.sqrt(1 - rho * rho) if rho > 0 else 0.0
    return a @ V + delta * r


def arnoldi_run(c, L, V, w, k, eta, orth_tol, layout="vec", gram=None):
    n = V.shape[1]
    Vd = Dev.of(V, layout, nvec=k + 2)
    wd = Dev.of(w, layout)
    rec = torch.full((K_MAX_BASIS + 2,), float("nan"), dtype=torch.float64, device="cuda")
    coef = torch.full((K_MAX_BASIS + 3,), float("nan"), dtype=torch.float64, device="cuda")
    coef[K_MAX_BASIS + 2] = 0.0                                    # running defect estimate, zeroed at the start of a cycle
    gp = None if gram is None else C.c_void_p(gram.data_ptr())
    st = L.v_arnoldi_step_dev(c.h, n, Vd.p(0), Vd.ld, k, wd.p(0), eta, orth_tol, C.c_void_p(rec.data_ptr()),
                              C.c_void_p(coef.data_ptr()), gp)
    torch.cuda.synchronize()
    return st, Vd, wd, rec.cpu().numpy(), coef.cpu().numpy()


def check_new_vector(V, w, k, h, beta, vnew, passes):
    """vnew against (w - V h) / beta in longdouble with the kernel's own h, beta: per element (k + 2) u sum |terms| / beta per
    pass (k fma, one scale) -- a second pass adds the same relative bound again."""
    Vl, wl = V.astype(np.longdouble), w.astype(np.longdouble)
    ref = (wl - h.astype(np.longdouble) @ Vl) / np.longdouble(beta)
    tb = (np.abs(wl) + np.abs(h.astype(np.longdouble)) @ np.abs(Vl)) / abs(beta)
    assert np.all(np.abs(vnew - ref) <= passes * (k + 3) * U * tb + 8 * U * np.abs(ref))


@pytest.mark.parametrize("layout", ["vec", "scalar"])
@pytest.mark.parametrize("k", [1, 2, 8, 13])
def test_arnoldi_step_dev_gate(vc, k, layout):
    """10x above eta: one pass, gate 0; 10x below: the DGKS second pass runs (gate 1, coefficients = -s, tiny)."""
    c, L = vc
    n, L_, eta = 65537, 4096, 1e-2
    rng = np.random.default_rng(k)
    V = ortho_basis(rng, k, n, L_)
    for rho, second in ((10 * eta, False), (eta / 10, True)):
        w = w_with_ratio(rng, V, n, k, L_, rho)
        st, Vd, wd, rec, coef = arnoldi_run(c, L, V, w, k, eta, 1e-6, layout)
        assert st == 0
        Vl, wl = V.astype(np.longdouble), w.astype(np.longdouble)
        h_ref = Vl @ wl
        hb = bound_red(n, np.abs(Vl) @ np.abs(wl))
        ww = np.dot(wl, wl)
        assert rec[K_MAX_BASIS + 1] == 0.0                          # trusted
        assert coef[K_MAX_BASIS + 1] == (1.0 if second else 0.0)
        beta_ref = np.sqrt(ww - np.dot(h_ref, h_ref))               # = delta; relative error ~ depth u / rho^2 before the 2nd pass
        if second:
            assert np.all(np.abs(coef[:k]) <= 4 * hb / beta_ref)    # -s: what the first pass left of V'w, divided by beta
            assert np.all(np.abs(rec[:k] - h_ref) <= 4 * hb)        # h + beta s
        else:
            assert np.array_equal(coef[:k], -rec[:k])
            assert np.all(np.abs(rec[:k] - h_ref) <= hb)
            assert abs(rec[K_MAX_BASIS] - beta_ref) <= 4 * red_depth(n) * U * ww / beta_ref
            assert coef[K_MAX_BASIS] == 1.0 / rec[K_MAX_BASIS]
        vnew = Vd.get(k + 1)[k].astype(np.longdouble)
        if not second:
            check_new_vector(V, w, k, rec[:k], rec[K_MAX_BASIS], vnew, 1)
        # orthogonality to V: after one pass |V'v| <= |h err| / beta; after two passes the second pass removes it down to the
        # rounding of one more projection of a unit vector
        orth = np.abs(Vl @ vnew).max()
        # (second pass: the error of s = V'v is <= 2 d u sum|V_j||v| <= 2 d u, the axpy's (k + 3) u: 8 d u covers both)
        assert orth <= (4 * hb.max() / beta_ref if not second else 8 * red_depth(n) * U)
        # ||v||: the Pythagorean beta^2 = w'w - |h|^2 carries 4 d u w'w absolute, i.e. 4 d u / rho^2 relative, until the second
        # pass renormalises with cn^2 = v'v - |s|^2
        assert abs(np.dot(vnew, vnew) - 1) <= 8 * red_depth(n) * U * (1.0 if second else 1.0 / rho ** 2)
        Vd.check(rows=k + 1)
        wd.check()


def test_arnoldi_step_dev_breakdown(vc):
    """w exactly in span(V): beta^2 = 0 -> flag 1 (the host repeats the step), beta recorded as 0."""
    c, L = vc
    n, k, L_ = 65537, 6, 4096
    rng = np.random.default_rng(5)
    V = ortho_basis(rng, k, n, L_)
    a = rng.integers(-8, 9, k).astype(np.float64)
    w = a @ V                                                       # exact: disjoint supports, entries +-a_j / 64
    st, Vd, wd, rec, coef = arnoldi_run(c, L, V, w, k, 1e-2, 1e-6)
    assert st == 0
    assert np.array_equal(rec[:k], a)                               # h = V'w exactly
    assert rec[K_MAX_BASIS + 1] == 1.0 and rec[K_MAX_BASIS] == 0.0
    assert coef[K_MAX_BASIS + 1] == 0.0                             # no second pass on an untrusted step
    Vd.check(rows=k + 1)


@pytest.mark.parametrize("k", [1, 2, 31, 32])
def test_arnoldi_step_dev_gram(vc, k):
    """Gram path: c = a - E a + E^2 a, E = G - I after column k-1 of G is replaced by the measured g = V'V_{k-1}; one pass."""
    c, L = vc
    n, L_ = 65537, 1024
    rng = np.random.default_rng(100 + k)
    V = ortho_basis(rng, k, n, L_)
    w = w_with_ratio(rng, V, n, k, L_, 0.3)
    ldg = K_MAX_BASIS + 1
    E = np.zeros((ldg, ldg))
    E[:k, :k] = 1e-9 * rng.standard_normal((k, k))
    E = E + E.T                                                     # known symmetric Gram defect of the earlier columns
    Gh = np.eye(ldg) + E
    G = torch.from_numpy(Gh.T.copy().reshape(-1)).to("cuda")        # column-major (symmetric anyway)
    st, Vd, wd, rec, coef = arnoldi_run(c, L, V, w, k, 1e-2, 1e-6, gram=G)
    assert st == 0
    Gd = G.cpu().numpy().reshape(ldg, ldg).T
    Vl, wl = V.astype(np.longdouble), w.astype(np.longdouble)
    g = Vl @ Vl[k - 1]                                              # = e_{k-1} exactly
    assert np.array_equal(Gd[:k, k - 1], g.astype(np.float64)) and np.array_equal(Gd[k - 1, :k], g.astype(np.float64))
    Gl = Gh.astype(np.longdouble)[:k, :k]
    Gl[:, k - 1] = g
    Gl[k - 1, :] = g
    El = Gl - np.eye(k, dtype=np.longdouble)
    a_ref = Vl @ wl
    e1 = El @ a_ref
    c_ref = a_ref - e1 + El @ e1
    hb = bound_red(n, np.abs(Vl) @ np.abs(wl))
    assert np.all(np.abs(rec[:k] - c_ref) <= 4 * hb + 8 * k * U * np.abs(c_ref).max())
    assert np.array_equal(coef[:k], -rec[:k])
    ww = np.dot(wl, wl)
    beta_ref = np.sqrt(ww - np.dot(c_ref, a_ref))
    assert abs(rec[K_MAX_BASIS] - beta_ref) <= 8 * red_depth(n) * U * ww / beta_ref
    assert rec[K_MAX_BASIS + 1] == 0.0 and coef[K_MAX_BASIS + 1] == 0.0 and coef[K_MAX_BASIS] == 1.0 / rec[K_MAX_BASIS]
    vnew = Vd.get(k + 1)[k].astype(np.longdouble)
    check_new_vector(V, w, k, rec[:k], rec[K_MAX_BASIS], vnew, 1)
    # in exact arithmetic V'v = (V'w - c) / beta (V exactly orthonormal): what is left is the rounding of the dots and the axpy
    assert np.abs(Vl @ vnew - (a_ref - rec[:k]) / rec[K_MAX_BASIS]).max() <= 4 * hb.max() / beta_ref
    Vd.check(rows=k + 1)


def test_arnoldi_step_dev_gram_rejects_k33(vc):
    c, L = vc
    n, k = 4098, 33
    V = np.ones((k, n))
    G = torch.eye(K_MAX_BASIS + 1, dtype=torch.float64, device="cuda").reshape(-1)
    st, Vd, *_ = arnoldi_run(c, L, V, np.ones(n), k, 1e-2, 1e-6, gram=G)
    assert st != 0
    Vd.check(rows=k)                                                # nothing written


@pytest.mark.parametrize("opts", [{}, dict(krylov_burst=0)])
@pytest.mark.parametrize("k", [8, 12])
def test_arnoldi_step_dev_big(vc, k, opts):
    c, L = vc
    n, L_ = BIG + 1, 4 ** 8
    rng = np.random.default_rng(k)
    V = ortho_basis(rng, k, n, L_)
    w = w_with_ratio(rng, V, n, k, L_, 0.5)
    with options(c, **opts):
        st, Vd, wd, rec, coef = arnoldi_run(c, L, V, w, k, 1e-2, 1e-6)
    assert st == 0 and coef[K_MAX_BASIS + 1] == 0.0 and rec[K_MAX_BASIS + 1] == 0.0
    wl = w.astype(np.longdouble)
    for j in range(k):                                              # per vector in longdouble
        vj = V[j].astype(np.longdouble)
        assert abs(rec[j] - np.dot(vj, wl)) <= bound_red(n, np.dot(abs(vj), abs(wl)))
    vnew = Vd.get(k + 1)[k]
    ref = (w - rec[:k] @ V) / rec[K_MAX_BASIS]
    tb = (np.abs(w) + np.abs(rec[:k]) @ np.abs(V)) / rec[K_MAX_BASIS]
    assert np.all(np.abs(vnew - ref) <= (k + 3) * U * tb + 4 * U * np.abs(ref))
    Vd.check(rows=k + 1)


# ------------------------------------------------------------------------------------------------ v_fill_random
def splitmix_ref(seed, goff, n):
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * (np.uint64(goff) + np.arange(1, n + 1, dtype=np.uint64))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def test_fill_random(vc):
    c, L = vc
    N, seed = 100003, 0x1234567
    full = Dev(1, N + 1)
    full.n, full.rows = N, 1
    ok(L.v_fill_random(c.h, N, 0, seed, full.p(0)), c, "fill")
    f = full.get()[0]
    assert np.array_equal(f, splitmix_ref(seed, 0, N))
    assert f.min() >= 0.0 and f.max() < 1.0
    full.check()
    for goff, n in ((0, 1), (1, 255), (4097, 3), (50000, 50003)):
        part = Dev(1, n + 1, 1)
        part.n, part.rows = n, 1
        ok(L.v_fill_random(c.h, n, goff, seed, part.p(0)), c, "fill part")
        assert np.array_equal(part.get()[0], f[goff:goff + n])
        part.check()


# ------------------------------------------------------------------------------------------------ norminf: NaN and inf
@pytest.mark.parametrize("n", [3, 4097, BIG + 1])
def test_nrminf_propagates_nan(vc, n):
    """norminf(x) = norm(x, Inf) (src/LinearSolver.jl:4) is NaN when any entry is NaN -- fmax would drop it."""
    c, L = vc
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n)
    d = Dev.of(x, "vec")
    out = HostOut(1)
    ok(L.v_nrminf(c.h, n, d.p(0), out.p()), c, "nrminf")
    assert out.v[0] == np.abs(x).max()
    body = d.body()[0]
    for pos in sorted({0, n - 1, min(256, n - 1), n // 2}):        # first, odd tail / last, a workgroup boundary, middle
        body[pos] = float("nan")
        ok(L.v_nrminf(c.h, n, d.p(0), out.p()), c, "nrminf")
        assert np.isnan(out.v[0]), pos
        body[pos] = float(x[pos])
    body[:n] = float("nan")
    ok(L.v_nrminf(c.h, n, d.p(0), out.p()), c, "nrminf")
    assert np.isnan(out.v[0])
    for s in (1.0, -1.0):
        body[:n] = torch.from_numpy(x).cuda()
        body[n // 3] = s * float("inf")
        ok(L.v_nrminf(c.h, n, d.p(0), out.p()), c, "nrminf")
        assert out.v[0] == np.inf
    out.check()
    d.check()
    # the public ABI too
    body[:n] = torch.from_numpy(x).cuda()
    body[n - 1] = float("nan")
    v = C.c_double()
    ok(c.lib.bk_vec_nrminf(c.h, n, d.p(0), C.byref(v)), c, "bk_vec_nrminf")
    assert np.isnan(v.value)


def test_newton_from_nan_state_does_not_converge(vc):
    """Newton.jl:76-111: residual NaN -> `while (... r > tol ...)` takes no step and converged = (NaN < tol) = false."""
    c, L = vc
    from bk_amd import hip
    dims, ls = (8, 6, 5), (np.pi, 2.0, 1.5)
    prob = hip.SwiftHohenberg(c, dims, ls, l=0.1, nu=1.2)
    x0 = prob.vec(np.full(int(np.prod(dims)), np.nan))
    gls = hip.GMRESKrylovKit(dim=10, rtol=1e-9, atol=1e-12, maxiter=20)
    s = hip.newton_native(prob, x0, 0.1, gls, tol=1e-9, max_iterations=3, norm_inf=True)
    assert not s["converged"] and s["itnewton"] == 0 and np.isnan(s["residuals"][0])
    root = prob.vec(np.zeros(int(np.prod(dims))))
    dfl = hip.DeflationOperator(2.0, 1.0, [root])
    s = hip.newton_deflated_native(prob, dfl, x0, 0.1, gls, tol=1e-9, max_iterations=3, norm_inf=True)
    assert not s["converged"] and s["itnewton"] == 0 and np.isnan(s["residuals"][0])


# ------------------------------------------------------------------------------------------------ public ABI at n >= 2^22
def test_public_abi_big(vc, big):
    c, L = vc
    n, k = BIG + 1, 9
    big.load(n, k)
    out = (C.c_double * (k + 1))()
    ok(c.lib.bk_krylov_multidot(c.h, n, big.V.p(0), big.V.ld, k, big.w.p(0), out), c, "bk_krylov_multidot")
    assert np.array_equal(np.array(out[:]), exact([big.dot(j, W, n) for j in range(k)] + [big.dot(W, W, n)]))
    v = C.c_double()
    ok(c.lib.bk_vec_dot(c.h, n, big.V.p(0), big.V.p(1), C.byref(v)), c, "bk_vec_dot")
    assert v.value == exact(big.dot(0, 1, n))
    ok(c.lib.bk_vec_nrm2(c.h, n, big.w.p(0), C.byref(v)), c, "bk_vec_nrm2")
    assert v.value == np.sqrt(exact(big.dot(W, W, n)))
    ok(c.lib.bk_vec_nrminf(c.h, n, big.w.p(0), C.byref(v)), c, "bk_vec_nrminf")
    assert v.value == float(np.abs(big.row(W, n)).max())
    coef = np.arange(1, k + 1, dtype=np.float64) - 5
    cc = (C.c_double * k)(*coef)
    nn = C.c_double()
    ok(c.lib.bk_krylov_multiaxpy(c.h, n, big.V.p(0), big.V.ld, k, cc, big.w.p(0), 0.25, big.dst.p(0), C.byref(nn)), c, "bk_krylov_multiaxpy")
    acc = big.row(W, n)
    for j in range(k):
        acc += int(coef[j]) * big.row(j, n)
    assert np.array_equal(big.dst.get()[0], exact(acc) * 0.25)
    assert nn.value == exact(int(acc @ acc)) / 16
    ok(c.lib.bk_vec_axpby(c.h, n, 2.0, big.V.p(0), -1.0, big.V.p(1)), c, "bk_vec_axpby")
    assert np.array_equal(big.V.get(2)[1], exact(2 * big.row(0, n) - big.row(1, n)))
    big.V.check(rows=k)


# ------------------------------------------------------------------------------------------------ coverage table
# every kernel launch expression of vecops.hip, as written (test_vecops_coverage_host.py extracts them) -> the tests reaching it
_BLAS = ["test_blas1_exact", "test_blas1_longdouble"]
COVERAGE = {
    "absmax_kernel": ["test_blas1_exact", "test_nrminf_propagates_nan"],
    "arnoldi_coef2_kernel": ["test_arnoldi_step_dev_gate"],
    "arnoldi_coef_kernel": ["test_arnoldi_step_dev_gate", "test_arnoldi_step_dev_breakdown", "test_arnoldi_step_dev_big"],
    "arnoldi_gram_coef_kernel": ["test_arnoldi_step_dev_gram"],
    "axpbyz_kernel<1>": ["test_blas1_exact"],
    "axpbyz_kernel<2, true>": ["test_blas1_exact", "test_public_abi_big"],
    "axpbyz_kernel<2>": ["test_blas1_exact"],
    "axpy_dot_kernel<1>": ["test_axpy_dot_exact"],
    "axpy_dot_kernel<2, true>": ["test_axpy_dot_exact"],
    "axpy_dot_kernel<2>": ["test_axpy_dot_exact"],
    "block_axpy_kernel<KB, 4, false>": ["test_block_axpy_exact"],
    "block_axpy_kernel<KB, 4, true>": ["test_block_axpy_big_exact"],
    "block_dots_kernel<4, true, 2, false>": ["test_block_dots_exact"],
    "block_dots_kernel<4, true, 2, true>": ["test_block_dots_big_exact"],
    "block_dots_kernel<8, false, 2, false>": ["test_block_dots_exact"],
    "block_dots_kernel<8, false, 2, true>": ["test_block_dots_big_exact"],
    "block_dots_kernel<8, true, 2, false, NR5>": ["test_block_dots_exact"],
    "block_dots_kernel<8, true, 2, true, NR5>": ["test_block_dots_big_exact"],
    "combine_kernel<16>": ["test_basis_combine_exact"],
    "combine_kernel<32>": ["test_basis_combine_exact"],
    "combine_kernel<48>": ["test_basis_combine_exact"],
    "combine_kernel<64>": ["test_basis_combine_exact"],
    "diff_nrm2_kernel<1>": ["test_blas1_exact"],
    "diff_nrm2_kernel<2, true>": _BLAS,
    "diff_nrm2_kernel<2>": _BLAS,
    "dot_kernel<1, 1>": ["test_blas1_exact"],
    "dot_kernel<1, 2>": ["test_blas1_exact"],
    "dot_kernel<2, 1, true>": _BLAS + ["test_public_abi_big"],
    "dot_kernel<2, 1>": _BLAS,
    "dot_kernel<2, 2, true>": _BLAS,
    "dot_kernel<2, 2>": _BLAS,
    "fill_random_kernel": ["test_fill_random"],
    "minres_update2_kernel<false>": ["test_minres_updates_exact", "test_minres_update2_equals_two_updates"],
    "minres_update2_kernel<true>": ["test_minres_updates_exact", "test_minres_update2_equals_two_updates"],
    "minres_update_kernel<1>": ["test_minres_updates_exact"],
    "minres_update_kernel<2, true>": ["test_minres_updates_exact", "test_minres_update2_equals_two_updates"],
    "minres_update_kernel<2>": ["test_minres_updates_exact", "test_minres_update2_equals_two_updates"],
    "multiaxpy_c_kernel<KB, 4, true, true, false>": ["test_multidot_multiaxpy_big_exact", "test_public_abi_big"],
    "multiaxpy_c_kernel<KB, 4, true, true, true>": ["test_arnoldi_step_dev_big"],
    "multiaxpy_kernel<KB, 1, false, false, 1, true>": ["test_arnoldi_step_dev_gate"],
    "multiaxpy_kernel<KB, 1>": ["test_multidot_multiaxpy_exact"],
    "multiaxpy_kernel<KB, 2, false, false, 1, true>": ["test_arnoldi_step_dev_gate", "test_arnoldi_step_dev_gram",
                                                       "test_arnoldi_step_dev_breakdown"],
    "multiaxpy_kernel<KB, 2, true, false, 2>": ["test_multidot_multiaxpy_big_exact"],
    "multiaxpy_kernel<KB, 2, true, true, 1>": ["test_multidot_multiaxpy_big_exact"],
    "multiaxpy_kernel<KB, 2, true, true, 2, true>": ["test_arnoldi_step_dev_big"],
    "multiaxpy_kernel<KB, 2, true, true, 2>": ["test_multidot_multiaxpy_big_exact"],
    "multiaxpy_kernel<KB, 2, true>": ["test_multidot_multiaxpy_exact", "test_multidot_multiaxpy_big_exact"],
    "multiaxpy_kernel<KB, 2>": ["test_multidot_multiaxpy_exact", "test_multidot_multiaxpy_big_exact"],
    "multidot_c_kernel<KB, 4, false, true>": ["test_multidot_gram_exact", "test_arnoldi_step_dev_gram"],
    "multidot_c_kernel<KB, 4, true>": ["test_multidot_multiaxpy_big_exact"],
    "multidot_c_kernel<KB, 8, true>": ["test_multidot_multiaxpy_big_exact", "test_arnoldi_step_dev_big", "test_public_abi_big"],
    "multidot_c_kernel<KB, UU, true, true>": ["test_multidot_gram_big_exact"],
    "multidot_kernel<KB, 1>": ["test_multidot_multiaxpy_exact", "test_arnoldi_step_dev_gate"],
    "multidot_kernel<KB, 2, true>": ["test_multidot_multiaxpy_big_exact", "test_arnoldi_step_dev_big"],
    "multidot_kernel<KB, 2>": ["test_multidot_multiaxpy_exact", "test_multidot_multiaxpy_big_exact", "test_arnoldi_step_dev_gate"],
    "pw_scale_kernel": ["test_blas1_exact"],
    "reduce_stage2_dev": ["test_arnoldi_step_dev_gate", "test_arnoldi_step_dev_big"],
}
