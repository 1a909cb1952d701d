"""The six-slot projection launch of ``csrc/block_dots_wide.hip`` through the pinned ``v_block_dots`` binding (``tests/vecops_abi.py``),
with option ``block_dots_wide`` at 0 (the routing of ``vecops.hip`` alone) and 1.

* integer data (entries in [-32, 127]: every partial sum is an integer below 2^53, so any summation order is exact): D and T equal
  the integer Gram matrix, and every unused right-hand slot holds an exact zero;
* random doubles: D and T are bitwise the same under both settings -- the new launch gives every accumulator the fma sequence
  it had in the launches it replaces (same grid, same items per lane, same load path);
* the profile counters show the routing itself: (kold, nr) = (8, 6) is ONE ``multidot`` launch of 8 n 14 bytes with the option
  on and two of 8 n 10 with it off; the routes next to it -- (4, 6), (8, 5), (8, 8) -- do not move.

One set of 20 vectors per length is shared by all cases (the basis is rows [0, kold), the right-hand vectors the rows after it);
the host Gram matrix is a float64 product, exact for these integers.  COVERAGE (checked by test_block_dots_wide_host.py) maps the
launch expressions of block_dots_wide.hip to the tests that reach them.
"""
import contextlib

import numpy as np
import pytest
import torch

import test_gpu_vecops_exact as gv
from vecops_abi import SSTEP_KR, SSTEP_KTRI, Launchers, sstep_tri

pytestmark = pytest.mark.gpu

BIG = 1 << 22                                   # nt_hint threshold: non-temporal loads from here on
NVEC = 20
# tiny; one full and one ragged item per lane; 4099: the odd last element (block 0 / thread 0); the non-temporal path, even and odd
SIZES = [2, 6, 4098, 4099, BIG, BIG + 1]
WIDE = [(5, 6), (8, 6), (12, 6)]                # routed to block_dots_wide.hip when the option is on
UNCHANGED = [(4, 6), (8, 5), (8, 8)]            # kold <= 4; the 5-slot launch; the 8-slot launches
LAUNCHES = {                                    # (kold, nr) -> [(basis vectors, right-hand vectors) per launch] with the option off / on
    (5, 6): ([(4, 6), (1, 6)], [(5, 6)]),
    (8, 6): ([(4, 6), (4, 6)], [(8, 6)]),
    (12, 6): ([(4, 6), (8, 6)], [(8, 6), (4, 6)]),
    (4, 6): ([(4, 6)], [(4, 6)]),
    (8, 5): ([(8, 5)], [(8, 5)]),
    (8, 8): ([(4, 8), (4, 8)], [(4, 8), (4, 8)]),
}


@pytest.fixture(scope="module")
def vc():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    from bk_amd import hip
    c = hip.Context(0)
    yield c, Launchers(c.lib)
    c.close()


@contextlib.contextmanager
def wide(c, on):
    c.set_option("block_dots_wide", on)
    try:
        yield
    finally:
        c.set_option("block_dots_wide", 1)


_DATA = {}


def data(n):
    """Per length, made once: the integer vectors on the device, their exact Gram matrix, and random doubles on the device."""
    if n not in _DATA:
        rng = np.random.default_rng(n)
        A = gv.ints(rng, (NVEC, n)).astype(np.float64)
        gram = A @ A.T                           # integers below 2^53 in every partial sum: exact in any order
        assert np.abs(gram).max() < 2.0 ** 53 and np.array_equal(gram, np.rint(gram))
        ld = n + 2 + (n & 1)                     # even and larger than n
        Vi = gv.Dev.of(A, "vec", ld=ld)
        del A
        Vr = gv.Dev(NVEC, ld)
        g = torch.Generator(device="cuda").manual_seed(n)
        Vr.set(torch.randn((NVEC, n), dtype=torch.float64, device="cuda", generator=g))
        _DATA[n] = (Vi, gram, Vr)
    return _DATA[n]


def block_dots(c, L, V, n, kold, nr):
    D, T = gv.HostOut(kold * SSTEP_KR), gv.HostOut(SSTEP_KTRI)
    gv.ok(L.v_block_dots(c.h, n, V.p(0), V.ld, kold, kold, nr, D.p(), T.p()), c, "block_dots")
    D.check()
    T.check()
    return D.v.copy(), T.v.copy()


@pytest.mark.parametrize("on", [0, 1])
@pytest.mark.parametrize("kold,nr", WIDE + UNCHANGED)
@pytest.mark.parametrize("n", SIZES)
def test_block_dots_wide_exact(vc, n, kold, nr, on):
    c, L = vc
    Vi, gram, _ = data(n)
    assert L.v_block_ok(c.h, n, Vi.p(0), Vi.ld) and Vi.ld % 2 == 0 and Vi.ld > n
    with wide(c, on):
        D, T = block_dots(c, L, Vi, n, kold, nr)
    Dref, Tref = np.zeros(kold * SSTEP_KR), np.zeros(SSTEP_KTRI)        # exact zeros in the unused right-hand slots
    for i in range(kold):
        Dref[i * SSTEP_KR:i * SSTEP_KR + nr] = gram[i, kold:kold + nr]
    for r in range(nr):
        for q in range(r, nr):
            Tref[sstep_tri(r, q)] = gram[kold + r, kold + q]
    assert np.array_equal(D, Dref), np.nonzero(D != Dref)
    assert np.array_equal(T, Tref), np.nonzero(T != Tref)
    Vi.check()


@pytest.mark.parametrize("kold,nr", WIDE + UNCHANGED)
@pytest.mark.parametrize("n", SIZES)
def test_block_dots_wide_bitwise(vc, n, kold, nr):
    c, L = vc
    _, _, Vr = data(n)
    with wide(c, 0):
        D0, T0 = block_dots(c, L, Vr, n, kold, nr)
    with wide(c, 1):
        D1, T1 = block_dots(c, L, Vr, n, kold, nr)
    assert np.isfinite(D0).all() and np.isfinite(T0).all()               # (a NaN would show an over-read into the padding)
    assert D0.tobytes() == D1.tobytes(), np.nonzero(D0 != D1)
    assert T0.tobytes() == T1.tobytes(), np.nonzero(T0 != T1)
    Vr.check()


@pytest.mark.parametrize("kold,nr", WIDE + UNCHANGED)
@pytest.mark.parametrize("n", [4098, BIG])
def test_block_dots_wide_routing(vc, n, kold, nr):
    """The launches as the context's profile counters saw them: every launch is one `multidot` scope of 8 n (kb + nr) bytes."""
    c, L = vc
    Vi, _, _ = data(n)
    c.prof_enable(True)
    try:
        for on in (0, 1):
            c.prof_reset()
            with wide(c, on):
                block_dots(c, L, Vi, n, kold, nr)
            got = c.prof_get("multidot")
            want = LAUNCHES[(kold, nr)][on]
            assert got["calls"] == len(want), (on, got)
            assert got["bytes"] == 8.0 * n * sum(kb + r for kb, r in want), (on, got)
    finally:
        c.prof_enable(False)
        c.prof_reset()


COVERAGE = {
    "block_dots_wide_kernel<8, 2, false, NRW>": ["test_block_dots_wide_exact", "test_block_dots_wide_bitwise", "test_block_dots_wide_routing"],
    "block_dots_wide_kernel<8, 2, true, NRW>": ["test_block_dots_wide_exact", "test_block_dots_wide_bitwise", "test_block_dots_wide_routing"],
}
