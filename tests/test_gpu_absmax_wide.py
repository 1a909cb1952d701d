"""``v_nrminf`` (csrc/vecops.hip: absmax_kernel, 16-byte loads with a scalar head and tail) against NumPy, exactly: a maximum of
absolute values involves no rounding.  Lengths around one item, one wave, one workgroup iteration (256 lanes x 4 items x 2
elements = 2048) and the non-temporal threshold 2^22; the vector on a 16-byte boundary and 8 bytes past one (then the first element
is the scalar head, and the parity of the rest decides whether the last one is a scalar tail); the maximum -- negative -- at the
first, the last, the one before the last and a middle element; zeros and -0.0; a NaN at any of those places comes out as NaN."""
import numpy as np
import pytest
import torch

import test_gpu_vecops_exact as gv
from vecops_abi import Launchers

pytestmark = pytest.mark.gpu

BIG = 1 << 22
SIZES = [1, 2, 3, 255, 256, 257, 4097, BIG - 1, BIG, BIG + 3]


@pytest.fixture(scope="module")
def vc():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    from bk_amd import hip
    c = hip.Context(0)
    yield c, Launchers(c.lib)
    c.close()


def nrminf(c, L, d, n):
    out = gv.HostOut(1)
    gv.ok(L.v_nrminf(c.h, n, d.p(0), out.p()), c, "nrminf")
    out.check()
    return out.v[0]


def places(n):
    return sorted({0, n // 2, max(n - 2, 0), n - 1})


@pytest.mark.parametrize("off", [0, 1])                     # doubles past a 16-byte boundary
@pytest.mark.parametrize("n", SIZES)
def test_nrminf_exact(vc, n, off):
    c, L = vc
    x = np.random.default_rng(2 * n + off).standard_normal(n)
    d = gv.Dev(1, n + 2 + (n & 1), off)
    assert d.p(0).value % 16 == 8 * off
    d.set(torch.from_numpy(x[None, :]))
    assert nrminf(c, L, d, n) == np.abs(x).max()
    row = d.body()[0]
    for i in places(n):                                     # the maximum, negative, at the head, in the middle and in the tail
        row[i] = -1.0e3 - i
        assert nrminf(c, L, d, n) == 1.0e3 + i
        row[i] = float(x[i])
    for i in places(n):                                     # a NaN anywhere is the result
        row[i] = float("nan")
        assert np.isnan(nrminf(c, L, d, n)), i
        row[i] = float(x[i])
    assert nrminf(c, L, d, n) == np.abs(x).max()
    d.check()


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_nrminf_zeros(vc, n, off):
    c, L = vc
    d = gv.Dev(1, n + 2 + (n & 1), off)
    for z in (0.0, -0.0):
        d.set(torch.full((1, n), z, dtype=torch.float64))
        r = nrminf(c, L, d, n)
        assert r == 0.0 and not np.signbit(r)
    row = d.body()[0]                                       # -0.0 everywhere but one tiny entry
    for i in places(n):
        row[i] = -1e-300
        assert nrminf(c, L, d, n) == 1e-300
        row[i] = -0.0
    d.check()
