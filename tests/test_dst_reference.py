"""The reference of the cGL sine-transform tests (tests/test_gpu_dst_transforms.py) under test itself.  CPU only.

oracle.operators.dst_block_preconditioner_cgl (scipy's DST-I) against an independent dense restatement in np.longdouble
(tests/dst_dense_ref.py), and the float64 version of that restatement against the long-double one: the second number is what a
correctly rounded dense fp64 implementation of the same four products delivers, and the GPU bound 1e-13 is justified by it."""
import functools

import numpy as np
import pytest

from dst_dense_ref import SYMBOLS, box, dense_apply
from oracle import operators

assert np.finfo(np.longdouble).eps < 1e-18, "the long-double reference needs a 64-bit mantissa (x86-64)"

# the folded shape, one step off it on either axis, both routes mixed, the switch at 32.  (384, 256) and (128, 768) stay out: their
# long-double products take 1-2 s each
DIMS = [(128, 256), (126, 256), (130, 254), (40, 24), (33, 32)]


def _input(dims):
    return np.random.default_rng(1000 * dims[0] + dims[1]).standard_normal(2 * dims[0] * dims[1])


@functools.lru_cache(maxsize=None)
def _longdouble(dims, a, b):
    return dense_apply(dims, box(dims), a, b, _input(dims), np.longdouble)


@pytest.mark.parametrize("name,a,b", SYMBOLS)
@pytest.mark.parametrize("dims", DIMS)
def test_scipy_oracle_against_the_long_double_dense_restatement(dims, name, a, b):
    """Two orthonormal FFT-based DST-I each way and one division per entry: a few eps (measured: at most 6.2e-16 of max|ref| at these
    shapes).  5e-15 leaves room for another FFT backend, and is 20 times below the bound the GPU paths are held to."""
    ref = _longdouble(dims, a, b)
    got = operators.dst_block_preconditioner_cgl(dims, box(dims), a, b)(_input(dims))
    scale = float(np.abs(ref).max())
    err = float(np.abs(got - ref).max())
    assert err <= 5e-15 * scale, (dims, name, err / scale)


@pytest.mark.parametrize("name,a,b", SYMBOLS)
@pytest.mark.parametrize("dims", DIMS)
def test_float64_dense_restatement_against_the_long_double_one(dims, name, a, b):
    """What the GPU bound rests on: the same four dense products with float64 tables and float64 accumulation stay within 3e-14 of
    max|ref| (measured: 1.1e-15 at (33, 32) to 8.1e-15 at (130, 254))."""
    ref = _longdouble(dims, a, b)
    got = dense_apply(dims, box(dims), a, b, _input(dims), np.float64)
    scale = float(np.abs(ref).max())
    err = float(np.abs(got - ref).max())
    assert err <= 3e-14 * scale, (dims, name, err / scale)
