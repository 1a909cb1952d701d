"""The reference of the Swift-Hohenberg DCT route tests (tests/test_gpu_dct_routes.py) under test itself.  CPU only.

oracle.operators.dct_preconditioner (scipy's DCT-II) and dct_symbol against an independent dense restatement in np.longdouble
(tests/dct_dense_ref.py), and the float64 version of that restatement against the long-double one: the second number is what a
correctly rounded dense fp64 implementation of the same products delivers, and the shift-0 bound of the GPU file is five times it.
On every small shape of the GPU file's route table (tests/test_dct_coverage_host.py checks the list), box h = pi / 16.

Measured on x86-64 (worst over DIMS of max|got - ref| / max|ref| against the long-double restatement):

    shift 1 (|Pl^-1| <= 1):          float64 dense 2.8e-15 at (16, 16, 512),   scipy oracle 8.7e-16 at (40, 24)
    shift 0 (|Pl^-1| 1e5 .. 7e8):    float64 dense 1.4e-12 at (33, 64),        scipy oracle 5.1e-12 at (33, 64)

Each is held to three times its worst value (F64_DENSE_WORST, ORACLE_WORST below).  At shift 0 the error follows the conditioning of
the shape: the symbol (1 + lam_x + lam_y [+ lam_z])^2 is the square of a cancelling sum, and the mode (2, 1) of (33, 64) leaves
1.4e-9 of it (|Pl^-1| = 7e8), where most shapes keep 1e-5 and err by 2.5e-14 (float64 dense) and 4.5e-14 (oracle); N = 256 .. 1024
on a box of that length comes close to the critical circle too and gives 1e-13 .. 4e-13.  dct_symbol is held to the rounding of that
sum (test_oracle_symbol_against_the_long_double_one; measured: 1.2e-15 of each entry at shift 1, 5.1e-12 at shift 0).

The eigen-relation dense_apply(mode) = mode / symbol, for the mode tuples of dct_dense_ref.mode_tuples on the shapes on which the GPU
file runs its single-mode test, shift 1: the long-double restatement leaves at most 1.1e-14 of the coefficient pointwise and
4.5e-16 in the projected coefficient -- the input mode is a float64 vector, so it carries 1e-16 of every other mode, and a mode
with symbol ~1e5 sits next to modes with symbol ~1.  (At shift 0, with symbols down to 1e-9, the same rounding of the INPUT leaves
up to 2e-6 of the coefficient: the relation is no test of an implementation there, and the GPU file runs it at shift 1 only.)
The float64 restatement gives 8.9e-15 and the scipy oracle 5.8e-14 (the Bluestein transform at N = 33) pointwise."""
import functools

import numpy as np
import pytest

from dct_dense_ref import SHIFTS, box, dense_apply, eigenvalues, mode_tuples, separable_mode, symbol
from oracle import operators

assert np.finfo(np.longdouble).eps < 1e-18, "the long-double reference needs a 64-bit mantissa (x86-64)"

# every dims of the route table of tests/test_gpu_dct_routes.py but its one large shape (64, 256, 256): 4 M points, whose
# long-double products would take minutes
DIMS = [(4, 8, 16), (16, 1024), (1024, 16), (9, 64), (15, 64, 64), (33, 64), (24, 64), (64, 8), (64, 3, 4), (64, 24),
        (64, 16), (16, 512), (32, 256), (64, 128), (128, 64), (64, 64, 64), (48, 128, 64), (16, 16, 512),
        (256, 64), (128, 64, 64), (128, 512), (64, 64), (40, 24)]
# the shapes of the GPU file's single-mode test
MODE_DIMS = [(4, 8, 16), (33, 64), (15, 64, 64), (64, 24), (128, 64), (64, 64, 64), (16, 16, 512), (256, 64)]

# worst measured relative error per shift (docstring); the GPU file's shift-0 bound is 5 * F64_DENSE_WORST[0.0]
F64_DENSE_WORST = {1.0: 2.8e-15, 0.0: 1.4e-12}
ORACLE_WORST = {1.0: 8.7e-16, 0.0: 5.1e-12}
MARGIN = 3.0


def _input(dims):
    return np.random.default_rng(1000 * dims[0] + dims[1]).standard_normal(int(np.prod(dims)))


@functools.lru_cache(maxsize=None)
def _longdouble(dims, shift):
    return dense_apply(dims, box(dims), shift, _input(dims), np.longdouble)


def _rel(got, ref):
    return float(np.abs(got - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("dims", DIMS)
def test_scipy_oracle_against_the_long_double_dense_restatement(dims, shift):
    """One orthonormal FFT-based DCT-II per axis each way and one division per entry."""
    err = _rel(operators.dct_preconditioner(dims, box(dims), shift)(_input(dims)), _longdouble(dims, shift))
    print("oracle", dims, shift, err)
    assert err <= MARGIN * ORACLE_WORST[shift], (dims, shift, err)


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("dims", DIMS)
def test_float64_dense_restatement_against_the_long_double_one(dims, shift):
    """What the GPU bounds rest on: the same dense products with float64 tables and float64 accumulation."""
    err = _rel(dense_apply(dims, box(dims), shift, _input(dims), np.float64), _longdouble(dims, shift))
    print("float64", dims, shift, err)
    assert err <= MARGIN * F64_DENSE_WORST[shift], (dims, shift, err)


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("dims", DIMS)
def test_oracle_symbol_against_the_long_double_one(dims, shift):
    """dct_symbol is what the tests take |Pl^-1| = 1 / min from.  t = 1 + lam_x + lam_y [+ lam_z] is a cancelling float64 sum of
    terms up to S = 1 + sum of max|lam|: |dt| <= 4 eps S (each eigenvalue to 2 ulp, three additions), so the symbol t^2 + shift is
    off by at most 2 |t| dt + dt^2 plus its own rounding, eps of the entry."""
    ls = box(dims)
    ref = symbol(dims, ls, shift, np.longdouble)
    got = operators.dct_symbol(dims, ls, shift)
    assert got.shape == ref.shape
    eps = np.finfo(float).eps
    dt = 4 * eps * (1.0 + sum(float(np.abs(eigenvalues(N, l)).max()) for N, l in zip(dims, ls)))
    bound = 2 * np.sqrt(np.abs(ref - shift)) * dt + dt * dt + eps * np.abs(ref)
    print("symbol", dims, shift, float((np.abs(got - ref) / np.abs(ref)).max()))
    assert (np.abs(got - ref) <= bound).all(), (dims, shift, float((np.abs(got - ref) / bound).max()))


@pytest.mark.parametrize("dims", MODE_DIMS)
def test_eigen_relation_of_the_long_double_restatement(dims):
    """dense_apply(mode) = mode / ((1 + lam_x + lam_y [+ lam_z])^2 + 1) in long double, on float64 input modes: the coefficient
    recovered by projection and the pointwise remainder, relative to the coefficient (measured: 4.5e-16 and 1.1e-14; held to three
    times that).  This is the figure the GPU file's bound 1e-13 is to be read against."""
    ls = box(dims)
    lam = [eigenvalues(N, l, np.longdouble) for N, l in zip(dims, ls)]
    worst = [0.0, 0.0]
    for ks in mode_tuples(dims):
        mode = separable_mode(dims, ks)
        coef = 1 / ((1 + sum(lm[k] for lm, k in zip(lam, ks))) ** 2 + 1)
        got = dense_apply(dims, ls, 1.0, mode, np.longdouble)
        worst[0] = max(worst[0], float(abs(got @ mode.astype(np.longdouble) - coef) / coef))
        worst[1] = max(worst[1], float(np.abs(got - coef * mode).max() / coef))
    print("eigen", dims, worst)
    assert worst[0] <= 1.4e-15 and worst[1] <= 3.3e-14, (dims, worst)
