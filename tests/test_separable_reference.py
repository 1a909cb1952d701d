"""The separable reference (oracle/separable.py) against the assembled oracle operator: the exact spectrum of the Swift-Hohenberg
Jacobian at a state that varies along one axis, its Weyl-pruned form, and the 1-D residual of an extended profile.  CPU only."""
import numpy as np
import pytest

from oracle import operators, palc
from oracle import separable as S

L, NU = 0.1, 1.2


def _profile(n, seed, amp=0.9):
    return amp * np.random.default_rng(seed).standard_normal(n)


# odd and even extents, unequal box lengths, extents 2 included (the smallest Neumann block with rows summing to zero)
CASES = [((12, 6, 5), (3.0, 2.1, 1.7)), ((7, 6, 4), (1.3, 2.9, 2.2)), ((5, 2, 9), (2.4, 1.1, 3.3)),
         ((9, 8), (2.5, 1.9)), ((6, 11), (1.7, 3.1))]


@pytest.mark.parametrize("dims,ls", CASES)
def test_separable_spectrum_is_the_dense_spectrum(dims, ls):
    """Union of the per-mode blocks' spectra == eigvalsh of the assembled -L1 + diag(g), for a profile along every axis.
    Both sides are backward stable: the difference is a few eps times |J|."""
    sh = operators.SwiftHohenberg(dims, ls)
    for axis in range(len(dims)):
        prof = _profile(dims[axis], seed=10 * axis + len(dims))
        u = S.extend_profile(dims, axis, prof)
        ref = np.linalg.eigvalsh(sh.J(u, L, NU).toarray())
        ev = S.sh_separable_spectrum(dims, ls, axis, prof, L, NU)
        assert ev.shape == ref.shape
        assert np.abs(ev - ref).max() <= 64 * np.finfo(float).eps * np.abs(ref).max(), (dims, axis)


@pytest.mark.parametrize("dims,ls", CASES)
def test_pruned_spectrum_equals_the_unpruned_one_in_the_window(dims, ls):
    """Weyl pruning drops only blocks with no eigenvalue in the window: the same eigenvalues, bitwise (the kept blocks are solved the
    same way), and on these grids at least one block is actually skipped."""
    for axis in range(len(dims)):
        prof = _profile(dims[axis], seed=7 + axis)
        ev = S.sh_separable_spectrum(dims, ls, axis, prof, L, NU)
        for lo, hi in ((-0.5, 0.4), (-3.0, 0.1), (ev[-3], ev[-1])):
            evw, (solved, total) = S.sh_separable_spectrum(dims, ls, axis, prof, L, NU, window=(lo, hi), return_counts=True)
            assert np.array_equal(evw, ev[(ev >= lo) & (ev <= hi)]), (dims, axis, lo, hi)
            assert solved <= total
        _, (solved, total) = S.sh_separable_spectrum(dims, ls, axis, prof, L, NU, window=(-0.5, 0.4), return_counts=True)
        assert solved < total, (dims, axis)


def test_spectrum_near_sigma_is_complete():
    """spectrum_near widens its window until it holds k + 1 eigenvalues: they are the k + 1 nearest sigma of the full spectrum."""
    dims, ls = (16, 9, 6), (3.1, 2.3, 1.9)
    for axis in range(3):
        prof = _profile(dims[axis], seed=axis, amp=0.5)
        ev = S.sh_separable_spectrum(dims, ls, axis, prof, L, NU)
        near, r = S.spectrum_near(dims, ls, axis, prof, L, NU, 0.1, 15, r0=1e-3)
        want = ev[np.argsort(np.abs(ev - 0.1), kind="stable")[:16]]
        assert np.array_equal(np.sort(near[:16]), np.sort(want)) and np.abs(near[:16] - 0.1).max() <= r
        assert np.array_equal(S.nearest(ev, 0.1, 15), np.sort(want[:15])[::-1])


def test_extend_profile_layout():
    """x-fastest flat layout (operators.SwiftHohenberg.guess): index i + nx (j + ny k)."""
    dims = (4, 3, 5)
    for axis in range(3):
        prof = np.arange(dims[axis], dtype=float) + 1.0
        u = S.extend_profile(dims, axis, prof).reshape(dims[::-1])           # [k, j, i]
        k, j, i = np.meshgrid(*[np.arange(n) for n in dims[::-1]], indexing="ij")
        assert np.array_equal(u, prof[(i, j, k)[axis]])
    u2 = S.extend_profile((4, 3), 1, np.array([1.0, 2.0, 3.0])).reshape(3, 4)
    assert np.array_equal(u2, np.repeat([[1.0], [2.0], [3.0]], 4, axis=1))
    with pytest.raises(ValueError):
        S.extend_profile((4, 1, 3), 0, np.zeros(4))                       # the oracle's 1-point Neumann difference is not zero


@pytest.mark.parametrize("n", [8, 13])
def test_residual_of_an_extended_profile_is_the_extended_1d_residual(n):
    """F on (n, 2) / (n, 2, 2) / (2, n, 2) / (2, 2, n) of an extended profile == the 1-D residual extended (the transverse Neumann
    rows sum to zero), to the rounding of two 25-term stencil sums; hence a 1-D steady state is an exact discrete steady state."""
    length = 2.7
    prof = _profile(n, seed=n, amp=0.8)
    r1 = S.sh_profile_residual(n, length, prof, L, NU)
    for dims, ls, axis in (((n, 2), (length, 1.3), 0), ((2, n), (0.9, length), 1), ((n, 2, 2), (length, 1.3, 0.7), 0),
                           ((2, n, 2), (1.1, length, 0.6), 1), ((2, 2, n), (0.8, 1.4, length), 2)):
        sh = operators.SwiftHohenberg(dims, ls)
        F = sh.F(S.extend_profile(dims, axis, prof), L, NU)
        h = min(2.0 * x / m for x, m in zip(ls, dims))
        floor = 64 * np.finfo(float).eps * (1.0 + 4.0 * len(dims) / h**2) ** 2 * np.abs(prof).max()
        assert np.abs(F - S.extend_profile(dims, axis, r1)).max() <= floor, (dims, axis)
    # a Newton solution of the 1-D problem is a steady state of (2, 2, n)
    D = operators.second_difference(n, length, operators.NEUMANN).toarray()
    A = np.eye(n) + D
    u = 0.5 * np.cos(np.pi * (np.arange(n) + 0.5) / n)
    for _ in range(40):
        J1 = -(A @ A) + np.diag(L + 2 * NU * u - 3 * u**2)
        u = u - np.linalg.solve(J1, S.sh_profile_residual(n, length, u, L, NU))
    assert palc.norminf(S.sh_profile_residual(n, length, u, L, NU)) < 1e-12
    sh = operators.SwiftHohenberg((2, 2, n), (0.8, 1.4, length))
    assert palc.norminf(sh.F(S.extend_profile((2, 2, n), 2, u), L, NU)) < 1e-11
