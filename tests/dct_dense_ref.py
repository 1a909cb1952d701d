"""Dense restatement of the Swift-Hohenberg spectral preconditioner in a chosen precision (helper of test_dct_reference.py and
test_gpu_dct_routes.py; no GPU, no scipy): the orthonormal DCT-II matrices and the eigenvalues of the Neumann-ghost Laplacian
(examples/SH3d.jl:21-32) from their closed forms, one dense product per axis each way and the symbol

    ((1 + lam_x + lam_y [+ lam_z])^2 + shift)^-1,       Pl = (I + Lap)^2 + shift I.

With dtype = np.longdouble (64-bit mantissa on x86-64) it is the reference the scipy oracle is judged by; with np.float64 it is
what a correctly rounded dense implementation -- the HIP kernels' arithmetic -- can be expected to deliver."""
import numpy as np

# the two preconditioner pairings of the reference's examples: lu(L1 + I) and cholesky(Symmetric(L1))
SHIFTS = [1.0, 0.0]


def box(dims):
    """h = pi / 16 on every axis, the spacing of the dense DCT tests."""
    return tuple(np.pi * d / 32 for d in dims)


def _pi(dtype):
    return np.arccos(dtype(-1))


def cosine_matrix(N, dtype=np.float64):
    """T[k][q] = s_k cos(pi (2 q + 1) k / (2 N)), s_0 = sqrt(1 / N), s_k = sqrt(2 / N): orthonormal, T T' = I.  The integer
    argument (2 q + 1) k is reduced mod 4 N exactly before the multiplication by pi."""
    k = np.arange(N, dtype=np.int64)
    arg = np.outer(k, 2 * k + 1) % (4 * N)
    T = np.sqrt(dtype(2) / dtype(N)) * np.cos(_pi(dtype) * arg.astype(dtype) / dtype(2 * N))
    T[0] = np.sqrt(dtype(1) / dtype(N))
    return T


def eigenvalues(N, l, dtype=np.float64):
    """lam[k] = -(4 / h^2) sin^2(pi k / (2 N)), h = 2 l / N."""
    h = dtype(2) * dtype(l) / dtype(N)
    s = np.sin(_pi(dtype) * np.arange(N).astype(dtype) / dtype(2 * N))
    return -(dtype(4) / (h * h)) * s * s


def cosine_mode(N, k):
    """Column k of cosine_matrix(N)' -- the unit-norm eigenvector of index k -- in float64, as a test input."""
    q = np.arange(N, dtype=np.int64)
    return np.sqrt((1.0 if k == 0 else 2.0) / N) * np.cos(np.pi * (((2 * q + 1) * k) % (4 * N)) / (2.0 * N))


def separable_mode(dims, ks):
    """The flat x-fastest product of cosine_mode(N, k) over the axes: a unit-norm eigenvector of the preconditioner."""
    m = cosine_mode(dims[0], ks[0])
    for N, k in zip(dims[1:], ks[1:]):
        m = np.multiply.outer(cosine_mode(N, k), m)
    return m.reshape(-1)


def mode_tuples(dims):
    """The mode indices the single-mode tests use, at most eight per shape: the first and the last mode, the two sides of the
    even / odd seam N/2 - 1 | N/2 of the Makhoul permutation crossed over the axes, and low modes (1, 2[, 0]) rotated through the
    axes, which tell them apart.  Indices are clipped to the extent (N = 3, 4)."""
    nd = len(dims)
    h = [N // 2 for N in dims]
    clip = lambda t: tuple(min(max(int(k), 0), N - 1) for k, N in zip(t, dims))
    out = [clip([0] * nd), clip([N - 1 for N in dims]), clip([h[0] - 1] + h[1:]), clip([h[0]] + [x - 1 for x in h[1:]])]
    out += [clip((1, 2)), clip((2, 1))] if nd == 2 else [clip((1, 2, 0)), clip((2, 0, 1)), clip((0, 1, 2))]
    return out


def symbol(dims, ls, shift, dtype=np.float64):
    """(1 + sum of the axes' eigenvalues)^2 + shift, array axes ([z,] y, x)."""
    lam = [eigenvalues(N, l, dtype) for N, l in zip(dims, ls)]
    s = dtype(1)
    for a, lm in enumerate(lam):
        s = s + lm.reshape([-1 if b == a else 1 for b in range(len(dims) - 1, -1, -1)])
    return s * s + dtype(shift)


def _along(T, a, axis):
    """Apply T along `axis` of a."""
    return np.moveaxis(np.tensordot(T, a, axes=([1], [axis])), 0, axis)


def dense_apply(dims, ls, shift, v, dtype=np.float64):
    """The preconditioner on a flat x-fastest vector in 2-D or 3-D, every table and every product in `dtype`."""
    dims = tuple(int(d) for d in dims)
    assert len(dims) in (2, 3)
    T = [cosine_matrix(N, dtype) for N in dims]
    a = np.asarray(v, dtype=np.float64).astype(dtype).reshape(dims[::-1])
    nd = len(dims)
    for ax in range(nd):                       # array axis nd - 1 - ax holds grid axis ax
        a = _along(T[ax], a, nd - 1 - ax)
    a = a / symbol(dims, ls, shift, dtype)
    for ax in range(nd):
        a = _along(T[ax].T, a, nd - 1 - ax)
    return a.reshape(-1)
