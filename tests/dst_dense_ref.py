"""Dense restatement of the cGL sine-transform preconditioners in a chosen precision (helper of test_dst_reference.py and
test_gpu_dst_transforms.py; no GPU, no scipy): the DST-I matrices and eigenvalues of the Dirichlet Laplacian
(examples/cGL2d.jl:6-22) from their closed forms, two dense products each way and the 2 x 2 symbol

    (Lap (x) I_2 + [[a, -b], [b, a]])^-1,       Laplace preconditioner (Lap - c)^-1: a = -c, b = 0.

With dtype = np.longdouble (64-bit mantissa on x86-64) it is the reference the scipy oracle is judged by; with np.float64 it is
what a correctly rounded dense implementation -- the HIP kernels' arithmetic -- can be expected to deliver."""
import numpy as np

# the two symbol cases every test uses: (name, a, b)
SYMBOLS = [("laplace", -1.0, 0.0), ("block", 0.5, 1.0)]


def box(dims):
    """h = pi / 16 on every axis, the spacing of the dense DCT tests."""
    return tuple(np.pi * d / 32 for d in dims)


def _pi(dtype):
    return np.arccos(dtype(-1))


def sine_matrix(N, dtype=np.float64):
    """S[k][j] = sqrt(2 / (N + 1)) sin(pi (k + 1)(j + 1) / (N + 1)): symmetric and its own inverse.  The integer argument is reduced
    mod 2 (N + 1) exactly before the multiplication by pi."""
    k = np.arange(1, N + 1, dtype=np.int64)
    arg = np.outer(k, k) % (2 * (N + 1))
    return np.sqrt(dtype(2) / dtype(N + 1)) * np.sin(_pi(dtype) * arg.astype(dtype) / dtype(N + 1))


def eigenvalues(N, l, dtype=np.float64):
    """lam[k] = -(4 / h^2) sin^2(pi (k + 1) / (2 (N + 1))), h = 2 l / N."""
    h = dtype(2) * dtype(l) / dtype(N)
    s = np.sin(_pi(dtype) * np.arange(1, N + 1).astype(dtype) / dtype(2 * (N + 1)))
    return -(dtype(4) / (h * h)) * s * s


def sine_mode(N, k):
    """Column k of sine_matrix(N) in float64, as a test input."""
    j = np.arange(1, N + 1, dtype=np.int64)
    return np.sqrt(2.0 / (N + 1)) * np.sin(np.pi * ((j * (k + 1)) % (2 * (N + 1))) / (N + 1))


def dense_apply(dims, ls, a, b, v, dtype=np.float64):
    """The preconditioner on the flat stacked vector [u1; u2] (x fastest), every table and every product in `dtype`."""
    n0, n1 = dims
    S0, S1 = sine_matrix(n0, dtype), sine_matrix(n1, dtype)
    m = eigenvalues(n1, ls[1], dtype)[:, None] + eigenvalues(n0, ls[0], dtype)[None, :] + dtype(a)
    det = m * m + dtype(b) * dtype(b)
    x = np.asarray(v, dtype=np.float64).astype(dtype).reshape(2, n1, n0)
    s1, s2 = (S1 @ (f @ S0) for f in x)
    y1 = (m * s1 + dtype(b) * s2) / det
    y2 = (m * s2 - dtype(b) * s1) / det
    return np.stack([S1 @ (y @ S0) for y in (y1, y2)]).reshape(-1)
