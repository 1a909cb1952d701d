"""The cGL sine-transform preconditioners (bk_precond_lap_create, bk_precond_cgl_create: DST-I forward, symbol, DST-I back) on every
route of dst_apply (csrc/dct.hip), at the smallest shapes that reach each one, against the exact CPU operator
oracle.operators.dst_block_preconditioner_cgl (itself pinned to a long-double dense restatement by tests/test_dst_reference.py):

  1. direct       dct_axis_direct, one thread per output: extents below 32, and option dct_gemm = 0;
  2. guarded MFMA gemm_f64_any_kernel through dense_gemm_axis_pass with the two fields as a batch of 2: extents from 32 on;
  3. folded MFMA  fold_x/y_kernel, the unguarded half-size gemm_f64_kernel, unfold_x/y_kernel, the spectrum in the permuted order
                  [even k | odd k] and the symbol kernels on the permuted tables: n0 % 128 == 0 and n1 % 256 == 0 (option dst_mfma).

Random vectors bound every path; single sine modes name the mode whose coefficient is wrong (a bad even/odd table, a bad order of
the permuted eigenvalues); point sources sit on the mirror line of fold / unfold; aliasing and the left-inverse close the file.
The last test reaches the second row-tile slice of dense_gemm_axis_pass (more than 65535 * 128 rows) through the Swift-Hohenberg
preconditioner.  Every option a test sets is restored in a finally block: the context is the session's."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import probe
from dst_dense_ref import SYMBOLS, box, eigenvalues, sine_mode
from oracle import operators

pytestmark = pytest.mark.gpu

FOLDED = [(128, 256),      # one tile everywhere
          (384, 256),      # three column tiles in the x products (h = 192 = 3 * 64)
          (128, 768)]      # three row tiles in the y products (h = 384 = 3 * 128)
OFF_FOLDED = [(126, 256), (130, 254), (128, 255)]                 # guarded product with overhang and odd K
MIXED = [(40, 24), (24, 40), (31, 33), (32, 31), (33, 32)]        # routes 1 and 2 mixed across the axes, the switch at 32

DEFAULTS = dict(dst_mfma=1, dct_gemm=1)
GEMM_PATHS = {"mfma_guarded": dict(dst_mfma=0, dct_gemm=1), "rocblas": dict(dst_mfma=0, dct_gemm=2),
              "direct": dict(dst_mfma=0, dct_gemm=0)}
FOLDED_PATHS = dict({"mfma_folded": dict(dst_mfma=1, dct_gemm=1)}, **GEMM_PATHS)

# Error of one application relative to max|ref|.  A plain float64 dense restatement of the same four products errs by 6.3e-15 to
# 1.9e-14 against an 80-bit reference at these shapes (tests/test_dst_reference.py holds it to 3e-14), the scipy oracle by 7e-16:
# 1e-13 is five times the worst of them, and the bound of the project's FFT path.  (Measured on an MI355X: at most 3.3e-15 on every
# path, at (384, 256) with the Laplace symbol; the guarded MFMA product and the direct kernel agree bitwise -- the fp64 MFMA
# accumulates along k in the order of the direct kernel's fma chain.)
BOUND, TIGHT = 1e-13, 3e-14


def _hip():
    from bk_amd import hip
    return hip


@contextlib.contextmanager
def _options(ctx, **kv):
    try:
        for k, v in kv.items():
            ctx.set_option(k, v)
        yield
    finally:
        for k, v in DEFAULTS.items():
            ctx.set_option(k, v)


def _precond(ctx, dims, a, b):
    """(problem, preconditioner) of a symbol case: b = 0 is the Laplace preconditioner (Lap - c)^-1 with c = -a, else the block one.
    The problem carries nu = b, so that its Jacobian at u = 0 with r = a is the operator the preconditioner inverts."""
    hip = _hip()
    prob = hip.CGL2d(ctx, dims, box(dims), nu=b)
    P = hip.LaplacePreconditioner(prob, -a) if b == 0.0 else hip.CGLBlockPreconditioner(prob, a, b)
    return prob, P


def _oracle(dims, a, b):
    return operators.dst_block_preconditioner_cgl(dims, box(dims), a, b)


def _random(dims):
    return np.random.default_rng(1000 * dims[0] + dims[1]).standard_normal(2 * dims[0] * dims[1])


@functools.lru_cache(maxsize=None)
def _random_ref(dims, a, b):
    ref = _oracle(dims, a, b)(_random(dims))
    ref.setflags(write=False)
    return ref


def _probe_all(items):
    """probe() every (name, value, bound, info) -- all of them are logged before the first failure is raised."""
    bad = []
    for name, value, bound, info in items:
        try:
            probe(name, value, bound, tight=TIGHT * bound / BOUND, **info)
        except AssertionError as e:
            bad.append(e.args[0])
    assert not bad, bad


def _apply_paths(ctx, P, V, paths):
    got = {}
    for path, opts in paths.items():
        with _options(ctx, **opts):
            got[path] = P.ldiv(V).numpy()
    return got


# ---------------------------------------------------------------------------------- 1. every path, random vector
@pytest.mark.parametrize("name,a,b", SYMBOLS)
@pytest.mark.parametrize("dims", FOLDED + OFF_FOLDED + MIXED)
def test_every_path_against_the_exact_operator(ctx, dims, name, a, b):
    """max|got - ref| <= 1e-13 max|ref| for every path the shape can take, and the paths agree pairwise within the same bound."""
    prob, P = _precond(ctx, dims, a, b)
    ref = _random_ref(dims, a, b)
    scale = float(np.abs(ref).max())
    paths = FOLDED_PATHS if dims in FOLDED else GEMM_PATHS
    got = _apply_paths(ctx, P, prob.vec(_random(dims)), paths)
    info = dict(dims=list(dims), symbol=name)
    items = [("dst_path_vs_oracle", np.abs(g - ref).max() / scale, BOUND, dict(info, path=p)) for p, g in got.items()]
    keys = list(got)
    items += [("dst_path_vs_path", np.abs(got[p] - got[q]).max() / scale, BOUND, dict(info, path=p, other=q))
              for i, p in enumerate(keys) for q in keys[i + 1:]]
    _probe_all(items)


# ---------------------------------------------------------------------------------- 2. single modes
@pytest.mark.parametrize("name,a,b", SYMBOLS)
@pytest.mark.parametrize("dims", [(128, 256), (384, 256)])
def test_single_sine_modes_pin_the_permuted_spectrum(ctx, dims, name, a, b):
    """Input e1 (x) sin-mode(kx, ky): the output is the same mode in both fields with the coefficients (m, -b) / (m^2 + b^2),
    m = lam_x + lam_y + a (Laplace: 1 / (lam_x + lam_y - c) and zero).  The first and the last mode, the four around the seam of the
    permuted order [even k | odd k] at h = N / 2 and two low modes that tell x from y, on the folded path and on the guarded one.
    Both the coefficient recovered by projection and the pointwise remainder are held to 1e-13 of the larger coefficient (the
    float64 dense restatement and the scipy oracle give at most 8e-16 and 1e-16 of it on the CPU)."""
    n0, n1 = dims
    h0, h1 = n0 // 2, n1 // 2
    lx, ly = eigenvalues(n0, box(dims)[0]), eigenvalues(n1, box(dims)[1])
    prob, P = _precond(ctx, dims, a, b)
    items = []
    for kx, ky in [(0, 0), (n0 - 1, n1 - 1), (h0 - 1, h1), (h0, h1 - 1), (1, 2), (2, 1)]:
        mode = np.outer(sine_mode(n1, ky), sine_mode(n0, kx)).reshape(-1)
        m = lx[kx] + ly[ky] + a
        coef = np.array([m, -b]) / (m * m + b * b)
        cmax = float(np.abs(coef).max())
        V = prob.vec(np.concatenate([mode, np.zeros_like(mode)]))
        got = _apply_paths(ctx, P, V, {"mfma_folded": FOLDED_PATHS["mfma_folded"], "mfma_guarded": GEMM_PATHS["mfma_guarded"]})
        for path, g in got.items():
            g = g.reshape(2, -1)
            info = dict(dims=list(dims), symbol=name, path=path, mode=[kx, ky])
            items.append(("dst_mode_coefficient", max(abs(float(g[f] @ mode) - coef[f]) for f in range(2)) / cmax, BOUND, info))
            items.append(("dst_mode_remainder", max(np.abs(g[f] - coef[f] * mode).max() for f in range(2)) / cmax, BOUND, info))
    _probe_all(items)


# ---------------------------------------------------------------------------------- 3. point sources
@pytest.mark.parametrize("name,a,b", SYMBOLS)
def test_point_sources_pin_fold_and_unfold_at_the_mirror_line(ctx, name, a, b):
    """Unit impulses in field 2 at the corners, on either side of the mirror line j = h - 1 | h of both folds, and across it."""
    dims = n0, n1 = (128, 256)
    h0, h1 = n0 // 2, n1 // 2
    prob, P = _precond(ctx, dims, a, b)
    Po = _oracle(dims, a, b)
    items = []
    for j0, j1 in [(0, 0), (n0 - 1, n1 - 1), (h0 - 1, h1 - 1), (h0, h1), (h0 - 1, h1), (0, n1 - 1)]:
        v = np.zeros(2 * n0 * n1)
        v[n0 * n1 + j1 * n0 + j0] = 1.0
        ref = Po(v)
        scale = float(np.abs(ref).max())
        got = _apply_paths(ctx, P, prob.vec(v), {"mfma_folded": FOLDED_PATHS["mfma_folded"], "mfma_guarded": GEMM_PATHS["mfma_guarded"]})
        items += [("dst_point_source", np.abs(g - ref).max() / scale, BOUND, dict(dims=list(dims), symbol=name, path=p, at=[j0, j1]))
                  for p, g in got.items()]
    _probe_all(items)


# ---------------------------------------------------------------------------------- 4. aliasing, determinism
@pytest.mark.parametrize("name,a,b", SYMBOLS)
@pytest.mark.parametrize("dims", [(128, 256), (130, 254)])
def test_in_place_application_and_determinism_are_bitwise(ctx, dims, name, a, b):
    """bk_precond_apply(P, w, w) -- out aliasing in, which dst_apply promises is safe -- equals the out-of-place result bitwise, on
    the folded route and on the guarded one; so do two applications of the same input, which is left untouched."""
    prob, P = _precond(ctx, dims, a, b)
    v = _random(dims)
    V = prob.vec(v)
    first, second = P.ldiv(V).numpy(), P.ldiv(V).numpy()
    assert np.array_equal(V.numpy(), v)
    assert np.array_equal(first, second)
    W = V.copy()
    ctx.check(ctx.lib.bk_precond_apply(P.h, C.c_void_p(W.t.data_ptr()), C.c_void_p(W.t.data_ptr())), "bk_precond_apply")
    assert np.array_equal(W.numpy(), first)
    assert np.isfinite(first).all() and np.abs(first).max() > 0.0


# ---------------------------------------------------------------------------------- 5. left inverse
@pytest.mark.parametrize("name,a,b", SYMBOLS)
@pytest.mark.parametrize("dims", FOLDED)
def test_left_inverse_of_the_trivial_state_jacobian(ctx, dims, name, a, b):
    """P (J0 v) = v with J0 the Jacobian at u = 0 (r = a, nu = b; Laplace: r = -c, nu = 0).  The stencil evaluates J0 v with an
    absolute rounding error of a few eps (|Lap|_inf + |a| + |b|) max|v| per entry, and the exact inverse amplifies it by at most
    |P| = 1 / min over the modes of |symbol| = 1 / min sqrt(m^2 + b^2), from the closed-form eigenvalues: 64 eps of that product
    (about 1e-11 max|v| here), in place of the flat 1e-9 used at 1024^2."""
    hip = _hip()
    n = dims[0] * dims[1]
    prob, P = _precond(ctx, dims, a, b)
    v = _random(dims)
    V = prob.vec(v)
    J0 = prob.jacobian(hip.HipVec.from_numpy(ctx, np.zeros(2 * n)), a)
    back = P.ldiv(J0(V)).numpy()
    hs = [2.0 * l / d for l, d in zip(box(dims), dims)]
    lap_inf = sum(4.0 / h ** 2 for h in hs)
    m = eigenvalues(dims[1], box(dims)[1])[:, None] + eigenvalues(dims[0], box(dims)[0])[None, :] + a
    pnorm = 1.0 / float(np.sqrt(m * m + b * b).min())
    bound = 64 * np.finfo(float).eps * (lap_inf + abs(a) + abs(b)) * pnorm * float(np.abs(v).max())
    probe("dst_left_inverse", float(np.abs(back - v).max()), bound, tight=bound / 4, dims=list(dims), symbol=name)


# ---------------------------------------------------------------------------------- row tiles beyond 65535
def _cos_mode(N, k):
    """cos(pi k (j + 1/2) / N), the DCT-II eigenvector of the Neumann-ghost Laplacian (examples/SH3d.jl:21-32), argument reduced exactly."""
    j = np.arange(N, dtype=np.int64)
    return np.cos(np.pi * (((2 * j + 1) * k) % (4 * N)) / (2.0 * N))


def test_dense_x_pass_beyond_65535_row_tiles(ctx):
    """dense_gemm_axis_pass slices the row tiles of an x pass in steps of 65535 (a 16-bit launch dimension) and offsets A and C per
    slice.  (33, 1024, 8192) has 8 388 608 rows = 65536 tiles of 128: exactly one tile -- the last 128 rows -- falls in the second
    slice.  Input: five separable cosine eigenmodes, among them kx = 0 and kx = 32 = N0 - 1; expected: each divided by
    (1 + lam_x + lam_y + lam_z)^2 + 1.  Both are formed on the device from 1-D host tables (2.2 GB per vector: nothing of that size
    touches the host), and compared to the project's dense bound 1e-12 over the whole array and over the last 128 rows alone.
    Wall time on an MI355X: 1.1 s (measured error: 2.7e-15 of max|ref| overall, 2.4e-15 on the last tile)."""
    import torch
    hip = _hip()
    dims = n0, n1, n2 = (33, 1024, 8192)
    ls = box(dims)
    modes = [(0, 3, 5), (32, 1, 2), (7, 0, 11), (16, 40, 0), (1, 100, 300)]
    dev = ctx.torch_device
    lam = [-(4.0 / (2.0 * l / N) ** 2) * np.sin(np.pi * np.arange(N) / (2.0 * N)) ** 2 for N, l in zip(dims, ls)]
    prob = P = None
    try:
        u = torch.zeros(n2, n1, n0, dtype=torch.float64, device=dev)
        ref = torch.zeros_like(u)
        for kx, ky, kz in modes:
            cx, cy, cz = (torch.from_numpy(_cos_mode(N, k)).to(dev) for N, k in zip(dims, (kx, ky, kz)))
            term = (cz[:, None] * cy[None, :])[:, :, None] * cx[None, None, :]
            u += term
            ref.add_(term, alpha=1.0 / ((1.0 + lam[0][kx] + lam[1][ky] + lam[2][kz]) ** 2 + 1.0))
            del term
        u, ref = u.reshape(-1), ref.reshape(-1)
        tail = slice(u.numel() - 128 * n0, u.numel())                     # the rows of the second slice
        assert float(u[tail].abs().max()) > 0.0 and float(ref[tail].abs().max()) > 0.0
        prob = hip.SwiftHohenberg(ctx, dims, ls)
        P = hip.DCTPreconditioner(prob, 1.0)
        got = P.ldiv(hip.HipVec(ctx, u, prob.nglobal))
        ctx.sync()
        scale = float(ref.abs().max())
        err = got.t.sub_(ref).abs_()
        info = dict(dims=list(dims))
        _probe_all([("dense_row_slices_all", float(err.max()) / scale, 1e-12, info),
                    ("dense_row_slices_last_tile", float(err[tail].max()) / scale, 1e-12, info)])
    finally:
        del prob, P
        u = ref = got = err = None
        torch.cuda.empty_cache()
