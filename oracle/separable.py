"""ORACLE (test infrastructure) -- exact spectra of the Swift-Hohenberg Jacobian at states that vary along one axis only.

``J = -L1 + diag(g)`` with ``L1 = (I + Lap)^2`` and ``g = l + 2 nu u - 3 u^2`` (operators.SwiftHohenberg).  ``Lap`` is the Kronecker
sum of the Neumann-ghost second differences ``D_k`` (operators.second_difference).  When ``u`` varies along axis ``a`` only, so does
``g``; the transverse ``D_k`` are diagonalised by the orthonormal DCT-II with eigenvalues ``mu_k,j = -(4/h_k^2) sin^2(pi j / 2 n_k)``
(the symbol of operators.dct_symbol), and ``J`` splits exactly into one dense block of size ``n_a`` per transverse mode pair:

    J_mu = -(I + D_a + mu I)^2 + diag(g),      mu = sum of the transverse eigenvalues.

The union of the blocks' spectra is the spectrum of ``J``.  ``I + D_a + mu I`` has the eigenvalues ``1 + nu_i + mu`` (``nu_i`` those of
``D_a``), so by Weyl's inequality every eigenvalue of ``J_mu`` lies in ``-(1 + nu_i + mu)^2 + [min g, max g]`` for some ``i``: a block
none of whose intervals meets a window has no eigenvalue in it and needs no dense solve.

The Neumann rows of every ``D_k`` (extent >= 2) sum to zero, so a 1-D state extended as a constant along the other axes has the
extended 1-D residual (``sh_profile_residual``): a 1-D steady state is a steady state of the 2-D / 3-D problem.
"""
from __future__ import annotations

import numpy as np

from . import operators


def _symbol(n: int, length: float) -> np.ndarray:
    """Eigenvalues of the n-point Neumann-ghost second difference on [-length, length) (n >= 2), DCT-II mode order."""
    h = 2.0 * length / n
    return -(4.0 / h**2) * np.sin(np.pi * np.arange(n) / (2.0 * n)) ** 2


def _check(dims, ls, axis, profile):
    dims = tuple(int(d) for d in dims)
    if len(dims) not in (2, 3) or len(ls) != len(dims):
        raise ValueError("dims / ls: 2-D or 3-D grids")
    if min(dims) < 2:
        # the 1-point Neumann difference has eigenvalue 0; operators.second_difference(1, ...) gives -1/h^2 instead
        raise ValueError("every extent must be >= 2")
    if not 0 <= axis < len(dims):
        raise ValueError("axis")
    profile = np.asarray(profile, dtype=float).reshape(-1)
    if profile.shape[0] != dims[axis]:
        raise ValueError("profile length != dims[axis]")
    return dims, profile


def extend_profile(dims, axis, profile) -> np.ndarray:
    """The flat x-fastest state vector on ``dims`` that equals ``profile`` along ``axis`` and is constant along the others."""
    dims, profile = _check(dims, (1.0,) * len(dims), axis, profile)
    shape = dims[::-1]                                   # array axes (z, y, x) of a C-ordered reshape of an x-fastest vector
    bshape = [1] * len(dims)
    bshape[len(dims) - 1 - axis] = dims[axis]
    return np.ascontiguousarray(np.broadcast_to(profile.reshape(bshape), shape).reshape(-1))


def sh_profile_residual(n: int, length: float, profile, l: float, nu: float) -> np.ndarray:
    """1-D Neumann-ghost Swift-Hohenberg residual ``-(I + D)^2 u + l u + nu u^2 - u^3`` on ``n >= 2`` points of [-length, length)."""
    if n < 2:
        raise ValueError("n >= 2")
    u = np.asarray(profile, dtype=float).reshape(-1)
    D = operators.second_difference(n, length, operators.NEUMANN).toarray()
    A = np.eye(n) + D
    return -(A @ (A @ u)) + l * u + nu * u**2 - u**3


def transverse_symbols(dims, ls, axis) -> np.ndarray:
    """Every sum ``mu`` of the transverse eigenvalues, one per transverse mode pair (flat, any order)."""
    mus = [_symbol(n, length) for k, (n, length) in enumerate(zip(dims, ls)) if k != axis]
    return sum(np.meshgrid(*mus, indexing="ij")).reshape(-1) if len(mus) > 1 else mus[0].copy()


def sh_separable_spectrum(dims, ls, axis, profile, l, nu, window=None, return_counts=False):
    """Eigenvalues (ascending) of ``-L1 + diag(l + 2 nu u - 3 u^2)`` for the state ``u = extend_profile(dims, axis, profile)``.

    ``window = (lo, hi)``: only the eigenvalues in [lo, hi], with a dense solve only for the blocks whose Weyl intervals meet the
    window.  ``return_counts``: also return (blocks solved, blocks in all)."""
    dims, profile = _check(dims, ls, axis, profile)
    n = dims[axis]
    g = l + 2.0 * nu * profile - 3.0 * profile**2
    D = operators.second_difference(n, ls[axis], operators.NEUMANN).toarray()
    nua = _symbol(n, ls[axis])
    mus = transverse_symbols(dims, ls, axis)
    if window is not None:
        lo, hi = float(window[0]), float(window[1])
        # block mu may hold an eigenvalue in [lo, hi] only if some -(1 + nu_i + mu)^2 + [gmin, gmax] meets it
        c = -(1.0 + nua[None, :] + mus[:, None]) ** 2
        keep = np.any((c + g.max() >= lo) & (c + g.min() <= hi), axis=1)
        todo = mus[keep]
    else:
        todo = mus
    # blocks with equal mu (up to rounding) have equal spectra: solve each distinct value once
    uniq, counts = np.unique(todo, return_counts=True)
    out = []
    for mu, c in zip(uniq, counts):
        A = (1.0 + mu) * np.eye(n) + D
        ev = np.linalg.eigvalsh(-(A @ A) + np.diag(g))
        if window is not None:
            ev = ev[(ev >= lo) & (ev <= hi)]
        out.append(np.repeat(ev, c))
    ev = np.sort(np.concatenate(out)) if out else np.zeros(0)
    return (ev, (len(uniq), len(mus))) if return_counts else ev


def nearest(ev, sigma, k):
    """The ``k`` eigenvalues nearest ``sigma`` (the :LM set of (J - sigma)^-1), sorted by decreasing value."""
    ev = np.asarray(ev)
    return np.sort(ev[np.argsort(np.abs(ev - sigma), kind="stable")[:k]])[::-1]


def spectrum_near(dims, ls, axis, profile, l, nu, sigma, k, r0=0.25):
    """The ``k + 1`` eigenvalues nearest ``sigma``, found by widening a pruned window [sigma - r, sigma + r] until it holds at least
    ``k + 1`` of them.  Returns (eigenvalues sorted by distance to sigma, radius of the final window): every eigenvalue closer than
    the radius is in the list, so the (k+1)-th is the true (k+1)-th and the gap between the k-th and (k+1)-th is exact."""
    r = float(r0)
    while True:
        ev = sh_separable_spectrum(dims, ls, axis, profile, l, nu, window=(sigma - r, sigma + r))
        if ev.size >= k + 1:
            d = np.argsort(np.abs(ev - sigma), kind="stable")
            return ev[d], r
        r *= 2.0
