"""Plain host references of the stencil operators of ``csrc/stencil.hip`` -- Swift-Hohenberg 2-D / 3-D, 1-D cubic-quintic
Swift-Hohenberg, 2-D complex Ginzburg-Landau and the parameter derivatives -- written from the operators' definitions
(``oracle/operators.py``: second differences, A = I + Lap applied twice, the pointwise terms), not from the kernels.

Every function is generic in its array type:

* ``Ex`` arrays: exact dyadic rationals ``num / 2^sh`` with int64 numerators.  Integer data and dyadic coefficients (-0.5, 2,
  0.25, 0.75, mesh widths 1, 2, 4) go in; the exact result comes out together with ``bnd``, the sum of the absolute values of
  all terms of the fully expanded polynomial in units of the finest granularity ``2^-sh`` (max-norm over the grid).  When
  ``bnd < 2^53`` every product and every partial sum of ANY evaluation order, fused or not, is a multiple of ``2^-sh`` below
  ``2^53`` units, i.e. an exact double: a correct kernel must then return ``Ex.exact()`` bit for bit.
* ``np.longdouble`` arrays: the same formulas in a 64-bit mantissa, for random real data.

Arrays are C-ordered ``(nz, ny, nx)`` / ``(ny, nx)`` / ``(2, ny, nx)`` (x fastest, as the flat device vectors).
"""
import numpy as np

LIMIT = 2 ** 53


def _dyadic(x):
    """float -> (numerator, log2 denominator); every finite double is a dyadic rational."""
    num, den = float(x).as_integer_ratio()
    sh = den.bit_length() - 1
    assert den == 1 << sh
    return num, sh


class Ex:
    """Exact dyadic array ``num / 2^sh`` (int64 numerators, or a Python int for a scalar) with the bound ``bnd``: a Python
    int >= the sum of absolute values of all expanded terms of any entry, in units of ``2^-sh``."""

    __slots__ = ("num", "sh", "bnd")

    def __init__(self, num, sh, bnd):
        assert bnd < 2 ** 62, "numerators would leave int64"
        self.num, self.sh, self.bnd = num, int(sh), int(bnd)

    @classmethod
    def of(cls, x):
        if isinstance(x, Ex):
            return x
        if isinstance(x, np.ndarray):
            assert x.dtype == np.int64, "integer data only: real data goes through the longdouble evaluation"
            return cls(x, 0, int(np.abs(x).max(initial=0)))
        num, sh = _dyadic(x)
        return cls(num, sh, abs(num))

    def _at(self, sh):
        k = sh - self.sh
        assert k >= 0
        return self.num * (1 << k), self.bnd << k

    def __add__(self, o):
        o = Ex.of(o)
        sh = max(self.sh, o.sh)
        (a, ab), (b, bb) = self._at(sh), o._at(sh)
        return Ex(a + b, sh, ab + bb)

    def __neg__(self):
        return Ex(-self.num, self.sh, self.bnd)

    def __sub__(self, o):
        return self + (-Ex.of(o))

    def __mul__(self, o):
        o = Ex.of(o)
        assert self.bnd * o.bnd < 2 ** 62, "numerators would leave int64"
        return Ex(self.num * o.num, self.sh + o.sh, self.bnd * o.bnd)

    __radd__ = __add__
    __rmul__ = __mul__

    def __rsub__(self, o):
        return Ex.of(o) - self

    def map(self, f):
        """An index operation (pad, slice, reshape, concatenate): no arithmetic, the bound stays."""
        return Ex(f(self.num), self.sh, self.bnd)

    def sum(self):
        return Ex(int(self.num.sum()), self.sh, self.bnd * self.num.size)

    def matvec_from(self, M):
        """M @ self for an int64 matrix M."""
        return Ex(M @ self.num, self.sh, int(np.abs(M).sum(axis=1).max()) * self.bnd)

    def exact(self):
        """The exact value as float64; asserts the condition that makes a bitwise comparison valid."""
        assert self.bnd < LIMIT, f"sum of |terms| = {self.bnd} units of 2^-{self.sh} is not below 2^53: narrow the data"
        return np.ldexp(np.asarray(self.num, dtype=np.float64), -self.sh)

    @property
    def bits(self):
        """Mantissa bits the largest possible entry needs (the tests keep this above 24)."""
        return self.bnd.bit_length()


def _lift(a):
    return Ex.of(a) if isinstance(a, np.ndarray) and a.dtype == np.int64 else a


def _map(a, f):
    return a.map(f) if isinstance(a, Ex) else f(a)


def _shift(a, axis, d, mode):
    """Entry i of the result is a[i + d] along `axis`; beyond the ends: even reflection about the half-points
    (mode "symmetric") or zero (mode "constant")."""
    def f(x):
        pad = [(0, 0)] * x.ndim
        pad[axis] = (1, 1)
        p = np.pad(x, pad, mode=mode)
        idx = [slice(None)] * x.ndim
        idx[axis] = slice(1 + d, x.shape[axis] + 1 + d)
        return p[tuple(idx)]
    return _map(a, f)


# ------------------------------------------------------------------------------------------------ Swift-Hohenberg 2-D / 3-D
def sh_A(w, ainv):
    """A w = (I + Lap) w with the Neumann-ghost second differences: c0 w + sum_axes a (w[i-1] + w[i+1]) on the array extended
    by one cell of even reflection.  `ainv` = (1/hx^2, 1/hy^2[, 1/hz^2]); w has one array axis per entry, x last."""
    c0 = 1.0 - 2.0 * sum(ainv)
    out = c0 * w
    for k, a in enumerate(ainv):
        axis = w_ndim(w) - 1 - k
        out = out + a * (_shift(w, axis, -1, "symmetric") + _shift(w, axis, 1, "symmetric"))
    return out


def w_ndim(w):
    return (w.num if isinstance(w, Ex) else w).ndim


def sh_g(mode, l, nu, u):
    """mode 0 (JVP): l + 2 nu u - 3 u^2; mode 1 (residual, u is the state itself): l + nu u - u^2."""
    return l + (2.0 * nu) * u - 3.0 * (u * u) if mode == 0 else l + nu * u - u * u


def sh_apply(v, u, ainv, l, nu, a0, a1, ag=None, mode=0):
    """out = a0 v + a1 (-A^2 v) + ag g(u) v (ag = a1 unless given).  v, u: int64 (-> Ex) or longdouble arrays of shape
    (nz, ny, nx) or (ny, nx); in mode 1 the state is v and `u` is ignored."""
    v = _lift(v)
    u = v if mode == 1 else _lift(u)
    ag = a1 if ag is None else ag
    return a0 * v + a1 * (-sh_A(sh_A(v, ainv), ainv)) + ag * (sh_g(mode, l, nu, u) * v)


def sh_fused(v, u, r, ainv, l, nu, a0, a1, c):
    """The Lanczos step of MINRES / CG: out = a0 v + a1 J(u) v + c r (r may be None) and the dot product v . out."""
    out = sh_apply(v, u, ainv, l, nu, a0, a1, None, 0)
    if r is not None:
        out = out + c * _lift(r)
    return out, (_lift(v) * out).sum()


def sh_abs(v, u, ainv, l, nu, a0, a1, ag=None, mode=0):
    """|a0 v| + |a1| |A| (|A| |v|) + |ag g(u) v| elementwise in float64: the scale of the rounding error of any evaluation."""
    v, u = np.asarray(v, dtype=np.float64), np.asarray(v if mode == 1 else u, dtype=np.float64)
    ag = a1 if ag is None else ag
    c0 = abs(1.0 - 2.0 * sum(ainv))

    def absA(w):
        out = c0 * w
        for k, a in enumerate(ainv):
            out = out + a * (_shift(w, w.ndim - 1 - k, -1, "symmetric") + _shift(w, w.ndim - 1 - k, 1, "symmetric"))
        return out
    gabs = abs(l) + 2.0 * abs(nu) * np.abs(u) + 3.0 * u * u if mode == 0 else abs(l) + abs(nu) * np.abs(u) + u * u
    return abs(a0) * np.abs(v) + abs(a1) * absA(absA(np.abs(v))) + abs(ag) * gabs * np.abs(v)


# ------------------------------------------------------------------------------------------------ Swift-Hohenberg 1-D
def sh1d_matrix(n):
    """The Dirichlet second difference tridiag(1, -2, 1) (before the 1/h^2) as a dense int64 matrix."""
    return (np.diag(np.full(n, -2)) + np.diag(np.ones(n - 1, dtype=np.int64), 1) +
            np.diag(np.ones(n - 1, dtype=np.int64), -1)).astype(np.int64)


def sh1d_apply(v, u, ax, lam, nu, a0, a1, mode=0):
    """out = a0 v + a1 (g(u) v - (I + D)^2 v), D = ax tridiag(1, -2, 1) as a dense matrix product;
    mode 0: g = lam + 3 nu u^2 - 5 u^4, mode 1 (u = v): g = lam + nu u^2 - u^4."""
    n = len(v)
    T = sh1d_matrix(n)
    v = _lift(v)
    u = v if mode == 1 else _lift(u)

    def A(w):
        return w + ax * (w.matvec_from(T) if isinstance(w, Ex) else T.astype(w.dtype) @ w)
    u2 = u * u
    g = lam + (3.0 * nu) * u2 - 5.0 * (u2 * u2) if mode == 0 else lam + nu * u2 - u2 * u2
    return a0 * v + a1 * (g * v - A(A(v)))


def sh1d_abs(v, u, ax, lam, nu, a0, a1, mode=0):
    v, u = np.asarray(v, dtype=np.float64), np.asarray(v if mode == 1 else u, dtype=np.float64)
    M = np.abs(np.eye(len(v)) + ax * sh1d_matrix(len(v)))
    u2 = u * u
    gabs = abs(lam) + 3.0 * abs(nu) * u2 + 5.0 * u2 * u2 if mode == 0 else abs(lam) + abs(nu) * u2 + u2 * u2
    return abs(a0) * np.abs(v) + abs(a1) * (gabs * np.abs(v) + M @ (M @ np.abs(v)))


# ------------------------------------------------------------------------------------------------ cGL 2-D
def cgl_lap(f, ainv):
    """5-point Dirichlet Laplacian of one field (ny, nx): zero beyond the ends."""
    out = (-2.0 * sum(ainv)) * f
    for k, a in enumerate(ainv):
        out = out + a * (_shift(f, 1 - k, -1, "constant") + _shift(f, 1 - k, 1, "constant"))
    return out


def cgl_apply(v, u, ainv, r, mu, nu, c3, c5, gamma, a0, a1, mode):
    """out = a0 v + a1 op(v) on the stacked fields (2, ny, nx).
    mode 1: op = Lap + NL (examples/cGL2d.jl:24-40, oracle.operators.CGL2d.NL), the state is v;
    mode 0: op = Lap + Jnl(u) with the closed-form 2x2 block of cGL2d.jl:66-69 (oracle.operators.CGL2d.J);
    mode 2: the same with the block transposed (the adjoint Jacobian; the Laplacian is symmetric)."""
    v = _lift(v)
    x1, x2 = _map(v, lambda a: a[0]), _map(v, lambda a: a[1])
    d1, d2 = cgl_lap(x1, ainv), cgl_lap(x2, ainv)
    if mode == 1:
        ua = x1 * x1 + x2 * x2
        o1 = d1 + (r * x1 - nu * x2 - ua * (c3 * x1 - mu * x2) - c5 * (ua * ua) * x1 + gamma)
        o2 = d2 + (r * x2 + nu * x1 - ua * (c3 * x2 + mu * x1) - c5 * (ua * ua) * x2)
    else:
        u = _lift(u)
        u1, u2 = _map(u, lambda a: a[0]), _map(u, lambda a: a[1])
        ua = u1 * u1 + u2 * u2
        f1u = r - 2.0 * (u1 * (c3 * u1 - mu * u2)) - c3 * ua - (4.0 * c5) * (ua * (u1 * u1)) - c5 * (ua * ua)
        f1v = -nu - 2.0 * (u2 * (c3 * u1 - mu * u2)) + mu * ua - (4.0 * c5) * (ua * (u1 * u2))
        f2u = nu - 2.0 * (u1 * (c3 * u2 + mu * u1)) - mu * ua - (4.0 * c5) * (ua * (u1 * u2))
        f2v = r - 2.0 * (u2 * (c3 * u2 + mu * u1)) - c3 * ua - (4.0 * c5) * (ua * (u2 * u2)) - c5 * (ua * ua)
        if mode == 2:
            f1v, f2u = f2u, f1v
        o1 = d1 + f1u * x1 + f1v * x2
        o2 = d2 + f2u * x1 + f2v * x2
    return stack([a0 * x1 + a1 * o1, a0 * x2 + a1 * o2])


def stack(parts):
    """The stacked array [p0; p1; ...] along a new leading axis."""
    if isinstance(parts[0], Ex):
        sh = max(p.sh for p in parts)
        at = [p._at(sh) for p in parts]
        return Ex(np.stack([np.broadcast_to(a, at[0][0].shape) if np.ndim(a) == 0 else a for a, _ in at]), sh,
                  max(b for _, b in at))
    return np.stack(parts)


def cgl_abs(v, u, ainv, r, mu, nu, c3, c5, gamma, a0, a1, mode):
    """Sum of |terms| of cgl_apply elementwise in float64 (every coefficient, operand and sign made non-negative)."""
    r, mu, nu, c3, c5, gamma = (abs(x) for x in (r, mu, nu, c3, c5, gamma))
    x1, x2 = np.abs(np.asarray(v, dtype=np.float64))

    def lap(f):
        out = 2.0 * sum(abs(a) for a in ainv) * f
        for k, a in enumerate(ainv):
            out = out + abs(a) * (_shift(f, 1 - k, -1, "constant") + _shift(f, 1 - k, 1, "constant"))
        return out
    if mode == 1:
        ua = x1 * x1 + x2 * x2
        o1 = lap(x1) + r * x1 + nu * x2 + ua * (c3 * x1 + mu * x2) + c5 * ua * ua * x1 + gamma
        o2 = lap(x2) + r * x2 + nu * x1 + ua * (c3 * x2 + mu * x1) + c5 * ua * ua * x2
    else:
        u1, u2 = np.abs(np.asarray(u, dtype=np.float64))
        ua = u1 * u1 + u2 * u2
        f1u = r + 2 * u1 * (c3 * u1 + mu * u2) + c3 * ua + 4 * c5 * ua * u1 * u1 + c5 * ua * ua
        f1v = nu + 2 * u2 * (c3 * u1 + mu * u2) + mu * ua + 4 * c5 * ua * u1 * u2
        f2u = nu + 2 * u1 * (c3 * u2 + mu * u1) + mu * ua + 4 * c5 * ua * u1 * u2
        f2v = r + 2 * u2 * (c3 * u2 + mu * u1) + c3 * ua + 4 * c5 * ua * u2 * u2 + c5 * ua * ua
        if mode == 2:
            f1v, f2u = f2u, f1v
        o1 = lap(x1) + f1u * x1 + f1v * x2
        o2 = lap(x2) + f2u * x1 + f2v * x2
    return np.stack([abs(a0) * x1 + abs(a1) * o1, abs(a0) * x2 + abs(a1) * o2])


# ------------------------------------------------------------------------------------------------ dF/dparam
PDE_SH, PDE_SH1D, PDE_CGL2D = 1, 2, 3           # BK_PDE_* of include/bkhip.h
DPARAM_CASES = [(PDE_SH, 0), (PDE_SH, 1), (PDE_SH1D, 0), (PDE_SH1D, 1)] + [(PDE_CGL2D, i) for i in range(6)]


def dparam(pde, ipar, c, u):
    """c * dF/dp_ipar of the pointwise part.  SH (l, nu): u, u^2 of F = -L1 u + l u + nu u^2 - u^3.  SH 1-D (lam, nu): u, u^3 of
    R = L1 u + lam u + nu u^3 - u^5.  cGL (r, mu, nu, c3, c5, gamma), u of shape (2, n), from NL of cGL2d.jl:24-40:
    f1 = r u1 - nu u2 - ua (c3 u1 - mu u2) - c5 ua^2 u1 + gamma,  f2 = r u2 + nu u1 - ua (c3 u2 + mu u1) - c5 ua^2 u2."""
    u = _lift(u)
    if pde == PDE_SH:
        return c * (u if ipar == 0 else u * u)
    if pde == PDE_SH1D:
        return c * (u if ipar == 0 else u * u * u)
    u1, u2 = _map(u, lambda a: a[0]), _map(u, lambda a: a[1])
    ua = u1 * u1 + u2 * u2
    one = 0 * u1 + 1
    d1, d2 = [(u1, u2), (ua * u2, -(ua * u1)), (-u2, u1), (-(ua * u1), -(ua * u2)), (-(ua * ua * u1), -(ua * ua * u2)),
              (one, 0 * u1)][ipar]
    return stack([c * d1, c * d2])
