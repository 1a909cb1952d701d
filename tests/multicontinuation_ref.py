"""CPU restatement of the first-points search of multicontinuation (get_first_points_on_branch,
src/bifdiagram/BranchSwitching.jl:298-352) for the tests (test side only): the deflation operator with its exact derivative
(DeflationOperator(2, 1, roots; autodiff = true), src/DeflationOperator.jl:61-169), the Newton step of DeflatedProblemCustomLS
(:264-312) in its two-solve form and in the one-solve form of bk_newton_deflated_exact, Newton on M(u) F(u) with a sparse LU, and
the walk over the predictor's zeros on both sides of the point.

With t_i = u - r_i, d_i = <t_i, t_i>, e_i = <t_i, h>, m_i = d_i^-power + alpha:
    M = prod_i m_i,   dM . h = sum_i (prod_{j != i} m_j) (-2 power d_i^(-power - 1)) e_i        (the mean: both sums over k)
"""
from __future__ import annotations

import itertools
import math

import numpy as np
import scipy.sparse.linalg as spla


# ---------------------------------------------------------------------------------------------- deflation
def sums(u, roots, h=None, dtype=float):
    """(d, e) in ``dtype`` (np.longdouble: the reference of the device sums); e is None without h."""
    u = np.asarray(u, dtype=dtype)
    ts = [u - np.asarray(r, dtype=dtype) for r in roots]
    d = [np.sum(t * t) for t in ts]
    e = None if h is None else [np.sum(t * np.asarray(h, dtype=dtype)) for t in ts]
    return d, e


def sum_terms(u, roots, h=None):
    """The per-element terms of d_i and e_i as the device forms them in fp64: t = u - r_i rounded, then t t and t h."""
    ts = [np.asarray(u, dtype=float) - np.asarray(r, dtype=float) for r in roots]
    return [t * t for t in ts], (None if h is None else [t * np.asarray(h, dtype=float) for t in ts])


def combine(d, e=None, power=2, alpha=1.0, mean=False):
    """(M, dM . h) from the sums, in the type of the sums."""
    k = len(d)
    if k == 0:
        return 1.0, (None if e is None else 0.0)
    one = type(d[0])(1.0) if not isinstance(d[0], float) else 1.0
    m = [(math.inf if di == 0 else one / di ** power) + alpha for di in d]
    M = sum(m[1:], m[0]) / k if mean else math.prod(m[1:], start=m[0])
    if e is None:
        return M, None
    s = 0 * one
    for i in range(k):
        g = (-2 * power * (math.inf if d[i] == 0 else d[i] ** (-power - 1))) * e[i]
        s = s + (g if mean else math.prod(m[:i] + m[i + 1:], start=one) * g)
    return M, (s / k if mean else s)


def M_of(u, roots, **kw):
    return combine(sums(u, roots)[0], **kw)[0]


def dM_exact(u, h, roots, dtype=float, **kw):
    return combine(*sums(u, roots, h, dtype), **kw)[1]


def dM_fd(u, h, roots, delta=1e-8, **kw):
    """The finite difference of autodiff = false (:160-169)."""
    return (M_of(np.asarray(u) + delta * np.asarray(h), roots, **kw) - M_of(u, roots, **kw)) / delta


# ---------------------------------------------------------------------------------------------- the Newton step
def step_two_solves(solve, F, u, roots, **kw):
    """DeflatedProblemCustomLS (:264-312) with the right-hand side M F of Newton: h1 = J^-1 (M F), h2 = J^-1 F,
    h = (h1 - z h2) / M, z = dM.h1 / (M + dM.h2)."""
    M = M_of(u, roots, **kw)
    h1, h2 = solve(M * F), solve(F)
    z = dM_exact(u, h1, roots, **kw) / (M + dM_exact(u, h2, roots, **kw))
    return (h1 - z * h2) / M


def step_one_solve(solve, F, u, roots, **kw):
    """h1 = M h2: h = M / (M + dM.h2) h2, one solve."""
    M = M_of(u, roots, **kw)
    h2 = solve(F)
    return (M / (M + dM_exact(u, h2, roots, **kw))) * h2


def deflated_newton(F, J, roots, x0, tol=1e-10, max_iterations=50, stop_plain=True, norm=lambda v: float(np.abs(v).max()), **kw):
    """_newton (src/Newton.jl:66-114) on M(u) F(u) with the one-solve step and a sparse LU of J; stops on |F| (stop_plain) or on
    |M| |F|.  A root on x (M infinite) is not converged."""
    x = np.array(x0, dtype=float)

    def residual():
        f = F(x)
        M = M_of(x, roots, **kw)
        return f, M, (norm(f) if stop_plain else abs(M) * norm(f))

    f, M, r = residual()
    res, step = [r], 0
    while step < max_iterations and math.isfinite(M) and r > tol:
        lu = spla.splu(J(x).tocsc())
        x = x - step_one_solve(lu.solve, f, x, roots, **kw)
        f, M, r = residual()
        res.append(r)
        step += 1
    dist = [float(np.linalg.norm(x - q)) for q in roots]
    return dict(u=x, converged=bool(math.isfinite(M) and res[-1] < tol), itnewton=step, residuals=res, M=M,
                min_dist=min(dist) if dist else math.inf)


# ---------------------------------------------------------------------------------------------- first points
def first_points(F, J, x0, p0, state, zeros, dp, tol=1e-10, max_iterations=50, stop_plain=True):
    """The walk of :325-349 with F(x, p), J(x, p), state(z) = x0 + sum_i z_i zeta_i and zeros = dict(before=[...], after=[...]):
    dict(before=[x0, states...], after=[...], records=[dict(side, index, status, itnewton, residual, min_dist)])."""
    out, records = {}, []
    for name, sgn in (("after", 1.0), ("before", -1.0)):
        p = p0 + sgn * abs(dp)
        roots = [np.array(x0, dtype=float)]
        for k, z in enumerate(zeros[name]):
            z = np.asarray(z, dtype=float)
            rec = dict(side=name, index=k, status="trivial", itnewton=0, residual=None, min_dist=None)
            records.append(rec)
            if not np.abs(z).max() > 0:
                continue
            s = deflated_newton(lambda x: F(x, p), lambda x: J(x, p), roots, state(z), tol, max_iterations, stop_plain)
            rec.update(itnewton=s["itnewton"], residual=s["residuals"][-1], min_dist=s["min_dist"])
            if not s["converged"]:
                rec["status"] = "lost"
            elif not s["min_dist"] > 1e-6 * (1 + np.linalg.norm(s["u"])):
                rec["status"] = "duplicate"
            else:
                rec["status"] = "found"
                roots.append(s["u"])
        out[name] = roots
    out["records"] = records
    return out


def count(fp, side, status):
    return sum(1 for r in fp["records"] if r["side"] == side and r["status"] == status)


def smallest_pairwise_distance(states):
    return min(float(np.linalg.norm(a - b)) for a, b in itertools.combinations(states, 2))


def mode_class(Q, x, rel=1e-3):
    """The number of kernel modes (columns of Q, orthonormal) a state lives on: mode coordinates above ``rel`` of the largest.
    2-d kernel: 1 = roll, 2 = square; 3-d: 1, 2, 3."""
    m = np.abs(Q.T @ x)
    return int(np.sum(m > rel * m.max()))


def class_counts(Q, states):
    out = {}
    for x in states:
        c = mode_class(Q, x)
        out[c] = out.get(c, 0) + 1
    return out


# ---------------------------------------------------------------------------------------------- the Swift-Hohenberg cases
CASES = {
    2: dict(dims=(16, 16), ls=(np.pi, np.pi), modes=[(1, 2), (2, 1)], nu=1.3),
    3: dict(dims=(8, 8, 8), ls=(2.5, 2.5, 2.5), modes=[(2, 0, 0), (0, 2, 0), (0, 0, 2)], nu=0.9),
}
_case_cache = {}


def sh_case(N, theta=0.0):
    """The branch point of u = 0 of 2-D / 3-D SH on the N cosine modes of CASES[N], the kernel basis rotated by ``theta`` in its
    first plane, with the restatement's normal form there: dict(op, dims, ls, nu, p, Q (the modes), Z (the basis), nf, F(x, p),
    J(x, p)).  Computed once per (N, theta)."""
    import minaug_fold_ref as R
    import normal_form1d_ref as N1R
    import normal_form_nd_ref as M
    from oracle import operators
    key = (N, float(theta))
    if key not in _case_cache:
        c = CASES[N]
        dims, ls, nu = c["dims"], c["ls"], c["nu"]
        lz = [M.sh_cos_mode(dims, ls, m) for m in c["modes"]]
        p = lz[0][0]
        assert all(l == p for l, _ in lz)
        Q = np.stack([z for _, z in lz], axis=1)
        Rm = np.eye(N)
        Rm[:2, :2] = [[math.cos(theta), math.sin(theta)], [-math.sin(theta), math.cos(theta)]]
        Z = Q @ Rm.T
        op = operators.SwiftHohenberg(dims, ls)
        model = R.sh_model(op, "sh", dict(l=p, nu=nu), "l")
        nf = M.normal_form_nd(model, N1R.sh_d3F("sh", ["l", "nu"]), np.zeros(op.N), model.at(p), "l", list(Z.T))
        _case_cache[key] = dict(op=op, dims=dims, ls=ls, nu=nu, p=p, Q=Q, Z=Z, nf=nf, F=lambda x, q: op.F(x, q, nu),
                                J=lambda x, q: op.J(x, q, nu))
    return _case_cache[key]


def sh_first_points(N, theta, dp, stop_plain=True, tol=1e-10):
    """first_points of sh_case(N, theta) from the restatement's predictor at dp, computed once per argument set."""
    import normal_form_nd_ref as M
    key = ("fp", N, float(theta), float(dp), bool(stop_plain), float(tol))
    if key not in _case_cache:
        c = sh_case(N, theta)
        zeros = M.predictor(c["nf"], dp)
        fp = first_points(c["F"], c["J"], np.zeros(c["op"].N), c["p"], lambda z: c["Z"] @ z, zeros, dp, tol=tol, stop_plain=stop_plain)
        fp["zeros"] = zeros
        _case_cache[key] = fp
    return _case_cache[key]
