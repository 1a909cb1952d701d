"""CPU restatement of deflated continuation (deflatedContinuation, src/DeflatedContinuation.jl:251-356) for the tests (test side
only): the loop over parameter steps and branches on F(x, p), J(x, p) with the deflated Newton of multicontinuation_ref (sparse
LU), the counter-based uniform of bk_vec_perturb in NumPy uint64 arithmetic, and the extended-precision / exact forms of the two
distances of bk_deflation_dist.

Bookkeeping as in bk_amd.deflated_continuation: branch i starts from root i, the roots are taken as given, a branch's first
record is its first continued point (for a branch found by a seek: the solution the seek returned).
"""
from __future__ import annotations

import math

import numpy as np

import multicontinuation_ref as MC

LD = np.longdouble
GOLDEN = np.uint64(0x9E3779B97F4A7C15)
M1 = np.uint64(0xBF58476D1CE4E5B9)
M2 = np.uint64(0x94D049BB133111EB)


# ---------------------------------------------------------------------------------------------- the hash
def mix64(z):
    """The finaliser on a uint64 array (wrapping arithmetic)."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * M1
        z = (z ^ (z >> np.uint64(27))) * M2
    return z ^ (z >> np.uint64(31))


def hash_u01(seed, g):
    """U(seed, g) in [0, 1) for the global indices g: z = seed + (g + 1) golden, finalised, the top 53 bits times 2^-53."""
    g = np.asarray(g, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(int(seed) & (2 ** 64 - 1)) + (g + np.uint64(1)) * GOLDEN
    return (mix64(z) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def hash_u01_int(seed, g):
    """The same for one index in Python integers (the independent form the hash is pinned to)."""
    m = 2 ** 64
    z = (seed + (g + 1) * 0x9E3779B97F4A7C15) % m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % m
    z ^= z >> 31
    return (z >> 11) / 2 ** 53


def perturb(x, amp, seed, index0=0):
    """x + amp U(seed, index0 + i): the product rounded, then the sum (NumPy rounds each operation)."""
    x = np.asarray(x, dtype=np.float64)
    t = np.float64(amp) * hash_u01(seed, np.uint64(index0) + np.arange(x.size, dtype=np.uint64))
    return x + t


def derive_seed(seed, branch, count):
    """The per-call seed of UniformPerturbation from (seed, branch id, call count), in Python integers."""
    m = 2 ** 64

    def fin(z):
        z %= m
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % m
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % m
        return z ^ (z >> 31)

    return fin(fin(seed + (branch + 1) * 0x9E3779B97F4A7C15) + (count + 1) * 0x9E3779B97F4A7C15)


class UniformPerturbation:
    """The restatement of bk_amd.deflated_continuation.UniformPerturbation on NumPy vectors."""

    def __init__(self, amp, seed, index0=0):
        self.amp, self.seed, self.index0, self.count = amp, seed, index0, 0

    def __call__(self, x, p, id):
        s = derive_seed(self.seed, id, self.count)
        self.count += 1
        return perturb(x, self.amp, s, self.index0)


# ---------------------------------------------------------------------------------------------- the distances
def dist_terms(u, root):
    """The fp64 terms of d2 as the device forms them: t = u - r rounded, then t t."""
    t = np.asarray(u, dtype=np.float64) - np.asarray(root, dtype=np.float64)
    return t * t


def dist_ref(u, roots):
    """[(d2 in longdouble of the fp64 terms, sum |terms|, dinf exact)] per root.  The max has no rounding; one NaN makes it NaN."""
    out = []
    for r in roots:
        tt = dist_terms(u, r)
        t = np.abs(np.asarray(u, dtype=np.float64) - np.asarray(r, dtype=np.float64))
        out.append((float(np.sum(tt.astype(LD))), float(np.abs(tt).sum()), float(np.max(t)) if t.size else 0.0))
    return out


# ---------------------------------------------------------------------------------------------- the loop
norminf = lambda v: float(np.abs(v).max())
norm2 = lambda v: float(np.linalg.norm(v))


def seek(F, J, roots, x, p, tol, max_iterations, stop_plain, norm, **kw):
    """_DC_get_new_solution (:269-286) from the perturbed guess: the deflated Newton, then converged / plain residual < tol /
    every root at least tol away.  reason: 0 accepted, 1 not converged, 2 plain residual, 3 known root."""
    s = MC.deflated_newton(lambda v: F(v, p), lambda v: J(v, p), roots, x, tol, max_iterations, stop_plain=stop_plain, norm=norm, **kw)
    plain = norm(F(s["u"], p))
    dmin = min((norm(s["u"] - r) for r in roots), default=math.inf)
    s["reason"] = 1 if not s["converged"] else 2 if not plain < tol else 3 if not dmin >= tol else 0
    s.update(accepted=s["reason"] == 0, plain_residual=plain, min_dist_normC=dmin)
    return s


def deflated_continuation(F, J, roots, p0, ds, p_min=-math.inf, p_max=math.inf, max_steps=400, tol=1e-10, max_iterations=25,
                          max_branches=100, seek_every_step=1, max_iter_defop=5, perturb_solution=lambda x, p, id: x,
                          accept_solution=lambda x, p: True, power=2, alpha=1.0, stop_plain=None, norm=norm2):
    """dict(branches=[dict(param, normu, itnewton, states, active)], seeks=[dict(step, branch, reason, itnewton)], sol)."""
    if not roots:
        raise ValueError("You must provide at least one guess")
    kw = dict(power=power, alpha=alpha)
    stop_plain = (alpha >= 1) if stop_plain is None else stop_plain
    states = [dict(x=np.array(r, dtype=float), active=True) for r in roots]
    branches = [dict(param=[], normu=[], itnewton=[], states=[], active=True) for _ in states]
    seeks = []
    held = []
    p, nstep = float(p0), 0

    def record(br, u, s):
        br["param"].append(p)
        br["normu"].append(norm(u))
        br["itnewton"].append(s["itnewton"])
        br["states"].append(u.copy())

    while ((p_min < p < p_max) or nstep == 0) and nstep < max_steps:
        p = min(max(p + ds, p_min), p_max)
        held.clear()
        for st, br in zip(states, branches):
            if not st["active"]:
                continue
            s = MC.deflated_newton(lambda v: F(v, p), lambda v: J(v, p), held, st["x"], tol, max_iterations, stop_plain=stop_plain,
                                   norm=norm, **kw)
            if s["converged"]:
                st["x"] = s["u"]
                held.append(st["x"])
                record(br, st["x"], s)
            else:
                st["active"] = br["active"] = False
        nbrs = len(states)
        if nstep % seek_every_step == 0 and sum(st["active"] for st in states) < max_branches:
            n_active = 0
            for idb in range(nbrs):
                st = states[idb]
                if not (st["active"] and n_active < max_branches):
                    continue
                n_active += 1
                success = True
                while success:
                    x = perturb_solution(st["x"].copy(), p, idb)
                    s = seek(F, J, held, x, p, tol, max_iter_defop * max_iterations, stop_plain, norm, **kw)
                    success = s["accepted"]
                    ok = success and accept_solution(s["u"], p)
                    seeks.append(dict(step=nstep, branch=idb, reason=s["reason"] if (ok or not success) else 4, itnewton=s["itnewton"]))
                    if ok:
                        held.append(s["u"])
                        states.append(dict(x=s["u"], active=n_active + 1 < max_branches))
                        branches.append(dict(param=[], normu=[], itnewton=[], states=[], active=states[-1]["active"]))
                        record(branches[-1], s["u"], s)
        nstep += 1
    return dict(branches=branches, seeks=seeks, sol=[st["x"] for st in states if st["active"]])


# ---------------------------------------------------------------------------------------------- the problems
def scalar_problem():
    """F2 of test/continuation/simple_continuation.jl:408: (F(u, p), J(u, p) as a 1 x 1 sparse matrix, closed-form roots(p))."""
    import scipy.sparse as sp

    def F(u, p):
        return -u * (p + u * (2 - 5 * u)) * (p - 0.15 - u * (2 + 20 * u))

    def J(u, p):
        a, b = p + u * (2 - 5 * u), p - 0.15 - u * (2 + 20 * u)
        da, db = 2 - 10 * u, -2 - 40 * u
        return sp.csc_matrix(np.atleast_2d(-(a * b) - u * (da * b + a * db)))

    def roots(p):
        out = [0.0]
        if 4 + 20 * p >= 0:
            out += [(2 + math.sqrt(4 + 20 * p)) / 10, (2 - math.sqrt(4 + 20 * p)) / 10]
        if 4 - 80 * (0.15 - p) >= 0:
            out += [(-2 + math.sqrt(4 - 80 * (0.15 - p))) / 40, (-2 - math.sqrt(4 - 80 * (0.15 - p))) / 40]
        return out

    return F, J, roots


_cache = {}


SH_RUN = dict(back=0.035, ds=0.01, tol=1e-10, amp=0.1, seed=2024, max_iterations=15)


def sh_run(N=2, steps=8, max_branches=12, max_iter_defop=3, seek_every_step=1):
    """Deflated continuation on MC.sh_case(N) from u = 0 at l* - 0.035 with ds = +0.01, tol 1e-10 in the inf-norm, power 2,
    alpha 1, 15 Newton iterations along a branch and 15 max_iter_defop in a seek, the hashed uniform perturbation of amplitude 0.1
    and seed 2024.  Computed once per argument set."""
    key = (N, steps, max_branches, max_iter_defop, seek_every_step)
    if key not in _cache:
        c, o = MC.sh_case(N), SH_RUN
        _cache[key] = deflated_continuation(c["F"], c["J"], [np.zeros(c["op"].N)], c["p"] - o["back"], o["ds"], max_steps=steps,
                                            tol=o["tol"], max_iterations=o["max_iterations"], max_branches=max_branches,
                                            seek_every_step=seek_every_step, max_iter_defop=max_iter_defop,
                                            perturb_solution=UniformPerturbation(o["amp"], o["seed"]), norm=norminf)
    return _cache[key]


def pairwise_min_inf(states):
    """The smallest inf-norm distance between two of the states (inf for fewer than two)."""
    return min((norminf(a - b) for i, a in enumerate(states) for b in states[:i]), default=math.inf)
