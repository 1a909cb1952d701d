"""The Krylov solvers of csrc/solver.hip where the Krylov space runs out (n < dim), against dense solves in extended precision.

Every system has at most 64 unknowns, so the basis must hold more vectors than the space has dimensions: the last Arnoldi step leaves a
remainder at rounding level, a speculated block runs on noise behind the last meaningful vector, a block is truncated and refused in the
cycle in which the solve ends, and for n in 33..62 all of that happens after the hand-over to the device-resident chunks.
tests/test_krylov_exhaustion_reference.py shows on the reference alone that each case is such a case -- the tolerance sits three orders
away from the residuals at steps n - 1 and n -- which is why every count here is asserted EXACTLY and is the same for every option
combination.  References: tests/krylov_dense_ref.py (dense solve, sigma_min, true residuals in numpy.longdouble) and the oracle's numbers in
tests/golden/krylov_exhaustion.json.

What each solve asserts (``_check``): converged, the golden count of its flavor, a finite x between untouched NaN guards, a right-hand
side that is bitwise what went in, the true residual ||b - A x|| within the flavor's bound (KrylovKit: < tol, checked explicitly by the code;
the flavors that stop on the Arnoldi estimate: <= max(1.5 tol, 4 x the oracle's true residual)) and ||x - x_dense|| <= residual / sigma_min.

Options whose default is a constant are set on the shared context and put back in ``finally``; ``gmres_predict`` has a computed default
that cannot be put back, so its toggle runs on a context of this module's own (``own``), as does the fresh-context leg of group F.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

import krylov_dense_ref as R
from conftest import probe

pytestmark = pytest.mark.gpu

GUARD = 64                      # doubles of NaN on both sides of every output (as tests/test_gpu_potrap.py)
DEFAULTS = {"gmres_sstep": -1, "gmres_chunk": 4, "gmres_defer_update": 1, "gmres_fuse_v0": 1, "gmres_newton": 1, "block_dots_wide": 1,
            "gmres_stencil_free": 1, "gmres_block_log": 0, "minres_fused": 1, "minres_pair_update": 1, "minres_fuse_axpy": 1}
# group A: the full product of block length and chunk length, and on top of the defaults each switch alone
OPTION_MATRIX = ([{"gmres_sstep": s, "gmres_chunk": c} for s in range(5) for c in (1, 4, 16)] +
                 [{k: 0} for k in ("gmres_defer_update", "gmres_fuse_v0", "gmres_newton", "block_dots_wide")])
GOLDEN = R.golden()


def _hip():
    from bk_amd import hip
    return hip


class _Options:
    """Set options on a context and put back what was there: the value read before (an option that was never set on the context has
    none: then the library's default, DEFAULTS, which tests/test_krylov_exhaustion_reference.py holds against the sources)."""

    def __init__(self, ctx, opts):
        self.ctx, self.opts, self.prior = ctx, opts, {}
        assert set(opts) <= set(DEFAULTS), opts

    def __enter__(self):
        for k, v in self.opts.items():
            try:
                self.prior[k] = self.ctx.get_option(k)
            except Exception:
                self.prior[k] = DEFAULTS[k]
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.opts:
            self.ctx.set_option(k, self.prior.get(k, DEFAULTS[k]))


class _Device:
    """The device side of the systems of krylov_dense_ref on one context: problem, Jacobian, preconditioner, right-hand side."""

    def __init__(self, ctx):
        self.ctx, self.cache = ctx, {}

    def __call__(self, sid):
        if sid not in self.cache:
            hip = _hip()
            s = R.SYSTEMS[sid]
            u, b, _ = R.state(sid)
            if s.kind == "sh1d":
                prob = hip.SwiftHohenberg1D(self.ctx, s.dims[0], 6.0, **R.SH1D_PARAMS)
                J, P = prob.jacobian(prob.vec(np.array(u)), R.SH1D_PARAMS["lam"]), None
            elif s.kind == "sh":
                prob = hip.SwiftHohenberg(self.ctx, s.dims, s.ls, **R.SH_PARAMS)
                J, P = prob.jacobian(prob.vec(np.array(u)), R.SH_PARAMS["l"]), hip.DCTPreconditioner(prob, 1.0)
            else:
                prob = hip.CGL2d(self.ctx, s.dims, s.ls, **R.CGL_PARAMS)
                J = prob.jacobian(prob.vec(np.array(u)), R.CGL_PARAMS["r"])
                P = hip.CGLBlockPreconditioner(prob, R.CGL_PARAMS["r"], R.CGL_PARAMS["nu"])
            self.cache[sid] = dict(prob=prob, J=J, P=P, b=b, rhs=prob.vec(np.array(b)))
        return self.cache[sid]


@pytest.fixture(scope="module")
def dev(ctx):
    d = _Device(ctx)
    yield d
    d.cache.clear()


@pytest.fixture(scope="module")
def own(ctx):
    """A context of this module's own (after the session's: one device, two contexts), for what cannot be undone on the shared one."""
    c = _hip().Context(0)
    d = _Device(c)
    yield d
    d.cache.clear()
    c.close()


def _solver(flavor, rtol, Pl=None, budget=None):
    hip = _hip()
    if flavor == "krylovkit":
        return hip.GMRESKrylovKit(dim=R.DIM, rtol=rtol, atol=0.0, maxiter=budget or 100, Pl=Pl)
    if flavor == "iterativesolvers":
        return hip.GMRESIterativeSolvers(reltol=rtol, abstol=0.0, restart=R.DIM, maxiter=budget or 4000, Pl=Pl)
    if flavor == "krylovjl":
        return hip.KrylovLS(atol=0.0, rtol=rtol, memory=R.DIM, restart=False, itmax=budget or 4000, Pl=Pl)
    return hip.KrylovLSSymmetric(KrylovAlg=flavor, atol=0.0, rtol=rtol, itmax=0, Pl=Pl)


def _guarded(ctx, n):
    import torch
    full = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float64, device=ctx.torch_device)
    return full, C.c_void_p(full[GUARD:GUARD + n].data_ptr())


def _download(ctx, full, n):
    ctx.sync()
    a = full.cpu().numpy()
    assert np.isnan(a[:GUARD]).all() and np.isnan(a[GUARD + n:]).all(), "the solve wrote outside its output"
    return a[GUARD:GUARD + n].copy()


def _same_bits(vec, a):
    return np.array_equal(vec.numpy().view(np.uint64), np.ascontiguousarray(a, dtype=np.float64).view(np.uint64))


def _solve(d, ls, a0, a1):
    """One bk_gmres call into a guarded output: (x, converged, niter)."""
    ctx, rhs = d["prob"].ctx, d["rhs"]
    n = rhs.n
    full, px = _guarded(ctx, n)
    cv, it, rn = C.c_int(), C.c_int(), C.c_double()
    o = ls._opts()
    ctx.check(ctx.lib.bk_gmres(ctx.h, d["J"].h, C.c_void_p(rhs.t.data_ptr()), px, float(a0), float(a1), C.byref(o), ls._pl(),
                               C.byref(cv), C.byref(it), C.byref(rn)), "bk_gmres")
    x = _download(ctx, full, n)
    assert _same_bits(rhs, d["b"]), "the solve changed its right-hand side"
    return x, bool(cv.value), it.value


def _bound(ref, flavor, oracle_res):
    """The flavor's bound on the true residual and whether it is strict: KrylovKit checks ||b - A x|| < tol explicitly before it returns;
    the flavors that stop on the Arnoldi estimate get max(1.5 tol, 4 x the oracle's) -- 1.5 tol is also the code's own rule for operators
    with hessenberg_shift(), which check explicitly in every flavor."""
    if flavor == "krylovkit":
        return ref.tol, True
    return max(1.5 * ref.tol, 4.0 * oracle_res), False


def _check(ref, flavor, count, x, ok, it, what, worst):
    g = GOLDEN[what[0]]
    assert ok, what
    assert it == count, (what, it, count)
    assert np.isfinite(x).all(), what
    res = ref.residual(x)
    bound, strict = _bound(ref, flavor, g["true_residual"][flavor])
    assert (res < bound) if strict else (res <= bound), (what, res, bound)
    err = ref.error(x)
    assert err <= ref.error_bound(res), (what, err, ref.error_bound(res), res)
    w = worst.setdefault(flavor, [0.0, None])
    if res / bound >= w[0]:
        w[:] = [res / bound, what]


def _log_worst(group, worst):
    for flavor, (ratio, what) in worst.items():
        probe(f"krylov exhaustion {group}: true residual / bound", ratio, 1.0, 0.1, flavor=flavor, worst=str(what))


# ------------------------------------------------------------------------------------------------------------------ A
@pytest.mark.parametrize("sid", R.A_SIDS)
def test_unpreconditioned_gmres_at_exhaustion(ctx, dev, own, sid):
    """Group A: dim = 63, rtol = 1e-8, atol = 0 on every system, both shift forms, the three flavors, every option combination."""
    worst = {}
    for case in (c for c in R.A_CASES if c.sid == sid):
        ref = R.reference(case)
        counts = GOLDEN[case.cid]["counts"]
        for flavor in case.flavors:
            ls = _solver(flavor, case.rtol)
            for opts in OPTION_MATRIX:
                with _Options(ctx, opts):
                    x, ok, it = _solve(dev(sid), ls, case.a0, case.a1)
                _check(ref, flavor, counts[flavor], x, ok, it, (case.cid, flavor, opts), worst)
            try:
                for predict in (0, 1):                       # (the default is computed from the other options: a context of its own)
                    own.ctx.set_option("gmres_predict", predict)
                    x, ok, it = _solve(own(sid), ls, case.a0, case.a1)
                    _check(ref, flavor, counts[flavor], x, ok, it, (case.cid, flavor, {"gmres_predict": predict}), worst)
            finally:
                own.ctx.set_option("gmres_predict", 1)       # what the computed default gives wherever the blocks are on, as here
    _log_worst("A", worst)


# ------------------------------------------------------------------------------------------------------------------ B
# (converged, niter) of every solve of group B on the MI355X, per case, flavor and gmres_sstep (-1: blocks, 0: single steps).  KrylovKit
# checks every converged cycle explicitly and uses its 3 cycles up.  IterativeSolvers stops on the Arnoldi estimate, which collapses below
# even this tolerance at the exhausting step: converged at step n -- but for n = 33 with blocks, where the estimate of step 33 stays above
# it: one more step on a noise vector for (0, 1), the whole budget for (0.3, 0.9).  These are NOT the oracle's counts (the restated package
# clamps its restart length to n and reports converged after 2 n iterations: golden file, "<case>/unattainable"); DESIGN.md section 4.
B_OUTCOMES = {
    "sh1d-5/plain/0_1": {("krylovkit", -1): (False, 18), ("krylovkit", 0): (False, 19),
                         ("iterativesolvers", -1): (True, 5), ("iterativesolvers", 0): (True, 5)},
    "sh1d-5/plain/0.3_0.9": {("krylovkit", -1): (False, 19), ("krylovkit", 0): (False, 19),
                             ("iterativesolvers", -1): (True, 5), ("iterativesolvers", 0): (True, 5)},
    "sh1d-33/plain/0_1": {("krylovkit", -1): (False, 104), ("krylovkit", 0): (False, 103),
                          ("iterativesolvers", -1): (True, 34), ("iterativesolvers", 0): (True, 33)},
    "sh1d-33/plain/0.3_0.9": {("krylovkit", -1): (False, 104), ("krylovkit", 0): (False, 103),
                              ("iterativesolvers", -1): (False, 71), ("iterativesolvers", 0): (True, 33)},
    "sh1d-40/plain/0_1": {("krylovkit", -1): (False, 124), ("krylovkit", 0): (False, 124),
                          ("iterativesolvers", -1): (True, 40), ("iterativesolvers", 0): (True, 40)},
    "sh1d-40/plain/0.3_0.9": {("krylovkit", -1): (False, 124), ("krylovkit", 0): (False, 124),
                              ("iterativesolvers", -1): (True, 40), ("iterativesolvers", 0): (True, 40)},
    "sh1d-63/plain/0_1": {("krylovkit", -1): (False, 193), ("krylovkit", 0): (False, 193),
                          ("iterativesolvers", -1): (True, 63), ("iterativesolvers", 0): (True, 63)},
    "sh1d-63/plain/0.3_0.9": {("krylovkit", -1): (False, 193), ("krylovkit", 0): (False, 193),
                              ("iterativesolvers", -1): (True, 63), ("iterativesolvers", 0): (True, 63)},
}


def _b_solves(ctx, dev, case):
    """The solves of group B on one case, each after a long solve of the same system: (flavor, gmres_sstep) -> (x, converged, niter)."""
    d = dev(case.sid)
    _solve(d, _solver("krylovkit", R.RTOL), case.a0, case.a1)
    out = {}
    for flavor in ("krylovkit", "iterativesolvers"):
        for sstep in (-1, 0):
            with _Options(ctx, {"gmres_sstep": sstep}):
                out[flavor, sstep] = _solve(d, _solver(flavor, R.B_RTOL, budget=R.b_budget(flavor, case.n)), case.a0, case.a1)
    return out


@pytest.mark.parametrize("case", R.B_CASES, ids=lambda c: c.cid)
def test_tolerance_that_cannot_be_met(ctx, dev, case):
    """Group B: rtol = 1e-17 with a budget of 3 cycles (KrylovKit) / 2 n + 5 iterations (IterativeSolvers).  Not converged is not an error;
    GMRES is monotone within a cycle and restarts from the true residual, so going on past exhaustion may not make the answer worse than the
    solve of group A: a division by a rounding-level R(k, k) that damages x fails here.  KrylovKit reports ``converged = false``, as the
    issue behind this test asks; the IterativeSolvers flavor does not keep to "false, count = budget" (B_OUTCOMES above says why), so its
    documented outcome is asserted exactly, solve by solve."""
    ref = R.reference(case)
    for (flavor, sstep), (x, ok, it) in _b_solves(ctx, dev, case).items():
        what = (case.cid, flavor, sstep)
        assert np.isfinite(x).all(), what
        probe("krylov exhaustion B: true residual / (1e-8 ||b||)", ref.residual(x) / ref.bnorm, 1e-8, 1e-10, case=case.cid, flavor=flavor,
              sstep=sstep, converged=ok, niter=it)
        assert (ok, it) == B_OUTCOMES[case.cid][flavor, sstep], (what, ok, it)
        if flavor == "krylovkit":
            assert not ok, what


# ------------------------------------------------------------------------------------------------------------------ C
C_RUNS = [{"gmres_stencil_free": sf, "gmres_sstep": sstep} for sf, sstep in itertools.product((0, 1), (-1, 0))]


@pytest.mark.parametrize("sid", R.C_SIDS)
def test_preconditioned_gmres_at_exhaustion(ctx, dev, sid):
    """Group C: through ShiftPrecOp and the transform kernels -- SH with (L1 + I)^-1, cGL at a state of amplitude 2 with the exact inverse of
    the trivial state's Jacobian -- with the stencil-free form off and on.  Each flavor is held against the system it solves: KrylovKit
    (a0 + a1 Pl^-1 J) x = Pl^-1 b, the others Pl^-1 (a0 + a1 J) x = Pl^-1 b."""
    worst = {}
    d = dev(sid)
    for case in R.c_cases(sid):
        ref = R.reference(case)
        counts = GOLDEN[case.cid]["counts"]
        for flavor in case.flavors:
            ls = _solver(flavor, case.rtol, Pl=d["P"])
            for opts in C_RUNS:
                with _Options(ctx, opts):
                    x, ok, it = _solve(d, ls, case.a0, case.a1)
                _check(ref, flavor, counts[flavor], x, ok, it, (case.cid, flavor, opts), worst)
    _log_worst("C", worst)


# applications of the (4,3,3) case at rtol = 1e-12 per gmres_sstep, measured on the MI355X (the same with the stencil-free form off and on)
TIGHT_APPLICATIONS = {0: 38, 1: 38, 2: 40, 3: 73, 4: 74}


def test_preconditioned_tight_tolerance_where_the_block_restatement_restarts(ctx, dev):
    """(4,3,3) with the DCT preconditioner at rtol = 1e-12: the step-by-step restatement takes 38 applications, the block restatement fails
    its explicit check after the exhausting cycle and runs a second one (72).  The library converges, meets the tolerance on the true
    residual and keeps x within tol / sigma_min for every block length.  Blocks of 3 and 4 take 73 and 74 applications, above the
    restatement's 72 that the issue behind this test set as the ceiling: a second cycle forced by the explicit check, documented with its
    numbers in DESIGN.md section 4 and asserted exactly here (TIGHT_APPLICATIONS); the counts hold consumed Arnoldi steps only (gmres_block_unconsumed, below)."""
    case = R.C_TIGHT_CASE
    ref = R.reference(case)
    counts = GOLDEN[case.cid]["counts"]
    assert counts == dict(krylovkit=38, block=72)
    d = dev(case.sid)
    ls = _solver("krylovkit", case.rtol, Pl=d["P"])
    _solve(d, ls, case.a0, case.a1)              # (every measured solve below follows a long solve: the ramp of the first is the others')
    for sf, sstep in itertools.product((1, 0), range(5)):
        with _Options(ctx, {"gmres_stencil_free": sf, "gmres_sstep": sstep}):
            unconsumed = ctx.get_option("gmres_block_unconsumed")
            x, ok, it = _solve(d, ls, case.a0, case.a1)
            unconsumed = ctx.get_option("gmres_block_unconsumed") - unconsumed
        what = (case.cid, sf, sstep)
        assert ok and np.isfinite(x).all(), what
        res = ref.residual(x)
        assert res < ref.tol, (what, res, ref.tol)
        assert ref.error(x) <= ref.error_bound(ref.tol), (what, ref.error(x))
        probe("krylov exhaustion C (4,3,3) rtol 1e-12: applications", it, 2 * (case.n + 2), counts["block"], stencil_free=sf, sstep=sstep,
              residual_over_tol=res / ref.tol, unconsumed=unconsumed)
        assert it == TIGHT_APPLICATIONS[sstep], (what, it)
        # accepted block steps the solve never consumed (they are never counted: niter counts consumed columns).  None where the count
        # exceeds the restatement's -- 73 and 74 are Arnoldi steps the solve needed; blocks of 2 converge on the first column of their
        # last block and leave its second step unused, outside the 40
        assert unconsumed == (1 if sstep == 2 else 0), (what, unconsumed)


# ------------------------------------------------------------------------------------------------------------------ D
def _bordered_solve(d, ls, sid, use_pl):
    ctx, hip = d["prob"].ctx, _hip()
    dR, dzu, dzp, nn = R.border(sid)
    n = d["rhs"].n
    vR, vz = d["prob"].vec(np.array(dR)), d["prob"].vec(np.array(dzu))
    full, px = _guarded(ctx, n)
    dl, cv, it = C.c_double(), C.c_int(), C.c_int()
    o = ls._opts()
    p = lambda v: C.c_void_p(v.t.data_ptr())      # noqa: E731
    args = (ctx.h, d["J"].h, p(vR), p(vz), float(dzp), p(d["rhs"]), float(nn), R.THETA, 1.0 - R.THETA, 0, 0.0, 1.0 / n, C.byref(o))
    if use_pl:
        ctx.check(ctx.lib.bk_bls_matrixfree_pl(*args, ls._pl(), px, C.byref(dl), C.byref(cv), C.byref(it)), "bk_bls_matrixfree_pl")
    else:
        ctx.check(ctx.lib.bk_bls_matrixfree(*args, px, C.byref(dl), C.byref(cv), C.byref(it)), "bk_bls_matrixfree")
    x = _download(ctx, full, n)
    assert _same_bits(d["rhs"], d["b"]) and _same_bits(vR, dR) and _same_bits(vz, dzu), "the bordered solve changed an input"
    return np.concatenate([x, [dl.value]]), bool(cv.value), it.value


@pytest.mark.parametrize("case", R.D_CASES, ids=lambda c: c.cid)
def test_bordered_matrixfree_solve_at_exhaustion(ctx, dev, case):
    """Group D: the tails and the host path (nt != 0) -- bk_bls_matrixfree, and bk_bls_matrixfree_pl where the problem has a preconditioner --
    against the dense (n + 1) x (n + 1) solve; itlinear equals the count of oracle.bordered.matrixfree_bls on the oracle's solvers."""
    worst = {}
    ref = R.reference(case)
    counts = GOLDEN[case.cid]["counts"]
    d = dev(case.sid)
    use_pl = case.form == "bordered_pl"
    for flavor in case.flavors:
        ls = _solver(flavor, case.rtol, Pl=d["P"] if use_pl else None)
        for opts in ({}, {"gmres_chunk": 1}, {"gmres_sstep": 0}):
            with _Options(ctx, opts):
                x, ok, it = _bordered_solve(d, ls, case.sid, use_pl)
            _check(ref, flavor, counts[flavor], x, ok, it, (case.cid, flavor, opts), worst)
    _log_worst("D", worst)


# ------------------------------------------------------------------------------------------------------------------ E
@pytest.mark.parametrize("label,kind,case", R.e_cases(), ids=[e[0] for e in R.e_cases()])
def test_minres_and_cg_take_exactly_n_iterations(ctx, dev, label, kind, case):
    """Group E: SH1D with n in 2, 3, 5 -- MINRES on J, MINRES and CG on (lambda_max + 1) I - J -- with each of minres_fused,
    minres_pair_update and minres_fuse_axpy at 0 and 1.  (No preconditioner applies: the 1-D problem has none.)"""
    ref = R.reference(case)
    g = GOLDEN[label]
    ls = _solver(kind, case.rtol)
    worst = 0.0
    for fused, pair, fuse_axpy in itertools.product((0, 1), repeat=3):
        opts = {"minres_fused": fused, "minres_pair_update": pair, "minres_fuse_axpy": fuse_axpy}
        with _Options(ctx, opts):
            x, ok, it = _solve(dev(case.sid), ls, case.a0, case.a1)
        what = (label, opts)
        assert ok, what
        assert it == case.n == g["counts"][kind], (what, it)
        assert np.isfinite(x).all(), what
        res = ref.residual(x)
        bound = max(1.5 * ref.tol, 4.0 * g["true_residual"][kind])
        assert res <= bound, (what, res, bound)
        assert ref.error(x) <= ref.error_bound(res), (what, ref.error(x), ref.error_bound(res))
        worst = max(worst, res / bound)
    probe("krylov exhaustion E: true residual / bound", worst, 1.0, 0.1, case=label)


# ------------------------------------------------------------------------------------------------------------------ F
@pytest.mark.parametrize("flavor", ["krylovkit", "iterativesolvers"])
def test_counts_do_not_depend_on_the_previous_solve(ctx, dev, flavor):
    """Group F: the n = 40 case after a solve that ended in one step (the same system at rtol = 0.9: the next solve starts with single steps
    and a chunk ramp of 1), after a long solve, and on a fresh context: "block boundaries move, iterates and counters do not"."""
    case = R.F_CASE
    ref = R.reference(case)
    count = GOLDEN[case.cid]["counts"][flavor]
    ls = _solver(flavor, case.rtol)
    worst, its = {}, {}
    d = dev(case.sid)
    _, ok1, it1 = _solve(d, _solver(flavor, 0.9), case.a0, case.a1)
    assert ok1 and it1 <= 3, (ok1, it1)                 # one Arnoldi step (KrylovKit counts applications: x0, the step, the check)
    x, ok, its["after a one-step solve"] = _solve(d, ls, case.a0, case.a1)
    _check(ref, flavor, count, x, ok, its["after a one-step solve"], (case.cid, flavor, "after a one-step solve"), worst)
    x, ok, its["after a long solve"] = _solve(d, ls, case.a0, case.a1)
    _check(ref, flavor, count, x, ok, its["after a long solve"], (case.cid, flavor, "after a long solve"), worst)
    fresh = _hip().Context(0)
    try:
        x, ok, its["fresh context"] = _solve(_Device(fresh)(case.sid), ls, case.a0, case.a1)
    finally:
        fresh.close()
    _check(ref, flavor, count, x, ok, its["fresh context"], (case.cid, flavor, "fresh context"), worst)
    assert len(set(its.values())) == 1, its
    _log_worst("F", worst)


# ------------------------------------------------------------------------------------------------------------------ G
def _counters(ctx):
    return {k: ctx.get_option(k) for k in ("gmres_block_steps", "gmres_block_truncated", "gmres_block_folded", "gmres_chunk_handover")}


@pytest.mark.parametrize("sstep", [2, 3, 4])
@pytest.mark.parametrize("sid", R.G_FOLD_SIDS)
def test_exhaustion_truncates_and_refuses_a_block(ctx, dev, sid, sstep):
    """Group G, the block path: the solves of group A with gmres_sstep >= 2 on n = 5, 9 did run blocks, and the cycle in which the solve
    ends holds a truncated block (void tail: the speculated steps behind the last meaningful vector) and a refused one (got = 0: not even
    one column of the last step passes the pivot test, the column comes from the single-vector path with its cancellation branch)."""
    case = R.Case(sid)
    ls = _solver("krylovkit", case.rtol)
    _solve(dev(sid), ls, case.a0, case.a1)         # (a predecessor of more than two steps: the measured solve starts with full blocks)
    with _Options(ctx, {"gmres_sstep": sstep, "gmres_block_log": 1}):
        ctx.solver_block_log(reset=True)
        before = _counters(ctx)
        x, ok, it = _solve(dev(sid), ls, case.a0, case.a1)
        after = _counters(ctx)
        log = ctx.solver_block_log(reset=True)
    assert ok and it == GOLDEN[case.cid]["counts"]["krylovkit"]
    assert after["gmres_block_steps"] > before["gmres_block_steps"] and log
    assert after["gmres_block_truncated"] > before["gmres_block_truncated"], log
    assert after["gmres_block_folded"] == before["gmres_block_folded"]
    assert log[-1]["got"] == 0 and log[-1]["j"] == case.n - 1, log          # the exhausting column: refused, handed to the single step
    assert max(r["steps"] for r in log) >= 2


@pytest.mark.parametrize("defer", [1, 0])
def test_a_solve_that_ends_inside_a_block_folds_the_deferred_update_in(ctx, dev, defer):
    """Group G, the fold: a solve that exhausts the space never ends inside a deferred block (above: its last column comes from the
    single-vector path, after the pending update has run; ``gmres_block_folded`` stays 0 in every solve of group A), so the branch
    ``pend.active && k > pend.k`` is shown on the same n = 5 system with a tolerance between the residuals at steps 3 and 4: with blocks of
    2 the solve ends on the second column of the block [2, 3], at step n - 1, and the solution update goes through
    sstep::fold_solution_coefficients.  Same count (6 = x0, four steps, the check), residual and error bounds as everywhere."""
    case = R.G_INSIDE_CASE
    ref = R.reference(case)
    worst = {}
    _solve(dev(case.sid), _solver("krylovkit", R.RTOL), case.a0, case.a1)      # (as above: full blocks from the first one on)
    with _Options(ctx, {"gmres_sstep": 2, "gmres_block_log": 1, "gmres_defer_update": defer}):
        ctx.solver_block_log(reset=True)
        before = _counters(ctx)
        x, ok, it = _solve(dev(case.sid), _solver("krylovkit", case.rtol), case.a0, case.a1)
        after = _counters(ctx)
        log = ctx.solver_block_log(reset=True)
    _check(ref, "krylovkit", GOLDEN[case.cid]["counts"]["krylovkit"], x, ok, it, (case.cid, "krylovkit", defer), worst)
    assert [(r["j"], r["steps"], r["got"]) for r in log] == [(0, 2, 2), (2, 2, 2)], log
    assert after["gmres_block_folded"] - before["gmres_block_folded"] == defer
    assert after["gmres_block_truncated"] == before["gmres_block_truncated"]


@pytest.mark.parametrize("chunk", [4, 16])
@pytest.mark.parametrize("sid", R.G_CHUNK_SIDS)
def test_exhaustion_behind_the_hand_over_to_the_device_chunks(ctx, dev, sid, chunk):
    """Group G, the chunk path: with n in 33, 36, 40 and gmres_chunk > 1 the cycle is handed to the device-resident chunks at the 33rd basis
    vector, and the space runs out behind the hand-over."""
    case = R.Case(sid)
    ls = _solver("krylovkit", case.rtol)
    with _Options(ctx, {"gmres_chunk": chunk}):
        before = _counters(ctx)
        x, ok, it = _solve(dev(sid), ls, case.a0, case.a1)
        after = _counters(ctx)
    assert ok and it == GOLDEN[case.cid]["counts"]["krylovkit"]
    assert after["gmres_chunk_handover"] == before["gmres_chunk_handover"] + 1
    with _Options(ctx, {"gmres_chunk": 1}):
        before = _counters(ctx)
        _solve(dev(sid), ls, case.a0, case.a1)
        assert _counters(ctx)["gmres_chunk_handover"] == before["gmres_chunk_handover"]
