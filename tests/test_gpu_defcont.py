"""GPU tests of deflated continuation (bk_amd.deflated_continuation; csrc/defcont.hip): the distance pass bk_deflation_dist
against bk_deflation_dots (bitwise), extended-precision sums and the exact NumPy max; the counter-based perturbation
bk_vec_perturb against its uint64 restatement (bitwise); bk_defcont_seek against bk_newton_deflated_exact and its call-by-call
mirror; and the driver end to end on 16 x 16 and 8 x 8 x 8 Swift-Hohenberg, native and mirror, against invariants checked with
the oracle's F and the restatement (tests/defcont_ref.py).  Every bound is logged next to its measured value by ``probe``."""
import itertools
import math

import numpy as np
import pytest

import defcont_ref as R
import multicontinuation_ref as MC
from conftest import probe

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
RELTOL = 1e-10
TOL = 1e-10
LENGTHS = [2, 3, 255, 256, 257, 4097, 1 << 22]
NROOTS = [1, 7, 8, 9, 17]


def _lib():
    from bk_amd import deflated_continuation as DC
    from bk_amd import hip
    return hip, DC


def _guarded(hip, ctx, a, off):
    """A device vector holding ``a`` between NaN guards, ``off`` doubles (2: 16-byte aligned, 1: one double off) into a fresh buffer."""
    import torch
    n = a.shape[0]
    t = torch.full((n + 4,), float("nan"), dtype=torch.float64, device=ctx.torch_device)
    t[off:off + n] = torch.from_numpy(np.ascontiguousarray(a)).to(ctx.torch_device)
    v = type("GuardedVec", (hip.HipVec,), {})(ctx, t[off:off + n], n)
    assert v.t.data_ptr() % 16 == (0 if off == 2 else 8)
    v._whole, v._off = t, off
    return v


def _guards_intact(v):
    w = v._whole.cpu().numpy()
    return bool(np.isnan(w[:v._off]).all() and np.isnan(w[v._off + v.n:]).all())


def _set(v, i, val):
    v.t[i] = val


# ------------------------------------------------------------------------------------------ 1: bk_deflation_dist
@pytest.mark.parametrize("n", LENGTHS)
def test_deflation_dist_matches_dots_bitwise_and_the_exact_max(ctx, n):
    """For 1, 7, 8, 9 and 17 roots (one launch; 8 + 1; 8 + 8 + 1), every stream 16-byte aligned and again with root 0 one double off
    (the element path; n = 2^22 aligned takes the non-temporal instantiation), operands between NaN guards: d2 is the d of
    bk_deflation_dots bit for bit and within 4 n eps sum |terms| of the longdouble sum of the fp64 terms; dinf is EXACTLY the
    NumPy max of |u - r_i| (a max has no rounding).  Then the extreme element is moved, in turn, to index 0, to the last element
    (the odd tail for odd n) and to both sides of the workgroup seams (element 256 of the element path; 512 and 1024, the 4-KiB
    chunk of a workgroup with 1 and 2 items per lane in flight), with 9 roots on both paths."""
    hip, _ = _lib()
    rng = np.random.default_rng(300 + n % 9973)
    u = rng.random(n) - 0.5
    roots = [rng.random(n) - 0.5 for _ in range(max(NROOTS))]
    ref = R.dist_ref(u, roots)
    seams = sorted({0, n - 1} | {s + d for s in (256, 512, 1024) for d in (-1, 0) if s < n})
    for mis in (False, True):
        U = _guarded(hip, ctx, u, 2)
        Rv = [_guarded(hip, ctx, r, 1 if (mis and i == 0) else 2) for i, r in enumerate(roots)]
        tag = f"n{n}.{'off8' if mis else 'aligned'}"
        for k in NROOTS:
            op = hip.DeflationOperator(2, 1.0, Rv[:k], autodiff=True)
            d2, dinf = op.dist(U)
            assert len(d2) == len(dinf) == k
            assert d2 == op.dots(U)[0], (tag, k)
            for i in range(k):
                probe(f"defcont.dist_d2.{tag}", abs(d2[i] - ref[i][0]) / (4 * n * EPS * ref[i][1] + 1e-300), 1.0, k=k)
                assert dinf[i] == ref[i][2], (tag, k, i)
        op = hip.DeflationOperator(2, 1.0, Rv[:9], autodiff=True)
        for pos in seams:
            old = u[pos]
            _set(U, pos, 7.0 + pos % 3)
            d2, dinf = op.dist(U)
            assert dinf == [abs((7.0 + pos % 3) - r[pos]) for r in roots[:9]], (tag, pos)
            assert d2 == op.dots(U)[0]
            _set(U, pos, old)
        assert op.dist(U)[1] == [ref[i][2] for i in range(9)]
        assert all(_guards_intact(v) for v in [U] + Rv)


@pytest.mark.parametrize("n", [3, 257, 4097])
def test_deflation_dist_zero_nan_and_no_roots(ctx, n):
    """A root that holds u's values (its own buffer) gives (0, 0) exactly and leaves the others alone; one NaN in u makes every
    dinf NaN (and every d2); no roots is accepted and returns nothing."""
    hip, _ = _lib()
    rng = np.random.default_rng(n)
    u = rng.standard_normal(n)
    roots = [rng.standard_normal(n) for _ in range(9)]
    roots[3] = u.copy()
    V = lambda a: _guarded(hip, ctx, a, 2)
    op = hip.DeflationOperator(2, 1.0, [V(r) for r in roots], autodiff=True)
    U = V(u)
    d2, dinf = op.dist(U)
    assert d2[3] == 0.0 and dinf[3] == 0.0
    assert all(a > 0 and b == np.abs(u - r).max() for i, (a, b, r) in enumerate(zip(d2, dinf, roots)) if i != 3)
    assert hip.DeflationOperator(2, 1.0, [], autodiff=True).dist(U) == ([], [])
    for pos in (0, n // 2, n - 1):
        W = V(u)
        _set(W, pos, float("nan"))
        d2, dinf = op.dist(W)
        assert all(math.isnan(x) for x in dinf) and all(math.isnan(x) for x in d2), pos
    assert all(_guards_intact(v) for v in [U] + op.roots)


# ------------------------------------------------------------------------------------------ 2: bk_vec_perturb
SEEDS = [2024, 2 ** 64 - 59]


def _perturb(ctx, v, amp, seed, index0):
    ctx.check(ctx.lib.bk_vec_perturb(ctx.h, v.n, v.t.data_ptr(), float(amp), seed, index0), "bk_vec_perturb")


@pytest.mark.parametrize("n", LENGTHS)
def test_vec_perturb_is_the_restatement_bit_for_bit(ctx, n):
    """x + amp U(seed, index0 + i) against the NumPy uint64 restatement, exactly: x = 0 and x random, aligned and one double off,
    amp in {1, 0.1, -3.5}, two seeds, index0 in {0, 12345} -- the full product up to n = 4097; at n = 2^22 (non-temporal path
    when aligned) three combinations that cover every value.  Guards intact.  The vector perturbed as one piece equals the vector
    perturbed as three pieces (cuts at n / 3 and 2 n / 3 + 1, so the pieces start on either alignment) with their offsets."""
    hip, _ = _lib()
    rng = np.random.default_rng(n)
    xs = dict(zero=np.zeros(n), random=rng.standard_normal(n))
    full = list(itertools.product(xs, [1.0, 0.1, -3.5], SEEDS, [0, 12345]))
    combos = full if n < (1 << 22) else [("zero", 1.0, SEEDS[0], 0), ("random", 0.1, SEEDS[1], 12345), ("random", -3.5, SEEDS[0], 12345)]
    for off in (2, 1):
        for kind, amp, seed, i0 in combos:
            v = _guarded(hip, ctx, xs[kind], off)
            _perturb(ctx, v, amp, seed, i0)
            assert np.array_equal(v.numpy(), R.perturb(xs[kind], amp, seed, i0)), (n, off, kind, amp, seed, i0)
            assert _guards_intact(v)
        amp, seed, i0 = 0.1, SEEDS[0], 12345
        v = _guarded(hip, ctx, xs["random"], off)
        cuts = [0, n // 3, min(n, 2 * n // 3 + 1), n]
        for a, b in zip(cuts[:-1], cuts[1:]):
            _perturb(ctx, hip.HipVec(ctx, v.t[a:b], b - a), amp, seed, i0 + a)
        assert np.array_equal(v.numpy(), R.perturb(xs["random"], amp, seed, i0)) and _guards_intact(v)


def test_vec_perturb_accepts_an_empty_vector(ctx):
    hip, _ = _lib()
    v = _guarded(hip, ctx, np.zeros(0), 2)
    _perturb(ctx, v, 1.0, 1, 0)
    ctx.check(ctx.lib.bk_vec_perturb(ctx.h, 0, None, 1.0, 1, 0), "bk_vec_perturb")
    assert _guards_intact(v)


# ------------------------------------------------------------------------------------------ 3: bk_defcont_seek
def _solver(hip, prob, maxiter=50):
    return hip.GMRESKrylovKit(dim=40, rtol=RELTOL, atol=1e-13, maxiter=maxiter, Pl=hip.DCTPreconditioner(prob, 1.0))


def test_seek_against_the_deflated_newton_and_its_acceptance_tests(ctx):
    """16 x 16 at l* + 0.008 from the restatement's predicted square with the trivial state and three rolls deflated (the setup
    of test_exact_deflated_newton_native_mirror_and_restatement): the seek is accepted with the state (8 ulp) and the counts of
    bk_newton_deflated_exact, and the mirror agrees; plain_residual < tol; min_dist_normC is DeflationOperator.dist of the result.
    With the found state deflated too, a seek from a copy of it (M infinite) and from the copy moved by a few ulp (inside tol of
    it) gives reason 1 or 3, never accepted.  tol below the rounding floor of the plain residual gives reason 1 or 2; the same call
    with max_iterations = 200 and residuals_cap = 16 returns the last 16 entries of the 201 a cap of 256 returns.  x aliasing a
    root is refused with a message; a call that works follows each error path."""
    hip, DC = _lib()
    from bk_amd import _lib as L
    c = MC.sh_case(2, 0.0)
    dp = 0.008
    fp = MC.sh_first_points(2, 0.0, dp)
    rolls = [x for x in fp["after"][1:] if MC.mode_class(c["Q"], x) == 1][:3]
    zsq = next(z for z in fp["zeros"]["after"][1:] if np.abs(z).min() > 1e-3 * np.abs(z).max())
    start = c["Z"] @ zsq
    p = c["p"] + dp
    prob = hip.SwiftHohenberg(ctx, c["dims"], c["ls"], l=p, nu=c["nu"])
    ls = _solver(hip, prob)
    op = hip.DeflationOperator(2, 1.0, [prob.vec(r) for r in [np.zeros(c["op"].N)] + rolls], autodiff=True)
    X0 = prob.vec(start)
    kw = dict(tol=TOL, max_iterations=50, norm_inf=True, stop_plain=True)
    works = lambda: DC.seek(prob, op, X0.copy(), p, ls, **kw)
    na = hip.newton_deflated_native(prob, op, X0, p, ls, **kw)
    s, m = works(), DC.seek(prob, op, X0.copy(), p, ls, native=False, **kw)
    for r in (s, m):
        assert r["accepted"] and r["reason"] == 0 and r["converged"] and na["converged"]
        assert (r["itnewton"], r["itlineartot"]) == (na["itnewton"], na["itlineartot"]) and r["itnewton_total"] == na["itnewton"] + 1
        probe("defcont.seek_vs_newton_native", np.abs(r["u"].numpy() - na["u"].numpy()).max(), 8 * EPS * np.abs(na["u"].numpy()).max(), tight=0.0)
        assert len(r["residuals"]) == len(na["residuals"]) and r["plain_residual"] < TOL
        assert r["min_dist_normC"] == min(op.dist(r["u"])[1]) >= TOL
    assert s["residuals"] == na["residuals"] and s["plain_residual"] == na["residuals"][-1]      # the same loop
    assert abs(s["min_dist"] - na["min_dist"]) <= 8 * EPS * na["min_dist"] and s["M"] == na["M"]
    # the found state deflated as well
    found = s["u"]
    op2 = hip.DeflationOperator(2, 1.0, op.roots + [found], autodiff=True)
    on = DC.seek(prob, op2, found.copy(), p, ls, **kw)
    assert not on["accepted"] and on["reason"] == 1 and on["itnewton"] == 0 and math.isinf(on["M"]) and on["min_dist_normC"] == 0.0
    near = found.copy()
    _perturb(ctx, near, 4 * EPS, 1, 0)
    for native in (True, False):
        nr = DC.seek(prob, op2, near.copy(), p, ls, native=native, **kw)
        assert not nr["accepted"] and nr["reason"] in (1, 3), nr
        print(f"near the deflated state (native = {native}): reason {nr['reason']}, {nr['itnewton']} iterations, distance {nr['min_dist_normC']:.2e}")
    assert works()["accepted"]
    # tol below the floor; the ring
    low = dict(kw, tol=1e-17, max_iterations=200)
    a = DC.seek(prob, op, X0.copy(), p, ls, cap=16, **low)
    b = DC.seek(prob, op, X0.copy(), p, ls, cap=256, **low)
    assert not a["accepted"] and a["reason"] in (1, 2) and a["reason"] == b["reason"]
    assert a["itnewton_total"] == b["itnewton_total"] == a["itnewton"] + 1 == 201 and len(b["residuals"]) == 201
    assert len(a["residuals"]) == 16 and a["residuals"] == b["residuals"][-16:] and b["residuals"][:len(na["residuals"])] == na["residuals"]
    assert works()["accepted"]
    # x aliasing a root
    x = X0.copy()
    with pytest.raises(L.BkHipError, match="bk_defcont_seek: x aliases root 1"):
        DC.seek(prob, hip.DeflationOperator(2, 1.0, [op.roots[0], x], autodiff=True), x, p, ls, **kw)
    assert np.array_equal(x.numpy(), start) and works()["accepted"]
    none = DC.seek(prob, hip.DeflationOperator(2, 1.0, [], autodiff=True), X0.copy(), p, ls, **kw)
    s0 = hip.newton_native(prob, X0, p, ls, tol=TOL, max_iterations=50, norm_inf=True)
    assert none["accepted"] and none["itnewton"] == s0["itnewton"] and np.array_equal(none["u"].numpy(), s0["u"].numpy())
    assert math.isinf(none["min_dist_normC"]) and none["M"] == 1.0


# ------------------------------------------------------------------------------------------ 4: end to end
_runs = {}


def _run(ctx, N, native, steps, max_branches, max_iter_defop, seek_every_step=1):
    """deflated_continuation on MC.sh_case(N) with the parameters of defcont_ref.sh_run, GMRESKrylovKit(40) and
    DCTPreconditioner(prob, 1.0); every state is saved.  Computed once per argument set."""
    key = (N, native, steps, max_branches, max_iter_defop, seek_every_step)
    if key not in _runs:
        hip, DC = _lib()
        from bk_amd import continuation as Cn
        c, o = MC.sh_case(N), R.SH_RUN
        prob = hip.SwiftHohenberg(ctx, c["dims"], c["ls"], l=c["p"] - o["back"], nu=c["nu"])
        ls = _solver(hip, prob)
        op = hip.DeflationOperator(2, 1.0, [prob.vec(np.zeros(c["op"].N))], autodiff=True)
        alg = DC.DefCont(deflation_operator=op, max_branches=max_branches, seek_every_step=seek_every_step,
                         max_iter_defop=max_iter_defop, perturb_solution=DC.uniform_perturbation(o["amp"], o["seed"]))
        cp = Cn.ContinuationPar(ds=o["ds"], p_min=-1.0, p_max=1.0, max_steps=steps, save_sol_every_step=1,
                                newton_options=Cn.NewtonPar(tol=o["tol"], max_iterations=o["max_iterations"], linsolver=ls))
        res = DC.deflated_continuation(prob, alg, cp, normC=Cn.norminf, native=native)
        assert len(op.roots) == 1 and alg.stop_plain is None                       # the caller's operator is left alone
        host = [[s["x"].numpy() for s in b.sol if not s.get("lost")] for b in res.branches]
        _runs[key] = (res, host)
    return _runs[key]


def _check_invariants(N, res, host, steps, ref, tag):
    """The trivial branch has all its points; at least 2 non-trivial branches at the first parameter value (< l*); every recorded
    state a zero of the ORACLE's F to 10 tol; the states at one parameter value pairwise >= tol apart (inf-norm); along each
    branch normu changes by less than 2 x the restatement's largest step-to-step change; every final state, polished by the
    restatement's plain Newton (sparse LU), moves by <= 10 tol / |lambda_min(J)|."""
    c = MC.sh_case(N)
    b0 = res.branches[0]
    p1 = c["p"] - R.SH_RUN["back"] + R.SH_RUN["ds"]
    assert len(b0.param) == steps and all(x == 0.0 for x in b0.normu) and abs(b0.param[0] - p1) < 1e-14 and p1 < c["p"]
    for b, h in zip(res.branches, host):
        assert len(h) == len(b.param) == len(b.normu) == len(b.itnewton) == len(b.itlinear) >= 1
        assert [s["p"] for s in b.sol if not s.get("lost")] == b.param and (b.active or b.sol[-1]["lost"]) and b.step == list(range(1, len(b.param) + 1))
        for x, nu_ in zip(h, b.normu):
            assert nu_ == np.abs(x).max()
    first = [b for b in res.branches[1:] if b.param[0] == b0.param[0]]
    assert len(first) >= 2 and all(b.normu[0] > 0.5 for b in first), [b.normu[0] for b in first]
    worst = max(R.norminf(c["F"](x, p)) for b, h in zip(res.branches, host) for p, x in zip(b.param, h))
    probe(f"defcont.e2e_oracle_residual.{tag}", worst, 10 * TOL)
    for p in b0.param:
        at = [x for b, h in zip(res.branches, host) for q, x in zip(b.param, h) if q == p]
        assert R.pairwise_min_inf(at) >= TOL
    dref = max(float(np.abs(np.diff(b["normu"])).max()) for b in ref["branches"] if len(b["normu"]) > 1)
    dgpu = max((float(np.abs(np.diff(b.normu)).max()) for b in res.branches if len(b.normu) > 1), default=0.0)
    probe(f"defcont.e2e_normu_step.{tag}", dgpu, 2 * dref, restatement=dref)
    for b, h in zip(res.branches, host):
        p, x = b.param[-1], h[-1]
        pol = MC.deflated_newton(lambda v: c["F"](v, p), lambda v: c["J"](v, p), [], x, 1e-13, 10)
        lam = float(np.abs(np.linalg.eigvalsh(c["J"](pol["u"], p).toarray())).min())
        probe(f"defcont.e2e_polish.{tag}", R.norminf(pol["u"] - x), 10 * TOL / lam, lam=lam)
    print(f"{tag}: {len(res.branches)} branches ({sum(b.active for b in res.branches)} active), {len(first)} non-trivial at l = {p1:.4f}; "
          f"Newton {sum(map(sum, (b.itnewton for b in res.branches)))}, linear {sum(map(sum, (b.itlinear for b in res.branches)))}; "
          f"{len(res.seeks)} seeks, {sum(s['itnewton'] for s in res.seeks)} seek iterations; worst oracle |F| {worst:.2e}")


def test_end_to_end_16x16_native(ctx):
    """The 16 x 16 run (u = 0 at l* - 0.035, ds = 0.01, 8 steps, max_branches = 12, uniform_perturbation(0.1, seed)) as library
    calls: the invariants, not the discovered set -- Newton from noise amplifies solver differences."""
    res, host = _run(ctx, 2, True, 8, 12, 3)
    _check_invariants(2, res, host, 8, R.sh_run(2, 8, 12, 3), "16x16.native")
    assert len(res.sol) == sum(b.active for b in res.branches)


def test_end_to_end_16x16_mirror_agrees_with_native(ctx):
    """The call-by-call mirror from the same seed: the same kernels in the same order, so the same branch count, activity flags,
    parameters, Newton and linear counts and seek log, and every state to 8 ulp."""
    nat, hn = _run(ctx, 2, True, 8, 12, 3)
    mir, hm = _run(ctx, 2, False, 8, 12, 3)
    _check_invariants(2, mir, hm, 8, R.sh_run(2, 8, 12, 3), "16x16.mirror")
    assert len(nat.branches) == len(mir.branches) and nat.seeks == mir.seeks
    for a, b, xa, xb in zip(nat.branches, mir.branches, hn, hm):
        assert (a.active, a.param, a.itnewton, a.itlinear, a.step) == (b.active, b.param, b.itnewton, b.itlinear, b.step)
        for x, y in zip(xa, xb):
            probe("defcont.e2e_native_vs_mirror", np.abs(x - y).max(), 8 * EPS * max(np.abs(x).max(), 1e-300), tight=0.0)


def test_max_branches_and_seek_every_step(ctx):
    """max_branches = 3: every branch the first step finds from the trivial one is active (:344 counts the OLD branches visited),
    which makes 3 or more, and no later step seeks.  seek_every_step = 3 seeks on steps 0, 3 and 6 only.  An operator without
    roots raises, as the reference does."""
    hip, DC = _lib()
    from bk_amd import continuation as Cn
    res, _ = _run(ctx, 2, True, 3, 3, 3)
    assert sum(b.active for b in res.branches) >= 3 and {s["step"] for s in res.seeks} == {0}
    assert [s["reason"] for s in res.seeks].count(0) == len(res.branches) - 1 and res.seeks[-1]["reason"] != 0
    res, _ = _run(ctx, 2, True, 8, 100, 1, seek_every_step=3)
    assert {s["step"] for s in res.seeks} == {0, 3, 6}
    c = MC.sh_case(2)
    prob = hip.SwiftHohenberg(ctx, c["dims"], c["ls"], l=0.0, nu=c["nu"])
    with pytest.raises(ValueError, match="at least one guess"):
        DC.deflated_continuation(prob, DC.DefCont(deflation_operator=hip.DeflationOperator(2, 1.0, [], autodiff=True)),
                                 Cn.ContinuationPar(newton_options=Cn.NewtonPar(linsolver=_solver(hip, prob))))


def test_end_to_end_8x8x8(ctx):
    """One 3-D run: 8 x 8 x 8 (MC.sh_case(3)), 3 steps, max_branches = 4, max_iter_defop = 2; the same invariants."""
    res, host = _run(ctx, 3, True, 3, 4, 2)
    _check_invariants(3, res, host, 3, R.sh_run(3, 3, 4, 2), "8x8x8.native")
