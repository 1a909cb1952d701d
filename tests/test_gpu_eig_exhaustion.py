"""The Krylov-Schur eigensolvers of csrc/eig.hip (bk_eig_shiftinvert, bk_eig_krylovkit, bk_eig_krylovkit_lm) where the Krylov space runs
out, against dense spectra.  The eigensolver half of tests/test_gpu_krylov_exhaustion.py.

Every problem has at most 384 unknowns; in group A the basis is asked to hold more vectors (krylovdim up to 63) than the space has
dimensions (n = 24, 30, 32), so the n-th operator application leaves a remainder at rounding level and eig_core must notice: it stops
expanding only on the `beta == 0.0` that arnoldi_step returns when the explicit remainder satisfies `!(nn > 1e-30 * ww)`.
tests/test_eig_exhaustion_reference.py shows on the reference alone (tests/eig_exhaustion_ref.py) that each case is such a case, that the
float64 restatement of the step sees nn / ww = 2.5e-32 .. 1.6e-31 there, and what a solver that misses the breakdown returns (13 to 21
Ritz values off the spectrum, the unstable count up by 9 to 21, 45 applications instead of n).  The Python classes clamp krylovdim to
n - 1, so every solve here goes through ctx.lib.bk_eig_* with _lib.EigOpts directly; one leg per case goes through the classes as the
control.

What every solve asserts (``_check``): status 0; nvals <= d, NaN behind nvals, untouched NaN guards around values and vectors; every
value matches a dense eigenvalue OF ITS OWN within E (injective assignment: a ghost copy or an off-spectrum value fails); the set is the
reference's wanted set in the documented order; where krylovdim >= d no NaN among the first min(nev, d) and nconv >= min(nev, d); the
count of Re > tol_stability equals the dense count inside the wanted set; |J v - lambda v| <= R |v| on the dense J in longdouble (which
also ties vector i to value i), hermitian vectors orthonormal to 1e-10; and the number of operator applications equals d EXACTLY
wherever krylovdim >= d, the same for every such krylovdim and both eig_gram settings -- the d-th application is the one that reveals
the breakdown, one more means it was missed by a step.  Bounds E, R: eig_exhaustion_ref.bounds_from, every term from the dense reference.

Measured on the MI355X (MEASURED below).  Before the fix in csrc/eig.hip (breakdown at beta <= 64 eps |H|, basis capped at the global
dimension) this file failed on every A case: krylovdim = n + 1 took n + 1 applications, the hermitian solves returned NaN only, the
cGL solves returned values such as 0.99996665 + 4.9e-6 i next to sigma = 1, and the native branch counted [0, 0, 0, 0] unstable
eigenvalues for the dense [0, 0, 1, 1].
"""
import ctypes as C

import numpy as np
import pytest

import eig_exhaustion_ref as R
from conftest import probe

pytestmark = pytest.mark.gpu

GUARD = 64                      # doubles of NaN on both sides of every output
ETA, ATOL = 1e-12, 1e-14        # inner solves: rtol, atol
TAU = 1e-12                     # eigensolver tol (SH3dEig's)
MAXITER = 20
B_TAU, B_ETA = 1e-9, 1e-10      # group B converges on the tolerance, through MINRES + Pl: the pair of tests/test_gpu_eigensolve_at_size.py
ENTRY = {"si": "bk_eig_shiftinvert", "lr": "bk_eig_krylovkit", "lm": "bk_eig_krylovkit_lm"}

# What the run this file was committed with measured on the MI355X (documentation; nothing reads it).
MEASURED = {
    "operator applications, group A, every krylovdim >= n, nev and eig_gram": "n exactly (24, 24, 24, 30, 32), all three modes",
    "beta / |H| at the exhausting step (option eig_last_beta_over_h; the library's threshold is 64 eps = 1.4e-14)":
        "0 .. 8.9e-29 over all A solves: sh-4x3x2 si 8.9e-29, lr / lm 2.1e-29; sh-6x5 si 1.6e-29, lr / lm 3.8e-31; sh-8x4 si 1.2e-29, "
        "lr / lm 9.9e-31; cgl-4x3-rand si 5.5e-30",
    "the device's nn / ww of arnoldi_step at the exhausting step": "not measured (beta above is the product of both passes' remainders)",
    "largest eigenvalue error / residual, group A, krylovdim >= n (worst share of E / R)":
        "si 6.3e-13 / 1.3e-11 (0.36 / 0.084), lr 1.8e-13 / 1.8e-13 (0.009 / 0.011), lm 3.8e-13 / 3.9e-13 (0.022 / 0.023); with the "
        "preconditioned inner solver 8.5e-14 / 1.5e-12 (0.008 / 0.014)",
    "group B / group C, largest eigenvalue error / residual": "B 1.1e-12 / 3.9e-11 (6e-4 / 8e-6 of E / R); C 3.2e-15 / 3.1e-15",
    "krylovdim = n - 1, the legs that pass (all SH, cgl-4x3-rand si)": "si 1.8e-11 / 2.0e-9 (0.35 / 0.088), lr 1.8e-14 / 1.5e-13, lm 5.6e-13 / 5.6e-13",
    "control through the classes, eigenvalue error / E": "si 0.35 / 0.21 / 0.16 (SH), 4e-4 (cGL); lr <= 2.5e-3; cgl-4x3-rand lr misses",
    "native branch and mirror, largest eigenvalue error": "1.04e-13 (E: 0.18 used), n_unstable [0, 0, 1, 1] on both, 32 solves per step",
    "restarted non-symmetric (krylovdim = n - 1 = 23, eig_gram = 1; fails, see test_one_vector_short_of_the_space)":
        "cgl-4x3-zero lm nev 1: residual 9.5e-7 for R = 2.2e-12; si nev 22: eigenvalue error 1.9e-6 for E = 9.6e-8; cgl-4x3-rand lr nev 1: "
        "eigenvalue error 3.5e-10 for E = 3.6e-12, lm nev 1: 6.3e-8 for 3.6e-12; control cgl-4x3-rand lr: error / E = 2.1e6",
}


def _hip():
    from bk_amd import hip
    return hip


class _EigGram:
    """eig_gram on the shared context, put back on exit (default 1: csrc/eig.hip)."""

    def __init__(self, ctx, value):
        self.ctx, self.value = ctx, value

    def __enter__(self):
        try:
            self.prior = self.ctx.get_option("eig_gram")
        except Exception:
            self.prior = 1.0
        self.ctx.set_option("eig_gram", self.value)

    def __exit__(self, *exc):
        self.ctx.set_option("eig_gram", self.prior)


class _Device:
    """The device side of a case: problem, Jacobian, inner solvers, start vector."""

    def __init__(self, ctx, cid):
        hip = _hip()
        c = R.case(cid)
        u, _ = R.state(cid)
        self.ctx, self.cid, self.case = ctx, cid, c
        if c.kind == "sh":
            self.prob = hip.SwiftHohenberg(ctx, c.dims, c.ls, **R.SH_PARAMS)
            self.J = self.prob.jacobian(self.prob.vec(np.array(u)), R.SH_PARAMS["l"])
            self.P = hip.DCTPreconditioner(self.prob, 1.0)
        else:
            self.prob = hip.CGL2d(ctx, c.dims, c.ls, **R.CGL_PARAMS)
            self.J = self.prob.jacobian(self.prob.vec(np.array(u)), R.CGL_PARAMS["r"])
            self.P = hip.CGLBlockPreconditioner(self.prob, R.CGL_PARAMS["r"] - c.sigma, R.CGL_PARAMS["nu"])
        x, upload = R.start_vector(cid)
        self.x0 = self.prob.vec(np.array(x)) if upload else None

    def inner(self, preconditioned, eta=ETA):
        hip = _hip()
        if not preconditioned:
            return hip.GMRESKrylovKit(dim=min(self.case.n, 60), rtol=eta, atol=ATOL, Pl=None)
        if self.case.kind == "sh":                                   # (M-norm stop: the sqrt(1 + Lmax) factor)
            return hip.KrylovLSSymmetric("minres", rtol=eta, atol=ATOL, itmax=4000, Pl=self.P)
        return hip.GMRESKrylovKit(dim=min(self.case.n, 60), rtol=eta, atol=ATOL, Pl=self.P)


@pytest.fixture(scope="module")
def dev(ctx):
    cache = {}

    def get(cid):
        if cid not in cache:
            cache[cid] = _Device(ctx, cid)
        return cache[cid]
    yield get
    cache.clear()


def _solve(d, mode, nev, krylovdim, ls=None, tau=TAU):
    """One bk_eig_* call into guarded outputs: dict(vals, vecs, nvals, nconv, nops).  vals: the nev + 1 slots as complex; vecs: n x
    nvals complex."""
    import torch
    from bk_amd import _lib as L
    ctx, c = d.ctx, d.case
    n = c.n
    ld = (n + 31) // 32 * 32
    slots = nev + 1
    re = np.full(slots + 2 * GUARD, np.nan)
    im = np.full(slots + 2 * GUARD, np.nan)
    dp = lambda a: a[GUARD:].ctypes.data_as(C.POINTER(C.c_double))      # noqa: E731
    full = [torch.full((ld * slots + 2 * GUARD,), float("nan"), dtype=torch.float64, device=ctx.torch_device)
            for _ in range(1 if c.hermitian else 2)]
    pv = [C.c_void_p(f[GUARD:GUARD + ld * slots].data_ptr()) for f in full] + ([None] if c.hermitian else [])
    eo = L.EigOpts(float(c.sigma), int(krylovdim), MAXITER, float(tau), 1 if c.hermitian else 0, R.SEED)
    nvals, nconv, nops = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    if d.x0 is not None:
        ctx.check(ctx.lib.bk_eig_set_start_vector(ctx.h, C.c_void_p(d.x0.t.data_ptr())), "bk_eig_set_start_vector")
    tail = (dp(re), dp(im), pv[0], pv[1], ld, C.byref(nvals), C.byref(nconv), C.byref(nops))
    if mode == "si":
        lo = ls._opts()
        st = ctx.lib.bk_eig_shiftinvert(ctx.h, d.J.h, nev, C.byref(eo), C.byref(lo), ls._pl(), *tail)
    else:
        st = getattr(ctx.lib, ENTRY[mode])(ctx.h, d.J.h, nev, C.byref(eo), *tail)
    ctx.check(st, ENTRY[mode])                                        # status 0: no "did not converge" / "restart basis has rank"
    ctx.sync()
    for a in (re, im):
        assert np.isnan(a[:GUARD]).all() and np.isnan(a[GUARD + slots:]).all(), "the solve wrote outside its value arrays"
    V = []
    for f in full:
        a = f.cpu().numpy()
        assert np.isnan(a[:GUARD]).all() and np.isnan(a[GUARD + ld * slots:]).all(), "the solve wrote outside its vector array"
        V.append(a[GUARD:GUARD + ld * slots].reshape(slots, ld)[:, :n].T)
    m = nvals.value
    vecs = (V[0] + (1j * V[1] if len(V) == 2 else 0.0))[:, :max(m, 0)]
    if d.x0 is not None:
        x, _ = R.start_vector(d.cid)
        assert np.array_equal(d.x0.numpy(), x), "the solve changed its start vector"
    return dict(vals=re[GUARD:GUARD + slots] + 1j * im[GUARD:GUARD + slots], vecs=vecs, nvals=m, nconv=nconv.value, nops=nops.value)


def _check(d, mode, nev, krylovdim, out, what, worst, preconditioned=False, grade=None, exact=True):
    """Checks 1 to 8 of the module docstring on one solve (1: _solve).  ``exact``: krylovdim >= d, the solve ends by breakdown."""
    c, cid = d.case, d.cid
    sp = R.spectrum(cid)
    dgrade = c.n if grade is None else grade
    w = R.wanted(cid, mode, nev)
    vals, m = out["vals"], out["nvals"]
    # 2
    assert 0 <= m <= min(dgrade, nev + 1) and m <= w.nvals, (what, m, w.nvals)
    assert np.isnan(vals[m:].real).all() and np.isnan(vals[m:].imag).all(), (what, vals)
    got = vals[:m]
    ok = ~np.isnan(got.real)
    assert not np.isnan(got[ok].imag).any() and (ok[:int(ok.sum())].all()), (what, got)          # NaNs last
    if c.hermitian:
        assert np.all(got[ok].imag == 0.0), (what, got)
    # 5
    if exact:
        assert m == w.nvals and ok.all(), (what, got)
        assert out["nconv"] >= min(nev, dgrade), (what, out["nconv"])
    # 3: injective assignment to the whole dense spectrum, each value within the bound of the eigenvalue it is assigned to
    lam = np.asarray(sp.lam, dtype=complex)
    cols, dist = R.match(got[ok], lam)
    E, Rb = R.bounds(cid, mode, lam[cols], eta=ETA if mode == "si" else 0.0, preconditioned=preconditioned)
    if not exact:
        dE, dR = _accepted(d, mode, lam[cols], out["nconv"] >= m)
        E, Rb = E + dE, Rb + dR
    bad = dist > E
    assert not bad.any(), (what, "off the spectrum or a ghost copy", got[ok][bad], dist[bad], E[bad])
    # 4: the set is the wanted set, in the documented order
    wanted_idx = {int(np.argmin(np.abs(lam - z))) for z in w.values}
    assert set(int(i) for i in cols) <= wanted_idx, (what, got, w.values)
    if exact:
        assert set(int(i) for i in cols) == wanted_idx, (what, got, w.values)
    key = np.abs(got[ok]) if mode == "lm" else got[ok].real
    assert np.all(np.diff(key) <= 2 * E.max()), (what, "order", got)
    # 6
    if exact:
        assert int(np.sum(got.real > R.TOL_STABILITY)) == w.n_unstable, (what, got, w.n_unstable)
    else:
        assert int(np.sum(got[ok].real > R.TOL_STABILITY)) == int(np.sum(lam[cols].real > R.TOL_STABILITY)), (what, got)
    # 7
    V = out["vecs"][:, :m][:, ok]
    res = np.array([R.residual(cid, z, V[:, i]) for i, z in enumerate(got[ok])])
    assert np.all(res <= Rb), (what, "residual", res, Rb)
    if c.hermitian and V.shape[1]:
        G = V.real.T @ V.real
        assert np.abs(G - np.eye(V.shape[1])).max() <= 1e-10, (what, np.abs(G - np.eye(V.shape[1])).max())
    # 8
    if exact:
        assert out["nops"] == dgrade, (what, "operator applications", out["nops"], dgrade)
    wk = worst.setdefault(mode, dict(eig=0.0, res=0.0, eig_abs=0.0, res_abs=0.0))
    if ok.any():
        wk["eig"] = max(wk["eig"], float((dist / E).max()))
        wk["res"] = max(wk["res"], float((res / Rb).max()))
        wk["eig_abs"] = max(wk["eig_abs"], float(dist.max()))
        wk["res_abs"] = max(wk["res_abs"], float(res.max()))


def _accepted(d, mode, lam_ref, strict, tau=TAU):
    """What a solve that ends on its tolerance instead of a breakdown (krylovdim < d) adds to (E, R): the library reports a Ritz pair
    whose residual rho = |A y - mu y| is below tau (strictly converged: nconv covers it) or below max(tau, sqrt(eps) |mu|) (its
    documented "usable" rule, csrc/eig.hip).  Bauer-Fike: |dmu| <= kappa rho; for shift-invert mu = 1 / (lambda - sigma), so the
    eigenvalue moves by 2 d^2 kappa rho and the vector's residual on J by |J - sigma| d rho; on J itself by kappa rho and rho."""
    sp, c = R.spectrum(d.cid), d.case
    lam_ref = np.asarray(lam_ref, dtype=complex)
    dist = np.abs(lam_ref - c.sigma)
    mu = 1.0 / dist if mode == "si" else np.abs(lam_ref)
    rho = np.full(len(lam_ref), tau) if strict else np.maximum(tau, np.sqrt(R.EPS) * mu)
    if mode == "si":
        return 2.0 * dist ** 2 * sp.kappa * rho, sp.normJs * dist * rho
    return sp.kappa * rho, rho


def _log(group, cid, worst, **kw):
    for mode, wk in worst.items():
        probe(f"eig exhaustion {group}: eigenvalue error / E", wk["eig"], 1.0, 0.1, case=cid, mode=mode, largest=wk["eig_abs"], **kw)
        probe(f"eig exhaustion {group}: residual / R", wk["res"], 1.0, 0.1, case=cid, mode=mode, largest=wk["res_abs"], **kw)


# ------------------------------------------------------------------------------------------------------------------ A
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("cid", list(R.A_CASES))
def test_whole_space_exhausted(ctx, dev, cid, mode):
    """Group A: krylovdim in {n, n + 1, 45, 63} x nev in {1, 6, n - 2} x eig_gram in {1, 0}; shift-invert with the unpreconditioned
    GMRES(min(n, 60)) whose solves end by exhaustion themselves, :LR and :LM on the same Jacobian.  (krylovdim = n - 1: the next test.)"""
    d = dev(cid)
    n = d.case.n
    ls = d.inner(False) if mode == "si" else None
    worst, counts, ratios = {}, {}, []
    for gram in (1, 0):
        with _EigGram(ctx, gram):
            for nev in R.nev_grid(cid, mode):
                for kd in R.krylovdims(n)[1:]:
                    what = (cid, mode, dict(nev=nev, krylovdim=kd, eig_gram=gram))
                    out = _solve(d, mode, nev, kd, ls)
                    _check(d, mode, nev, kd, out, what, worst)
                    counts[nev, kd, gram] = out["nops"]
                    ratios.append(ctx.get_option("eig_last_beta_over_h"))
    assert set(counts.values()) == {n}, counts
    probe("eig exhaustion A: operator applications - d", max(counts.values()) - n, 0, 0, case=cid, mode=mode)
    # the device's remainder at the exhausting step, beta / |H| (diagnostic option of csrc/eig.hip), under the library's threshold 64 eps:
    # the breakdown is seen as one, not merely cut off by the cap at n vectors
    probe("eig exhaustion A: beta / |H| at step d", max(ratios), 64 * R.EPS, 8 * R.EPS, case=cid, mode=mode, smallest=min(ratios))
    _log("A", cid, worst)


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("cid", list(R.A_CASES))
def test_one_vector_short_of_the_space(ctx, dev, cid, mode):
    """Group A, krylovdim = n - 1: the largest basis that does not exhaust the space; the solve restarts and ends on its tolerance.  Same
    checks but 5 and 8 (NaN slots are allowed), with the acceptance rule's terms added to E and R (``_accepted``).  Every leg is run and
    every miss reported, not only the first.
    The cGL cases are what found the restart's noise direction (csrc/eig.hip: a real Ritz value's vector with a negligible imaginary part):
    with 23 of 24 vectors the solver called pairs converged at an estimate of 8e-18 whose true residual was 9.5e-7."""
    d = dev(cid)
    n = d.case.n
    ls = d.inner(False) if mode == "si" else None
    worst, misses = {}, []
    for gram in (1, 0):
        with _EigGram(ctx, gram):
            for nev in R.nev_grid(cid, mode):
                what = (cid, mode, dict(nev=nev, krylovdim=n - 1, eig_gram=gram))
                out = _solve(d, mode, nev, n - 1, ls)
                try:
                    _check(d, mode, nev, n - 1, out, what, worst, exact=False)
                except AssertionError as e:
                    misses.append(" ".join(str(e).split())[:400])
    assert not misses, misses
    _log("A (krylovdim n - 1)", cid, worst)


@pytest.mark.parametrize("cid", list(R.A_CASES))
def test_whole_space_exhausted_with_the_preconditioned_inner_solver(ctx, dev, cid):
    """Group A, one leg per case through the transform preconditioners: SH with MINRES + (L1 + I)^-1, cGL with GMRES and the exact inverse
    of the trivial state's shifted Jacobian; the bound carries the inner solver's factor (eig_exhaustion_ref.inner_factor)."""
    d = dev(cid)
    n = d.case.n
    worst = {}
    for kd in (n, 63):
        out = _solve(d, "si", 6, kd, d.inner(True))
        _check(d, "si", 6, kd, out, (cid, "si+Pl", kd), worst, preconditioned=True)
    _log("A+Pl", cid, worst, factor=R.inner_factor(cid, True))


@pytest.mark.parametrize("cid", list(R.A_CASES))
def test_control_through_the_classes_without_exhaustion(ctx, dev, cid):
    """The control: the Python classes clamp krylovdim to n - 1, so the solve ends on its tolerance; same values, same bounds (with the
    acceptance rule's terms, ``_accepted``)."""
    hip = _hip()
    d = dev(cid)
    c, sp = d.case, R.spectrum(cid)
    lam = np.asarray(sp.lam, dtype=complex)
    for mode, eig in (("si", hip.ShiftInvert(c.sigma, d.inner(False), tol=TAU, maxiter=MAXITER, krylovdim=63, hermitian=c.hermitian,
                                             seed=R.SEED, x0=d.x0)),
                      ("lr", hip.EigKrylovKit(tol=TAU, maxiter=MAXITER, krylovdim=63, hermitian=c.hermitian, seed=R.SEED,
                                              save_vectors=True, x0=d.x0))):
        vals, vecs, cv, nops = eig(d.J, 6)
        w = R.wanted(cid, mode, 6)
        got = vals[~np.isnan(vals.real)]
        assert len(vals) == w.nvals and len(got) == len(vals), (cid, mode, vals)
        cols, dist = R.match(got, lam)
        E, Rb = R.bounds(cid, mode, lam[cols], eta=ETA if mode == "si" else 0.0)
        dE, dR = _accepted(d, mode, lam[cols], cv)
        E, Rb = E + dE, Rb + dR
        wanted_idx = {int(np.argmin(np.abs(lam - z))) for z in w.values}
        assert set(int(i) for i in cols) == wanted_idx, (cid, mode, vals, w.values)
        probe("eig exhaustion control: eigenvalue error / E", float((dist / E).max()), 1.0, 0.1, case=cid, mode=mode, numops=nops)
        assert int(np.sum(got.real > R.TOL_STABILITY)) == w.n_unstable
        res = [R.residual(cid, z, vecs[i][0].numpy() + (0.0 if vecs[i][1] is None else 1j * vecs[i][1].numpy()))
               for i, z in enumerate(vals)]
        probe("eig exhaustion control: residual / R", float((np.array(res) / Rb).max()), 1.0, 0.1, case=cid, mode=mode)


# ------------------------------------------------------------------------------------------------------------------ C
@pytest.mark.parametrize("kd", [24, 45, 63])
def test_conjugate_pair_at_the_cut_is_returned_whole(ctx, dev, kd):
    """Group C: cGL (4,3) at u = 0, nev = 3 -- position 3 splits a conjugate pair: nvals = nev + 1, both members present."""
    d = dev(R.C_CASE)
    nev = R.pair_split_nev(R.C_CASE)
    worst = {}
    out = _solve(d, "si", nev, kd, d.inner(False))
    assert out["nvals"] == nev + 1, out
    _check(d, "si", nev, kd, out, (R.C_CASE, "pair", kd), worst)
    got = out["vals"][:nev + 1]
    for z in got:
        assert np.abs(got - np.conj(z)).min() <= 1e-9 and abs(z.imag) > 0.5, got
    _log("C", R.C_CASE, worst, krylovdim=kd)


# ------------------------------------------------------------------------------------------------------------------ B
@pytest.mark.parametrize("cid", list(R.B_CASES))
def test_start_vector_in_an_invariant_subspace(ctx, dev, cid):
    """Group B: SH (8,8,6), x0 = a sum of six dense eigenvectors (nev = 6 and nev = 10, more than the subspace holds) or a single one
    (nev = 3), krylovdim 30.  The subspace is invariant only to the eigenvectors' accuracy (remainder ratio 2e-24 in the restatement, far
    above the breakdown threshold): the solve goes on past it on the remainder and converges on its tolerance, so no claim on counts --
    the values must be the nev nearest sigma, each once, with their vectors."""
    start, nev = R.B_CASES[cid]
    d = dev(cid)
    c, sp = d.case, R.spectrum(cid)
    out = _solve(d, "si", nev, R.B_KRYLOVDIM, d.inner(True, B_ETA), tau=B_TAU)
    w = R.wanted(cid, "si", nev)
    vals, m = out["vals"], out["nvals"]
    assert m == nev and not np.isnan(vals[:m].real).any() and np.all(vals[:m].imag == 0.0), (cid, vals)
    assert np.isnan(vals[m:].real).all()
    lam = np.asarray(sp.lam, dtype=complex)
    cols, dist = R.match(vals[:m], lam)
    E, Rb = R.bounds(cid, "si", lam[cols], eta=B_ETA, preconditioned=True, tau=B_TAU)
    assert len(set(int(i) for i in cols)) == nev                                     # none twice
    assert set(int(i) for i in cols) == {int(np.argmin(np.abs(lam - z))) for z in w.values}, (cid, vals, w.values)
    assert np.all(np.diff(vals[:m].real) <= 0.0), vals
    near = np.argsort(np.abs(sp.lam - c.sigma), kind="stable")
    assert set(int(i) for i in near[:min(nev, R.grade(cid))]) <= set(int(i) for i in cols)     # the subspace's own values are among them
    if start == "eig1":
        assert int(near[0]) in set(int(i) for i in cols)                             # that eigenvector's value: the one nearest sigma
    probe("eig exhaustion B: eigenvalue error / E", float((dist / E).max()), 1.0, 0.1, case=cid, largest=float(dist.max()),
          numops=out["nops"], nconv=out["nconv"])
    V = out["vecs"][:, :m].real
    res = np.array([R.residual(cid, z, V[:, i]) for i, z in enumerate(vals[:m])])
    probe("eig exhaustion B: residual / R", float((res / Rb).max()), 1.0, 0.1, case=cid, largest=float(res.max()))
    assert np.abs(V.T @ V - np.eye(m)).max() <= 1e-10
    assert int(np.sum(vals[:m].real > R.TOL_STABILITY)) == w.n_unstable


# ------------------------------------------------------------------------------------------------------------------ native branch
def _branch_bounds(p, vals):
    """Dense spectrum of J(0, p) of SH (8,4), the assignment of the reported values to it, and E per value."""
    ev = R.branch_spectrum(p)
    n = len(ev)
    cols, dist = R.match(vals, ev)
    E, _ = R.bounds_from("si", ev[cols], n, 0.1, 1.0, float(np.abs(ev - 0.1).min()), float(np.abs(ev).max()), float(np.abs(ev - 0.1).max()),
                         eta=ETA)
    return ev, cols, dist, E


def test_native_branch_past_exhaustion_counts_like_the_dense_spectrum_and_the_mirror(ctx):
    """continuation_native along u = 0 of SH (8,4) through the first l*: 3 steps at the native default krylovdim (36 > n = 32), hermitian
    ShiftInvert(0.1), detect_bifurcation = 3.  n_unstable equals the dense count at every point and the eigenvalues pass checks 3 to 6;
    the Python mirror of the same branch, which clamps krylovdim to n - 1, reports the same counts and the same eigenvalues within E."""
    from bk_amd import continuation as Cn
    hip = _hip()
    params, counts, _ = R.branch_reference()
    ls_half = R.LS[:2]
    prob = hip.SwiftHohenberg(ctx, R.BRANCH_DIMS, ls_half, **R.SH_PARAMS)
    n = prob.nglobal
    P = hip.DCTPreconditioner(prob, 1.0)
    ls = hip.GMRESKrylovKit(dim=30, rtol=1e-10, atol=1e-13, maxiter=150, Pl=P)
    els = hip.GMRESKrylovKit(dim=min(n, 60), rtol=ETA, atol=ATOL, Pl=None)
    eig = hip.ShiftInvert(0.1, els, tol=TAU, maxiter=MAXITER, hermitian=True, save_vectors=False, seed=R.SEED)
    assert eig.krylovdim is None                                       # the native default: max(30, nev + 30) = 36
    nopt = Cn.NewtonPar(tol=1e-9, max_iterations=15, linsolver=ls, eigsolver=eig)
    cp = Cn.ContinuationPar(ds=R.BRANCH_DS, dsmin=1e-4, dsmax=R.BRANCH_DSMAX, p_min=-0.1, p_max=0.15, max_steps=R.BRANCH_STEPS,
                            nev=R.BRANCH_NEV, detect_bifurcation=3, newton_options=nopt)
    alg = Cn.PALC(tangent="bordered", theta=0.5, bls=hip.BorderingBLS(None, check_precision=False))
    ops = []
    bn = Cn.continuation_native(prob, prob.vec(np.zeros(n)), params[0], alg, cp, normC=Cn.norminf,
                                finalise_solution=lambda get, r: ops.append(r.eig_numops) or True)
    bm = Cn.continuation(prob, prob.vec(np.zeros(n)), params[0], alg, cp, normC=Cn.norminf)
    for name, br in (("native", bn), ("mirror", bm)):
        assert len(br.param) == len(params), (name, br.param)
        assert np.allclose(br.param, params, rtol=0, atol=1e-9), (name, br.param, params)
        assert list(br.n_unstable) == counts, (name, br.n_unstable, counts)
        for k, (p, vals) in enumerate(zip(br.param, br.eig)):
            vals = np.asarray(vals)
            assert len(vals) == R.BRANCH_NEV and not np.isnan(vals.real).any() and np.all(vals.imag == 0.0), (name, k, vals)
            ev, cols, dist, E = _branch_bounds(p, vals.real)
            probe(f"eig exhaustion branch ({name}): eigenvalue error / E", float((dist / E).max()), 1.0, 0.1, point=k,
                  largest=float(dist.max()))
            near = np.argsort(np.abs(ev - 0.1), kind="stable")[:R.BRANCH_NEV]
            assert set(int(i) for i in cols) == set(int(i) for i in near), (name, k, vals)
            assert np.all(np.diff(vals.real) <= 0.0), (name, k, vals)
            assert int(np.sum(vals.real > R.TOL_STABILITY)) == counts[k] == int(np.sum(ev > R.TOL_STABILITY))
    for k, (a, b) in enumerate(zip(bn.eig, bm.eig)):
        _, _, _, E = _branch_bounds(params[k], np.asarray(b).real)
        assert np.all(np.abs(np.asarray(a).real - np.asarray(b).real) <= 2 * E), (k, a, b)
    assert [sp["step"] for sp in bn.specialpoint] == [sp["step"] for sp in bm.specialpoint] == [counts.index(1)]
    # every eigensolve of the native branch ran past exhaustion and stopped at the n-th solve
    assert ops and all(o == n for o in ops), ops
