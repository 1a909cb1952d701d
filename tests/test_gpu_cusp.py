"""GPU tests of the cusp on fold curves (csrc/cusp.hip: bk_cusp_dots, bk_cusp_rhs, bk_cusp_contract, bk_cusp_normal_form;
bk_amd.codim2: continuation_fold(detect_codim2 = 1 | 2), cusp_normal_form, cusp_normal_form_native, get_normal_form on a "cusp"
point): the three passes against exact sums on integer data, the normal form at the cusp of tests/golden/sh_cusp_128x2.npz against
the dense value, and the detection and bisection on the fold curve against the CPU restatement (tests/cusp_ref.py)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import cusp_ref as Cr
import minaug_fold_ref as R
from conftest import probe
from oracle import operators

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
NU = 1.5                                                      # dyadic: every factor of the integer cases is an integer


def _lib():
    from bk_amd import codim2, hip
    return codim2, hip


def _ulps(a, b):
    return np.abs(a - b) / np.maximum(np.spacing(np.maximum(np.abs(a), np.abs(b))), np.finfo(float).tiny)


# ------------------------------------------------------------------------------------------ the passes
# SH1D: the n list of test_fold_contract_matches_an_exact_sum, the first size past one grid stride of a reducing pass (1024
# workgroups x 256 lanes x 2 items x 2 doubles = 2^20 elements) and the first past one of the writing pass (4096 workgroups: 2^22
# elements), which is also past the non-temporal threshold.  n = 1 does not exist: bk_problem_create refuses an axis shorter than 2.
SH1D_N = [2, 3, 127, 128, 4099, 4100, 65537, (1 << 20) + 1031, (1 << 22) + 1031]
SH_DIMS = [(2, 2), (3, 3), (127, 3), (64, 2), (4099, 3), (1025, 1025)]
CASES = [("sh1d", (n,), off) for n in SH1D_N for off in (0, 1) if off == 0 or n in (3, 4099, 4100)] + \
        [("sh", d, off) for d in SH_DIMS for off in (0, 1) if off == 0 or d == (4099, 3)]


def _problem(hip, ctx, kind, dims):
    if kind == "sh":
        return hip.SwiftHohenberg(ctx, dims, (np.pi,) * len(dims), l=-0.25, nu=NU)
    return hip.SwiftHohenberg1D(ctx, dims[0], 6.0, lam=-0.25, nu=NU)


def _guarded(ctx, hip, a, off, fill=None):
    """``a`` on the device between NaN guards: two doubles in front (one more with ``off``: every operand then starts one double
    off a 16-byte boundary) and two behind.  Returns (HipVec on the payload, the whole buffer)."""
    import torch
    n = a.size
    t = torch.full((n + 5,), float("nan"), dtype=torch.float64, device=ctx.torch_device)
    lo = 2 + off
    if fill is None:
        t[lo:lo + n] = torch.from_numpy(np.ascontiguousarray(a)).to(ctx.torch_device)
    v = hip.HipVec(ctx, t[lo:lo + n], n)
    assert v.t.data_ptr() % 16 == 8 * off
    return v, t


def _guards_intact(t, n, off):
    h = t.cpu().numpy()
    lo = 2 + off
    return bool(np.isnan(h[:lo]).all() and np.isnan(h[lo + n:]).all())


def _ints(rng, n, lo, hi):
    return rng.integers(lo, hi + 1, size=n).astype(np.float64)


@pytest.mark.parametrize("kind,dims,off", CASES)
def test_cusp_passes_match_exact_sums_on_integer_data(ctx, kind, dims, off):
    """u in -2..2, the vectors in -3..3, nu = 3/2 and b2 = 3/8: every factor, product and partial sum is an integer (or a dyadic
    fraction) below 2^53, so the device sums equal the restatement's bit for bit in any order.  Operands sit between NaN guards,
    the outputs are preset to NaN."""
    codim2, hip = _lib()
    prob = _problem(hip, ctx, kind, dims)
    n = prob.nlocal
    rng = np.random.default_rng(n + off)
    u, v, w, g = _ints(rng, n, -2, 2), _ints(rng, n, -3, 3), _ints(rng, n, -3, 3), _ints(rng, n, -3, 3)
    (U, tu), (V, tv), (W, tw), (G, tg) = (_guarded(ctx, hip, a, off) for a in (u, v, w, g))
    pars = [-0.25, NU]
    arr = (C.c_double * 2)(*pars)
    ptr = lambda x: C.c_void_p(x.t.data_ptr())
    out4 = (C.c_double * 4)(*[math.nan] * 4)
    ctx.check(ctx.lib.bk_cusp_dots(prob.h, ptr(U), arr, 2, ptr(V), ptr(W), out4), "bk_cusp_dots")
    assert np.array_equal(np.array(list(out4)), Cr.cusp_dots(kind, NU, u, v, w)), (list(out4), Cr.cusp_dots(kind, NU, u, v, w))
    out4 = (C.c_double * 4)(*[math.nan] * 4)
    ctx.check(ctx.lib.bk_cusp_dots(prob.h, ptr(U), arr, 2, ptr(V), ptr(V), out4), "bk_cusp_dots")        # p is q itself
    assert np.array_equal(np.array(list(out4)), Cr.cusp_dots(kind, NU, u, v, v))
    out2 = (C.c_double * 2)(math.nan, math.nan)
    ctx.check(ctx.lib.bk_cusp_contract(prob.h, ptr(U), arr, 2, ptr(V), ptr(W), ptr(G), out2), "bk_cusp_contract")
    assert np.array_equal(np.array(list(out2)), Cr.cusp_contract(kind, NU, u, v, w, g))
    O, to = _guarded(ctx, hip, u, off, fill="nan")
    ctx.check(ctx.lib.bk_cusp_rhs(prob.h, ptr(U), arr, 2, ptr(V), 0.375, ptr(O)), "bk_cusp_rhs")
    assert np.array_equal(O.numpy(), Cr.cusp_rhs(kind, NU, u, v, 0.375))
    assert all(_guards_intact(t, n, off) for t in (tu, tv, tw, tg, to))
    # the wrappers of the package return the same numbers
    if off == 0 and n <= 4100:
        assert np.array_equal(np.array(codim2.cusp_dots(prob, U, pars, V, W)), Cr.cusp_dots(kind, NU, u, v, w))
        assert np.array_equal(np.array(codim2.cusp_contract(prob, U, pars, V, W, G)), Cr.cusp_contract(kind, NU, u, v, w, g))
        assert np.array_equal(codim2.cusp_rhs(prob, U, pars, V, 0.375).numpy(), Cr.cusp_rhs(kind, NU, u, v, 0.375))


@pytest.mark.parametrize("kind,dims", [("sh1d", (4099,)), ("sh", (127, 33))])
def test_cusp_passes_on_random_reals(ctx, kind, dims):
    """Reductions within 1e-12 of the sum of |terms|; the written vector within one ulp of the same expression in NumPy (the
    bound of fold.d2F_ulps: every product and the difference are rounded on their own on both sides)."""
    codim2, hip = _lib()
    prob = _problem(hip, ctx, kind, dims)
    n = prob.nlocal
    rng = np.random.default_rng(17)
    u, v, w, g = (rng.standard_normal(n) for _ in range(4))
    U, V, W, G = (prob.vec(a) for a in (u, v, w, g))
    pars = [-0.25, 1.3]
    d = np.array(codim2.cusp_dots(prob, U, pars, V, W))
    ref, scale = Cr.cusp_dots(kind, 1.3, u, v, w), Cr.cusp_dots_abs(kind, 1.3, u, v, w)
    for k in range(4):
        probe(f"cusp.dots_rel.{kind}.{k}", abs(d[k] - ref[k]) / scale[k], 1e-12)
    c = np.array(codim2.cusp_contract(prob, U, pars, V, W, G))
    ref, scale = Cr.cusp_contract(kind, 1.3, u, v, w, g), Cr.cusp_contract_abs(kind, 1.3, u, v, w, g)
    for k in range(2):
        probe(f"cusp.contract_rel.{kind}.{k}", abs(c[k] - ref[k]) / scale[k], 1e-12)
    r = codim2.cusp_rhs(prob, U, pars, V, 0.7).numpy()
    probe(f"cusp.rhs_ulps.{kind}", _ulps(r, Cr.cusp_rhs(kind, 1.3, u, v, 0.7)).max(), 1.0, tight=0.0)
    probe(f"cusp.b2_host.{kind}", abs(codim2.cusp_b2(prob, U, pars, V, W) - d[0] / (math.sqrt(d[1]) * d[3])), 0.0)


# ------------------------------------------------------------------------------------------ the normal form at the SH cusp
@pytest.fixture(scope="module")
def fixture():
    d = np.load(os.path.join(os.path.dirname(__file__), "golden", "sh_cusp_128x2.npz"))
    dims, ls = tuple(int(k) for k in d["dims"]), tuple(float(x) for x in d["ls"])
    return d, dims, ls, operators.SwiftHohenberg(dims, ls)


def _device(hip, dims, ls, l, nu, maxiter=200):
    """A fresh context with the problem, Pl = lu(L1 + I) (examples/SH2d-fronts.jl:121) and the solver of the fold tests."""
    c = hip.Context(0)
    prob = hip.SwiftHohenberg(c, dims, ls, l=l, nu=nu)
    return c, prob, hip.GMRESKrylovKit(dim=40, rtol=1e-10, atol=1e-13, maxiter=maxiter, Pl=hip.DCTPreconditioner(prob, 1.0))


@pytest.mark.parametrize("flavor", ["bordering", "matrixfree_pl"])
def test_cusp_normal_form_at_the_sh_cusp(fixture, flavor):
    """bk_cusp_normal_form and its call-by-call mirror, each on a fresh context (the GMRES solves carry state from one solve to the
    next), at the stored cusp state against the dense normal form.  The bordered system [J q; q' 0] has the spectrum of J with the
    kernel removed: its smallest |eigenvalue| is the gap 0.049, so a solve to the relative residual rtol = 1e-10 leaves H2 within
    rtol |rhs| / gap of the dense one (the preconditioned residual bounds the true one: |Pl| <= 1), and c = (<p, C(q, q, q)> +
    3 <p, B(q, H2)>) / 6 within max|h| max|q| / 2 of that."""
    codim2, hip = _lib()
    d, dims, ls, op = fixture
    lc, nuc, u, q = float(d["cusp_l"]), float(d["cusp_nu"]), d["cusp_u"], d["cusp_q"]
    gap = float(d["cusp_eig"][1])
    assert 0.04 <= gap <= 0.06
    rhs = Cr.cusp_rhs("sh", nuc, u, q, float(d["cusp_b2"]))
    h = R.horner(R.sh_polys("sh", nuc, 0)[0], u)
    bound_H2 = 1e-10 * np.linalg.norm(rhs) / gap
    bound_c = 0.5 * np.abs(h).max() * np.abs(q).max() * bound_H2
    out = {}
    for name, fn in (("native", codim2.cusp_normal_form_native), ("mirror", codim2.cusp_normal_form)):
        c, prob, lsv = _device(hip, dims, ls, lc, nuc)
        bls = hip.MatrixFreeBLS(lsv, use_pl=True) if flavor == "matrixfree_pl" else hip.BorderingBLS(lsv, check_precision=False)
        Q = prob.vec(q)
        cu = fn(prob, prob.vec(u), [lc, nuc], Q, Q, lsv, bls, lens2="nu")
        out[name] = dict(c=cu.nf.c, b2=cu.b2, H2=cu.H2.numpy(), cv=cu.converged, it=cu.itlinear, bad=cu.unconverged_solves)
        assert cu.lens == ("l", "nu") and cu.params == [lc, nuc]
        if name == "native":
            # fold_bordered was put back, and the counter agrees with the flag
            assert c.get_option("cusp_unconverged_solves") == (0.0 if cu.converged else 1.0) == float(cu.unconverged_solves)
            if flavor == "matrixfree_pl":
                assert c.get_option("fold_bordered") == 0.0
        c.close()
    n_, m_ = out["native"], out["mirror"]
    print(f"cusp normal form ({flavor}): c native {n_['c']:.10f} mirror {m_['c']:.10f} dense {float(d['cusp_c']):.10f}; b2 {n_['b2']:.3e}; "
          f"itlinear {n_['it']} / {m_['it']}; converged {n_['cv']} / {m_['cv']}")
    if flavor == "matrixfree_pl":
        assert n_["cv"] and m_["cv"]                            # the bordered system is regular at the cusp
    assert n_["cv"] == m_["cv"]
    probe(f"cusp.nf.b2_vs_dense.{flavor}", abs(n_["b2"] - float(d["cusp_b2"])), 4 * u.size * EPS * np.abs(h * q ** 3).sum())
    probe(f"cusp.nf.H2_vs_dense.{flavor}", np.linalg.norm(n_["H2"] - d["cusp_H2"]), bound_H2)
    probe(f"cusp.nf.c_vs_dense.{flavor}", abs(n_["c"] - float(d["cusp_c"])), bound_c)
    probe(f"cusp.nf.mirror_c_vs_dense.{flavor}", abs(m_["c"] - float(d["cusp_c"])), bound_c)
    # native against mirror: the same solves on right-hand sides that differ in their last bits (b2 summed in another order), so
    # what separates them is rounding, eps |J| with |J| <= (1 + 8 / h^2)^2 on this grid, amplified by 1 / gap -- an order of
    # magnitude below the solver tolerance
    hx = 2 * ls[0] / dims[0]
    amp = EPS * (1 + 8 / hx ** 2) ** 2 / gap
    bound_nm = amp * np.abs(d["cusp_H2"]).max()                                        # largest entry
    bound_nm_c = 0.5 * np.abs(h).max() * np.abs(q).max() * amp * np.linalg.norm(d["cusp_H2"])      # through the 2-norm, as bound_c
    assert bound_nm <= 0.2 * bound_H2 and bound_nm_c <= 0.6 * bound_c
    probe(f"cusp.nf.native_vs_mirror_H2.{flavor}", np.abs(n_["H2"] - m_["H2"]).max(), bound_nm)
    probe(f"cusp.nf.native_vs_mirror_c.{flavor}", abs(n_["c"] - m_["c"]), bound_nm_c)
    probe(f"cusp.nf.native_vs_mirror_itlinear.{flavor}", abs(sum(n_["it"]) - sum(m_["it"])), 2)


# ------------------------------------------------------------------------------------------ detection and bisection on the curve
TOL, DSMIN_B = 1e-9, 1e-4


def _curve(codim2, hip, fixture, detect, spy=None):
    """continuation_fold in nu from the stored fold point with the stored steps, on a fresh context."""
    from bk_amd import continuation as Cn
    d, dims, ls, _ = fixture
    l0, nu0 = float(d["fold_l"]), float(d["fold_nu"])
    dss = [float(x) for x in d["ds_sequence"]]
    c, prob, lsv = _device(hip, dims, ls, l0, nu0)
    if spy is not None:
        c.lib = spy(c.lib)
    V = prob.vec(d["fold_v"])
    cp = Cn.ContinuationPar(ds=dss[0], dsmin=1e-4, dsmax=0.05, p_min=float(d["p_min"]), p_max=float(d["p_max"]), max_steps=len(dss),
                            n_inversion=8, max_bisection_steps=25, dsmin_bisection=DSMIN_B,
                            newton_options=Cn.NewtonPar(tol=TOL, max_iterations=int(d["max_iterations"])))
    br = codim2.continuation_fold(prob, hip.BorderedArray(prob.vec(d["fold_u"]), l0), nu0, "nu", V, V, lsv, cp, ds_sequence=dss,
                                  bls=hip.MatrixFreeBLS(lsv, use_pl=True), detect_codim2=detect)
    return c, prob, lsv, br


@pytest.fixture(scope="module")
def restated(fixture):
    d, _, _, op = fixture
    m = Cr.sh_cusp_model(op, "sh", dict(l=float(d["fold_l"]), nu=float(d["fold_nu"])), "l", "nu")
    dss = [float(x) for x in d["ds_sequence"]]
    return m, Cr.continuation_fold(m, d["fold_u"], float(d["fold_l"]), float(d["fold_nu"]), d["fold_v"], d["fold_v"], ds=dss[0],
                                   ds_sequence=dss, max_steps=len(dss), p_min=float(d["p_min"]), p_max=float(d["p_max"]),
                                   max_iterations=int(d["max_iterations"]), tol=TOL, detect_codim2=2, n_inversion=8,
                                   max_bisection_steps=25, dsmin_bisection=DSMIN_B)


def test_continuation_fold_locates_the_sh_cusp(fixture, restated):
    """detect_codim2 = 2 from the stored fold point: one "cusp", CP and b2 of opposite sign on its two sides, the located (l, nu)
    against the restatement run with the same steps and options, against the dense cusp, and its normal form.

    Reach of the bisection.  It ends within 3 ``reach`` of the crossing along the curve (reach = the ds of the last step that
    passed it; the secant event sees a crossing one step late, so it lies in that step or in the second half of the twice as long
    one before), and along that stretch |d nu / ds| is at most the larger |CP| of the two end states (CP = d nu / ds in the PALC
    arclength, monotone through the extremum).  So |nu - nu_cusp| <= 3 reach max|CP_interval|, and |l - l_cusp| is that times
    the slope |dl / dnu| of the fold curve, taken from the stored curve points.  The figures come from the restatement."""
    codim2, hip = _lib()
    d, dims, ls, op = fixture
    m, rr = restated
    c, prob, lsv, br = _curve(codim2, hip, fixture, 2)
    print("fold curve: l", br.p1, "nu", br.p2, "CP", br.CP, "b2", br.b2, "itnewton", br.itnewton, "itlinear", br.itlinear)
    assert [s["type"] for s in br.specialpoint] == ["cusp"] and [s["type"] for s in rr["specialpoint"]] == ["cusp"]
    sp, sr = br.specialpoint[0], rr["specialpoint"][0]
    print("located:", {k: v for k, v in sp.items() if k not in ("x", "a", "b")})
    print("restated:", {k: v for k, v in sr.items() if k not in ("X", "a", "b")})
    i = sp["idx"]
    assert i == sr["idx"] == len(br.p2) - 1 and sp["status"] == sr["status"] != "guess"
    assert (sp["bisection_steps"], sp["n_inversion"]) == (sr["bisection_steps"], sr["n_inversion"]) and sp["n_inversion"] >= 1
    assert sp["CP_interval"][0] * sp["CP_interval"][1] < 0 and br.CP[i - 1] * br.CP[i] < 0
    assert br.b2[i - 2] * br.b2[i] < 0                        # b2 changes sign within the bracket the bisection was handed
    probe("cusp.curve_vs_restatement_p1", max(abs(a - b) for a, b in zip(br.p1, rr["p1"])), 1e-8)
    probe("cusp.curve_vs_restatement_p2", max(abs(a - b) for a, b in zip(br.p2, rr["p2"])), 1e-8)
    probe("cusp.curve_vs_restatement_b2", max(abs(a - b) for a, b in zip(br.b2, rr["b2"])), 1e-6)
    probe("cusp.located_vs_restatement_l", abs(sp["p1"] - sr["p1"]), 1e-8)
    probe("cusp.located_vs_restatement_nu", abs(sp["p2"] - sr["p2"]), 1e-8)
    for e_, f_ in zip(sp["end_points"], sr["end_points"]):
        probe("cusp.end_points_vs_restatement", max(abs(e_[0] - f_[0]), abs(e_[1] - f_[1])), 1e-8)
    assert sp["reach"] == sr["reach"]
    slope = np.abs(np.diff(d["curve_l"][:-1]) / np.diff(d["curve_nu"][:-1])).max()
    bound_nu = 3 * sr["reach"] * max(abs(x) for x in sr["CP_interval"])
    probe("cusp.located_vs_dense_nu", abs(sp["p2"] - float(d["cusp_nu"])), bound_nu)
    probe("cusp.located_vs_dense_l", abs(sp["p1"] - float(d["cusp_l"])), slope * bound_nu)
    # the normal form at the refined fold point of the located nu
    cu = codim2.get_normal_form(br, 0, prob, lsv, tol=TOL, max_iterations=10, norm_inf=True, bls=hip.MatrixFreeBLS(lsv, use_pl=True))
    assert isinstance(cu, codim2.Cusp) and cu.lens == ("l", "nu") and cu.converged
    assert abs(cu.params[1] - sp["p2"]) == 0.0
    # against the dense normal form at the state the device refined: H2 to rtol |rhs| / gap as in
    # test_cusp_normal_form_at_the_sh_cusp; the null vector comes from a solve of the same tolerance and enters c through five
    # factors, so ten times the bound of c there
    xr, qr = cu.x0.numpy(), cu.zeta.numpy()
    pars = m.at(cu.params[0], cu.params[1])
    qd, pd = Cr.null_vectors(m.J(xr, pars))
    sgn = 1.0 if qd @ qr > 0 else -1.0                         # b2 is odd in q: the dense null vector in the device's orientation
    nf = Cr.cusp_normal_form(m, xr, pars, sgn * qd, sgn * pd)
    gap = float(d["cusp_eig"][1])
    h = R.horner(R.sh_polys("sh", cu.params[1], 0)[0], xr)
    bound_c = 10 * 0.5 * np.abs(h).max() * np.abs(qr).max() * 1e-10 * np.linalg.norm(Cr.cusp_rhs("sh", cu.params[1], xr, qr, nf["b2"])) / gap
    print(f"get_normal_form: l {cu.params[0]:.10f} nu {cu.params[1]:.10f} c {cu.nf.c:.8f} b2 {cu.b2:.3e} (dense at that state: c "
          f"{nf['c']:.8f} b2 {nf['b2']:.3e}; dense cusp c {float(d['cusp_c']):.8f}); itlinear {cu.itlinear}")
    assert np.abs(op.F(xr, cu.params[0], cu.params[1])).max() <= 10 * TOL
    probe("cusp.get_normal_form_c_vs_dense", abs(cu.nf.c - nf["c"]), bound_c)
    probe("cusp.get_normal_form_b2_vs_dense", abs(cu.b2 - nf["b2"]), 10 * 1e-10 / gap * np.abs(h).max())
    assert abs(cu.b2) <= 0.1 * min(abs(br.b2[i - 2]), abs(br.b2[i])), (cu.b2, br.b2)
    assert prob.params["nu"] == float(d["fold_nu"])           # the problem's own parameters were put back
    c.close()


def test_detect_codim2_records_and_calls(fixture):
    """detect_codim2 = 0 issues the library calls of the plain curve -- no bk_cusp_* call, no solver_state_hold -- and
    detect_codim2 = 1 the same calls plus one bk_cusp_dots per point inside a held solver state: the same points, CP, Newton and
    GMRES counts, plus b2 and a "guess"."""
    codim2, hip = _lib()
    logs = []

    def spy():
        calls = []
        logs.append(calls)

        class Spy:
            def __init__(self, lib):
                self._lib = lib

            def __getattr__(self, name):
                if name.startswith("bk_"):
                    calls.append(name)
                return getattr(self._lib, name)
        return Spy

    out = []
    for detect in (0, 1):
        c, prob, lsv, br = _curve(codim2, hip, fixture, detect, spy())
        out.append(br)
        c.close()
    b0, b1 = out
    assert not [n for n in logs[0] if n.startswith("bk_cusp")]
    extra = [n for n in logs[1] if n == "bk_cusp_dots"]
    assert len(extra) == len(b1.p2)
    # everything that computes -- residuals, Jacobians, bordered vectors, linear solves -- in the same order; what detection adds
    # are the b2 passes, the hold, and the copy of the state the special point keeps
    work = ("bk_residual", "bk_jacobian", "bk_op_", "bk_fold_", "bk_gmres", "bk_bls_", "bk_newton", "bk_palc", "bk_precond", "bk_d2f",
            "bk_djdp", "bk_d3f", "bk_nf1d")
    plain = lambda log: [n for n in log if n.startswith(work) and not n.endswith("_destroy")]      # destructors run when collected
    assert len(plain(logs[0])) > 20 and plain(logs[0]) == plain(logs[1])
    assert logs[1].count("bk_ctx_set_option") - logs[0].count("bk_ctx_set_option") == 2 * len(b1.p2)      # the hold, on and off
    for k in ("p1", "p2", "CP", "BT", "itnewton", "itlinear", "residuals"):
        assert getattr(b0, k) == getattr(b1, k), k
    assert b0.b2 == [] and b0.specialpoint == [] and len(b1.b2) == len(b1.p2)
    assert [(s["type"], s["status"], s["bisection_steps"]) for s in b1.specialpoint] == [("cusp", "guess", 0)]
    s = b1.specialpoint[0]
    assert s["idx"] == len(b1.p2) - 1 and s["b2"] == b1.b2[-1] and s["CP_interval"] == (b1.CP[-2], b1.CP[-1])
    assert s["end_points"] == ((b1.p1[-2], b1.p2[-2]), (b1.p1[-1], b1.p2[-1]))


# ------------------------------------------------------------------------------------------ error paths
def test_cusp_error_paths(ctx, fixture):
    codim2, hip = _lib()
    from bk_amd import _lib as L
    from bk_amd import continuation as Cn
    cgl = hip.CGL2d(ctx, (8, 8), (1.0, 1.0))
    x = cgl.vec(np.zeros(cgl.nglobal))
    pv = cgl._pvec(0.5)
    with pytest.raises(L.BkHipError, match="fold formulation"):
        codim2.cusp_dots(cgl, x, pv, x, x)
    with pytest.raises(L.BkHipError, match="fold formulation"):
        codim2.cusp_rhs(cgl, x, pv, x, 0.5)
    with pytest.raises(L.BkHipError, match="fold formulation"):
        codim2.cusp_contract(cgl, x, pv, x, x, x)
    d, dims, ls, _ = fixture
    prob = hip.SwiftHohenberg(ctx, dims, ls, l=float(d["cusp_l"]), nu=float(d["cusp_nu"]))
    lsv = hip.GMRESKrylovKit(dim=40, rtol=1e-10, atol=1e-13, maxiter=50, Pl=hip.DCTPreconditioner(prob, 1.0))
    with pytest.raises(L.BkHipError, match="fold formulation"):
        codim2.cusp_normal_form_native(cgl, x, pv, x, x, lsv)
    pars = [float(d["cusp_l"]), float(d["cusp_nu"])]
    U, Q = prob.vec(d["cusp_u"]), prob.vec(d["cusp_q"])
    Q2 = prob.vec(d["cusp_q"] * (1 + 1e-7))                   # <q, p> - 1 = 1e-7 > 1e-8
    with pytest.raises(L.BkHipError, match="normalization"):
        codim2.cusp_normal_form_native(prob, U, pars, Q, Q2, lsv)
    with pytest.raises(ValueError, match="normalization"):
        codim2.cusp_normal_form(prob, U, pars, Q, Q2, lsv)
    with pytest.raises(L.BkHipError, match="alias"):
        ctx.check(ctx.lib.bk_cusp_rhs(prob.h, C.c_void_p(U.t.data_ptr()), (C.c_double * 2)(*pars), 2, C.c_void_p(Q.t.data_ptr()), 0.5,
                                      C.c_void_p(Q.t.data_ptr())), "bk_cusp_rhs")
    cp = Cn.ContinuationPar(ds=-0.01, dsmax=0.05, p_min=1.0, p_max=2.5, max_steps=2)
    with pytest.raises(ValueError, match="update_minaug_every_step"):
        codim2.continuation_fold(prob, hip.BorderedArray(U, pars[0]), pars[1], "nu", Q, Q, lsv, cp, update_minaug_every_step=0,
                                 detect_codim2=1)
    with pytest.raises(L.BkHipError, match="axis"):
        hip.SwiftHohenberg1D(ctx, 1, 6.0)
