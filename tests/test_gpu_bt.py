"""GPU tests of the Bogdanov-Takens machinery (csrc/bt.hip: bk_bt_border, bk_bt_terms, bk_bt_linsolve, bk_newton_bt, bk_bt_nf_dots,
bk_bt_nf_rhs, bk_bt_nf_k2, bk_bt_normal_form; bk_amd.codim2): the fused passes against the pointwise restatement in extended
precision, the bordered solves against sparse LU, newton_bt -- native against the call-by-call mirror and the CPU restatement --
from the point where the example's Hopf curve stops and from the Hopf point before it, the normal form at the refined point, the
"bt" special point end to end, and the Hopf curve restarted from the Bogdanov-Takens point through its predictor.

The yardsticks (points, coefficients, sparse LU next to SciPy GMRES under the same preconditioner and tolerance, iteration counts)
are tests/golden/bt_cgl.json, which tests/test_bt_reference.py certifies on the CPU."""
import json
import math
import os

import numpy as np
import pytest
import torch

import bt_ref as BT
import minaug_hopf_ref as R
from conftest import probe
from oracle import operators

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
LD = np.longdouble
LS, PARS, LENSES = BT.CGL_LS, BT.CGL_PARS, BT.CGL_LENSES
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bt_cgl.json")) as _f:
    GOLD = json.load(_f)
GRIDS = {"8x6": (8, 6), "12x9": (12, 9)}


def _lib():
    from bk_amd import codim2, hip
    return codim2, hip


def _pv(pars):
    return [pars[k] for k in R.CGL_PARAMS]


def _vec_at(ctx, hip, x, offset):
    """x on the device, starting `offset` doubles into its allocation (offset 1: every 16-B vector access is misaligned)."""
    t = torch.empty(len(x) + offset, dtype=torch.float64, device=ctx.torch_device)
    v = t[offset:]
    v.copy_(torch.from_numpy(np.asarray(x, dtype=np.float64)))
    return hip.HipVec(ctx, v)


# ------------------------------------------------------------------------------------------ the pointwise restatement
def _hess_abs(u1, u2, q):
    """cgl_hessians with every monomial taken with a plus sign."""
    u1, u2, mu, c3, c5 = np.abs(u1), np.abs(u2), abs(q["mu"]), abs(q["c3"]), abs(q["c5"])
    ua = u1 * u1 + u2 * u2
    q1, q2 = u1 * (8.0 * u1 * u1 + 12.0 * ua), u2 * (8.0 * u1 * u1 + 4.0 * ua)
    q3, q4 = u1 * (8.0 * u2 * u2 + 4.0 * ua), u2 * (8.0 * u2 * u2 + 12.0 * ua)
    return (6 * c3 * u1 + 2 * mu * u2 + c5 * q1, 2 * c3 * u2 + 2 * mu * u1 + c5 * q2, 2 * c3 * u1 + 6 * mu * u2 + c5 * q3,
            2 * c3 * u2 + 6 * mu * u1 + c5 * q2, 2 * c3 * u1 + 2 * mu * u2 + c5 * q3, 6 * c3 * u2 + 2 * mu * u1 + c5 * q4)


class _Pointwise:
    """B(u)[v, .]' w, B(u)[x, y] and D_k v per grid point on the stacked fields, in the precision of the arrays handed in;
    ``absolute``: the sums of the moduli of the monomials (every argument and coefficient by its modulus)."""

    def __init__(self, u, q, absolute=False):
        self.n = len(u) // 2
        self.absolute = absolute
        self.u1, self.u2 = u[:self.n], u[self.n:]
        self.h = _hess_abs(self.u1, self.u2, q) if absolute else R.cgl_hessians(self.u1, self.u2, q["mu"], q["c3"], q["c5"])

    def _a(self, v):
        return np.abs(v) if self.absolute else v

    def adj(self, v, w):
        n, h = self.n, self.h
        va, vb, wa, wb = self._a(v[:n]), self._a(v[n:]), self._a(w[:n]), self._a(w[n:])
        return np.concatenate([wa * (h[0] * va + h[1] * vb) + wb * (h[3] * va + h[4] * vb),
                               wa * (h[1] * va + h[2] * vb) + wb * (h[4] * va + h[5] * vb)])

    def B(self, x, y):
        n, h = self.n, self.h
        a1, a2, b1, b2 = self._a(x[:n]), self._a(x[n:]), self._a(y[:n]), self._a(y[n:])
        return np.concatenate([a1 * (h[0] * b1 + h[1] * b2) + a2 * (h[1] * b1 + h[2] * b2),
                               a1 * (h[3] * b1 + h[4] * b2) + a2 * (h[4] * b1 + h[5] * b2)])

    def D(self, ipar, v):
        n = self.n
        d = R.cgl_djdp(ipar, np.abs(self.u1) if self.absolute else self.u1, np.abs(self.u2) if self.absolute else self.u2)
        if self.absolute:
            d = [np.abs(x) for x in d]
        va, vb = self._a(v[:n]), self._a(v[n:])
        return np.concatenate([d[0] * va + d[1] * vb, d[2] * va + d[3] * vb])


def _sum_check(name, n, got, terms):
    bound = 4 * n * EPS * np.abs(terms).sum() + 1e-300
    probe(name, abs(got - math.fsum(terms)) / bound, 1.0)


LENS_PAIRS = (("r", "gamma"), ("r", "c3"), ("c3", "c5"))


# ------------------------------------------------------------------------------------------ 1: BtBorder
@pytest.mark.parametrize("dims, offset", [((24, 16), 0), ((24, 16), 1), ((23, 17), 0), ((64, 41), 0)])
def test_bt_border_matches_the_restatement(ctx, dims, offset):
    """bk_bt_border on random u, v, w against the pointwise restatement in extended precision, s = +-1 and the lens pairs (r, gamma)
    (a zero D), (r, c3) and (c3, c5) (state-dependent D).  Rows in units of eps * (sum of the moduli of the monomials): a Hessian
    entry carries at most 8 roundings, H v two more, w . (H v) two, the sum of the two products of row2 one: 13, i.e. 6.5 units; the
    bound is the 16 of the sibling passes.  Sums within 4 n eps sum |terms|.  (23, 17): an odd point count (misaligned second field,
    odd tail); (64, 41): more than one workgroup with a partial last one; offset 1: every pointer misaligned."""
    codim2, hip = _lib()
    rng = np.random.default_rng(7 + offset + dims[0])
    pars = dict(PARS, r=0.3, gamma=0.2)
    prob = hip.CGL2d(ctx, dims, LS, **pars)
    n = prob.nlocal
    u = 0.6 * rng.standard_normal(n)
    v1, v2, w1, w2 = (rng.standard_normal(n) for _ in range(4))
    dev = lambda x: _vec_at(ctx, hip, x, offset)
    U, V1, V2, W1, W2 = dev(u), dev(v1), dev(v2), dev(w1), dev(w2)
    ext = _Pointwise(u.astype(LD), pars)
    mod = _Pointwise(u, pars, absolute=True)
    dbl = _Pointwise(u, pars)
    xl = lambda x: x.astype(LD)
    ref1 = ext.adj(xl(v1), xl(w1))
    ref2 = ext.adj(xl(v1), xl(w2)) + ext.adj(xl(v2), xl(w1))
    unit1 = mod.adj(v1, w1)
    unit2 = mod.adj(v1, w2) + mod.adj(v2, w1)
    tag = f"{dims[0]}x{dims[1]}+{offset}"
    for l1, l2 in LENS_PAIRS:
        i1, i2 = R.CGL_PARAMS.index(l1), R.CGL_PARAMS.index(l2)
        for s in (-1.0, 1.0):
            r1, r2, blk = codim2.bt_border(prob, U, _pv(pars), i1, i2, s, V1, V2, W1, W2)
            probe(f"bt.border_row1_ulps.{tag}.{l1}{l2}", float((np.abs(r1.numpy() - s * ref1) / (EPS * unit1)).max()), 16.0, tight=4.0)
            probe(f"bt.border_row2_ulps.{tag}.{l1}{l2}", float((np.abs(r2.numpy() - s * ref2) / (EPS * unit2)).max()), 16.0, tight=4.0)
            for k, ip in enumerate((i1, i2)):
                t1 = s * w1 * dbl.D(ip, v1)
                t2 = s * np.concatenate([w2 * dbl.D(ip, v1), w1 * dbl.D(ip, v2)])
                _sum_check(f"bt.border_sum1.{tag}.{l1}{l2}.{k}", n, blk[0, k], t1)
                _sum_check(f"bt.border_sum2.{tag}.{l1}{l2}.{k}", n, blk[1, k], t2)
            if l2 == "gamma":
                assert blk[0, 1] == 0.0 and blk[1, 1] == 0.0            # dJ/dgamma = 0 exactly


def test_bt_border_misaligned_operands_give_the_same_bits(ctx):
    """Every operand one double into its allocation: the rows AND the four sums carry the same bits as with aligned operands (the
    pass walks pairs of elements in one order on both load paths), at a size with several workgroups and a ragged end."""
    codim2, hip = _lib()
    rng = np.random.default_rng(11)
    pars = dict(PARS, r=0.3, gamma=0.2)
    dims = (64, 41)
    prob = hip.CGL2d(ctx, dims, LS, **pars)
    n = prob.nlocal
    xs = [0.6 * rng.standard_normal(n)] + [rng.standard_normal(n) for _ in range(4)]
    out = []
    for offset in (0, 1):
        D = [_vec_at(ctx, hip, x, offset) for x in xs]
        assert all(d.t.data_ptr() % 16 == 8 * offset for d in D)
        r1, r2, blk = codim2.bt_border(prob, D[0], _pv(pars), 3, 4, -1.0, *D[1:])
        out.append((r1.numpy(), r2.numpy(), blk))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert [float(v).hex() for v in out[0][2].ravel()] == [float(v).hex() for v in out[1][2].ravel()], (out[0][2], out[1][2])
    again = codim2.bt_border(prob, D[0], _pv(pars), 3, 4, -1.0, *D[1:])[2]
    assert np.array_equal(again, out[1][2])                              # and run to run


def test_bt_border_refuses_aliased_outputs(ctx):
    codim2, hip = _lib()
    from bk_amd import _lib as L
    import ctypes as C
    prob = hip.CGL2d(ctx, (8, 6), LS, **PARS)
    n = prob.nlocal
    vs = [prob.vec(np.full(n, 0.1 * (k + 1))) for k in range(7)]
    p = lambda v: C.c_void_p(v.t.data_ptr())
    pv = (C.c_double * 6)(*_pv(PARS))
    out = (C.c_double * 4)()
    for r1, r2 in ((vs[1], vs[6]), (vs[5], vs[0]), (vs[5], vs[4]), (vs[5], vs[5])):
        st = ctx.lib.bk_bt_border(prob.h, p(vs[0]), pv, 6, 0, 5, -1.0, p(vs[1]), p(vs[2]), p(vs[3]), p(vs[4]), p(r1), p(r2), out)
        assert st != 0
        msg = ctx.lib.bk_last_error(ctx.h).decode()
        assert "alias" in msg or "distinct" in msg, msg
    with pytest.raises(L.BkHipError, match="must differ"):
        codim2.bt_border(prob, vs[0], _pv(PARS), 0, 0, -1.0, *vs[1:5])


# ------------------------------------------------------------------------------------------ 2: the normal-form passes
@pytest.mark.parametrize("dims, offset", [((24, 16), 0), ((24, 16), 1), ((23, 17), 0), ((64, 41), 0)])
def test_bt_nf_passes_match_the_restatement(ctx, dims, offset):
    """bk_bt_nf_dots, bk_bt_nf_rhs (both modes) and bk_bt_nf_k2 against the same restatement under the same bounds: sums within
    4 n eps sum |terms|, written vectors within 16 units of eps * (sum of the moduli of the monomials) (Hessian entry 8, H q0 two,
    q . (H q0) two, k q1 one, + H one, the subtraction one: 15, i.e. 7.5 units)."""
    codim2, hip = _lib()
    rng = np.random.default_rng(23 + offset + dims[0])
    pars = dict(PARS, r=0.3, gamma=0.2)
    prob = hip.CGL2d(ctx, dims, LS, **pars)
    n = prob.nlocal
    u = 0.6 * rng.standard_normal(n)
    q0, q1, p0, p1, H = (rng.standard_normal(n) for _ in range(5))
    dev = lambda x: _vec_at(ctx, hip, x, offset)
    U, Q0, Q1, P0, P1, HH = dev(u), dev(q0), dev(q1), dev(p0), dev(p1), dev(H)
    ext, mod, dbl = _Pointwise(u.astype(LD), pars), _Pointwise(u, pars, absolute=True), _Pointwise(u, pars)
    xl = lambda x: x.astype(LD)
    tag = f"{dims[0]}x{dims[1]}+{offset}"
    d = codim2.bt_nf_dots(prob, U, _pv(pars), Q0, Q1, P0, P1)
    B00, B01, B11 = dbl.B(q0, q0), dbl.B(q0, q1), dbl.B(q1, q1)
    for k, (p, Bq) in enumerate(((p1, B00), (p0, B00), (p1, B01), (p0, B01), (p1, B11), (p0, B11))):
        _sum_check(f"bt.nf_dots_{k}.{tag}", n, d[k], p * Bq)
    ka, kb = 0.375, -1.25
    r0 = codim2.bt_nf_rhs(prob, U, _pv(pars), 0, ka, Q0, Q1).numpy()
    ref0 = LD(ka) * xl(q1) - ext.B(xl(q0), xl(q0))
    unit0 = abs(ka) * np.abs(q1) + mod.B(q0, q0)
    probe(f"bt.nf_rhs0_ulps.{tag}", float((np.abs(r0 - ref0) / (EPS * unit0)).max()), 16.0, tight=4.0)
    r1 = codim2.bt_nf_rhs(prob, U, _pv(pars), 1, kb, Q0, Q1, HH).numpy()
    ref1 = LD(kb) * xl(q1) + xl(H) - ext.B(xl(q0), xl(q1))
    unit1 = abs(kb) * np.abs(q1) + np.abs(H) + mod.B(q0, q1)
    probe(f"bt.nf_rhs1_ulps.{tag}", float((np.abs(r1 - ref1) / (EPS * unit1)).max()), 16.0, tight=4.0)
    for l1, l2 in LENS_PAIRS:
        i1, i2 = R.CGL_PARAMS.index(l1), R.CGL_PARAMS.index(l2)
        k = codim2.bt_nf_k2(prob, U, _pv(pars), i1, i2, P1, HH)
        _sum_check(f"bt.nf_k2_B.{tag}.{l1}{l2}", n, k[0], p1 * dbl.B(H, H))
        _sum_check(f"bt.nf_k2_D1.{tag}.{l1}{l2}", n, k[1], p1 * dbl.D(i1, H))
        _sum_check(f"bt.nf_k2_D2.{tag}.{l1}{l2}", n, k[2], p1 * dbl.D(i2, H))


# ------------------------------------------------------------------------------------------ the device setting of a golden grid
class _Case:
    """A golden grid on the device: problem at the parameters of the curve, the solver of the yardstick (GMRESIterativeSolvers with
    the restart and rtol of BT.GMRES, left-preconditioned by the cGL block of the stop point's r) and its adjoint twin."""

    def __init__(self, ctx, key):
        codim2, hip = _lib()
        self.key, self.dims, self.g = key, GRIDS[key], GOLD[key]
        self.op = operators.CGL2d(self.dims, LS)
        self.model = BT.cgl_model(self.op, dict(PARS), *LENSES)
        self.prob = hip.CGL2d(ctx, self.dims, LS, **PARS)
        a0, b0 = self.g["precond"]
        self.ls = hip.GMRESIterativeSolvers(reltol=BT.GMRES["rtol"], restart=BT.GMRES["restart"], maxiter=600,
                                            Pl=hip.CGLBlockPreconditioner(self.prob, a0, b0))
        self.ls_adj = codim2.bt_adjoint_solver(self.prob, self.ls, a0, b0)

    def start(self, name):
        codim2, _ = _lib()
        st = self.g["starts"][name]
        return codim2.BTVec(self.prob.vec(np.array(st["x"])), st["p"])

    def margin(self, diff, value, cond=1.0):
        """10 x max(|LU - GMRES| of the restatement, 8 eps cond |value|)"""
        return 10 * max(float(diff), 8 * EPS * cond * float(np.abs(np.asarray(value)).max()))


_cases = {}


def _case(ctx, key):
    if key not in _cases:
        _cases[key] = _Case(ctx, key)
    return _cases[key]


# ------------------------------------------------------------------------------------------ 3: the bordered solves
def test_bt_terms_match_sparse_lu_at_the_stop_point(ctx):
    """bk_bt_terms at the committed Bogdanov-Takens neighbour state of 12 x 9 (where the Hopf curve stops: J is singular there,
    the bordered systems are not) with the start vectors of the yardstick: v1, v2, w1, w2 against sparse LU within
    10 x max(|SciPy GMRES - LU|, 8 eps |sol|_inf), iteration counts within 4 of SciPy's per solve."""
    codim2, hip = _lib()
    c = _case(ctx, "12x9")
    t, st = c.g["terms"], c.g["starts"]["stop"]
    a, b = np.array(t["a"]), np.array(t["b"])
    x, q = np.array(st["x"]), BT._at(c.model, LENSES, st["p"])
    lu = BT.bordered_vectors(c.model, x, q, a, b)
    X = c.start("stop")
    got = codim2.bt_terms(c.prob, X.u, _pv(q), c.prob.vec(a), c.prob.vec(b), c.ls, c.ls_adj)
    print("bt_terms: iterations", got["itlinear"], "SciPy", t["its"], "sigma", got["sigma"], "LU", lu["sigma"])
    assert all(got["converged"]), got["converged"]
    for k, name in enumerate(("v1", "v2", "w1", "w2")):
        d = float(np.abs(got[name].numpy() - lu[name]).max())
        probe(f"bt.terms_{name}", d, c.margin(t[name]["diff"], t[name]["norminf"]), relative=d / t[name]["norminf"])
        assert abs(got["itlinear"][k] - t["its"][k]) <= 4, (name, got["itlinear"], t["its"])
    for k in range(2):
        assert abs(got["sigma"][k] - lu["sigma"][k]) <= c.margin(max(t["v1"]["diff"], t["v2"]["diff"]), lu["sigma"][k]) + 1e-300
    # the pairs alone give the same bits as both together
    gv = codim2.bt_terms(c.prob, X.u, _pv(q), c.prob.vec(a), c.prob.vec(b), c.ls, None, "v")
    gw = codim2.bt_terms(c.prob, X.u, _pv(q), c.prob.vec(a), c.prob.vec(b), c.ls, c.ls_adj, "w")
    assert torch.equal(gv["v1"].t, got["v1"].t) and torch.equal(gv["v2"].t, got["v2"].t) and gv["sigma"] == got["sigma"]
    assert torch.equal(gw["w1"].t, got["w1"].t) and torch.equal(gw["w2"].t, got["w2"].t)


# ------------------------------------------------------------------------------------------ 4: newton_bt
_refined = {}


def _refine(ctx, key, name):
    """(native, mirror) results of newton_bt from the start ``name`` with the reference's default start vectors, once per session."""
    if (key, name) not in _refined:
        codim2, _ = _lib()
        c = _case(ctx, key)
        X = c.start(name)
        a, b = codim2.bt_start_vectors(c.prob, X, "gamma", c.ls, c.ls_adj, seed=0)
        tol = BT.CGL_CURVE["tol"]
        na = codim2.newton_bt_native(c.prob, X, "gamma", a, b, c.ls, c.ls_adj, tol=tol, max_iterations=10)
        mi = codim2.newton_bt(c.prob, X, "gamma", a, b, c.ls, c.ls_adj, tol=tol, max_iterations=10)
        _refined[key, name] = (na, mi, a, b)
    return _refined[key, name]


@pytest.mark.parametrize("name", ["stop", "before"])
@pytest.mark.parametrize("key", ["8x6", "12x9"])
def test_newton_bt_refines_the_stop_point_to_the_golden_point(ctx, key, name):
    """newton_bt_native and the mirror from the Hopf curve's stop point and from the Hopf point before it: converged within 6
    iterations (the restatement takes 3), the golden (r, gamma) and |x|_inf within 10 x max(|LU - GMRES|, 8 eps |value|), native =
    mirror bit for bit, and the two smallest |eigenvalues| of the dense oracle Jacobian at the device result <= 10 x the
    restatement's from the same start at the same Newton tolerance and <= 1e-5 -- at the stop point itself the second one is 0.022 /
    0.047, so the test fails without the refinement.  The solver tolerance matters here: the double eigenvalue moves like the square root of
    what the last Newton update leaves, the linear solver's error included; with rtol 1e-12 the device left 1.9e-7 ... 5.4e-7 (11.4 x
    the restatement's LU value at 8 x 6 from the Hopf point, at equal Newton residuals), exactly what the restatement leaves with
    SciPy GMRES at that rtol; BT.GMRES therefore carries the 1e-13 of the Hopf tests (the restatement: at most 2.4 x its LU value)."""
    import scipy.linalg as sla
    c = _case(ctx, key)
    na, mi, _, _ = _refine(ctx, key, name)
    lu, gd = c.g["lu"][name], c.g["gmres"]["diff"]
    assert c.g["starts"][name]["eig2"][1] >= 0.02 or name == "before"
    for kind, s in (("native", na), ("mirror", mi)):
        print(f"{key} {name} {kind}: p = {s['u'].p}, residuals {s['residuals']}, per solve {s['itsolves']}, unconverged "
              f"{s['unconverged_solves']} (restatement: {lu['p']}, {lu['residuals']}; SciPy per solve {c.g['gmres']['its'][4:13]})")
        assert s["converged"] and s["itnewton"] <= 6 and s["unconverged_solves"] == 0, s["residuals"]
        for j in range(2):
            probe(f"bt.newton_p{j}.{key}.{name}.{kind}", abs(s["u"].p[j] - lu["p"][j]), c.margin(gd["p"], lu["p"][j]))
        xinf = s["u"].u.norminf()
        probe(f"bt.newton_xinf.{key}.{name}.{kind}", abs(xinf - lu["xinf"]), c.margin(gd["xinf"], lu["xinf"]))
    x = na["u"].u.numpy()
    q = BT._at(c.model, LENSES, na["u"].p)
    ev = np.sort(np.abs(sla.eigvals(c.op.J(x, **q).toarray())))[:2]
    print(f"{key} {name}: two smallest |eigenvalues| at the device result {ev}, restatement {lu['eig2']}, at the start "
          f"{c.g['starts'][name]['eig2']}")
    probe(f"bt.newton_eig2.{key}.{name}", float(ev.max()), min(10 * max(lu["eig2"]), 1e-5))
    # native = mirror, bit for bit
    assert na["itnewton"] == mi["itnewton"] and na["residuals"] == mi["residuals"] and na["itsolves"] == mi["itsolves"]
    assert list(na["u"].p) == list(mi["u"].p) and na["sigma"] == tuple(mi["sigma"])
    for k in ("v1", "v2", "w1", "w2"):
        assert torch.equal(na[k].t, mi[k].t), k
    assert torch.equal(na["u"].u.t, mi["u"].u.t)


# ------------------------------------------------------------------------------------------ 5: the normal form
def _oriented(nf):
    """a > 0: under q0 -> -q0 the coefficients a, b, gamma, c and K10 change sign, K11 and K2 do not."""
    if nf["a"] > 0:
        return nf
    out = dict(nf)
    for k in ("a", "b", "gamma", "c", "K10"):
        out[k] = -out[k]
    return out


_records = {}


def _record(ctx, key):
    """(Jordan basis record, native normal form, mirror normal form) at the point newton_bt_native returns from the stop point."""
    if key not in _records:
        codim2, _ = _lib()
        c = _case(ctx, key)
        na, _, a, b = _refine(ctx, key, "stop")
        X = na["u"]
        w1 = codim2.bt_terms(c.prob, X.u, _pv(BT._at(c.model, LENSES, X.p)), a, b, c.ls, c.ls_adj, "w")["w1"]
        bt = codim2.bt_jordan_basis(c.prob, X, "gamma", na["v1"], w1, c.ls, c.ls_adj)
        _records[key] = (bt, codim2.bogdanov_takens_normal_form_native(c.prob, bt, c.ls),
                         codim2.bogdanov_takens_normal_form(c.prob, bt, c.ls))
    return _records[key]


@pytest.mark.parametrize("key", ["8x6", "12x9"])
def test_normal_form_at_the_refined_point_matches_golden(ctx, key):
    """bt_jordan_basis and the normal form (native and mirror) at the point newton_bt_native returns from the stop point: a, b,
    gamma, c, K10, K11, K2 against golden after orienting a > 0, within 10 x max(|LU - GMRES|, 8 eps cond(J_BT) |value|); the
    Jordan identities J q0 = 0, J q1 = q0, J' p1 = 0, J' p0 = p1 on the dense oracle Jacobian and <p_i, q_j> = delta_ij within
    10 x the Newton tolerance (the chain is solved at a point converged to that tolerance, J q0 = -sigma vl with |sigma| below it);
    detailed = False returns the same a and b; native = mirror bit for bit."""
    codim2, _ = _lib()
    c = _case(ctx, key)
    lu, gd = c.g["lu"]["stop"], c.g["gmres"]["diff"]
    bt, n, m = _record(ctx, key)
    X = codim2.BTVec(bt.x0, bt.p)
    assert all(bt.converged), bt.converged
    G, GJ = bt.basis
    tol10 = 10 * BT.CGL_CURVE["tol"]
    assert np.abs(G - np.eye(2)).max() <= tol10 and np.abs(GJ - np.array([[0.0, 1.0], [0.0, 0.0]])).max() <= tol10, (G, GJ)
    q0, q1, p0, p1 = (v.numpy() for v in (*bt.zeta, *bt.zeta_star))
    defect = BT.jordan_defect(c.model, X.u.numpy(), BT._at(c.model, LENSES, X.p), q0, q1, p0, p1)
    probe(f"bt.jordan_defect.{key}", defect, tol10)
    for kind, r, f in (("native", n, codim2.bogdanov_takens_normal_form_native), ("mirror", m, codim2.bogdanov_takens_normal_form)):
        print(f"{key} {kind}:", {k: r.nf[k] for k in BT.NF_KEYS}, "iterations", r.itlinear, "golden", {k: lu[k] for k in BT.NF_KEYS})
        assert all(r.converged) and len(r.itlinear) == 4
        nf = _oriented(r.nf)
        for k in BT.NF_KEYS:
            d = float(np.abs(np.asarray(nf[k]) - np.asarray(lu[k])).max())
            probe(f"bt.nf_{k}.{key}.{kind}", d, c.margin(gd[k], lu[k], lu["cond"]), relative=d / float(np.abs(np.asarray(lu[k])).max()))
        short = f(c.prob, bt, c.ls, detailed=False)
        assert short.nf == dict(a=r.nf["a"], b=r.nf["b"]) and short.itlinear == []
    assert n.itlinear == m.itlinear
    for k in BT.NF_KEYS:
        assert np.array_equal(np.asarray(n.nf[k]), np.asarray(m.nf[k])), (k, n.nf[k], m.nf[k])
    for k in ("H2000", "H1100", "H0010", "H0001"):
        assert torch.equal(n.nf[k].t, m.nf[k].t), k


# ------------------------------------------------------------------------------------------ 6: end to end
def _hopf_curve(ctx, detect):
    codim2, hip = _lib()
    from bk_amd import continuation as Cn
    dims = GRIDS["8x6"]
    rstar, z = BT.cgl_hopf_start(dims)
    prob = hip.CGL2d(ctx, dims, LS, **dict(PARS, r=rstar))
    ls = hip.GMRESIterativeSolvers(reltol=1e-13, restart=60, maxiter=600, Pl=hip.CGLBlockPreconditioner(prob, rstar, PARS["nu"]))
    Z = (prob.vec(np.ascontiguousarray(z.real)), prob.vec(np.ascontiguousarray(z.imag)))
    cv = BT.CGL_CURVE
    cp = Cn.ContinuationPar(ds=cv["ds"], dsmin=cv["dsmin"], dsmax=cv["dsmax"], p_min=-10.0, p_max=10.0, max_steps=cv["max_steps"],
                            newton_options=Cn.NewtonPar(tol=cv["tol"], max_iterations=cv["max_iterations"]))
    br = codim2.continuation_hopf(prob, codim2.HopfVec(prob.vec(np.zeros(prob.nlocal)), [rstar, PARS["nu"]]), 0.0, "gamma", Z, Z,
                                  ls, cp, detect_codim2=detect)
    return prob, ls, br


def test_hopf_curve_ends_with_a_bt_point_and_unfolds_it(ctx):
    """continuation_hopf(..., "gamma", detect_codim2 = 1) from the closed-form Hopf point of 8 x 6 with the example's steps: the
    curve of the restatement (same step count, every record to 1e-8), stopped_at_bt, exactly one "bt" special point, at the last
    index, holding the stop state; get_normal_form on it refines to the golden Bogdanov-Takens point (the margin of
    test_newton_bt_refines_the_stop_point_to_the_golden_point) and returns its a, b and unfolding.  With detect_codim2 = 0 the run
    records the restatement's curve as well and no special point."""
    codim2, hip = _lib()
    g = GOLD["8x6"]
    prob, ls, br = _hopf_curve(ctx, 1)
    ref = g["curve"]
    print("device curve", len(br.p2) - 1, "steps, restatement", g["steps"], "omega tail", br.omega[-3:], "special points",
          [{k: v for k, v in sp.items() if k not in ("x", "a", "b")} for sp in br.specialpoint])
    assert br.stopped_at_bt and len(br.p2) == g["steps"] + 1
    for k in range(len(br.p2)):
        assert max(abs(br.p1[k] - ref["p1"][k]), abs(br.p2[k] - ref["p2"][k]), abs(br.omega[k] - ref["omega"][k])) <= 1e-8, k
    bts = [i for i, sp in enumerate(br.specialpoint) if sp["type"] == "bt"]
    assert len(bts) == 1 and bts[0] == len(br.specialpoint) - 1
    sp = br.specialpoint[bts[0]]
    assert sp["idx"] == sp["step"] == len(br.p2) - 1 and sp["p1"] == br.p1[-1] and sp["p2"] == br.p2[-1] and sp["omega"] == br.omega[-1]
    assert abs(sp["omega"]) < 100 * BT.CGL_CURVE["tol"]
    assert np.abs(sp["x"].numpy() - np.array(g["starts"]["stop"]["x"])).max() <= 1e-7
    X = codim2.bt_point(br, bts[0])
    assert list(X.p) == [sp["p1"], sp["p2"]]
    r_stop = sp["p1"]
    ls_bt = hip.GMRESIterativeSolvers(reltol=BT.GMRES["rtol"], restart=BT.GMRES["restart"], maxiter=600,
                                      Pl=hip.CGLBlockPreconditioner(prob, r_stop, PARS["nu"]))
    ls_adj = codim2.bt_adjoint_solver(prob, ls_bt, r_stop, PARS["nu"])
    bt = codim2.get_normal_form(br, bts[0], prob, ls_bt, ls_adj=ls_adj, tol=BT.CGL_CURVE["tol"])
    lu, gd = g["lu"]["stop"], g["gmres"]["diff"]
    margin = lambda diff, value, cond=1.0: 10 * max(diff, 8 * EPS * cond * float(np.abs(np.asarray(value)).max()))
    print("get_normal_form: p =", bt.p, "golden", lu["p"], "newton", bt.newton["residuals"], {k: bt.nf[k] for k in BT.NF_KEYS})
    assert isinstance(bt, codim2.BogdanovTakens) and bt.lens == ("r", "gamma") and bt.newton["converged"]
    # the start is the device's own stop state (1e-8 from the restatement's), so the point carries that start's Newton remainder
    for j in range(2):
        probe(f"bt.end_to_end_p{j}", abs(bt.p[j] - lu["p"][j]), margin(gd["p"], lu["p"][j], lu["cond"]))
    nf = _oriented(bt.nf)
    for k in BT.NF_KEYS:
        d = float(np.abs(np.asarray(nf[k]) - np.asarray(lu[k])).max())
        probe(f"bt.end_to_end_{k}", d, margin(gd[k], lu[k], lu["cond"]))
    short = codim2.get_normal_form(br, bts[0], prob, ls_bt, ls_adj=ls_adj, tol=BT.CGL_CURVE["tol"], detailed=False)
    assert short.nf == dict(a=bt.nf["a"], b=bt.nf["b"])
    assert prob.params["gamma"] == PARS["gamma"]                          # the problem's own parameters are untouched
    # detection off: the restatement's curve, no special point
    _, _, br0 = _hopf_curve(ctx, 0)
    assert br0.stopped_at_bt and br0.specialpoint == [] and br0.l1 == [] and len(br0.p2) == g["steps"] + 1
    for k in range(len(br0.p2)):
        assert max(abs(br0.p1[k] - ref["p1"][k]), abs(br0.p2[k] - ref["p2"][k]), abs(br0.omega[k] - ref["omega"][k])) <= 1e-8, k
    assert br0.p1 == br.p1 and br0.p2 == br.p2 and br0.omega == br.omega      # and the points of the run with detection, bit for bit


# ------------------------------------------------------------------------------------------ 7: the predictor round trip
def test_hopf_curve_restarts_from_the_bt_point(ctx):
    """continuation_hopf_from_bt at 12 x 9 with ds = omega^4 / (4 |a|) for a predicted omega of 0.1: newton_hopf_native converges
    from the predictor within the restatement's count + 2, the point is a Hopf point of the dense Jacobian (|Re lambda| <= 1e-8,
    |Im lambda - omega| <= 1e-8), and three further steps of ds = -0.01 (away from the Bogdanov-Takens point) reproduce the
    restatement's curve from the same start to 1e-8."""
    import scipy.linalg as sla
    codim2, hip = _lib()
    from bk_amd import continuation as Cn
    c = _case(ctx, "12x9")
    bt = _record(ctx, "12x9")[1]
    tol = BT.CGL_CURVE["tol"]
    ds = 0.1 ** 4 / (4 * abs(bt.nf["a"]))
    pr = codim2.predictor(bt, "HopfCurve", ds)
    assert abs(pr["omega"] - 0.1) <= 1e-12
    # the restatement from ITS normal form at the golden point
    st = c.g["starts"]["stop"]
    x, p = np.array(st["x"]), np.array(st["p"])
    a0, b0 = BT.start_vectors(c.model, x, BT._at(c.model, LENSES, p))
    s = BT.newton_bt(c.model, x, p, LENSES, a0, b0, tol=tol)
    q = BT._at(c.model, LENSES, s["p"])
    basis = BT.jordan_basis(c.model, s["u"], q, s["terms"]["v1"], s["terms"]["w1"])
    nf = BT.normal_form(c.model, s["u"], q, LENSES, *basis)
    h = BT.predictor_hopf(nf, s["p"], *basis, 0.1 ** 4 / (4 * abs(nf["a"])))
    assert np.abs(pr["pars"] - h["pars"]).max() <= 1e-9 and np.abs(pr["x0"].numpy() - h["x0"]).max() <= 1e-9
    hm = R.cgl_model(c.op, dict(PARS), *LENSES)
    nrm = lambda zz: zz / np.linalg.norm(zz)
    sh = R.newton_hopf(hm, s["u"] + h["x0"], h["pars"][0], h["omega"], nrm(h["EigenVecAd"]), nrm(h["EigenVec"]), p2=h["pars"][1],
                       tol=tol, max_iterations=15)
    assert sh["converged"]
    seq = [-0.01] * 3
    ref = R.continuation_hopf(hm, sh["u"], sh["p"], sh["omega"], h["pars"][1], nrm(sh["w"]), nrm(sh["v"]), ds=-0.01, dsmax=0.01,
                              tol=tol, max_iterations=15, ds_sequence=seq)
    ls = hip.GMRESIterativeSolvers(reltol=1e-13, restart=60, maxiter=600,
                                   Pl=hip.CGLBlockPreconditioner(c.prob, float(h["pars"][0]), PARS["nu"]))
    cp = Cn.ContinuationPar(ds=-0.01, dsmin=1e-4, dsmax=0.01, p_min=-10.0, p_max=10.0, max_steps=10,
                            newton_options=Cn.NewtonPar(tol=tol, max_iterations=15))
    br, sd, _ = codim2.continuation_hopf_from_bt(bt, c.prob, ls, cp, ds, ds_sequence=seq, save_sol=True)
    print("newton_hopf from the predictor:", sd["residuals"], "restatement", sh["residuals"], "landed on", sd["u"].p,
          "restatement", (sh["p"], sh["omega"]))
    assert sd["converged"] and sd["itnewton"] <= sh["itnewton"] + 2
    xg = sd["u"].u.numpy()
    ev = sla.eigvals(c.op.J(xg, **dict(PARS, r=sd["u"].p[0], gamma=float(pr["pars"][1]))).toarray())
    k = np.argmin(np.abs(ev - 1j * sd["u"].p[1]))
    assert abs(ev[k].real) <= 1e-8 and abs(ev[k].imag - sd["u"].p[1]) <= 1e-8, ev[k]
    assert len(br.p2) == len(ref["p2"]) == 4 and 0.25 <= br.omega[-1] <= 0.3
    for i in range(4):
        assert max(abs(br.p1[i] - ref["p1"][i]), abs(br.p2[i] - ref["p2"][i]), abs(br.omega[i] - ref["omega"][i])) <= 1e-8, (i, br.p1, ref["p1"])
    assert c.prob.params["gamma"] == PARS["gamma"]
    f = codim2.predictor(bt, "FoldCurve", 1e-3)
    assert np.abs(f["pars"] - (bt.p + bt.nf["K11"] * 1e-3 + bt.nf["K2"] * 5e-7)).max() <= 1e-15 and f["EigenVec"] is bt.zeta[0]


# ------------------------------------------------------------------------------------------ 8: errors
def test_bt_entries_refuse_what_they_cannot_do(ctx):
    """A non-cGL problem, a missing adjoint preconditioner and an index that is no "bt" point are refused with a message, before any
    launch."""
    codim2, hip = _lib()
    from bk_amd import _lib as L
    c = _case(ctx, "8x6")
    X = c.start("stop")
    n = c.prob.nlocal
    a, b = c.prob.vec(np.full(n, 0.1)), c.prob.vec(np.full(n, 0.2))
    pv = _pv(BT._at(c.model, LENSES, X.p))
    with pytest.raises(L.BkHipError, match="adjoint"):
        codim2.bt_terms(c.prob, X.u, pv, a, b, c.ls, None, "vw")
    with pytest.raises(L.BkHipError, match="adjoint"):
        codim2.newton_bt_native(c.prob, X, "gamma", a, b, c.ls, None)
    with pytest.raises(TypeError, match="adjoint"):
        codim2.newton_bt(c.prob, X, "gamma", a, b, c.ls, None)
    with pytest.raises(ValueError, match="2 different parameters"):
        codim2.newton_bt_native(c.prob, X, "r", a, b, c.ls, c.ls_adj)
    sh = hip.SwiftHohenberg(ctx, (8, 8), (np.pi, np.pi), l=0.1, nu=1.2)
    u = sh.vec(np.zeros(sh.nlocal))
    with pytest.raises(L.BkHipError, match="BK_PDE_CGL2D only"):
        codim2.bt_border(sh, u, [0.1, 1.2], 0, 1, -1.0, u, u, u, u)
    with pytest.raises(L.BkHipError, match="BK_PDE_CGL2D only"):
        codim2.bt_nf_dots(sh, u, [0.1, 1.2], u, u, u, u)
    br = codim2.HopfBranch(lens2="gamma")
    br.specialpoint.append(dict(type="gh"))
    with pytest.raises(ValueError, match="BT point"):
        codim2.bt_point(br, 0)
    br.specialpoint.append(dict(type="bt", x=X.u, p1=X.p[0], p2=X.p[1]))
    with pytest.raises(TypeError, match="ls_adj"):
        codim2.get_normal_form(br, 1, c.prob, c.ls)
