#!/usr/bin/env python
"""Measurements of the Bogdanov-Takens layer, one process, appended to profiles/bt_probe.jsonl.  Per size (41 x 21, the
example's grid, and 256 x 256):

  * the BtBorder pass (scope bt_border: 5 vectors read, 2 written, 4 sums) against the literal sequence of the reference for the
    same quantities (MinAugBT.jl:176-220: differences of the adjoint Jacobian at x + eps v for sigma_x, dJ/dp products and dots
    for sigma_p), with the number of library calls of each;
  * one preconditioned bordered solve [J a; b' 0] and one bk_bt_linsolve (the m = 2 block-bordered solve with its border pass) on a
    smooth state, wall time and GMRES count;
  * at 41 x 21 only: the Hopf curve of the example in gamma from the closed-form Hopf point to its stop, the "bt" special point,
    newton_bt_native against the call-by-call mirror from it, and the point, a and b found (no reference value exists for this
    grid: reported, not asserted).

Warm buffers, ONE synchronisation per timed call, median and spread (min, max) reported.  The working sets sit in the Infinity Cache
and the small grid is launch-bound: the record counts launches and passes, it claims no bandwidth.

Usage: python scripts/bt_probe.py [--out profiles/bt_probe.jsonl] [--reps 15] [--cases 41x21,256x256]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from floquet_probe import LS, NAMES, PARS, scope, timed  # noqa: E402


def literal_border(codim2, prob, x, pv, r, i1, i2, v1, v2, w1, w2, eps=1e-6):
    """sigma_x and sigma_p as the reference forms them, on the entry points that existed before the fused pass: (row1, row2, block,
    the number of vector passes -- copies, updates, operator applications, dots)."""
    Jt = lambda y: prob.jacobian_adjoint(y, r)
    x1, x2 = x.copy().add_(v1, eps), x.copy().add_(v2, eps)                            # 4 passes
    J0, J1, J2 = Jt(x), Jt(x1), Jt(x2)
    u12, u22 = J0(w1), J0(w2)                                                          # 2
    row1 = J1(w1).add_(u12, 1.0 / eps, -1.0 / eps)                                     # 2
    row2 = J1(w2).add_(u22, 1.0 / eps, -1.0 / eps)                                     # 2
    row2.add_(J2(w1).add_(u12, 1.0 / eps, -1.0 / eps), 1.0)                            # 3
    blk = np.zeros((2, 2))
    for k, ip in enumerate((i1, i2)):                                                  # 2 x (2 products + 3 dots)
        D1, D2 = codim2.hopf_dJdp(prob, x, pv, ip, v1), codim2.hopf_dJdp(prob, x, pv, ip, v2)
        blk[0, k] = -w1.inner(D1)
        blk[1, k] = -w2.inner(D1) - w1.inner(D2)
    return row1, row2, blk, 23


def one_case(ctx, hip, codim2, Cn, dims, reps):
    nx, ny = dims
    lam11 = (-4 * (nx / (2 * LS[0])) ** 2 * math.sin(math.pi / (2 * (nx + 1))) ** 2
             - 4 * (ny / (2 * LS[1])) ** 2 * math.sin(math.pi / (2 * (ny + 1))) ** 2)
    rstar = -lam11
    pars = dict(PARS, r=rstar + 0.3, gamma=0.5)
    pv = [pars[k] for k in NAMES]
    prob = hip.CGL2d(ctx, dims, LS, **pars)
    n = prob.nlocal
    rec = dict(kind="bt", dims=list(dims), doubles_per_vector=n, working_set_MB=7 * 8.0 * n / 1e6,
               note="the working set sits in the 256 MB Infinity Cache: launch and pass counts, no bandwidth claim")
    sx = np.sin(np.pi * np.arange(1, nx + 1) / (nx + 1))
    sy = np.sin(np.pi * np.arange(1, ny + 1) / (ny + 1))
    mode = lambda i, j: np.outer(np.sin(j * np.pi * np.arange(1, ny + 1) / (ny + 1)), np.sin(i * np.pi * np.arange(1, nx + 1) / (nx + 1))).reshape(-1)
    phi = np.outer(sy, sx).reshape(-1)
    smooth = lambda a, b, i, j: prob.vec(np.concatenate([a * mode(i, j), b * mode(j, i)]))
    x = prob.vec(np.concatenate([0.8 * phi, 0.3 * phi]))
    v1, v2, w1, w2 = smooth(1.0, 0.4, 1, 1), smooth(0.3, -0.7, 2, 1), smooth(-0.5, 0.9, 1, 2), smooth(0.6, 0.2, 2, 2)
    # the pass against the literal sequence
    ctx.prof_enable(True)
    ms, per = scope(ctx, "bt_border", reps, lambda: codim2.bt_border(prob, x, pv, 0, 5, -1.0, v1, v2, w1, w2))
    ctx.prof_enable(False)
    rec["bt_border_kernel"] = dict(ms=ms, launches_per_call=per, bytes=7 * 8.0 * n)
    rec["bt_border"] = timed(ctx, reps, lambda: codim2.bt_border(prob, x, pv, 0, 5, -1.0, v1, v2, w1, w2))
    r1, r2, blk = codim2.bt_border(prob, x, pv, 0, 5, -1.0, v1, v2, w1, w2)
    l1, l2, lblk, ncalls = literal_border(codim2, prob, x, pv, pars["r"], 0, 5, v1, v2, w1, w2)
    rec["literal"] = dict(library_calls=ncalls, **timed(ctx, reps, lambda: literal_border(codim2, prob, x, pv, pars["r"], 0, 5, v1, v2, w1, w2)))
    rec["literal"]["row_difference"] = [float(r1.copy().add_(l1, -1.0).norminf()), float(r2.copy().add_(l2, -1.0).norminf())]
    rec["literal"]["block_difference"] = float(np.abs(blk - lblk).max())
    rec["literal_over_pass"] = rec["literal"]["median_ms"] / rec["bt_border"]["median_ms"]
    # one bordered solve and one BT linear solve
    ls = hip.GMRESIterativeSolvers(reltol=1e-10, restart=60, maxiter=600, Pl=hip.CGLBlockPreconditioner(prob, pars["r"], PARS["nu"]))
    ls_adj = codim2.bt_adjoint_solver(prob, ls, pars["r"], PARS["nu"])
    bls = hip.MatrixFreeBLS(ls, use_pl=True)
    J = prob.jacobian(x, pars["r"])
    _, _, cv, it = bls(J, w1, v1, 0.0, x.zerovector(), 1.0)
    rec["bordered_solve"] = dict(converged=cv, gmres_iterations=it, **timed(ctx, reps, lambda: bls(J, w1, v1, 0.0, x.zerovector(), 1.0)))
    t = codim2.bt_terms(prob, x, pv, w1, v1, ls, ls_adj)
    rec["bt_terms"] = dict(converged=t["converged"], gmres_iterations=t["itlinear"],
                           **timed(ctx, reps, lambda: codim2.bt_terms(prob, x, pv, w1, v1, ls, ls_adj)))
    F = codim2.residual(prob, x, pv)

    def linsolve():
        import ctypes as C
        dX = x.similar()
        dp, cvv, itt = (C.c_double * 2)(), C.c_int(), C.c_int()
        lo = ls._opts()
        ctx.check(ctx.lib.bk_bt_linsolve(ctx.h, prob.h, x.t.data_ptr(), (C.c_double * 6)(*pv), 6, 0, 5, t["v1"].t.data_ptr(),
                                         t["v2"].t.data_ptr(), t["w1"].t.data_ptr(), t["w2"].t.data_ptr(), F.t.data_ptr(),
                                         (C.c_double * 2)(*t["sigma"]), C.byref(lo), ls._pl(), dX.t.data_ptr(), dp, C.byref(cvv),
                                         C.byref(itt)), "bk_bt_linsolve")
        return dX, (dp[0], dp[1]), bool(cvv.value), itt.value
    _, _, cv, it = linsolve()
    rec["bt_linsolve"] = dict(converged=cv, gmres_iterations=it, **timed(ctx, reps, linsolve))
    if nx * ny > 4096:
        return rec
    # the example's Hopf curve to its stop, then the refinement
    probc = hip.CGL2d(ctx, dims, LS, **dict(PARS, r=rstar))
    lsc = hip.GMRESIterativeSolvers(reltol=1e-13, restart=60, maxiter=600, Pl=hip.CGLBlockPreconditioner(probc, rstar, PARS["nu"]))
    ph = phi / (np.linalg.norm(phi) * math.sqrt(2))
    z = np.zeros_like(ph)
    Z = (probc.vec(np.concatenate([ph, z])), probc.vec(np.concatenate([z, -ph])))
    cp = Cn.ContinuationPar(ds=0.01, dsmin=1e-3, dsmax=0.02, p_min=-10.0, p_max=10.0, max_steps=100,
                            newton_options=Cn.NewtonPar(tol=1e-10, max_iterations=25))
    t0 = time.perf_counter()
    br = codim2.continuation_hopf(probc, codim2.HopfVec(probc.vec(np.zeros(n)), [rstar, PARS["nu"]]), 0.0, "gamma", Z, Z, lsc, cp,
                                  detect_codim2=1)
    rec["hopf_curve"] = dict(steps=len(br.p2) - 1, stopped_at_bt=br.stopped_at_bt, seconds=time.perf_counter() - t0,
                             special_points=[sp["type"] for sp in br.specialpoint], last=[br.p1[-1], br.p2[-1], br.omega[-1]])
    bts = [i for i, sp in enumerate(br.specialpoint) if sp["type"] == "bt"]
    if not bts:
        return rec
    X = codim2.bt_point(br, bts[0])
    lsb = hip.GMRESIterativeSolvers(reltol=1e-13, restart=60, maxiter=600, Pl=hip.CGLBlockPreconditioner(probc, X.p[0], PARS["nu"]))
    lsb_adj = codim2.bt_adjoint_solver(probc, lsb, X.p[0], PARS["nu"])
    a, b = codim2.bt_start_vectors(probc, X, "gamma", lsb, lsb_adj)
    nat = codim2.newton_bt_native(probc, X, "gamma", a, b, lsb, lsb_adj, tol=1e-10)
    mir = codim2.newton_bt(probc, X, "gamma", a, b, lsb, lsb_adj, tol=1e-10)
    bt = codim2.get_normal_form(br, bts[0], probc, lsb, ls_adj=lsb_adj, tol=1e-10)
    rec["newton_bt"] = dict(converged=[nat["converged"], mir["converged"]], residuals=nat["residuals"], point=list(nat["u"].p),
                            xinf=nat["u"].u.norminf(), gmres_per_solve=nat["itsolves"],
                            native_equals_mirror=bool(list(nat["u"].p) == list(mir["u"].p) and nat["residuals"] == mir["residuals"]),
                            a=bt.nf["a"], b=bt.nf["b"], K10=list(bt.nf["K10"]), K11=list(bt.nf["K11"]), K2=list(bt.nf["K2"]),
                            normal_form_gmres=bt.itlinear)
    k = max(3, reps // 3)
    rec["newton_bt"]["native"] = timed(ctx, k, lambda: codim2.newton_bt_native(probc, X, "gamma", a, b, lsb, lsb_adj, tol=1e-10))
    rec["newton_bt"]["mirror"] = timed(ctx, k, lambda: codim2.newton_bt(probc, X, "gamma", a, b, lsb, lsb_adj, tol=1e-10))
    rec["newton_bt"]["mirror_over_native"] = rec["newton_bt"]["mirror"]["median_ms"] / rec["newton_bt"]["native"]["median_ms"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bt_probe.jsonl"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--cases", default="41x21,256x256")
    args = ap.parse_args()
    from bk_amd import codim2, hip
    from bk_amd import continuation as Cn
    ctx = hip.Context(0)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fo:
        for s in args.cases.split(","):
            nx, ny = (int(v) for v in s.split("x"))
            rec = one_case(ctx, hip, codim2, Cn, (nx, ny), args.reps)
            print(json.dumps(rec))
            fo.write(json.dumps(rec) + "\n")
            fo.flush()
    ctx.close()


if __name__ == "__main__":
    main()
