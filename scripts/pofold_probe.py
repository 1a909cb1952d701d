#!/usr/bin/env python
"""Measurements of the fold-of-limit-cycles layer, one process, appended to profiles/pofold_probe.jsonl.  Per size
(16 x 12, M = 12 -- the fold run of the tests -- and 41 x 21, M = 30, the example's grid):

  * kernel time of the adjoint and fold-border marching passes and of the transposed time solve (scopes potrap_jvp_adjoint,
    pofold_border, potrap_adjoint_timesolve) from the library's event scopes with their algorithmic bytes (4 streams of 8 M N bytes for the two marching kernels, 3 for the time solve), next to the
    forward potrap_jvp scope;
  * wall time and GMRES count of one doubly bordered solve (rtol 1e-9, IterativeSolvers flavor) next to the plain orbit solve;
  * the fold refinement: continuation_po_trap(save_sol=True, nev=2, detect_bifurcation=2) from dr = 0.15 until the fold is
    crossed, po_fold_point, then newton_fold_po_native against newton_fold_po, the call-by-call mirror from the same entry
    points (the baseline).  Where the branch records no fold within the steps, that is recorded and the Newton timing is left out.

Warm buffers, ONE synchronisation per timed call, median and spread (min, max) reported.

Usage: python scripts/pofold_probe.py [--out profiles/pofold_probe.jsonl] [--reps 15] [--cases 16x12x12,41x21x30]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from floquet_probe import LS, NAMES, PARS, scope, timed  # noqa: E402


def one_case(ctx, hip, PO, Cn, dims, M, reps):
    import math
    nx, ny = dims
    lam11 = (-4 * (nx / (2 * LS[0])) ** 2 * math.sin(math.pi / (2 * (nx + 1))) ** 2
             - 4 * (ny / (2 * LS[1])) ** 2 * math.sin(math.pi / (2 * (ny + 1))) ** 2)
    dr = 0.15
    r = -lam11 - dr
    pars = dict(PARS, r=r)
    pv = [pars[k] for k in NAMES]
    prob = hip.CGL2d(ctx, dims, LS, **pars)
    b = 2 * (-PARS["c3"] + 1j * PARS["mu"]) * 9 / (4 * (nx + 1) * (ny + 1))
    amp = math.sqrt(dr / b.real)
    om = PARS["nu"] - b.imag / b.real * dr
    phi = np.outer(np.sin(np.pi * np.arange(1, ny + 1) / (ny + 1)), np.sin(np.pi * np.arange(1, nx + 1) / (nx + 1))).reshape(-1)
    phi /= np.linalg.norm(phi) * math.sqrt(2)
    U0 = np.stack([np.concatenate([2 * amp * np.cos(t) * phi, 2 * amp * np.sin(t) * phi]) for t in 2 * np.pi * np.arange(M) / M])
    T0 = abs(2 * np.pi / om)
    po = PO.PeriodicOrbitTrap(prob, M)
    f = prob.residual(prob.vec(U0[0]), r)
    f.scale_(1.0 / f.norm())
    po.set_section(f)
    ls = hip.GMRESIterativeSolvers(reltol=1e-9, restart=60, maxiter=200)
    n = po.n
    rec = dict(kind="pofold", dims=list(dims), M=M, dr=dr, doubles_per_vector=n, working_set_MB=4 * 8.0 * n / 1e6,
               note="the working set sits in the 256 MB Infinity Cache: the bandwidth figures are cache figures, not HBM")
    rng = np.random.default_rng(5)
    u, w, v = po.vec(U0), po.vec(rng.standard_normal(n)), po.vec(rng.standard_normal(n))
    ctx.prof_enable(True)
    for name, nstreams, call in (
            ("potrap_jvp", 4, lambda: po.jvp(u, T0, pv, v, 0.3)),
            ("potrap_jvp_adjoint", 4, lambda: po.jvp_adjoint(u, T0, pv, w, 0.3)),
            ("pofold_border", 4, lambda: po.fold_border(u, T0, pv, 0, hip.BorderedArray(v, 0.3), w))):
        ms, _ = scope(ctx, name, reps, call)
        rec[name] = dict(ms=ms, bytes=nstreams * 8.0 * n, TBps=nstreams * 8.0 * n / (ms * 1e-3) / 1e12)
    PT = PO.PoTrapPreconditioner(po, r, PARS["nu"], adjoint=True).set_period(T0)
    P = PO.PoTrapPreconditioner(po, r, PARS["nu"]).set_period(T0)
    for name, pl in (("potrap_adjoint_timesolve", PT), ("potrap_timesolve", P)):
        ms, _ = scope(ctx, name, reps, lambda: pl.ldiv(w))
        rec[name] = dict(ms=ms, bytes=3 * 8.0 * n, TBps=3 * 8.0 * n / (ms * 1e-3) / 1e12)
    ctx.prof_enable(False)
    # one plain and one doubly bordered solve on the guess
    J = po.jacobian(u, T0, pv)
    B = hip.BorderedArray
    rhs = po.residual(u, T0, pv)
    _, cv, it = PO.po_solve(J, P, rhs, ls)
    rec["solve"] = dict(converged=cv, gmres_iterations=it, **timed(ctx, reps, lambda: PO.po_solve(J, P, rhs, ls)))
    a, bb = B(w, 0.2), B(v, -0.4)
    _, _, cv, it = PO.po_bordered_solve(J, P, a, bb, 0.3, rhs, 1.0, ls)
    rec["bordered_solve"] = dict(converged=cv, gmres_iterations=it,
                                 **timed(ctx, reps, lambda: PO.po_bordered_solve(J, P, a, bb, 0.3, rhs, 1.0, ls)))
    # the fold refinement
    cp = Cn.ContinuationPar(ds=-0.02, dsmin=1e-4, dsmax=0.04, a=0.5, eta=150.0, p_min=-10.0, p_max=10.0, max_steps=6,
                            detect_bifurcation=0, newton_options=Cn.NewtonPar(tol=1e-10, max_iterations=10))
    try:
        br = PO.continuation_po_trap(po, u, T0, pv, "r", cp, ls, nev=2, detect_bifurcation=2, tol_stability=1e-5, save_sol=True,
                                     eig=hip.EigKrylovKit(tol=1e-8, maxiter=20, krylovdim=20))
        folds = [k for k, s in enumerate(br["specialpoints"]) if s["type"] == "bp"]
        rec["branch"] = dict(p_minus_rhopf=[p + lam11 for p in br["p"]], n_unstable=br["n_unstable"], folds=len(folds))
    except RuntimeError as e:
        rec["branch"] = dict(error=str(e))
        folds = []
    if folds:
        fp = PO.po_fold_point(br, folds[0], po, pv, "r")
        pvf = list(pv)
        pvf[0] = fp["p"]
        nat = PO.newton_fold_po_native(po, fp["orbit"], fp["T"], pvf, "r", fp["a"], fp["b"], ls)
        mir = PO.newton_fold_po(po, fp["orbit"], fp["T"], pvf, "r", fp["a"], fp["b"], ls)
        rec["newton_fold"] = dict(converged=[nat["converged"], mir["converged"]], residuals=nat["residuals"],
                                  p_minus_rhopf=nat["p"] + lam11, T=nat["T"], amplitude=PO.amplitude(nat["u"]),
                                  gmres_counts=nat["itlinear"], native_vs_mirror=dict(p=abs(nat["p"] - mir["p"]), T=abs(nat["T"] - mir["T"])))
        k = max(3, reps // 3)
        rec["newton_fold"]["native"] = timed(ctx, k, lambda: PO.newton_fold_po_native(po, fp["orbit"], fp["T"], pvf, "r", fp["a"], fp["b"], ls))
        rec["newton_fold"]["mirror"] = timed(ctx, k, lambda: PO.newton_fold_po(po, fp["orbit"], fp["T"], pvf, "r", fp["a"], fp["b"], ls))
        rec["newton_fold"]["mirror_over_native"] = rec["newton_fold"]["mirror"]["median_ms"] / rec["newton_fold"]["native"]["median_ms"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pofold_probe.jsonl"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--cases", default="16x12x12,41x21x30")
    args = ap.parse_args()
    from bk_amd import hip
    from bk_amd import continuation as Cn
    from bk_amd import periodic_orbit as PO
    ctx = hip.Context(0)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fo:
        for s in args.cases.split(","):
            nx, ny, M = (int(v) for v in s.split("x"))
            rec = one_case(ctx, hip, PO, Cn, (nx, ny), M, args.reps)
            print(json.dumps(rec))
            fo.write(json.dumps(rec) + "\n")
            fo.flush()
    ctx.close()


if __name__ == "__main__":
    main()
