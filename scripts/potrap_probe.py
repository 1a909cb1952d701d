#!/usr/bin/env python
"""Measurements of the trapezoid periodic-orbit passes, one process, appended to profiles/potrap_probe.jsonl:

  1. per size (41 x 21, 256^2, 1024^2; M = 30): the marching residual and JVP (scopes potrap_residual / potrap_jvp), the time
     solve of the preconditioner (potrap_timesolve) and one whole preconditioner application, next to the LITERAL sequence built
     from existing entry points -- M - 1 bk_residual (and, for the JVP, M - 1 bk_op_apply) plus the bk_vec_axpby passes that
     combine them -- which is the comparison target, not the code under test.  Wall time per call with one synchronisation, and
     the algorithmic bytes of each (8-byte streams of M N doubles: marching residual 3 -- u, phi, out --, JVP 4, time solve 3;
     literal residual 2 per stencil launch + 3 for a fused combine, literal JVP 2 + 3 per stencil launch pair + 7; the literal
     combine is run as single bk_vec_axpby passes and moves more than that).
  2. the GMRES counts of the preconditioned solve on the first Newton system of the one-mode guess at r = r_hopf - dr
     (rtol 1e-3 and 1e-9), the GPU column of the table in DESIGN 9k.

Usage: python scripts/potrap_probe.py [--out profiles/potrap_probe.jsonl] [--reps 20] [--sizes 41x21,256x256,1024x1024]
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

PARS = dict(r=0.5, mu=0.1, nu=1.0, c3=-1.0, c5=1.0, gamma=0.0)
NAMES = ("r", "mu", "nu", "c3", "c5", "gamma")
LS = (np.pi, np.pi / 2)


def wall(ctx, reps, call):
    for _ in range(3):
        call()
    ctx.sync()
    rounds = []
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(reps):
            call()
        ctx.sync()
        rounds.append((time.perf_counter() - t0) / reps * 1e3)
    return float(np.median(rounds))


def scope(ctx, name, reps, call):
    for _ in range(3):
        call()
    ctx.prof_reset()
    for _ in range(reps):
        call()
    ctx.sync()
    g = ctx.prof_get(name)
    return g["ms"] / max(g["calls"], 1)


def kernels(ctx, hip, PO, dims, M, reps):
    prob = hip.CGL2d(ctx, dims, LS, **PARS)
    po = PO.PeriodicOrbitTrap(prob, M)
    N, n = prob.nlocal, prob.nlocal * M
    rng = np.random.default_rng(0)
    mk = lambda s=1.0: hip.HipVec.from_numpy(ctx, s * (rng.random(n) - 0.5))
    U, dU = mk(), mk()
    po.set_section(mk(), mk())
    pv = [PARS[k] for k in NAMES]
    T, dT = 6.3, 0.1
    sl = lambda v, i: hip.HipVec(ctx, v.t[i * N:(i + 1) * N])
    Fs, out, Jout = mk(), mk(), mk()
    K, hh = M - 1, T / M / 2
    # slices, parameter array and Jacobian handles are made once: the literal sequence is charged its launches only
    Us, dUs, Fsl, outs, Jouts = ([sl(v, i) for i in range(M)] for v in (U, dU, Fs, out, Jout))
    parr = PO._parr(pv)
    Js = [prob.jacobian(Us[i], PARS["r"]) for i in range(K)]

    def literal_residual():
        for i in range(K):
            ctx.check(ctx.lib.bk_residual(prob.h, hip._ptr(Us[i].t), parr, 6, hip._ptr(Fsl[i].t)))
        for i in range(K):
            j = K - 1 if i == 0 else i - 1
            o = outs[i]
            o.copyto_(Us[i])
            o.add_(Us[j], -1.0)
            o.add_(Fsl[i], -hh)
            o.add_(Fsl[j], -hh)

    dh = dT / M / 2

    def literal_jvp():
        for i in range(K):
            ctx.check(ctx.lib.bk_residual(prob.h, hip._ptr(Us[i].t), parr, 6, hip._ptr(Fsl[i].t)))
            ctx.check(ctx.lib.bk_op_apply(Js[i].h, hip._ptr(dUs[i].t), 0.0, 1.0, hip._ptr(Jouts[i].t)))
        for i in range(K):
            j = K - 1 if i == 0 else i - 1
            o = outs[i]
            o.copyto_(dUs[i])
            o.add_(dUs[j], -1.0)
            o.add_(Jouts[i], -hh)
            o.add_(Jouts[j], -hh)
            o.add_(Fsl[i], -dh)
            o.add_(Fsl[j], -dh)

    a = -(-4 * (dims[0] / (2 * LS[0])) ** 2 * math.sin(math.pi / (2 * (dims[0] + 1))) ** 2
          - 4 * (dims[1] / (2 * LS[1])) ** 2 * math.sin(math.pi / (2 * (dims[1] + 1))) ** 2) - 0.05
    P = PO.PoTrapPreconditioner(po, a, PARS["nu"]).set_period(T)
    rec = dict(kind="kernels", dims=list(dims), M=M, doubles=n, reps=reps)
    rec["residual_wall_ms"] = wall(ctx, reps, lambda: po.residual(U, T, pv))
    rec["jvp_wall_ms"] = wall(ctx, reps, lambda: po.jvp(U, T, pv, dU, dT))
    rec["literal_residual_wall_ms"] = wall(ctx, reps, literal_residual)
    rec["literal_jvp_wall_ms"] = wall(ctx, reps, literal_jvp)
    rec["precond_wall_ms"] = wall(ctx, reps, lambda: P.ldiv(U))
    ctx.prof_enable(True)
    rec["residual_kernel_ms"] = scope(ctx, "potrap_residual", reps, lambda: po.residual(U, T, pv))
    rec["jvp_kernel_ms"] = scope(ctx, "potrap_jvp", reps, lambda: po.jvp(U, T, pv, dU, dT))
    rec["timesolve_kernel_ms"] = scope(ctx, "potrap_timesolve", reps, lambda: P.ldiv(U))
    ctx.prof_enable(False)
    b = 8.0 * n
    rec["bytes"] = dict(residual=3 * b, jvp=4 * b, timesolve=3 * b, literal_residual=(2 + 3) * b * K / M,
                        literal_jvp=(2 + 3 + 7) * b * K / M)
    for k in ("residual", "jvp", "timesolve"):
        rec[f"{k}_TBps"] = rec["bytes"][k] / (rec[f"{k}_kernel_ms"] * 1e-3) / 1e12
    return rec


def counts(ctx, hip, PO, dims, M, dr):
    nx, ny = dims
    lam11 = (-4 * (nx / (2 * LS[0])) ** 2 * math.sin(math.pi / (2 * (nx + 1))) ** 2
             - 4 * (ny / (2 * LS[1])) ** 2 * math.sin(math.pi / (2 * (ny + 1))) ** 2)
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
    U = po.vec(U0)
    f = prob.residual(prob.vec(U0[0]), r)
    f.scale_(1.0 / f.norm())
    po.set_section(f)
    G = po.residual(U, T0, pv)
    P = PO.PoTrapPreconditioner(po, r, PARS["nu"]).set_period(T0)
    J = po.jacobian(U, T0, pv)
    rec = dict(kind="gmres_counts", dims=list(dims), M=M, dr=dr)
    for rtol in (1e-3, 1e-9):
        _, cv, it = PO.po_solve(J, P, G, hip.GMRESIterativeSolvers(reltol=rtol, restart=60, maxiter=200))
        rec[f"rtol_{rtol:g}"] = dict(converged=cv, iterations=it)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "potrap_probe.jsonl"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="41x21,256x256,1024x1024")
    args = ap.parse_args()
    from bk_amd import hip
    from bk_amd import periodic_orbit as PO
    ctx = hip.Context(0)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fo:
        for s in args.sizes.split(","):
            dims = tuple(int(x) for x in s.split("x"))
            rec = kernels(ctx, hip, PO, dims, 30, args.reps if dims[0] < 1024 else max(3, args.reps // 5))
            print(json.dumps(rec))
            fo.write(json.dumps(rec) + "\n")
            fo.flush()
        for dims, M, dr in (((12, 9), 7, 0.01), ((16, 12), 12, 0.01), ((16, 12), 12, 0.1), ((32, 24), 20, 0.05), ((41, 21), 30, 0.01)):
            rec = counts(ctx, hip, PO, dims, M, dr)
            print(json.dumps(rec))
            fo.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
