#!/usr/bin/env python
"""Measurements of the monodromy application, one process, appended to profiles/floquet_probe.jsonl.  Per size
(41 x 21 and 256^2, M = 30; both sit in the Infinity Cache: 3 K N doubles are 1.2 MB and 91 MB of the 256 MB):

  * wall time of one application of the monodromy, native (PoTrapMonodromy: one space-time GMRES) against monodromy_sequential
    (the call-by-call mirror of Floquet.jl:285-315 from entry points that predate the native path: K slice solves), on the orbit
    of newton_po_trap from the one-mode guess at r = r_hopf - 0.01 (the guess itself where Newton does not converge -- the
    monodromy of a non-orbit is as good an operator to time; recorded).  Warm buffers, ONE synchronisation per timed call,
    `reps` timed calls, median and spread (min, max) reported;
  * the GMRES counts of both, rtol 1e-9, IterativeSolvers flavor;
  * kernel time of the monodromy's marching pass and time solve (scopes monodromy_march, monodromy_timesolve), with the algorithmic
    bytes over time (march: u, y read, out written = 3 x 8 K N; time solve: one read and one write of the spectrum = 2 x 8 K N).

Usage: python scripts/floquet_probe.py [--out profiles/floquet_probe.jsonl] [--reps 15] [--sizes 41x21,256x256]
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


def timed(ctx, reps, call):
    """median, min, max in ms of `reps` calls, each followed by its own synchronisation, after 3 warm-up calls."""
    for _ in range(3):
        call()
    ctx.sync()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ctx.sync()
        t.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=float(np.median(t)), min_ms=float(min(t)), max_ms=float(max(t)), reps=reps)


def scope(ctx, name, reps, call):
    for _ in range(3):
        call()
    ctx.prof_reset()
    for _ in range(reps):
        call()
    ctx.sync()
    g = ctx.prof_get(name)
    return g["ms"] / max(g["calls"], 1), g["calls"] / reps


def one_size(ctx, hip, PO, dims, M, dr, reps):
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
    f = prob.residual(prob.vec(U0[0]), r)
    f.scale_(1.0 / f.norm())
    po.set_section(f)
    ls = hip.GMRESIterativeSolvers(reltol=1e-9, restart=60, maxiter=200)
    s = PO.newton_po_trap(po, po.vec(U0), T0, pv, ls, tol=1e-10, max_iterations=10)
    u, T = (s["u"], s["T"]) if s["converged"] else (po.vec(U0), T0)
    K, N = M - 1, prob.nlocal
    rec = dict(kind="monodromy", dims=list(dims), M=M, dr=dr, doubles_per_vector=K * N, orbit_converged=bool(s["converged"]),
               newton_residuals=s["residuals"], working_set_MB=3 * 8.0 * K * N / 1e6,
               note="the working set of both sizes sits in the 256 MB Infinity Cache: the bandwidth figures are cache figures, not HBM")
    x = np.random.default_rng(5).standard_normal(N)
    xv = prob.vec(x / np.linalg.norm(x))
    mono = PO.PoTrapMonodromy(po, u, T, pv, ls)
    y_all, cv, it = mono.solve(xv)
    seq, its_seq, ok = PO.monodromy_sequential(po, u, T, pv, xv, ls)
    rec["native"] = dict(converged=cv, gmres_iterations=it, paths=list(mono.stats()["paths"]))
    rec["sequential"] = dict(converged=ok, gmres_iterations_summed=its_seq, solves=K)
    yl = y_all.numpy()[-N:]
    rec["native_vs_sequential_maxabs"] = float(np.abs(yl - seq.numpy()).max())
    rec["native"].update(timed(ctx, reps, lambda: mono(xv)))
    rec["sequential"].update(timed(ctx, max(3, reps // 3), lambda: PO.monodromy_sequential(po, u, T, pv, xv, ls)))
    rec["sequential_over_native"] = rec["sequential"]["median_ms"] / rec["native"]["median_ms"]
    ctx.prof_enable(True)
    Y = hip.HipVec.from_numpy(ctx, np.random.default_rng(1).standard_normal(K * N))
    out = Y.similar()
    P = PO.PoTrapIvpPreconditioner(po, r, PARS["nu"], T)
    ms, _ = scope(ctx, "monodromy_march", reps, lambda: PO.ivp_march(po, u, T, pv, Y, out))
    rec["march_kernel"] = dict(ms=ms, bytes=3 * 8.0 * K * N, TBps=3 * 8.0 * K * N / (ms * 1e-3) / 1e12)
    ms, _ = scope(ctx, "monodromy_timesolve", reps, lambda: P.ldiv(Y))
    rec["timesolve_kernel"] = dict(ms=ms, bytes=2 * 8.0 * K * N, TBps=2 * 8.0 * K * N / (ms * 1e-3) / 1e12)
    ms, per = scope(ctx, "monodromy_march", reps, lambda: mono(xv))
    rec["march_in_solve"] = dict(ms=ms, launches_per_application=per)
    ctx.prof_enable(False)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "floquet_probe.jsonl"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--sizes", default="41x21,256x256")
    args = ap.parse_args()
    from bk_amd import hip
    from bk_amd import periodic_orbit as PO
    ctx = hip.Context(0)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fo:
        for s in args.sizes.split(","):
            dims = tuple(int(v) for v in s.split("x"))
            rec = one_size(ctx, hip, PO, dims, 30, 0.01, args.reps)
            print(json.dumps(rec))
            fo.write(json.dumps(rec) + "\n")
            fo.flush()
    ctx.close()


if __name__ == "__main__":
    main()
