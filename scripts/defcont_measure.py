#!/usr/bin/env python
"""Measurements of the deflated-continuation passes (DESIGN: deflated continuation), one process, library profiling scopes
(bk_prof: HIP events around each launch):

  1. bk_vec_perturb next to the in-place passes that move the same 16 n bytes (bk_vec_scale; bk_vec_axpby with x = y), and
     bk_deflation_dist with 8 roots next to bk_deflation_dots without h (the same 9 read streams), at n = 2^24 on plain buffers
     and on the states of a 4096 x 4096 Swift-Hohenberg problem, with bk_vec_copy as the copy ceiling
        -> <out>/defcont_kernel_stats.txt
  2. deflated_continuation end to end at 256 x 256 (noise amplitude 0.1 and 1.6): steps, branches, Newton and linear iterations, and the share of the wall time
     spent in the deflation passes and the perturbation
        -> <out>/defcont_run.json

Usage: python scripts/defcont_measure.py [--out DIR] [--reps 10]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(ctx, name, reps, call):
    """Average ms of the scope ``name`` over ``reps`` calls after three warm-up calls; (ms, min over three such rounds)."""
    for _ in range(3):
        call()
    rounds = []
    for _ in range(3):
        ctx.prof_reset()
        for _ in range(reps):
            call()
        ctx.sync()
        g = ctx.prof_get(name)
        assert g["calls"] == reps, (name, g)
        rounds.append(g["ms"] / reps)
    return float(np.median(rounds)), float(min(rounds))


def kernel_stats(ctx, hip, out, reps):
    n = 1 << 24
    rng = np.random.default_rng(0)
    lines = [f"# n = 2^24 doubles per stream, {reps} calls per round, median (min) of three rounds, library profiling scopes",
             "# pass | streams | bytes | us | TB/s | fraction of bk_vec_copy"]
    prob = hip.SwiftHohenberg(ctx, (4096, 4096), (np.pi, np.pi), l=0.1, nu=1.3)
    for label, mk in [("plain 2^24", lambda: hip.HipVec.from_numpy(ctx, rng.random(n) - 0.5)),
                      ("SH 4096 x 4096", lambda: prob.vec(rng.random(n) - 0.5))]:
        x, y = mk(), mk()
        roots = [mk() for _ in range(8)]
        op = hip.DeflationOperator(2, 1.0, roots, autodiff=True)
        lib, h = ctx.lib, ctx.h
        cases = [
            ("bk_vec_copy (ceiling)", "blas1", 2, lambda: ctx.check(lib.bk_vec_copy(h, n, x.t.data_ptr(), y.t.data_ptr()))),
            ("bk_vec_scale in place", "blas1", 2, lambda: ctx.check(lib.bk_vec_scale(h, n, 1.0000001, y.t.data_ptr()))),
            ("bk_vec_axpby in place (x = y)", "blas1", 2,
             lambda: ctx.check(lib.bk_vec_axpby(h, n, 0.5, y.t.data_ptr(), 0.5, y.t.data_ptr()))),
            ("bk_vec_perturb", "vec_perturb", 2, lambda: ctx.check(lib.bk_vec_perturb(h, n, y.t.data_ptr(), 1e-9, 7, 0))),
            ("bk_deflation_dots, 8 roots, no h", "deflation_dots", 9, lambda: op.dots(x)),
            ("bk_deflation_dist, 8 roots", "deflation_dist", 9, lambda: op.dist(x)),
        ]
        lines.append(f"## {label}")
        ceiling = None
        for name, scope, streams, call in cases:
            ms, mn = timed(ctx, scope, reps, call)
            tbs = 8.0 * n * streams / (ms * 1e-3) / 1e12
            ceiling = tbs if ceiling is None else ceiling
            lines.append(f"{name} | {streams} | {8 * n * streams} | {ms * 1e3:.1f} ({mn * 1e3:.1f}) | {tbs:.2f} | {tbs / ceiling:.2f}")
        del x, y, roots, op
    with open(os.path.join(out, "defcont_kernel_stats.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def run_256(ctx, hip, amp, max_iter_defop, steps):
    from bk_amd import continuation as Cn
    from bk_amd import deflated_continuation as DC
    dims, ls, nu, l0 = (256, 256), (np.pi, np.pi), 1.3, 0.0209
    prob = hip.SwiftHohenberg(ctx, dims, ls, l=l0, nu=nu)
    lsv = hip.GMRESKrylovKit(dim=40, rtol=1e-10, atol=1e-13, maxiter=50, Pl=hip.DCTPreconditioner(prob, 1.0))
    op = hip.DeflationOperator(2, 1.0, [prob.vec(np.zeros(prob.nglobal))], autodiff=True)
    alg = DC.DefCont(deflation_operator=op, max_branches=6, max_iter_defop=max_iter_defop,
                     perturb_solution=DC.uniform_perturbation(amp, 2024))
    cp = Cn.ContinuationPar(ds=0.01, p_min=-1.0, p_max=1.0, max_steps=steps,
                            newton_options=Cn.NewtonPar(tol=1e-10, max_iterations=15, linsolver=lsv))
    ctx.prof_reset()
    t0 = time.perf_counter()
    res = DC.deflated_continuation(prob, alg, cp, normC=Cn.norminf, native=True)
    ctx.sync()
    wall = time.perf_counter() - t0
    scopes = {k: ctx.prof_get(k) for k in ("deflation_dots", "deflation_dist", "vec_perturb")}
    defl_ms = sum(v["ms"] for v in scopes.values())
    rec = dict(grid=list(dims), ls=list(ls), nu=nu, l0=l0, ds=cp.ds, steps=cp.max_steps, max_branches=alg.max_branches,
               max_iter_defop=alg.max_iter_defop, newton_max_iterations=15, tol=1e-10, amp=amp, seed=2024,
               branches=len(res.branches), active=sum(b.active for b in res.branches),
               points=[len(b.param) for b in res.branches], first_param=[b.param[0] for b in res.branches],
               normu_first=[b.normu[0] for b in res.branches],
               newton_branch=sum(sum(b.itnewton) for b in res.branches), linear_branch=sum(sum(b.itlinear) for b in res.branches),
               seeks=len(res.seeks), seeks_accepted=sum(s["reason"] == 0 for s in res.seeks),
               seek_reasons=[s["reason"] for s in res.seeks], newton_seek=sum(s["itnewton"] for s in res.seeks),
               linear_seek=sum(s["itlinear"] for s in res.seeks), wall_s=wall, timing=res.timing, scopes=scopes,
               deflation_ms=defl_ms, deflation_share_of_wall=defl_ms * 1e-3 / wall)
    print(json.dumps(rec))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out"))
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    import bk_amd  # noqa: F401
    from bk_amd import hip
    ctx = hip.Context(0)
    ctx.prof_enable(True)
    kernel_stats(ctx, hip, a.out, a.reps)
    # the example's amplitude, and the amplitude that gives the 256 x 256 noise the low-mode content 0.1 has on 16 x 16
    # (the first Newton step removes the grid-scale part; what is left scales with amp / sqrt(points))
    runs = [run_256(ctx, hip, 0.1, 10, 2), run_256(ctx, hip, 1.6, 10, 2)]
    with open(os.path.join(a.out, "defcont_run.json"), "w") as f:
        json.dump(runs, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
