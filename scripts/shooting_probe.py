"""One GPU run that records what the shooting path costs: per grid and segment count the time of one flow step and of
one application of the shooting Jacobian with the base trajectory stored and recomputed, and of one application of the monodromy.
Two figures are DERIVED, not measured: launches_per_step_by_formula is the count flow_march adds up itself (12 per step), and
op_stored_ms_per_step is the stored application divided by its step count -- a tangent-only march plus the closing pass, its
reduction and the call.  One process; run it under `timeout`.  Writes profiles/shooting_probe.jsonl anew (or the file given as
the first argument)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bk_amd import hip, shooting  # noqa: E402

LS = (np.pi, np.pi / 2)
PARS = dict(r=1.2, mu=0.1, nu=1.0, c3=-1.0, c5=1.0, gamma=0.0)
PV = [PARS[k] for k in ("r", "mu", "nu", "c3", "c5", "gamma")]
NSTEPS, T = 64, 6.9


def timed(ctx, f, reps):
    f()
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        f()
    ctx.sync()
    return (time.perf_counter() - t0) / reps * 1e3


def main(out):
    ctx = hip.Context(0)
    rng = np.random.default_rng(0)
    with open(out, "w") as fh:
        for dims in ((41, 21), (256, 256)):
            prob = hip.CGL2d(ctx, dims, LS, **PARS)
            for M in (1, 4):
                sh = shooting.ShootingProblem(prob, M, NSTEPS)
                x = sh.vec(0.5 * rng.standard_normal(sh.n) / np.sqrt(dims[0]))
                sh.update_section(x, T, PV)
                flow = shooting.Flow(prob, M)
                reps = 5 if dims[0] > 64 else 20
                l0 = flow.stats()["launches"]
                ms_flow = timed(ctx, lambda: flow.evolve(x, T / M, NSTEPS, PV), reps)
                launches = (flow.stats()["launches"] - l0) / (reps + 1) / NSTEPS
                dx = hip.BorderedArray(sh.vec(rng.standard_normal(sh.n)), 0.3)
                rec = dict(dims=dims, M=M, nsteps=NSTEPS, flow_step_ms=ms_flow / NSTEPS, launches_per_step_by_formula=launches)
                for key, store in (("stored", 1.0), ("recomputed", 0.0)):
                    ctx.set_option("shooting_store", store)
                    J = sh.jacobian(x, T, PV)
                    rec[f"op_{key}_ms"] = timed(ctx, lambda: J(dx), reps)
                    assert J.stats()["stored"] == bool(store)
                ctx.set_option("shooting_store", 1.0)
                rec["op_stored_ms_per_step"] = rec["op_stored_ms"] / NSTEPS
                mono = shooting.ShootingMonodromy(sh, x, T, PV)
                v = prob.vec(rng.standard_normal(prob.nlocal))
                rec["monodromy_ms"] = timed(ctx, lambda: mono(v), reps)
                rec["store_MiB"] = 2 * NSTEPS * sh.n * 8 / 2 ** 20
                print(json.dumps(rec))
                fh.write(json.dumps(rec) + "\n")
    ctx.close()


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "shooting_probe.jsonl"))
