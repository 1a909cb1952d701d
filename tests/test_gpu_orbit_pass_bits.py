"""Bitwise pin of the periodic-orbit marching passes and time solves built on the skeleton of csrc/potrap_pw.h (bk_potrap_residual,
bk_potrap_jvp, bk_potrap_jvp_adjoint, bk_potrap_fold_border, bk_potrap_ivp_march, bk_potrap_dparam and the forward, adjoint and
initial-value space-time preconditioners).

The rows of a marching pass are promised independent of the chunking and its sums bitwise reproducible for a given chunk count;
both are the walk, the grid mapping and the order of the fma calls of the shared skeleton, which the accuracy bounds of the other
tests (16 eps units per entry, 4 n eps sum |terms| per sum) do not see.  tests/golden/orbit_pass_bits.json holds what the library
computed BEFORE the passes were moved onto the shared skeleton: every sum as float.hex(), every written vector as the SHA-256 of
its bytes.  A key that is missing fails.

Inputs are exact integer arithmetic, ((i a + b) mod 1000003) / 1000003 - 0.5 with one (a, b) per stream, so they do not depend
on a random generator.  Shapes, the smallest that reach each branch of the skeleton (tiles of 256 grid points, K = M - 1 rows):
  12 x 9, M = 3      K = 2, the smallest cycle, prev(0) = 1 = next(0); 108 points, one partial tile; potrap_chunks 1, 2, default
  16 x 12, M = 12    K = 11; potrap_chunks 1, 2, 4, 11 and the default: C = 11, 6 / 5, 3 / 3 / 3 / 2, 1
  23 x 17, M = 9     391 points: two tiles, the second ragged; potrap_chunks 1, 3 and the default
  32 x 16, M = 5     512 points: two exact tiles, the idx < n guard is never false; potrap_chunks 1, 4
The default chunk count depends on the number of compute units, so under it only the rows are pinned; the sums are pinned under
the forced counts.  The preconditioners are pinned once per shape at the (a, b, T) of the preconditioner tests, a = r_hopf - 0.05,
b = nu, T = 2 pi, which passes both guards.

Re-record (only from a library whose bits are the reference):  BKHIP_LIB=<libbkhip.so> python tests/test_gpu_orbit_pass_bits.py --record
"""
import hashlib
import json
import math
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "orbit_pass_bits.json")
PRIME = 1000003
LS = (np.pi, np.pi / 2)
CGL_PARS = dict(r=0.3, mu=0.1, nu=1.0, c3=-1.0, c5=1.0, gamma=0.2)
PNAMES = ("r", "mu", "nu", "c3", "c5", "gamma")
T, DT, TAU, VT = 5.75, 0.375, -1.25, 0.625
CASES = [((12, 9), 3, (1, 2, 0)), ((16, 12), 12, (1, 2, 4, 11, 0)), ((23, 17), 9, (1, 3, 0)), ((32, 16), 5, (1, 4))]
GROUPS = [f"{d[0]}x{d[1]}-M{M}" for d, M, _ in CASES]


def _stream(k, n):
    """Stream k of n elements: exact in int64, one division in float64."""
    i = np.arange(n, dtype=np.int64)
    return ((i * (12347 + 7919 * k) + (101 + 1009 * k)) % PRIME).astype(np.float64) / PRIME - 0.5


def _hex(*vals):
    return [float(v).hex() for v in vals]


def _sha(*vecs):
    return [hashlib.sha256(v.numpy().tobytes()).hexdigest() for v in vecs]


def _group(ctx, name):
    import potrap_ref as R
    from bk_amd import hip, periodic_orbit as po_
    dims, M, chunks = next(c for c in CASES if f"{c[0][0]}x{c[0][1]}-M{c[1]}" == name)
    prob = hip.CGL2d(ctx, dims, LS, **CGL_PARS)
    pv = [CGL_PARS[k] for k in PNAMES]
    po = po_.PeriodicOrbitTrap(prob, M)
    n, KN = po.n, po.N * (M - 1)
    U, X, W, V, phi, xpi = (po.vec(_stream(k, n)) for k in range(6))
    Y, F = po.vec(_stream(6, KN)), po.vec(_stream(7, n))
    po.set_section(phi, xpi)
    out = {}
    try:
        for c in chunks:
            ctx.set_option("potrap_chunks", float(c))
            sums = c != 0                            # the default count follows the device: rows only
            for key, r in (("residual", po.residual(U, T, pv)), ("jvp", po.jvp(U, T, pv, X, DT)),
                           ("jvp_adjoint", po.jvp_adjoint(U, T, pv, W, TAU))):
                out[f"c{c}/{key}"] = _sha(r.u) + (_hex(r.p) if sums else [])
            for lens in ("r", "c5"):
                sx, sp = po.fold_border(U, T, pv, PNAMES.index(lens), hip.BorderedArray(V, VT), W)
                out[f"c{c}/fold_border/{lens}"] = _sha(sx.u) + (_hex(sx.p, sp) if sums else [])
            out[f"c{c}/ivp_march"] = _sha(po_.ivp_march(po, U, T, pv, Y))
            out[f"c{c}/dparam/c5"] = _sha(po.dparam(U, T, pv, PNAMES.index("c5")))
    finally:
        ctx.set_option("potrap_chunks", 0.0)
    a, b, Tp = -R.Model(dims, LS).lam.max() - 0.05, CGL_PARS["nu"], 2 * math.pi
    out["precond/forward"] = _sha(po_.PoTrapPreconditioner(po, a, b).set_period(Tp).ldiv(F))
    out["precond/adjoint"] = _sha(po_.PoTrapPreconditioner(po, a, b, adjoint=True).set_period(Tp).ldiv(F))
    out["precond/ivp"] = _sha(po_.PoTrapIvpPreconditioner(po, a, b, Tp).ldiv(Y))
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_file_names_its_source(golden):
    assert "parent commit" in golden["recorded_from"] and "MI355X" in golden["recorded_from"]


@pytest.mark.parametrize("name", GROUPS)
def test_orbit_pass_bits(ctx, golden, name):
    got = _group(ctx, name)
    assert len(got) >= 17
    bad = {k: (v, golden.get(f"{name}/{k}")) for k, v in got.items() if golden.get(f"{name}/{k}") != v}
    assert not bad, f"{len(bad)} of {len(got)} entries differ from (or are missing in) the recorded bits: {sorted(bad)[:8]}"


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], "usage: BKHIP_LIB=<reference libbkhip.so> python tests/test_gpu_orbit_pass_bits.py --record"
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from bk_amd import hip
    c = hip.Context(0)
    rec = {f"{g}/{k}": v for g in GROUPS for k, v in _group(c, g).items()}
    c.close()
    rec["recorded_from"] = ("libbkhip.so built from commit 4fe6e94, the parent commit of the change that moved the orbit passes "
                            "onto the shared marching skeleton, run on the MI355X")
    with open(GOLDEN, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(rec)} entries -> {GOLDEN}")
