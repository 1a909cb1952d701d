#!/usr/bin/env python
"""Writes tests/golden/sh_cusp_128x2.npz: a cusp on a fold curve of the quadratic-cubic Swift-Hohenberg equation, located by the
dense CPU restatement (tests/cusp_ref.py) and the oracle only.

Grid: oracle.operators.SwiftHohenberg((128, 2), (4 pi, 4 pi / 128)) -- hx = hy, Neumann, the states y-uniform.  A wall-attached
localized state (guess 1.3 cos(x + lx) for x + lx < 9, Newton at l = -0.30, nu = 1.8) snakes in l; its third fold
(l = -0.2723 at nu = 1.8) and the next one annihilate in a cusp as nu decreases.  The fold is followed in nu downward (PALC on the
minimally augmented fold system) until CP = tau.nu changes sign; the crossing is bisected by the sign of b2 = <p, B(q, q)> of the
state itself and the cusp normal form evaluated there (b2 and tau.nu vanish together: a genuine cusp).

Stored: a refined fold point three to five steps before the sign change (u, l, nu, the normalised null vector v = w), the ds sequence
that reaches the crossing from it, and the dense cusp (u, q, l, nu, c, b2, H2) with the options that located it.

    python scripts/gen_sh_cusp_fixture.py [--check]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cusp_ref as Cr                                     # noqa: E402
import minaug_fold_ref as R                               # noqa: E402
from oracle import bordered, operators, palc              # noqa: E402

DIMS, LS = (128, 2), (4 * np.pi, 4 * np.pi / 128)
NU0 = 1.8
STEPS_BEFORE = (5, 4, 3)                                  # the stored fold point: this many steps before the sign change of CP
CURVE = dict(ds=-0.01, dsmin=1e-4, dsmax=0.05, p_min=1.0, p_max=2.5, max_iterations=10)
TOL = 1e-10                                               # |G|_inf of the fold system: J \ F on the singular J stalls near 2e-11
DENSE = dict(tol=TOL, n_inversion=20, max_bisection_steps=60, dsmin_bisection=1e-6)
OUT = os.path.join(ROOT, "tests", "golden", "sh_cusp_128x2.npz")


def snaking_fold(op, which=2):
    """The ``which``-th turn in l of the localized state's branch at nu = NU0 (upward from l = -0.30): (x, l, tangent guess)."""
    x = operators.grid_axes(DIMS, LS)[0] + LS[0]
    u0 = np.tile(np.where(x < 9, 1.3 * np.cos(x), 0.0), DIMS[1])
    prob = palc.Problem(lambda u, p: op.F(u, p, NU0), lambda u, p: op.J(u, p, NU0), dparam_factor=lambda u, p: u)
    bls = lambda *a, **k: bordered.bordering_bls(bordered.default_ls, *a, check_precision=False, **k)
    br = palc.continuation(prob, u0, -0.30, ls=bordered.default_ls, bls=bls, ds=0.005, dsmax=0.02, dsmin=1e-5, p_min=-1.0, p_max=1.0,
                           max_steps=40, keep_solutions=True, normC=palc.norminf, tol=1e-10)
    dp = np.diff(br.param)
    k = [i + 1 for i in range(len(dp) - 1) if dp[i] * dp[i + 1] < 0][which]
    tau = br.sol[k + 1] - br.sol[k - 1]
    return br.sol[k], float(br.param[k]), tau / np.linalg.norm(tau)


def generate():
    op = operators.SwiftHohenberg(DIMS, LS)
    x, l, tau = snaking_fold(op)
    model = Cr.sh_cusp_model(op, "sh", dict(l=l, nu=NU0), "l", "nu")
    sn = R.newton_fold(model, x, l, tau, tau, p2=NU0, tol=TOL, max_iterations=20, normN=palc.norminf)
    assert sn["converged"], sn["residuals"]
    b = sn["v"] / np.linalg.norm(sn["v"])
    # the curve down to the sign change of CP, adaptive steps
    br = Cr.continuation_fold(model, sn["u"], sn["p"], NU0, b, b, max_steps=40, tol=TOL, detect_codim2=1, **CURVE)
    i = br["specialpoint"][0]["idx"]
    # The dense cusp is located by the sign of b2 of the state itself (cusp_ref: bisect = "b2"), not by the secant tangent the
    # library's event uses.  A bisection in PALC steps can still stall short of the crossing -- after an inversion the halved steps
    # that remain add up to the ds of the step that passed it, and where the curve bends that step's chord is longer than its ds
    #  -- so the stored start is the first of five, four, three steps before the sign change from which it closes in.
    for before in STEPS_BEFORE:
        s = i - before
        # the stored fold point, refined at its own nu, and the steps the curve took from there to the sign change
        Xs, nus = br["X"][s], br["p2"][s]
        f = R.newton_fold(model, Xs[:-1], Xs[-1], b, b, p2=nus, tol=TOL, max_iterations=20, normN=palc.norminf)
        assert f["converged"], f["residuals"]
        v = f["v"] / np.linalg.norm(f["v"])
        dss = [float(d) for d in br["ds"][s + 1:i + 1]]
        # the same curve with the prescribed steps, the crossing bisected
        kw = {k_: v_ for k_, v_ in CURVE.items() if k_ not in ("dsmin", "dsmax")}
        kw.update(ds=dss[0], max_steps=len(dss), ds_sequence=dss, detect_codim2=2, bisect="b2", **DENSE)
        br3 = Cr.continuation_fold(model, f["u"], f["p"], nus, v, v, **kw)
        sps = br3["specialpoint"]
        print(f"start {before} steps before: " + ", ".join(f"idx {q['idx']} b2 {q['b2']:+.2e} CP {q['CP']:+.2e} steps {q['bisection_steps']} "
                                                            f"inversions {q['n_inversion']} {q['status']}" for q in sps))
        if len(sps) == 1 and sps[0]["idx"] == len(dss) and abs(sps[0]["CP"]) <= 1e-3 and abs(sps[0]["b2"]) <= 1e-6:
            break
    else:
        raise SystemExit("no start closes in on the cusp")
    sp = sps[0]
    Xc, nuc = sp["X"], sp["p2"]
    pars = model.at(Xc[-1], nuc)
    q, p = Cr.null_vectors(model.J(Xc[:-1], pars))
    if q @ v < 0:
        q, p = -q, -p
    nf = Cr.cusp_normal_form(model, Xc[:-1], pars, q, p)
    eig = np.sort(np.abs(np.linalg.eigvalsh(model.J(Xc[:-1], pars).toarray())))[:3]
    return dict(dims=np.array(DIMS), ls=np.array(LS), fold_u=f["u"], fold_l=f["p"], fold_nu=nus, fold_v=v, ds_sequence=np.array(dss),
                curve_l=np.array(br3["p1"]), curve_nu=np.array(br3["p2"]), curve_b2=np.array(br3["b2"]), curve_CP=np.array(br3["CP"]),
                cusp_u=Xc[:-1], cusp_q=q, cusp_l=Xc[-1], cusp_nu=nuc, cusp_c=nf["c"], cusp_b2=nf["b2"], cusp_H2=nf["H2"],
                cusp_CP=sp["CP"], cusp_eig=eig, cusp_bisection_steps=sp["bisection_steps"],
                dense_tol=DENSE["tol"], dense_n_inversion=DENSE["n_inversion"], dense_max_bisection_steps=DENSE["max_bisection_steps"],
                dense_dsmin_bisection=DENSE["dsmin_bisection"], max_iterations=CURVE["max_iterations"], p_min=CURVE["p_min"],
                p_max=CURVE["p_max"])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare with the stored file instead of writing it")
    a = ap.parse_args()
    d = generate()
    print(f"fold point  l = {float(d['fold_l']):.10f}  nu = {float(d['fold_nu']):.10f}   ds = {d['ds_sequence']}")
    for l_, n_, b_, c_ in zip(d["curve_l"], d["curve_nu"], d["curve_b2"], d["curve_CP"]):
        print(f"   l = {l_:+.6f}  nu = {n_:.6f}  b2 = {b_:+.5f}  CP = {c_:+.4f}")
    print(f"cusp        l = {float(d['cusp_l']):.10f}  nu = {float(d['cusp_nu']):.10f}  c = {float(d['cusp_c']):.8f}  "
          f"b2 = {float(d['cusp_b2']):.2e}  CP = {float(d['cusp_CP']):.2e}  max|u| = {np.abs(d['cusp_u']).max():.3f}  "
          f"|eig J| = {d['cusp_eig']}  bisection steps {int(d['cusp_bisection_steps'])}")
    if a.check:
        old = np.load(OUT)
        for k_ in d:
            err = np.abs(np.asarray(d[k_], dtype=float) - old[k_]).max()
            print(f"   {k_:28s} max |new - stored| = {err:.2e}")
    else:
        np.savez(OUT, **d)
        print("wrote", OUT, os.path.getsize(OUT), "bytes")
