"""CPU restatement of the cusp on fold curves for the tests (test side only): the test_bt_cusp event of
src/codim2/MinAugFold.jl:432,551-576, its bisection (locate_event!, src/events/EventDetection.jl:28-175, as
bk_amd.codim2._locate_event runs it) and cusp_normal_form (src/codim2/NormalForms.jl:15-123; Kuznetsov 1999).

Generic: a minaug_fold_ref.FoldModel (F, J, J' -- default the transpose, so non-symmetric models work --, B = d2F) wrapped with
C = d3F.  Every linear solve is direct, so the restatement carries no Krylov tolerance.

  CuspModel            FoldModel + d3F
  null_vectors         q = zeta of J, p = zeta* of J', |q| = 1, <q, p> = 1
  b2_bordered          b2 = <p, B(q, q)> from the unnormalised bordered vectors v, w of a fold-curve point
  cusp_normal_form     (b2, c, H2) at a fold with normalised q, p
  continuation_fold    minaug_fold_ref.continuation_fold with b2 per point, the sign changes of CP as "cusp" points and their
                       bisection -- the loop of bk_amd.codim2.continuation_fold(detect_codim2 = 0 | 1 | 2)
  cusp_dots, cusp_rhs, cusp_contract   the device passes of csrc/cusp.hip element by element, in their operation order
"""
from __future__ import annotations

import math

import numpy as np

import minaug_fold_ref as R
from oracle import palc


class CuspModel:
    """A FoldModel and its third derivative d3F(x, pars, dx1, dx2, dx3); everything else is the wrapped model's."""

    def __init__(self, fold_model: R.FoldModel, d3F):
        self.fold, self.d3F = fold_model, d3F

    def __getattr__(self, name):
        return getattr(self.fold, name)


def sh_cusp_model(op, kind, pars, lens1, lens2=None) -> CuspModel:
    """CuspModel of an oracle SwiftHohenberg / SwiftHohenberg1D operator: d3F = t(u) dx1 dx2 dx3 with t = h'."""
    names = list(pars)

    def d3F(x, q, dx1, dx2, dx3):
        return R.horner(sh_poly_d3(kind, q[names[1]]), x) * dx1 * dx2 * dx3

    return CuspModel(R.sh_model(op, kind, pars, lens1, lens2), d3F)


def sh_poly_d3(kind, nu):
    """Coefficients (c0, c1, c2, c3) of t(u), d3F = t(u) dx1 dx2 dx3: "sh" t = -6, "sh1d" t = 6 nu - 60 u^2."""
    return np.array([-6.0, 0.0, 0.0, 0.0]) if kind == "sh" else np.array([6.0 * nu, 0.0, -60.0, 0.0])


def null_vectors(J, Jt=None):
    """(q, p): q the eigenvector of J for the eigenvalue nearest 0 with |q| = 1, p that of J' scaled to <q, p> = 1
    (NormalForms.jl:76-98)."""
    J = np.asarray(J.todense()) if hasattr(J, "todense") else np.asarray(J)
    Jt = J.T if Jt is None else (np.asarray(Jt.todense()) if hasattr(Jt, "todense") else np.asarray(Jt))
    w, V = np.linalg.eig(J)
    q = np.real(V[:, np.argmin(np.abs(w))])
    q = q / np.linalg.norm(q)
    wt, Vt = np.linalg.eig(Jt)
    p = np.real(Vt[:, np.argmin(np.abs(wt))])
    return q, p / np.dot(q, p)


def b2_bordered(model, x, q, v, w):
    """<p, B(q, q)> with q = v / |v|, p = w / <q, w>, written as the host forms it from bk_cusp_dots:
    <w, B(v, v)> / (|v| <v, w>)."""
    return float(np.dot(w, model.d2F(x, q, v, v)) / (np.linalg.norm(v) * np.dot(v, w)))


def cusp_normal_form(model, x, pars, q, p):
    """cusp_normal_form (:100-123): dict(b2, c, H2, s) at the fold (x, pars) with |q| = 1, <q, p> = 1."""
    if not abs(np.dot(q, p) - 1) <= 1e-8:
        raise ValueError(f"Error of precision in normalization: <q, p> = {np.dot(q, p)}, expected 1")
    J = model.J(x, pars)
    J = np.asarray(J.todense()) if hasattr(J, "todense") else np.atleast_2d(np.asarray(J, dtype=float))
    n = q.shape[0]
    h2 = model.d2F(x, pars, q, q)
    b2 = float(np.dot(p, h2))
    rhs = b2 * q - h2
    M = np.block([[J, q.reshape(-1, 1)], [p.reshape(1, -1), np.zeros((1, 1))]])
    y = np.linalg.solve(M, np.append(rhs, 0.0))
    H2 = y[:n]
    c = (float(np.dot(p, model.d3F(x, pars, q, q, q))) + 3.0 * float(np.dot(p, model.d2F(x, pars, q, H2)))) / 6.0
    return dict(b2=b2, c=c, H2=H2, s=float(y[n]))


def cusp_at_fold(model, x, pars):
    """cusp_normal_form at the fold (x, pars) with q, p from the eigenvectors of J and J'."""
    q, p = null_vectors(model.J(x, pars), model.Jt(x, pars))
    return cusp_normal_form(model, x, pars, q, p)


# ---------------------------------------------------------------------------------------------- the curve
def continuation_fold(model, x0, p1, p2, a, b, *, ds, dsmin=1e-4, dsmax=0.1, a_ctrl=0.5, theta=0.5, p_min=-np.inf,
                      p_max=np.inf, max_steps=100, eta=150.0, tol=1e-12, max_iterations=25, normC=palc.norminf, ds_sequence=None,
                      detect_codim2=0, n_inversion=2, max_bisection_steps=25, dsmin_bisection=1e-16, bisect="CP"):
    """minaug_fold_ref.continuation_fold (the same loop, statement by statement) with the cusp event: per point b2; with
    detect_codim2 >= 1 every sign change of CP = tau.p2 between consecutive points as a special point of type "cusp" (status
    "guess"), with 2 bisected along the curve.  The curve continues from its pre-bisection state.  ``bisect`` = "CP": the
    bisection follows the sign of the secant tangent's p2 component, as the library does; "b2": the sign of b2 of the state
    itself, which vanishes at the same point of a genuine cusp and has no secant in it (an independent, sharper location).
    Returns dict(p1, p2, BT, CP, b2, ds, itnewton, X, specialpoint)."""
    st = dict(a=np.asarray(a, dtype=float).copy(), b=np.asarray(b, dtype=float).copy())

    def G(X, p):
        return R._G(model, X, p, st["a"], st["b"])

    def linsolve(X, p, v, w, Rr):
        dX, dsig = R.fold_linsolve(model, X[:-1], model.at(X[-1], p), v, w, Rr[:-1], Rr[-1])
        return np.append(dX, dsig)

    def dGdp2(X, p, v, w):
        x, q = X[:-1], model.at(X[-1], p)
        return np.append(model.dFdp(x, q, model.lens2), -np.dot(w, model.dJvdp(x, q, model.lens2, v)))

    def newton(X, p):
        Rr, v, w = G(X, p)
        res = [normC(Rr)]
        while len(res) <= max_iterations and res[-1] > tol:
            X = X - linsolve(X, p, v, w, Rr)
            Rr, v, w = G(X, p)
            res.append(normC(Rr))
        return X, res[-1] < tol, len(res) - 1

    def newton_palc(z0, tau, zp, ds_):
        N = lambda X, p: palc.arc_length_eq(X, z0[0], p - z0[1], tau[0], tau[1], theta, ds_)
        X, p = zp[0].copy(), float(zp[1])
        Rr, v, w = G(X, p)
        rn = N(X, p)
        res = [max(normC(Rr), abs(rn))]
        n_ = X.shape[0]
        while len(res) <= max_iterations and res[-1] > tol:
            x1, dx = linsolve(X, p, v, w, Rr), linsolve(X, p, v, w, dGdp2(X, p, v, w))      # BEC, check_precision = false
            dl = (rn - np.dot(tau[0], x1) / n_ * theta) / (tau[1] * (1 - theta) - np.dot(tau[0], dx) / n_ * theta)
            X = X - (x1 - dl * dx)
            p = float(np.clip(p - dl, p_min, p_max))
            Rr, v, w = G(X, p)
            rn = N(X, p)
            res.append(max(normC(Rr), abs(rn)))
        return (X, p), res[-1] < tol, len(res) - 1

    def b2_at(X, p):
        _, v, w = G(X, p)
        return b2_bordered(model, X[:-1], model.at(X[-1], p), v, w)

    def update(X, p):
        _, v, w = G(X, p)
        b2 = b2_bordered(model, X[:-1], model.at(X[-1], p), v, w)
        zs, z = w / np.linalg.norm(w), v / np.linalg.norm(v)
        st["a"], st["b"] = zs, z
        return float(np.dot(zs, z)), b2

    def coords(z):
        return (float(z[0][-1]), float(z[1]))

    def locate(z, z_old, tau, ds_taken, ev_after):
        """bk_amd.codim2._locate_event with the event tau.p2 (or b2); a, b stay those of the point after the crossing.  ``reach``:
        |ds| of the last step that passed the crossing (the first, halved, step when none did)."""
        reach = abs(ds_taken) / 2.0
        zc, zp_ = (z[0].copy(), z[1]), (z_old[0].copy(), z_old[1])
        tau_b = tau
        ends, values = [coords(z_old), coords(z)], [math.nan, ev_after]
        ind, sign = 1, ev_after > 0
        ds_b = -ds_taken / 2.0
        ev, steps, n_inv, status = ev_after, 0, 0, "max_bisection_steps"
        while steps < max_bisection_steps:
            if n_inv >= n_inversion:
                status = "n_inversion"
                break
            if abs(ds_b) < dsmin_bisection:
                status = "dsmin_bisection"
                break
            sol, conv, _ = newton_palc(zc, tau_b, palc.add_tangent(zc, tau_b, ds_b), ds_b)
            if not conv:
                status = "unconverged"
                break
            zp_, zc = zc, sol
            steps += 1
            tau_b = palc.secant_tangent(zc, zp_, ds_b, theta)
            ev = float(tau_b[1]) if bisect == "CP" else b2_at(*zc)
            if (ev > 0) == sign:
                ds_b /= 2.0
            else:
                reach = abs(ds_b)
                ds_b /= -2.0
                n_inv += 1
                ind = 1 - ind
                sign = ev > 0
            ends[ind] = coords(zc)
            values[ind] = ev
        return dict(z=zc, value=ev, ends=ends, values=values, bisection_steps=steps, n_inversion=n_inv, status=status, reach=reach,
                    tau=tau_b)

    out = dict(p1=[], p2=[], BT=[], CP=[], b2=[], ds=[], itnewton=[], X=[], specialpoint=[])

    def record(z, bt_b2, cp, ds_, itn):
        out["p1"].append(float(z[0][-1])); out["p2"].append(float(z[1])); out["BT"].append(bt_b2[0]); out["CP"].append(float(cp))
        out["b2"].append(bt_b2[1]); out["ds"].append(ds_); out["itnewton"].append(itn); out["X"].append(z[0].copy())

    before = []                                      # (z_old, ds) of the previous step: the state two points back

    def after_record(z, z_old, tau, ds_taken):
        # CP of a point is the secant over the step that led to it, so a sign change between the points i - 1 and i puts the
        # extremum of p2 between the points i - 2 and i: the bisection starts from that bracket
        z_far, ds_far = before.pop() if before else (z_old, 0.0)
        before.append(((z_old[0].copy(), z_old[1]), ds_taken))
        cp_ = out["CP"]
        if not detect_codim2 or len(cp_) < 2 or not cp_[-2] * cp_[-1] < 0:
            return
        z_old, ds_taken = z_far, ds_taken + ds_far
        i = len(cp_) - 1
        sp = dict(type="cusp", idx=i, step=i, p1=float(z[0][-1]), p2=float(z[1]), end_points=(coords(z_old), coords(z)), CP=cp_[-1],
                  CP_interval=(cp_[-2], cp_[-1]), b2=out["b2"][-1], X=z[0].copy(), a=st["a"].copy(), b=st["b"].copy(),
                  bisection_steps=0, n_inversion=0, status="guess", reach=abs(ds_taken))
        if detect_codim2 > 1:
            r = locate(z, z_old, tau, ds_taken, cp_[-1] if bisect == "CP" else out["b2"][-1])
            zc = r["z"]
            first = cp_[-2] if bisect == "CP" else out["b2"][-3 if len(cp_) > 2 else -2]
            vals = [first if v != v else v for v in r["values"]]
            sp.update(p1=float(zc[0][-1]), p2=float(zc[1]), end_points=tuple(r["ends"]), CP=float(r["tau"][1]),
                      b2=b2_at(*zc) if r["bisection_steps"] else out["b2"][-1], X=zc[0].copy(), bisection_steps=r["bisection_steps"],
                      n_inversion=r["n_inversion"], status=r["status"], reach=r["reach"])
            sp["CP_interval" if bisect == "CP" else "b2_interval"] = tuple(vals)
        out["specialpoint"].append(sp)

    ds_ = ds if ds_sequence is None else ds_sequence[0]
    X0, c0, it0 = newton(np.append(np.asarray(x0, dtype=float), p1), p2)
    assert c0, "Newton failed on the initial fold guess"
    X1, c1, _ = newton(X0, p2 + ds_ / eta)
    assert c1, "Newton failed for the initial tangent"
    z, z1 = (X0, p2), (X1, p2 + ds_ / eta)
    tau = palc.secant_tangent(z1, z, ds_, theta)
    record(z, update(*z), tau[1], ds_, it0)
    zp = palc.add_tangent(z, tau, ds_)
    step = 0
    while step < max_steps and (p_min < z[1] < p_max or step == 0):
        sol, conv, itn = newton_palc(z, tau, zp, ds_)
        if conv:
            z_old, z = z, sol
            step += 1
        if ds_sequence is not None:
            assert conv, f"fold continuation step {step} did not converge with the prescribed ds"
            stop = step >= len(ds_sequence)
            ds_next = ds_ if stop else ds_sequence[step]
        else:
            ds_next, stop = palc.step_size_control(ds_, conv, itn, a=a_ctrl, Nmax=max_iterations, dsmin=dsmin, dsmax=dsmax)
        if conv:
            tau = palc.secant_tangent(z, z_old, ds_next, theta)
            record(z, update(*z), tau[1], ds_, itn)
            after_record(z, z_old, tau, ds_)
        ds_ = ds_next
        if stop:
            break
        zp = palc.add_tangent(z, tau, ds_)
    return out


# ---------------------------------------------------------------------------------------------- the device passes
def _polys(kind, nu):
    return R.sh_polys(kind, nu, 0)[0], sh_poly_d3(kind, nu)


def cusp_dots(kind, nu, u, v, w):
    """(<w, h v v>, <v, v>, <w, w>, <v, w>) with the element expressions of CuspDots; the sums are numpy's (exact on the
    integer data of the exact tests)."""
    h, _ = _polys(kind, nu)
    return np.array([np.sum(((R.horner(h, u) * v) * v) * w), np.sum(v * v), np.sum(w * w), np.sum(v * w)])


def cusp_dots_abs(kind, nu, u, v, w):
    """The sums of |terms| of cusp_dots: the scale of their rounding bounds."""
    h, _ = _polys(kind, nu)
    return np.array([np.sum(np.abs(((R.horner(h, u) * v) * v) * w)), np.sum(v * v), np.sum(w * w), np.sum(np.abs(v * w))])


def cusp_rhs(kind, nu, u, q, b2):
    """b2 q - (h(u) q) q, every product and the difference rounded on its own (CuspRhs)."""
    h, _ = _polys(kind, nu)
    return b2 * q - (R.horner(h, u) * q) * q


def _contract_terms(kind, nu, u, q, p, H2):
    h, t = _polys(kind, nu)
    return (((R.horner(t, u) * q) * q) * q) * p, ((R.horner(h, u) * q) * H2) * p


def cusp_contract(kind, nu, u, q, p, H2):
    """(<p, t q q q>, <p, h q H2>) with the element expressions of CuspContract."""
    t0, t1 = _contract_terms(kind, nu, u, q, p, H2)
    return np.array([np.sum(t0), np.sum(t1)])


def cusp_contract_abs(kind, nu, u, q, p, H2):
    t0, t1 = _contract_terms(kind, nu, u, q, p, H2)
    return np.array([np.sum(np.abs(t0)), np.sum(np.abs(t1))])
