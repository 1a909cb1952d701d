"""CPU restatement of the Hopf normal form, __hopf_normal_form (src/NormalForms.jl:1009-1076), and of the scalars of
predictor(::Hopf, ds) (:1227-1281) for the tests (test side only).

Generic over minaug_hopf_ref.HopfModel plus a trilinear ``d3F(x, q, a, b, c)`` that accepts complex arguments.  Every solve
is direct (dense or sparse LU, complex where shifted) unless ``solver`` is given, so the restatement carries no Krylov
tolerance.  inner(x, y) = sum conj(x) y (VectorInterface): np.vdot(x, y).  With R2 = d2F / 2, R3 = d3F / 6 the reference's

    Psi001 = -J \\ dpF,    Psi200 = (2 i om - J) \\ R2(zeta, zeta),    Psi110 = -J \\ 2 R2(zeta, conj zeta)
    a = < dJ/dp zeta + 2 R2(zeta, Psi001), zeta* >
    b = < 2 R2(zeta, Psi110) + 2 R2(conj zeta, Psi200) + 3 R3(zeta, zeta, conj zeta), zeta* >

read as below in d2F and d3F.
"""
from __future__ import annotations

import math

import numpy as np
import scipy.sparse as sp

import minaug_hopf_ref as R
from minaug_fold_ref import solve


def eigenpair(J, om):
    """(zeta, zeta*) for the eigenvalue of the dense J nearest i om: |zeta| = 1, <zeta, zeta*> = 1, zeta* the eigenvector of J'
    for the conjugate eigenvalue (:1141-1189)."""
    J = np.asarray(J.toarray() if sp.issparse(J) else J, dtype=float)
    w, V = np.linalg.eig(J)
    z = V[:, np.argmin(np.abs(w - 1j * om))]
    z = z / np.linalg.norm(z)
    wt, Vt = np.linalg.eig(J.T)
    zs = Vt[:, np.argmin(np.abs(wt + 1j * om))]
    return z, zs / np.vdot(z, zs)


def normalise(v, w):
    """(zeta, zeta*) from null vectors v of J - i om and w of J' + i om."""
    z = v / np.linalg.norm(v)
    return z, w / np.vdot(z, w)


def hopf_terms(model, d3F, x, q, lens, zeta, zeta_star, P001, P110, P200):
    """The vectors whose inner products with zeta* are a and b: (av, bv)."""
    cz = np.conj(zeta)
    av = model.dJvdp(x, q, lens, zeta) + model.d2F(x, q, zeta, P001)
    bv = model.d2F(x, q, zeta, P110) + model.d2F(x, q, cz, P200) + 0.5 * d3F(x, q, zeta, zeta, cz)
    return av, bv


def hopf_normal_form(model, d3F, x, q, lens, om, zeta, zeta_star, solver=None):
    """dict(a, b, Psi001, Psi110, Psi200, type, rhs = (dpF, r11, r20)).  ``solver(A, rhs)`` replaces the LU solves (A dense or
    sparse, complex for the shifted system)."""
    nrm = np.vdot(zeta, zeta_star)
    if not abs(nrm - 1) <= 1e-8:
        raise ValueError(f"Error of precision in normalization: <zeta, zeta*> = {nrm}")
    slv = solver if solver is not None else solve
    J = model.J(x, q)
    cz = np.conj(zeta)
    dpF = np.asarray(model.dFdp(x, q, lens), dtype=float)
    r11 = model.d2F(x, q, zeta, cz)
    assert np.abs(np.imag(r11)).max() <= 1e-14 * max(np.abs(r11).max(), 1e-300)
    r11 = np.real(r11)
    r20 = 0.5 * model.d2F(x, q, zeta, zeta)
    P001 = slv(J, -dpF)
    P110 = slv(J, -r11)
    P200 = slv(R._shift(-J, 2j * om), r20)
    av, bv = hopf_terms(model, d3F, x, q, lens, zeta, zeta_star, P001, P110, P200)
    a, b = np.vdot(av, zeta_star), np.vdot(bv, zeta_star)
    return dict(a=complex(a), b=complex(b), Psi001=P001, Psi110=P110, Psi200=P200, type=hopf_type(b), rhs=(dpF, r11, r20))


def hopf_type(b):
    return "SuperCritical" if b.real < 0 else ("SubCritical" if b.real > 0 else "Singular")


def predictor(p, om, a, b, ds, ampfactor=1.0):
    """The scalars of predictor(hp, ds) (:1241-1249, 1276-1279): dict(p, amp, amp_orbit, omega, period, dsfactor); ``amp`` is
    the returned 2 amp, ``amp_orbit`` the amplitude inside orbit(t)."""
    dsfactor = 1 if a.real * b.real < 0 else -1
    dsnew = abs(ds) * dsfactor
    amp = ampfactor * math.sqrt(-dsnew * a.real / b.real)
    omega = om + (a.imag - b.imag * a.real / b.real) * ds
    return dict(p=p + dsnew, amp=2 * amp, amp_orbit=amp, omega=omega, period=abs(2 * math.pi / omega), dsfactor=dsfactor)


def orbit(x0, zeta, P001, P110, P200, ds, amp, t):
    """orbit(t) of :1262-1271."""
    A = amp * np.exp(1j * t)
    return x0 + 2 * np.real(zeta * A) + ds * P001 + abs(A) ** 2 * np.real(P110) + 2 * np.real(A ** 2 * P200)


# ---------------------------------------------------------------------------------------------- cGL pieces
def cgl_d3_coefs(u1, u2, mu, c3, c5):
    """Per point the third derivative of the cGL nonlinearity: per field the entries (111, 112, 122, 222) of the symmetric
    2 x 2 x 2 tensor, field 1 first -- the order and the operation order of hopf_pw.h:cgl_d3."""
    a, b, m, s = u1 * u1, u2 * u2, 24.0 * (u1 * u2), 12.0 * (u1 * u1 + u2 * u2)
    return (-6.0 * c3 - c5 * (60.0 * a + 12.0 * b), 2.0 * mu - c5 * m, -2.0 * c3 - c5 * s, 6.0 * mu - c5 * m,
            -6.0 * mu - c5 * m, -2.0 * c3 - c5 * s, -2.0 * mu - c5 * m, -6.0 * c3 - c5 * (12.0 * a + 60.0 * b))


def cgl_d3F(u, q, a, b, c):
    """d3F(u)[a, b, c] of cGL (the Laplacian is linear); complex arguments by linearity."""
    n = len(u) // 2
    t = cgl_d3_coefs(u[:n], u[n:], q["mu"], q["c3"], q["c5"])
    a1, a2, b1, b2, c1, c2 = a[:n], a[n:], b[:n], b[n:], c[:n], c[n:]
    out = []
    for f in (0, 4):
        m11, m12, m22 = t[f] * c1 + t[f + 1] * c2, t[f + 1] * c1 + t[f + 2] * c2, t[f + 2] * c1 + t[f + 3] * c2
        out.append(a1 * (m11 * b1 + m12 * b2) + a2 * (m12 * b1 + m22 * b2))
    return np.concatenate(out)


def cgl_d2F_abs(u, q, a, b):
    """sum of |monomial| of cgl_d2F(u, q, a, b): every coefficient of the Hessian taken with a plus sign."""
    n = len(u) // 2
    u1, u2 = np.abs(u[:n]), np.abs(u[n:])
    mu, c3, c5 = abs(q["mu"]), abs(q["c3"]), abs(q["c5"])
    ua = u1 * u1 + u2 * u2
    q1, q2 = u1 * (8.0 * u1 * u1 + 12.0 * ua), u2 * (8.0 * u1 * u1 + 4.0 * ua)
    q3, q4 = u1 * (8.0 * u2 * u2 + 4.0 * ua), u2 * (8.0 * u2 * u2 + 12.0 * ua)
    h = (6 * c3 * u1 + 2 * mu * u2 + c5 * q1, 2 * c3 * u2 + 2 * mu * u1 + c5 * q2, 2 * c3 * u1 + 6 * mu * u2 + c5 * q3,
         2 * c3 * u2 + 6 * mu * u1 + c5 * q2, 2 * c3 * u1 + 2 * mu * u2 + c5 * q3, 6 * c3 * u2 + 2 * mu * u1 + c5 * q4)
    a1, a2, b1, b2 = np.abs(a[:n]), np.abs(a[n:]), np.abs(b[:n]), np.abs(b[n:])
    return np.concatenate([a1 * (h[0] * b1 + h[1] * b2) + a2 * (h[1] * b1 + h[2] * b2),
                           a1 * (h[3] * b1 + h[4] * b2) + a2 * (h[4] * b1 + h[5] * b2)])


def cgl_d3F_abs(u, q, a, b, c):
    """sum of |monomial| of cgl_d3F(u, q, a, b, c)."""
    n = len(u) // 2
    u1, u2 = np.abs(u[:n]), np.abs(u[n:])
    mu, c3, c5 = abs(q["mu"]), abs(q["c3"]), abs(q["c5"])
    aa, bb, m, s = u1 * u1, u2 * u2, 24.0 * (u1 * u2), 12.0 * (u1 * u1 + u2 * u2)
    t = (6 * c3 + c5 * (60 * aa + 12 * bb), 2 * mu + c5 * m, 2 * c3 + c5 * s, 6 * mu + c5 * m,
         6 * mu + c5 * m, 2 * c3 + c5 * s, 2 * mu + c5 * m, 6 * c3 + c5 * (12 * aa + 60 * bb))
    a1, a2, b1, b2, c1, c2 = (np.abs(v) for v in (a[:n], a[n:], b[:n], b[n:], c[:n], c[n:]))
    out = []
    for f in (0, 4):
        m11, m12, m22 = t[f] * c1 + t[f + 1] * c2, t[f + 1] * c1 + t[f + 2] * c2, t[f + 2] * c1 + t[f + 3] * c2
        out.append(a1 * (m11 * b1 + m12 * b2) + a2 * (m12 * b1 + m22 * b2))
    return np.concatenate(out)


def cgl_closed_form(dims, mu, c3):
    """(a, b) at the first Hopf point of the trivial state u = 0 (gamma = 0), r* = -lam_11, omega = +nu, zeta = phi (1, -i) /
    sqrt 2 with phi the unit-norm first sine mode: d2F(0) = 0, so every Psi vanishes and only the d3F term survives,
    a = 1, b = 2 (-c3 + i mu) sum phi^4 = 2 (-c3 + i mu) 9 / (4 (Nx + 1) (Ny + 1))."""
    return 1.0 + 0.0j, 2.0 * complex(-c3, mu) * 9.0 / (4.0 * (dims[0] + 1) * (dims[1] + 1))


def stuart_landau(r, mu, nu, c3, c5):
    """The Stuart-Landau model of test/normal_forms/testNF.jl:360-415: the cGL nonlinearity on one cell, J(0) = [[r, -nu], [nu, r]].
    Returns (HopfModel with lens r, d3F)."""
    pars = dict(r=r, mu=mu, nu=nu, c3=c3, c5=c5, gamma=0.0)

    def F(x, q):
        u1, u2 = x
        ua = u1 * u1 + u2 * u2
        return np.array([q["r"] * u1 - q["nu"] * u2 - ua * (q["c3"] * u1 - q["mu"] * u2) - q["c5"] * ua ** 2 * u1,
                         q["r"] * u2 + q["nu"] * u1 - ua * (q["c3"] * u2 + q["mu"] * u1) - q["c5"] * ua ** 2 * u2])

    def J(x, q):
        assert np.all(np.asarray(x) == 0), "the Jacobian is written out at the trivial state only"
        return np.array([[q["r"], -q["nu"]], [q["nu"], q["r"]]])

    return R.HopfModel(F, J, R.cgl_d2F, R.cgl_dFdp, R.cgl_dJvdp, pars, "r"), cgl_d3F
