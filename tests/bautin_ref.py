"""CPU restatement of the Bautin (generalised Hopf) normal form, bautin_normal_form (src/codim2/NormalForms.jl:642-829,
detailed = false), for the tests (test side only).

Generic over minaug_hopf_ref.HopfModel plus multilinear ``d3F(x, q, a, b, c)``, ``d4F(x, q, a, b, c, d)`` and
``d5F(x, q, a, b, c, d, e)`` that accept complex arguments.  Every solve is direct unless ``solver`` is given.
dot(p0, h) = sum conj(p0) h = np.vdot(p0, h).  With q = zeta, p0 = zeta*, B = d2F, C = d3F, D = d4F, E = d5F at the Hopf point:

    H20 = (2 i om - J) \\ B(q, q),   H11 = -J \\ B(q, conj q),   G21 = dot(p0, C(q, q, conj q) + B(conj q, H20) + 2 B(q, H11))
    H30 = (3 i om - J) \\ (C(q, q, q) + 3 B(q, H20))
    H21 : [J - i om, q; p0^H, 0][H21; s] = [G21 q - (C(q, q, conj q) + B(conj q, H20) + 2 B(q, H11)); 0]
    H31 = (2 i om - J) \\ h31,   H22 = -J \\ h22,   G32 = dot(p0, g32),   l2 = Re G32 / 12

with h31, h22 and g32 as written out in rhs4 and g32_vector (:772-812).  The reference differentiates d3F numerically for D and E
(:757-794); here they are closed forms (cgl_d4F, cgl_d5F: only the quintic term of cGL contributes).
"""
from __future__ import annotations

import functools

import numpy as np
import scipy.optimize as spo
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import minaug_hopf_ref as R
import normal_form_ref as NF
from minaug_fold_ref import solve


# ---------------------------------------------------------------------------------------------- the formulas
def rhs3(model, d3F, x, par, q, H20, H11, G21):
    """(h30, h21): the right-hand sides of the H30 solve and of the bordered H21 solve (:744-750)."""
    B = lambda a, b: model.d2F(x, par, a, b)
    C = lambda a, b, c: d3F(x, par, a, b, c)
    cq = np.conj(q)
    h30 = C(q, q, q) + 3 * B(q, H20)
    h21 = G21 * q - (C(q, q, cq) + B(cq, H20) + 2 * B(q, H11))
    return h30, h21


def g21_vector(model, d3F, x, par, q, H20, H11):
    cq = np.conj(q)
    return d3F(x, par, q, q, cq) + model.d2F(x, par, cq, H20) + 2 * model.d2F(x, par, q, H11)


def rhs4(model, d3F, d4F, x, par, q, H20, H11, H30, H21, G21):
    """(h31, h22) of :772-780; h22 is real up to rounding and returned complex."""
    B = lambda a, b: model.d2F(x, par, a, b)
    C = lambda a, b, c: d3F(x, par, a, b, c)
    D = lambda a, b, c, d: d4F(x, par, a, b, c, d)
    cq = np.conj(q)
    h31 = (D(q, q, q, cq) + 3 * C(q, q, H11) + 3 * C(q, cq, H20) + 3 * B(H20, H11) + B(cq, H30) + 3 * B(q, H21)
           - 3 * G21 * H20)
    h22 = (D(q, q, cq, cq) + 4 * C(q, cq, H11) + C(cq, cq, H20) + C(q, q, np.conj(H20)) + 2 * B(H11, H11)
           + 2 * B(q, np.conj(H21)) + 2 * B(cq, H21) + B(np.conj(H20), H20) - (2 * G21 + 2 * np.conj(G21)) * H11)
    return h31, h22


def g32_terms(model, d3F, d4F, d5F, x, par, q, H20, H11, H30, H21, H31, H22):
    """The fifteen vectors whose sum g32 gives G32 = dot(p0, g32) (:796-812), coefficients included."""
    B = lambda a, b: model.d2F(x, par, a, b)
    C = lambda a, b, c: d3F(x, par, a, b, c)
    D = lambda a, b, c, d: d4F(x, par, a, b, c, d)
    cq, c20, c21 = np.conj(q), np.conj(H20), np.conj(H21)
    return [d5F(x, par, q, q, q, cq, cq), D(q, q, q, c20), 3 * D(q, cq, cq, H20), 6 * D(q, q, cq, H11),
            C(cq, cq, H30), 3 * C(q, q, c21), 6 * C(q, cq, H21), 3 * C(q, c20, H20), 6 * C(q, H11, H11), 6 * C(cq, H20, H11),
            2 * B(cq, H31), 3 * B(q, H22), B(c20, H30), 3 * B(c21, H20), 6 * B(H11, H21)]


def g32_vector(*args):
    return sum(g32_terms(*args))


def bordered_solve(A, dR, dzu, R_, solver=None):
    """[A dR; dzu^H 0][X; s] = [R; 0]: direct on the bordered matrix, or, with ``solver``, one BorderingBLS pass (two solves with
    A, src/LinearBorderSolver.jl:88-166 with check_precision = false)."""
    n = dR.shape[0]
    if solver is not None:
        x1, dx = solver(A, R_, False), solver(A, dR, False)         # A is singular at a Hopf point: no convergence check
        dl = (0.0 - np.vdot(dzu, x1)) / (0.0 - np.vdot(dzu, dx))
        return x1 - dl * dx
    dR, dzu = np.asarray(dR, dtype=complex), np.asarray(dzu, dtype=complex)
    if sp.issparse(A):
        M = sp.bmat([[A, sp.csr_matrix(dR.reshape(-1, 1))], [sp.csr_matrix(dzu.conj().reshape(1, -1)), None]], format="csc")
    else:
        M = np.block([[A, dR.reshape(-1, 1)], [dzu.conj().reshape(1, -1), np.zeros((1, 1))]])
    return solve(M, np.concatenate([R_, [0.0]]))[:n]


def bautin_type(l2):
    """type(::Bautin): the sign of the second Lyapunov coefficient."""
    return "Subcritical" if l2 > 0 else "Supercritical"


def bautin_normal_form(model, d3F, d4F, d5F, x, par, om, zeta, zeta_star, solver=None):
    """dict(G21, G32, l2, H20, H11, H30, H21, H31, H22, type, rhs = (h30, h21, h31, h22)).  ``solver(A, rhs)`` replaces the LU
    solves (A dense or sparse, complex for the shifted systems) and turns the bordered solve into a BorderingBLS pass, whose two
    solves it is called for with a third argument False (the matrix is singular there: convergence is not required)."""
    nrm = np.vdot(zeta, zeta_star)
    if not abs(nrm - 1) <= 1e-8:
        raise ValueError(f"Error of precision in normalization: <zeta, zeta*> = {nrm}")
    slv = solver if solver is not None else solve
    J = model.J(x, par)
    q, p0 = zeta, zeta_star
    cq = np.conj(q)
    H20 = slv(R._shift(-J, 2j * om), model.d2F(x, par, q, q))
    H11 = slv(J, -np.real(model.d2F(x, par, q, cq)))
    G21 = np.vdot(p0, g21_vector(model, d3F, x, par, q, H20, H11))
    h30, h21 = rhs3(model, d3F, x, par, q, H20, H11, G21)
    H30 = slv(R._shift(-J, 3j * om), h30)
    H21 = bordered_solve(R._shift(J, -1j * om), q, p0, h21, solver)
    h31, h22 = rhs4(model, d3F, d4F, x, par, q, H20, H11, H30, H21, G21)
    H31 = slv(R._shift(-J, 2j * om), h31)
    H22 = -slv(J, np.real(h22))
    G32 = np.vdot(p0, g32_vector(model, d3F, d4F, d5F, x, par, q, H20, H11, H30, H21, H31, H22))
    l2 = G32.real / 12
    return dict(G21=complex(G21), G32=complex(G32), l2=float(l2), H20=H20, H11=H11, H30=H30, H21=H21, H31=H31, H22=H22,
                type=bautin_type(l2), rhs=(h30, h21, h31, h22))


# ---------------------------------------------------------------------------------------------- cGL pieces
def cgl_d4_coefs(u1, u2, c5):
    """Per point the fourth derivative of the cGL nonlinearity: per field the entries (1111, 1112, 1122, 1222, 2222) of the
    symmetric tensor, field 1 first -- the order of hopf_pw.h:cgl_d4.  Linear in u; only -c5 |z|^4 z contributes."""
    p, q = -24.0 * c5 * u1, -24.0 * c5 * u2
    return (5.0 * p, q, p, q, p, q, p, q, p, 5.0 * q)


def cgl_d5_coefs(c5):
    """The fifth derivative: per field the entries (11111, 11112, 11122, 11222, 12222, 22222), constant (hopf_pw.h:cgl_d5)."""
    a = -24.0 * c5
    return (5.0 * a, 0.0, a, 0.0, a, 0.0, 0.0, a, 0.0, a, 0.0, 5.0 * a)


def _sym(entries, args):
    """A symmetric 2-field tensor given by its K + 1 entries (entry j: j indices equal to 2) against K vectors (a1, a2)."""
    t = list(entries)
    for a1, a2 in args:
        t = [t[j] * a1 + t[j + 1] * a2 for j in range(len(t) - 1)]
    return t[0]


def _fields(n, vecs):
    return [(v[:n], v[n:]) for v in vecs]


def cgl_d4F(u, q, a, b, c, d):
    """d4F(u)[a, b, c, d] of cGL; complex arguments by linearity."""
    n = len(u) // 2
    t = cgl_d4_coefs(u[:n], u[n:], q["c5"])
    args = _fields(n, (a, b, c, d))
    return np.concatenate([_sym(t[:5], args), _sym(t[5:], args)])


def cgl_d5F(u, q, a, b, c, d, e):
    """d5F[a, b, c, d, e] of cGL (it does not depend on u); complex arguments by linearity."""
    n = len(u) // 2
    t = cgl_d5_coefs(q["c5"])
    args = _fields(n, (a, b, c, d, e))
    return np.concatenate([_sym(t[:6], args), _sym(t[6:], args)])


def cgl_d4F_abs(u, q, a, b, c, d):
    """sum of |monomial| of cgl_d4F."""
    n = len(u) // 2
    t = cgl_d4_coefs(np.abs(u[:n]), np.abs(u[n:]), -abs(q["c5"]))
    args = _fields(n, [np.abs(v) for v in (a, b, c, d)])
    return np.concatenate([_sym(t[:5], args), _sym(t[5:], args)])


def cgl_d5F_abs(u, q, a, b, c, d, e):
    """sum of |monomial| of cgl_d5F."""
    n = len(u) // 2
    t = cgl_d5_coefs(-abs(q["c5"]))
    args = _fields(n, [np.abs(v) for v in (a, b, c, d, e)])
    return np.concatenate([_sym(t[:6], args), _sym(t[6:], args)])


def cabs(z):
    """|Re z| + |Im z|: what a monomial with a complex factor is bounded with, component by component."""
    return np.abs(np.real(z)) + np.abs(np.imag(z))


def cgl_abs_model(pars, lens="r"):
    """A HopfModel whose d2F is the sum of the moduli of its monomials, with the matching d3F, d4F, d5F: rhs3, rhs4 and g32_terms
    evaluated on it with cabs(.) arguments (and |G21|) bound the monomials of the device expressions."""
    m = R.HopfModel(None, None, NF.cgl_d2F_abs, None, None, pars, lens)
    return m, NF.cgl_d3F_abs, cgl_d4F_abs, cgl_d5F_abs


def stuart_landau_reference(r, mu, nu, c3, c5):
    """Fsl2! of test/normal_forms/testNF.jl:564-571 -- r z + i nu z + (c3 + i mu) |z|^2 z + c5 |z|^4 z, the cGL nonlinearity of
    this library with the signs of c3, mu and c5 reversed -- as (HopfModel, d3F, d4F, d5F) in the reference's parameters."""
    model, d3F = NF.stuart_landau(r, -mu, nu, -c3, -c5)
    return model, d3F, cgl_d4F, cgl_d5F


# ---------------------------------------------------------------------------------------------- the Bautin point of a Hopf curve
def first_lyapunov(model, d3F, s, p2):
    """b of the Hopf normal form at a refined Hopf point ``s`` (a newton_hopf result) of the curve at p2."""
    par = model.at(s["p"], p2)
    z, zs = NF.normalise(s["v"], s["w"])
    return NF.hopf_normal_form(model, d3F, s["u"], par, model.lens1, s["omega"], z, zs)["b"]


def locate_bautin(model, d3F, x0, p1, om, a, b, p2, *, ds, max_steps=40, xtol=1e-11, **kw):
    """The sign change of Re b along minaug_hopf_ref.continuation_hopf from (x0, p1, om) at p2: the first pair of consecutive
    points of the curve with Re b of opposite signs, then Brent's method on p2 with a Newton refinement of the Hopf point (from
    the left point of the pair) at each evaluation.  dict(p2, p1, omega, u, v, w, b, bracket, curve = (p2, Re b) per point)."""
    br = R.continuation_hopf(model, x0, p1, om, p2, a, b, ds=ds, max_steps=max_steps, **kw)
    vw = []

    def refine(c, X):
        s = R.newton_hopf(model, X[:-2], X[-2], X[-1], vw[0], vw[1], p2=c, tol=1e-12, max_iterations=20)
        assert s["converged"], s["residuals"]
        return s

    reb, prev = [], None
    for c, X in zip(br["p2"], br["X"]):
        if not vw:
            vw[:] = [np.asarray(a, dtype=complex), np.asarray(b, dtype=complex)]
        s = refine(c, X)
        vw[:] = [s["w"] / np.linalg.norm(s["w"]), s["v"] / np.linalg.norm(s["v"])]
        reb.append(first_lyapunov(model, d3F, s, c).real)
        if prev is not None and reb[-1] * reb[-2] < 0:
            lo, hi, X0 = prev[0], c, prev[1]
            f = lambda cc: first_lyapunov(model, d3F, refine(cc, X0), cc).real
            root = spo.brentq(f, lo, hi, xtol=xtol, rtol=4 * np.finfo(float).eps)
            s = refine(root, X0)
            return dict(p2=float(root), p1=float(s["p"]), omega=float(s["omega"]), u=s["u"], v=s["v"], w=s["w"],
                        b=first_lyapunov(model, d3F, s, root), bracket=(lo, hi), curve=list(zip(br["p2"], reb)))
        prev = (c, X)
    raise AssertionError(f"Re b does not change sign along the curve: {list(zip(br['p2'], reb))}")


# ---------------------------------------------------------------------------------------------- the fixture of the GPU tests
DIMS, LS = (41, 21), (np.pi, np.pi / 2)            # the grid of examples/cGL2d.jl
PARS = dict(r=0.5, mu=0.1, nu=1.0, c3=-1.0, c5=1.0, gamma=0.0)
RELTOL = 1e-13                                     # of the device solves in the comparisons


def _hopf_mode(dims):
    x = np.sin(np.pi * np.arange(1, dims[0] + 1) / (dims[0] + 1))
    y = np.sin(np.pi * np.arange(1, dims[1] + 1) / (dims[1] + 1))
    phi = np.outer(y, x).reshape(-1)
    phi /= np.linalg.norm(phi) * np.sqrt(2)
    z = np.zeros_like(phi)
    return np.concatenate([phi, z]) + 1j * np.concatenate([z, -phi])


def first_hopf_r(dims, ls):
    """r* = -lam_11 of the Dirichlet Laplacian: the first Hopf point of the trivial state."""
    lam = [-(4 / (2 * l / n) ** 2) * np.sin(np.pi / (2 * (n + 1))) ** 2 for n, l in zip(dims, ls)]
    return -(lam[0] + lam[1])


@functools.lru_cache(maxsize=None)
def cgl_curve_start(c3=-0.2, gamma=0.1):
    """The Hopf point of cGL on the 41 x 21 grid off the trivial state (gamma = 0.1) at ``c3``, refined in r from u = 0:
    (op, pars, newton_hopf result)."""
    from oracle import operators
    op = operators.CGL2d(DIMS, LS)
    pars = dict(PARS, gamma=gamma, c3=c3)
    z = _hopf_mode(DIMS)
    m = R.cgl_model(op, pars, "r", "c3")
    s = R.newton_hopf(m, np.zeros(2 * DIMS[0] * DIMS[1]), first_hopf_r(DIMS, LS), PARS["nu"], z, z, p2=c3, tol=1e-12,
                      max_iterations=20)
    assert s["converged"], s["residuals"]
    return op, pars, s


@functools.lru_cache(maxsize=None)
def cgl_bautin_point():
    """The Bautin point of the Hopf curve of cGL in (r, c3) at gamma = 0.1 on the 41 x 21 grid, from c3 = -0.2 towards 0:
    (op, model, locate_bautin result)."""
    op, pars, s = cgl_curve_start()
    m = R.cgl_model(op, pars, "r", "c3")
    a, b = s["w"] / np.linalg.norm(s["w"]), s["v"] / np.linalg.norm(s["v"])
    loc = locate_bautin(m, NF.cgl_d3F, s["u"], s["p"], s["omega"], a, b, pars["c3"], ds=0.05, dsmax=0.05, max_steps=3)
    return op, m, loc


def block_preconditioner(op, pars, r0):
    """(Lap (x) I + [[r0, -nu], [nu, r0]])^-1, the Jacobian of the trivial state at r0 -- what hip.CGLBlockPreconditioner applies
    -- as a LinearOperator on real or complex vectors."""
    q = dict(pars, r=r0, gamma=0.0)
    n = 2 * op.n
    lu = spla.splu(sp.csc_matrix(op.J(np.zeros(n), **q)))

    def apply(v):
        v = np.asarray(v).reshape(-1)
        return lu.solve(v.real.copy()) + 1j * lu.solve(v.imag.copy()) if np.iscomplexobj(v) else lu.solve(v)

    return spla.LinearOperator((n, n), matvec=apply, dtype=complex)


def gmres_solver(reltol, Pl=None, restart=60, maxiter=600):
    """solver(A, rhs, strict = True): SciPy GMRES at ``reltol`` on the LEFT-preconditioned system Pl A x = Pl rhs, as the device's
    IterativeSolvers flavor runs it (the Arnoldi process on Pl^-1 (a0 + a1 J), stopped at |Pl^-1 r| <= reltol |Pl^-1 rhs|) and as
    normal_form1d_ref.bordered_bordering does.  SciPy's own ``M`` argument stops on the unpreconditioned residual instead, another
    rule than the device's.  ``Pl`` is a LinearOperator on complex vectors; ``strict`` asserts convergence."""
    def run(A, rhs, strict=True):
        cplx = np.iscomplexobj(rhs) or np.iscomplexobj(A.dtype.type(0))
        dt = complex if cplx else float
        rhs = np.asarray(rhs, dtype=dt)
        pl = (lambda v: v) if Pl is None else (lambda v: Pl.matvec(v) if cplx else np.real(Pl.matvec(v)))
        op = spla.LinearOperator(A.shape, matvec=lambda v: pl(A @ np.asarray(v).reshape(-1)), dtype=dt)
        x, info = spla.gmres(op, pl(rhs), rtol=reltol, atol=0.0, restart=restart, maxiter=maxiter if strict else 2)
        assert info == 0 or not strict, info
        return x
    return run


def summation_bound(terms):
    """4 n eps sum |terms| per component, added: what two fp64 sums of the same n terms in different orders may differ by."""
    n = len(terms)
    return 4 * n * np.finfo(float).eps * (np.abs(terms.real).sum() + np.abs(terms.imag).sum())


@functools.lru_cache(maxsize=None)
def cgl_bautin_yardstick():
    """At the Bautin point of cgl_bautin_point: the restatement with direct (sparse LU) solves (``lu``) and with SciPy GMRES at
    RELTOL, left-preconditioned by the block preconditioner of the device solves (``gm``).  ``spread`` = |gm - lu| for G21, G32, l2
    (absolute) and the H vectors (max norm) is the yardstick of the GPU comparisons.  ``allowed`` = 10 x spread, the rule of DESIGN
    9d / 9e; as there, a coefficient is also allowed the rounding of its own fixed-order sum, 4 n eps sum |terms|."""
    op, m, loc = cgl_bautin_point()
    par = m.at(loc["p1"], loc["p2"])
    z, zs = NF.normalise(loc["v"], loc["w"])
    args = (m, NF.cgl_d3F, cgl_d4F, cgl_d5F, loc["u"], par, loc["omega"], z, zs)
    lu = bautin_normal_form(*args)
    gm = bautin_normal_form(*args, solver=gmres_solver(RELTOL, block_preconditioner(op, par, loc["p1"])))
    spread = {k: abs(gm[k] - lu[k]) for k in ("G21", "G32", "l2")}
    spread.update({k: float(np.abs(gm[k] - lu[k]).max()) for k in ("H20", "H11", "H30", "H21", "H31", "H22")})
    t21 = np.conj(zs) * g21_vector(m, NF.cgl_d3F, loc["u"], par, z, lu["H20"], lu["H11"])
    t32 = np.conj(zs) * g32_vector(m, NF.cgl_d3F, cgl_d4F, cgl_d5F, loc["u"], par, z,
                                   *(lu[k] for k in ("H20", "H11", "H30", "H21", "H31", "H22")))
    summation = dict(G21=summation_bound(t21), G32=summation_bound(t32), l2=summation_bound(t32) / 12)
    allowed = {k: 10 * spread[k] + summation.get(k, 0.0) for k in ("G21", "G32", "l2", "H30", "H21", "H31", "H22")}
    return dict(lu=lu, gm=gm, spread=spread, summation=summation, allowed=allowed, par=par, zeta=z, zeta_star=zs, loc=loc, op=op,
                model=m)
