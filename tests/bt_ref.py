"""CPU restatement of the Bogdanov-Takens machinery of src/codim2/MinAugBT.jl and src/codim2/NormalForms.jl for the tests (test
side only).  Dense and direct: every linear solve is an LU of the bordered matrix, so the restatement carries no Krylov tolerance.

Generic over a model (minaug_hopf_ref.HopfModel): F, J (dense or scipy.sparse), d2F (bilinear), dF/dp, dJ/dp v, all with ``q`` a
dict of parameters, and the two lenses ``lenses = (lens1, lens2)``.  Optional model attribute ``d2F_adj(x, q, v, w)`` =
B(x)[v, .]' w (the gradient of y -> <w, d2F(x)[v, y]>); without it the vector is assembled from d2F on the unit vectors.

  bordered_vectors   the functional (:70-102) and the adjoint chain (:160-172):
                         [J a; b' 0][v1; s1] = [0; 1],  [J a; b' 0][v2; s2] = [v1; 0],
                         [J' b; a' 0][w1; .] = [0; 1],  [J' b; a' 0][w2; .] = [w1; 0]
  border             s B[v1, .]' w1,  s (B[v1, .]' w2 + B[v2, .]' w1)  and the 2 x 2 block  s <w1, D_k v1>,
                     s (<w2, D_k v1> + <w1, D_k v2>): s = -1 with the bordered vectors gives sigma_x and sigma_p (analytic where
                     :176-220 differences), s = +1 with (q0, q1, p1, p0) gives A12 and A22 of the normal form (:252-254)
  bt_jacobian        the dense (n + 2) x (n + 2) Jacobian [J dpF; sigma_x sigma_p] of G = (F, sigma1, sigma2)
  newton_bt          newton_bt under _newton (src/Newton.jl:66-114)
  start_vectors      the default of newton_bt(br, ind) (:417-435): random a, b, then a = w1 / |w1|, b = v1 / |v1|
  jordan_basis       (q0, q1, p0, p1) with J q0 = 0, J q1 = q0, J' p1 = 0, J' p0 = p1, <p_i, q_j> = delta_ij (NormalForms.jl:603-622)
  normal_form        a, b and, detailed, gamma, c, K10, K11, K2, H2000, H1100, H0010, H0001 (:180-272).  Parameters that enter F
                     linearly have no second parameter derivative; a model with one supplies ``d2Fdp2(x, q, l, m)``
  predictor_hopf     predictor(bt, Val(:HopfCurve), ds) (:342-400);  predictor_fold  predictor(bt, Val(:FoldCurve), ds) (:408-434)
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

from minaug_fold_ref import solve
from oracle import palc


class Krylov:
    """The solves of this module by SciPy GMRES on the left-preconditioned bordered systems diag(Pl^-1, I) [J A; B' C]
    (minaug_bordered_ref.block_gmres), as the device runs them: ``pl`` for J, ``pl_adj`` for J'; ``its`` collects the inner
    iteration count of every solve in call order, ``bad`` the solves SciPy reports unconverged."""

    def __init__(self, pl, pl_adj, **gm):
        self.pl, self.pl_adj, self.gm, self.its, self.bad = pl, pl_adj, gm, [], 0

    def block(self, J, A, Bm, Cm, rhst, rhsb, adjoint=False):
        from minaug_bordered_ref import block_gmres
        u1, u2, info, it = block_gmres(J, A, Bm, Cm, rhst, np.asarray(rhsb, dtype=float), self.pl_adj if adjoint else self.pl, **self.gm)
        self.its.append(it)
        self.bad += int(info != 0)
        return u1, u2


def _bordered(J, col, row, top, bot, sv=None, adjoint=False):
    """[J col; row' 0][y; s] = [top; bot]: one LU of the bordered matrix (regular where J is singular), or ``sv`` (Krylov)."""
    n = len(col)
    if sv is not None:
        y, s = sv.block(J, np.asarray(col).reshape(-1, 1), np.asarray(row).reshape(-1, 1), np.zeros((1, 1)), top, [bot], adjoint)
        return y, float(s[0])
    if sp.issparse(J):
        M = sp.bmat([[J, sp.csr_matrix(np.asarray(col).reshape(-1, 1))], [sp.csr_matrix(np.asarray(row).reshape(1, -1)), None]],
                    format="csc")
    else:
        M = np.block([[np.asarray(J), np.asarray(col).reshape(-1, 1)], [np.asarray(row).reshape(1, -1), np.zeros((1, 1))]])
    y = solve(M, np.concatenate([top, [bot]]))
    return y[:n], float(y[n])


def bordered_vectors(model, x, q, a, b, sv=None):
    """dict(v1, v2, w1, w2, sigma = (s1, s2))."""
    J = model.J(x, q)
    Jt = J.T.tocsr() if sp.issparse(J) else np.asarray(J).T
    z = np.zeros(len(x))
    v1, s1 = _bordered(J, a, b, z, 1.0, sv)
    v2, s2 = _bordered(J, a, b, v1, 0.0, sv)
    w1, _ = _bordered(Jt, b, a, z, 1.0, sv, True)
    w2, _ = _bordered(Jt, b, a, w1, 0.0, sv, True)
    return dict(v1=v1, v2=v2, w1=w1, w2=w2, sigma=np.array([s1, s2]))


def d2F_adj(model, x, q, v, w):
    """B(x)[v, .]' w."""
    f = getattr(model, "d2F_adj", None)
    if f is not None:
        return f(x, q, v, w)
    n = len(x)
    E = np.eye(n)
    return np.array([np.dot(w, model.d2F(x, q, v, E[j])) for j in range(n)])


def border(model, x, q, lenses, s, v1, v2, w1, w2):
    """(row1, row2, block): see the module docstring; block[i, k] belongs to row i and lens k."""
    row1 = s * d2F_adj(model, x, q, v1, w1)
    row2 = s * (d2F_adj(model, x, q, v1, w2) + d2F_adj(model, x, q, v2, w1))
    blk = np.zeros((2, 2))
    for k, l in enumerate(lenses):
        D1, D2 = model.dJvdp(x, q, l, v1), model.dJvdp(x, q, l, v2)
        blk[0, k] = s * np.dot(w1, D1)
        blk[1, k] = s * (np.dot(w2, D1) + np.dot(w1, D2))
    return row1, row2, blk


def _at(model, lenses, p):
    q = dict(model.pars)
    q[lenses[0]], q[lenses[1]] = float(p[0]), float(p[1])
    return q


def bt_jacobian(model, x, q, lenses, t):
    """Dense [J dp1F dp2F; sigma1_x sigma1_p; sigma2_x sigma2_p] with the bordered vectors ``t`` of (x, q)."""
    J = model.J(x, q)
    J = J.toarray() if sp.issparse(J) else np.asarray(J)
    r1, r2, blk = border(model, x, q, lenses, -1.0, t["v1"], t["v2"], t["w1"], t["w2"])
    cols = np.stack([model.dFdp(x, q, l) for l in lenses], axis=1)
    return np.block([[J, cols], [np.stack([r1, r2]), blk]])


def G(model, x, p, lenses, a, b, sv=None):
    q = _at(model, lenses, p)
    t = bordered_vectors(model, x, q, a, b, sv)
    return np.concatenate([model.F(x, q), t["sigma"]]), t, q


def newton_bt(model, x0, p0, lenses, a, b, tol=1e-10, max_iterations=25, normN=palc.norm2, sv=None):
    """dict(u, p, residuals, converged, itnewton, terms, cond): cond = the 2-norm condition number of J_BT at the last step.
    ``sv`` (Krylov): every solve by preconditioned GMRES, the step as ONE block-bordered solve with m = 2."""
    x, p = np.asarray(x0, dtype=float).copy(), np.asarray(p0, dtype=float).copy()
    R, t, q = G(model, x, p, lenses, a, b, sv)
    res, step, cond = [normN(R)], 0, None
    while step < max_iterations and res[-1] > tol:
        Jbt = bt_jacobian(model, x, q, lenses, t)
        cond = float(np.linalg.cond(Jbt))
        if sv is None:
            d = np.linalg.solve(Jbt, R)
        else:
            n = len(x)
            d = np.concatenate(sv.block(model.J(x, q), Jbt[:n, n:], Jbt[n:, :n].T, Jbt[n:, n:], R[:n], R[n:]))
        x, p = x - d[:-2], p - d[-2:]
        R, t, q = G(model, x, p, lenses, a, b, sv)
        res.append(normN(R))
        step += 1
    return dict(u=x, p=p, residuals=res, converged=res[-1] < tol, itnewton=step, terms=t, cond=cond)


def start_vectors(model, x, q, seed=0, sv=None):
    rng = np.random.default_rng(seed)
    n = len(x)
    a, b = rng.random(n), rng.random(n)
    t = bordered_vectors(model, x, q, a, b, sv)
    return t["w1"] / np.linalg.norm(t["w1"]), t["v1"] / np.linalg.norm(t["v1"])


def jordan_basis(model, x, q, vr, vl, sv=None):
    """(q0, q1, p0, p1) from guesses vr, vl of the right and left null vectors (:603-622)."""
    J = model.J(x, q)
    Jt = J.T.tocsr() if sp.issparse(J) else np.asarray(J).T
    z = np.zeros(len(x))
    q0, _ = _bordered(J, vl, vr, z, 1.0, sv)
    p1, _ = _bordered(Jt, vr, vl, z, 1.0, sv, True)
    q1, _ = _bordered(J, p1, q0, q0, 0.0, sv)
    p0, _ = _bordered(Jt, q0, p1, p1, 0.0, sv, True)
    mu = np.sqrt(abs(np.dot(q0, q0)))
    q0, q1 = q0 / mu, q1 / mu
    q1 = q1 - np.dot(q0, q1) * q0
    nu = np.dot(q0, p0)
    p1 = p1 / nu
    p0 = (p0 - np.dot(p0, q1) * p1) / nu
    return q0, q1, p0, p1


def jordan_defect(model, x, q, q0, q1, p0, p1):
    """max over the identities J q0 = 0, J q1 = q0, J' p1 = 0, J' p0 = p1, <p_i, q_j> = delta_ij (absolute)."""
    J = model.J(x, q)
    d = [np.abs(J @ q0).max(), np.abs(J @ q1 - q0).max(), np.abs(J.T @ p1).max(), np.abs(J.T @ p0 - p1).max(),
         abs(np.dot(p0, q0) - 1), abs(np.dot(p1, q1) - 1), abs(np.dot(p0, q1)), abs(np.dot(p1, q0))]
    return float(max(d))


def normal_form(model, x, q, lenses, q0, q1, p0, p1, detailed=True, sv=None):
    B = lambda u, v: model.d2F(x, q, u, v)
    J = model.J(x, q)
    B00 = B(q0, q0)
    a = 0.5 * np.dot(p1, B00)
    b = np.dot(p0, B00) + np.dot(p1, B(q0, q1))
    nf = dict(a=float(a), b=float(b))
    if not detailed:
        return nf
    Ainv = lambda r: _bordered(J, p1, q0, r, 0.0, sv)[0]
    B01, B11 = B(q0, q1), B(q1, q1)
    H2000 = Ainv(2 * a * q1 - B00)
    gamma = (-2 * np.dot(p0, H2000) + 2 * np.dot(p0, B01) + np.dot(p1, B11)) / 2
    H2000 = H2000 + gamma * q0
    H1100 = Ainv(b * q1 + H2000 - B01)
    c = 3 * np.dot(p0, H1100) - np.dot(p0, B11)
    A12_1, A12_2, A22 = border(model, x, q, lenses, 1.0, q0, q1, p1, p0)
    J1s = np.stack([model.dFdp(x, q, l) for l in lenses], axis=1)
    Jd = J.toarray() if sp.issparse(J) else np.asarray(J)
    M = np.block([[Jd, J1s], [np.stack([A12_1, A12_2]), A22]])
    n = len(x)
    rows = np.stack([A12_1, A12_2], axis=1)
    if sv is None:
        y = np.linalg.solve(M, np.concatenate([q1, [np.dot(p1, B11) / 2, c]]))
        H0010, K10 = y[:n], y[n:]
        y = np.linalg.solve(M, np.concatenate([np.zeros(n), [0.0, 1.0]]))
        H0001, K11 = y[:n], y[n:]
    else:
        H0010, K10 = sv.block(J, J1s, rows, A22, q1, [np.dot(p1, B11) / 2, c])
        H0001, K11 = sv.block(J, J1s, rows, A22, np.zeros(n), [0.0, 1.0])
    k1 = np.dot(p1, B(H0001, H0001))
    k2 = sum(np.dot(p1, model.dJvdp(x, q, l, H0001)) * K11[k] for k, l in enumerate(lenses))
    k3 = 0.0
    d2 = getattr(model, "d2Fdp2", None)
    if d2 is not None:
        l1, l2 = lenses
        k3 = np.dot(p1, d2(x, q, l1, l1) * K11[0] ** 2 + 2 * d2(x, q, l1, l2) * K11[0] * K11[1] + d2(x, q, l2, l2) * K11[1] ** 2)
    K2 = -(k1 + 2 * k2 + k3) * K10
    nf.update(gamma=float(gamma), c=float(c), K10=K10, K11=K11, K2=K2, H2000=H2000, H1100=H1100, H0010=H0010, H0001=H0001,
              cond=float(np.linalg.cond(M)))
    return nf


def flipped(nf):
    """The normal form of the basis (-q0, -q1, -p0, -p1): a, b, gamma, c and K10 change sign, K11, K2 and H0001 do not."""
    out = dict(nf)
    for k in ("a", "b", "gamma", "c", "K10", "H0010"):
        if k in out:
            out[k] = -out[k]
    return out


def _getx(a, s):
    return -np.sqrt(abs(s) / a) if a > 0 else np.sqrt(abs(s) / abs(a))


def predictor_hopf(nf, p_bt, q0, q1, p0, p1, s):
    """dict(pars, omega, x, EigenVec, EigenVecAd, x0) of the Hopf-curve predictor at s."""
    a, b = nf["a"], nf["b"]
    xx = _getx(a, s)
    beta1 = -abs(s) if a > 0 else abs(s)
    beta2 = -b * xx
    pars = np.asarray(p_bt) + nf["K10"] * beta1 + nf["K11"] * beta2 + nf["K2"] * (beta2 ** 2 / 2)
    A = np.array([[0.0, 1.0], [2 * xx * a, 0.0]])
    vals, vecs = np.linalg.eig(A)
    h = vecs[:, int(np.argmax(vals.imag))]
    vals, vecs = np.linalg.eig(A.T)
    ha = vecs[:, int(np.argmin(vals.imag))]
    return dict(pars=pars, omega=float(np.sqrt(-2 * xx * a)), x=xx, EigenVec=q0 * h[0] + q1 * h[1],
                EigenVecAd=p0 * ha[0] + p1 * ha[1], x0=xx * q0)


def predictor_fold(nf, p_bt, q0, p1, s):
    pars = np.asarray(p_bt) + nf["K11"] * s + nf["K2"] * (s ** 2 / 2)
    return dict(pars=pars, EigenVec=q0, EigenVecAd=p1, x0=_getx(nf["a"], s) * q0)


# ---------------------------------------------------------------------------------------------- cGL pieces
def cgl_d2F_adj(u, q, v, w):
    """B(u)[v, .]' w of the cGL nonlinearity per grid point: sum_f w_f H_f v."""
    from minaug_hopf_ref import cgl_hessians
    n = len(u) // 2
    h = cgl_hessians(u[:n], u[n:], q["mu"], q["c3"], q["c5"])
    va, vb, wa, wb = v[:n], v[n:], w[:n], w[n:]
    return np.concatenate([wa * (h[0] * va + h[1] * vb) + wb * (h[3] * va + h[4] * vb),
                           wa * (h[1] * va + h[2] * vb) + wb * (h[4] * va + h[5] * vb)])


def cgl_model(op, pars, lens1, lens2):
    from minaug_hopf_ref import cgl_model as hopf_model
    m = hopf_model(op, pars, lens1, lens2)
    m.d2F_adj = cgl_d2F_adj
    return m


# ---------------------------------------------------------------------------------------------- the cGL yardstick
CGL_PARS = dict(r=0.5, mu=0.1, nu=1.0, c3=-1.0, c5=1.0, gamma=0.0)
CGL_LS = (np.pi, np.pi / 2)
CGL_LENSES = ("r", "gamma")
CGL_CURVE = dict(ds=0.01, dsmin=1e-3, dsmax=0.02, tol=1e-10, max_iterations=25, max_steps=100)      # the example's steps
# What the GPU tests hand to GMRESIterativeSolvers.  rtol: the double zero eigenvalue at the refined point moves like the square root
# of what the last Newton update leaves, the linear solver's error included: with rtol 1e-12 the restatement's GMRES run leaves
# |lambda| = 1.9e-7 ... 5.4e-7 (up to 11 x the LU run's), with 1e-13 -- the tolerance of the Hopf tests on this problem -- 9.6e-8 ...
# 5.5e-7 (at most 2.4 x), with 1e-14 4.5e-8 ... 5.6e-7 (1.4 x)
GMRES = dict(restart=60, maxiter=10, rtol=1e-13)
NF_KEYS = ("a", "b", "gamma", "c", "K10", "K11", "K2")


def cgl_hopf_start(dims):
    """(r*, z): the closed-form Hopf point of the trivial state, r* = -lam_11, omega = nu, eigenvector (phi, -i phi)."""
    lam = []
    for n, l in zip(dims, CGL_LS):
        h = 2 * l / n
        lam.append(-(4 / h ** 2) * np.sin(np.pi * np.arange(1, n + 1) / (2 * (n + 1))) ** 2)
    x = np.sin(np.pi * np.arange(1, dims[0] + 1) / (dims[0] + 1))
    y = np.sin(np.pi * np.arange(1, dims[1] + 1) / (dims[1] + 1))
    phi = np.outer(y, x).reshape(-1)
    phi /= np.linalg.norm(phi) * np.sqrt(2)
    z = np.zeros_like(phi)
    return -(lam[0][0] + lam[1][0]), np.concatenate([phi, z]) + 1j * np.concatenate([z, -phi])


def cgl_preconditioners(op, a, b):
    """(pl, pl_adj): r -> L0^-1 r and r -> L0'^-1 r with L0 = Lap (x) I_2 + [[a, -b], [b, a]], the Jacobian of the trivial state."""
    import scipy.sparse.linalg as spla
    q = dict(CGL_PARS, r=a, nu=b)
    L0 = sp.csc_matrix(op.J(np.zeros(2 * op.n), **q))
    lu, lut = spla.splu(L0), spla.splu(sp.csc_matrix(L0.T))
    return lu.solve, lut.solve


def _two_smallest(op, x, q):
    import scipy.linalg as sla
    ev = np.abs(sla.eigvals(op.J(x, **q).toarray()))
    return np.sort(ev)[:2]


def _oriented(nf):
    return nf if nf["a"] > 0 else flipped(nf)


def _nf_at(model, s, sv=None):
    q = _at(model, CGL_LENSES, s["p"])
    t = s["terms"]
    basis = jordan_basis(model, s["u"], q, t["v1"], t["w1"], sv)
    return _oriented(normal_form(model, s["u"], q, CGL_LENSES, *basis, sv=sv)), basis, q


def richardson(curve, p_bt, k):
    """(p - p_BT) / omega^2 extrapolated to omega -> 0 as a polynomial in omega^2 through the last k Hopf points of the curve (the
    stop point, where omega = 0, left out)."""
    om2 = np.array([curve["omega"][i] ** 2 for i in range(-1 - k, -1)])
    out = []
    for j, key in enumerate(("p1", "p2")):
        f = np.array([(curve[key][i] - p_bt[j]) / curve["omega"][i] ** 2 for i in range(-1 - k, -1)])
        out.append(np.polyval(np.polyfit(om2, f, k - 1), 0.0))
    return np.array(out)


def cgl_yardstick(dims):
    """Everything tests/golden/bt_cgl.json holds for one grid, computed on the dense restatement: the Hopf curve of the example to
    its stop, newton_bt from the stop point and from the Hopf point before it (sparse LU), the normal form at the result, the same
    from the stop point with SciPy GMRES under the device's preconditioner and tolerance, and the bordered vectors at the stop point
    both ways."""
    import minaug_hopf_ref as R
    from oracle import operators
    op = operators.CGL2d(dims, CGL_LS)
    n = 2 * dims[0] * dims[1]
    rstar, z = cgl_hopf_start(dims)
    hm = R.cgl_model(op, dict(CGL_PARS), *CGL_LENSES)
    curve = R.continuation_hopf(hm, np.zeros(n), rstar, CGL_PARS["nu"], 0.0, z, z, **CGL_CURVE)
    m = cgl_model(op, dict(CGL_PARS), *CGL_LENSES)
    out = dict(dims=list(dims), steps=len(curve["p2"]) - 1, stopped_at_bt=bool(curve["stopped_at_bt"]), rstar=rstar,
               curve=dict(p1=curve["p1"], p2=curve["p2"], omega=curve["omega"]), starts={}, lu={})
    pl, pl_adj = cgl_preconditioners(op, float(curve["X"][-1][-2]), CGL_PARS["nu"])
    for name, i in (("stop", -1), ("before", -2)):
        X = curve["X"][i]
        x, p = X[:-2], np.array([X[-2], curve["p2"][i]])
        q = _at(m, CGL_LENSES, p)
        a, b = start_vectors(m, x, q)
        s = newton_bt(m, x, p, CGL_LENSES, a, b, tol=CGL_CURVE["tol"])
        nf, basis, qq = _nf_at(m, s)
        out["starts"][name] = dict(x=x.tolist(), p=p.tolist(), omega=float(X[-1]), eig2=_two_smallest(op, x, q).tolist())
        out["lu"][name] = dict(p=s["p"].tolist(), xinf=float(np.abs(s["u"]).max()), residuals=s["residuals"], itnewton=s["itnewton"],
                               cond=s["cond"], eig2=_two_smallest(op, s["u"], qq).tolist(), defect=jordan_defect(m, s["u"], qq, *basis),
                               **{k: np.asarray(nf[k]).tolist() for k in NF_KEYS})
        if name == "stop":
            keep = (x, p, q, a, b, s, nf)
    x, p, q, a, b, s, nf = keep
    out["precond"] = [float(p[0]), CGL_PARS["nu"]]
    # the bordered vectors at the stop point with the start vectors of the LU run, both ways
    sv = Krylov(pl, pl_adj, **GMRES)
    tl, tk = bordered_vectors(m, x, q, a, b), bordered_vectors(m, x, q, a, b, sv)
    out["terms"] = dict(a=a.tolist(), b=b.tolist(), its=list(sv.its), bad=sv.bad, sigma=tl["sigma"].tolist(),
                        **{k: dict(diff=float(np.abs(tl[k] - tk[k]).max()), norminf=float(np.abs(tl[k]).max())) for k in ("v1", "v2", "w1", "w2")})
    # Newton and the normal form from the stop point with GMRES throughout
    sv = Krylov(pl, pl_adj, **GMRES)
    ak, bk_ = start_vectors(m, x, q, sv=sv)
    sk = newton_bt(m, x, p, CGL_LENSES, ak, bk_, tol=CGL_CURVE["tol"], sv=sv)
    its_newton = list(sv.its)
    nfk, _, qk = _nf_at(m, sk, sv)
    out["gmres"] = dict(itnewton=sk["itnewton"], residuals=sk["residuals"], its=its_newton, its_all=list(sv.its), bad=sv.bad,
                        eig2=_two_smallest(op, sk["u"], qk).tolist(),
                        diff=dict(p=float(np.abs(sk["p"] - s["p"]).max()), xinf=float(abs(np.abs(sk["u"]).max() - np.abs(s["u"]).max())),
                                  **{k: float(np.abs(np.asarray(nfk[k]) - np.asarray(nf[k])).max()) for k in NF_KEYS}))
    e2, e3 = richardson(curve, s["p"], 2), richardson(curve, s["p"], 3)
    out["richardson"] = dict(two=e2.tolist(), three=e3.tolist(), limit=(nf["K11"] * nf["b"] / (2 * nf["a"])).tolist())
    return out


def cgl_golden(grids=((8, 6), (12, 9))):
    return {f"{d[0]}x{d[1]}": cgl_yardstick(d) for d in grids}




# ---------------------------------------------------------------------------------------------- two small models
def planar_model(pars):
    """x1' = x2, x2' = b1 + b2 x2 + a x1^2 + b x1 x2 (test/normal_forms/testNF.jl:474-480) in the lenses (b1, b2)."""
    from minaug_hopf_ref import HopfModel
    F = lambda x, q: np.array([x[1], q["b1"] + q["b2"] * x[1] + q["a"] * x[0] ** 2 + q["b"] * x[0] * x[1]])
    J = lambda x, q: np.array([[0.0, 1.0], [2 * q["a"] * x[0] + q["b"] * x[1], q["b2"] + q["b"] * x[0]]])
    d2F = lambda x, q, u, v: np.array([0.0, 2 * q["a"] * u[0] * v[0] + q["b"] * (u[0] * v[1] + u[1] * v[0])])
    dFdp = lambda x, q, l: np.array([0.0, 1.0 if l == "b1" else x[1]])
    dJvdp = lambda x, q, l, v: np.array([0.0, 0.0 if l == "b1" else v[1]])
    return HopfModel(F, J, d2F, dFdp, dJvdp, pars, "b1", "b2")


def lorenz84_model(pars):
    """Lorenz-84 (test/hopf_codim_2/lorenz84.jl:7-30) in the lenses (F, T), which enter linearly."""
    from minaug_hopf_ref import HopfModel

    def F(u, q):
        X, Y, Z, U = u
        return np.array([-Y ** 2 - Z ** 2 - q["alpha"] * X + q["alpha"] * q["F"] - q["gamma"] * U ** 2,
                         X * Y - q["beta"] * X * Z - Y + q["G"], q["beta"] * X * Y + X * Z - Z,
                         -q["delta"] * U + q["gamma"] * U * X + q["T"]])

    def J(u, q):
        X, Y, Z, U = u
        be, ga = q["beta"], q["gamma"]
        return np.array([[-q["alpha"], -2 * Y, -2 * Z, -2 * ga * U], [Y - be * Z, X - 1, -be * X, 0.0],
                         [be * Y + Z, be * X, X - 1, 0.0], [ga * U, 0.0, 0.0, -q["delta"] + ga * X]])

    def d2F(u, q, v, w):
        be, ga = q["beta"], q["gamma"]
        return np.array([-2 * v[1] * w[1] - 2 * v[2] * w[2] - 2 * ga * v[3] * w[3],
                         v[0] * w[1] + v[1] * w[0] - be * (v[0] * w[2] + v[2] * w[0]),
                         be * (v[0] * w[1] + v[1] * w[0]) + v[0] * w[2] + v[2] * w[0], ga * (v[0] * w[3] + v[3] * w[0])])
    dFdp = lambda u, q, l: np.array([q["alpha"], 0.0, 0.0, 0.0]) if l == "F" else np.array([0.0, 0.0, 0.0, 1.0])
    return HopfModel(F, J, d2F, dFdp, lambda u, q, l, v: np.zeros(4), pars, "F", "T")


def newton_fold_full(model, x, p, lens, q, tol=1e-14, max_iterations=20):
    """A fold point by Newton on the full system (F, J v, <v0, v> - 1) in (x, v, p) for small dense models."""
    n = len(x)
    x, p = np.asarray(x, dtype=float).copy(), float(p)
    ev, V = np.linalg.eig(model.J(x, dict(q, **{lens: p})))
    v = np.real(V[:, np.argmin(np.abs(ev))])
    v0 = v = v / np.linalg.norm(v)
    E = np.eye(n)
    for _ in range(max_iterations):
        qq = dict(q, **{lens: p})
        Jm = np.asarray(model.J(x, qq))
        R = np.concatenate([model.F(x, qq), Jm @ v, [np.dot(v0, v) - 1]])
        if np.abs(R).max() < tol:
            break
        M = np.zeros((2 * n + 1, 2 * n + 1))
        M[:n, :n], M[:n, 2 * n] = Jm, model.dFdp(x, qq, lens)
        M[n:2 * n, :n] = np.stack([model.d2F(x, qq, v, E[j]) for j in range(n)], axis=1)
        M[n:2 * n, n:2 * n], M[n:2 * n, 2 * n] = Jm, model.dJvdp(x, qq, lens, v)
        M[2 * n, n:2 * n] = v0
        d = np.linalg.solve(M, R)
        x, v, p = x - d[:n], v - d[n:2 * n], p - d[2 * n]
    return x, p, float(np.abs(R).max())


if __name__ == "__main__":                                # python tests/bt_ref.py > tests/golden/bt_cgl.json
    import json
    import sys
    json.dump(cgl_golden(), sys.stdout, indent=1)
