"""The shift-invert eigensolve of BASELINE config 5 (ShiftInvert(sigma = 0.1, nev = 15, Krylov dimension 45, hermitian) with
MINRES + Pl as its inner solver) at grid sizes where the fused transform kernels run, against EXACT spectra.

The reference side is oracle/separable.py: at a state that varies along one axis the Jacobian splits into one dense block per
transverse mode pair, so the eigenvalues nearest sigma of a 2^22-point operator cost a few dozen small eigvalsh calls.  Generic
(non-separable) states are checked against scipy's eigsh on the assembled 2-D operator, or through the eigenpairs' own residuals.

Bounds, with tau = eigensolver tol, eta = inner rtol, d_i = |lambda_i - sigma|, delta = min_k |lambda_k - sigma|:
  * eigenvalues.  A converged Ritz value theta of the inexact inverse A~ ~ (J - sigma)^-1 is within tau of an eigenvalue of A~,
    and |A~ - A| <= e_A, the inner solves' error per unit right-hand side.  MINRES stops on the M-norm of the residual (M = Pl =
    (L1 + I)^-1, |M| <= 1, |M^-1| = 1 + Lmax with Lmax = max of the symbol of L1): |r|_2 <= sqrt(1 + Lmax) eta, hence
    e_A <= sqrt(1 + Lmax) eta / delta.  lambda = sigma + 1 / theta turns an error e in theta into e d_i d_i' (d_i' the distance of
    the neighbouring exact value), so |lambda_i - lambda_i,ref| <= E_i = (tau + sqrt(1 + Lmax) eta / delta) d_i (d_i + 1e-7),
    capped by the 1e-7 of the 12^3 test (tests/test_gpu_parity.py: test_shift_invert_vs_dense).
  * a-posteriori.  J is symmetric: the Rayleigh quotient q_i of a returned vector is within rho_i^2 / gap_i of the exact eigenvalue
    (Kato-Temple; rho_i = |J v - q_i v| / |v|, gap_i = distance of q_i to the rest of the spectrum), whatever the solver did.
  * residuals.  With (J - sigma) A~ V = V + R (R: the inner residuals, |r_j| <= sqrt(1 + Lmax) eta) and the converged Ritz residual
    w = A~ v - theta v, |w| <= tau: (J - sigma) v - v / theta = (R y - (J - sigma) w) / theta, so
    |J v - lambda v| <= d_i (sqrt(m) sqrt(1 + Lmax) eta + |J - sigma| tau), m = 45 the basis size.  The hermitian Rayleigh-Ritz
    symmetrises the projected matrix; the dropped antisymmetric part (the inexact solves') is not in the estimate w, and is given
    the same size again: bound 2 d_i (...).
  * pairing.  |q_i - lambda_i,ref| <= E_i + rho_i^2 / gap_i: vector i must belong to value i.  Orthonormality to 1e-10.
Every bound is checked through conftest.probe, which logs the measured value next to it.
"""
import numpy as np
import pytest
import scipy.sparse.linalg as spla

from conftest import probe
from oracle import bordered, bifurcations, krylov, operators, palc
from oracle import separable as S

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
SIGMA, NEV, L0, NU = 0.1, 15, 0.1, 1.2
TOL, ETA = 1e-9, 1e-10              # eigensolver tol / inner rtol: config 5's pair (1e-8 / 1e-9) ten times tighter
CAP = 1e-7                          # the 12^3 test's eigenvalue bound
GAP_RATIO = 1.05                    # |1/(l15 - sigma)| >= 1.05 |1/(l16 - sigma)|: the 15 wanted values are well defined


def smooth_profile(n, seed, amp=0.6, modes=6):
    """A random smooth profile on n cell centres: a few cosines with decaying random weights, max |u| = amp."""
    rng = np.random.default_rng(seed)
    t = (np.arange(n) + 0.5) / n
    c = rng.standard_normal(modes) / (1.0 + np.arange(modes))
    u = sum(ci * np.cos(np.pi * k * t) for k, ci in enumerate(c))
    return amp * u / np.abs(u).max()


def lmax(dims, ls):
    """Largest eigenvalue of L1 = (I + Lap)^2: (1 - sum_k 4 / h_k^2)^2 (operators.dct_symbol at the highest mode, bounded above)."""
    return (1.0 - sum(4.0 / (2.0 * l / n) ** 2 for n, l in zip(dims, ls))) ** 2


def reference_set(ev_by_distance):
    """The 15 values nearest sigma (sorted by decreasing value, as the solver returns them) from a list sorted by distance to sigma
    that holds at least the 16 nearest; asserts the set is well defined."""
    d = np.abs(ev_by_distance - SIGMA)
    assert d[NEV] >= GAP_RATIO * d[NEV - 1], ("no clear gap between the 15th and 16th eigenvalue", d[NEV - 1], d[NEV])
    want = np.sort(ev_by_distance[:NEV])[::-1]
    assert np.diff(want).max() <= -10 * CAP, ("two wanted eigenvalues closer than 10x the bound", np.diff(want).max())
    return want, float(d.min())


def inner_solver(hip, P, kind):
    assert kind == "minres"
    return hip.KrylovLSSymmetric("minres", rtol=ETA, atol=1e-14, itmax=4000, Pl=P)


def eig_bound(kind, dims, ls, want, delta):
    e_a = TOL + np.sqrt(1.0 + lmax(dims, ls)) * ETA / delta
    tight = e_a * np.abs(want - SIGMA) * (np.abs(want - SIGMA) + CAP)
    return np.minimum(CAP, tight), tight


def check_pairs(name, ctx, prob, J, vals, vecs, Jm=None, exact=None, radius=None, want=None, bound=None):
    """Residuals, Rayleigh quotients and orthonormality of the returned pairs.  Jm: the oracle's sparse J (else the GPU stencil,
    pinned to the CPU restatement at 2^22 points in test_gpu_fullsize.py).  exact: the reference spectrum near sigma (sorted by
    distance), complete within `radius` of sigma; want / bound: the reference values in the returned order and their bounds."""
    V = [v for v, _ in vecs[:NEV]]
    lm = lmax(prob.dims, prob.ls)
    jn = lm + 3.0 * NU ** 2                                          # |J - sigma| <= Lmax + max|g - sigma|, generously
    floor = 64 * EPS * jn
    for i, (lam, v) in enumerate(zip(vals[:NEV].real, V)):
        if Jm is not None:
            x = v.numpy()
            jv = Jm @ x
            vv = float(x @ x)
            q = float(x @ jv) / vv
            rho = np.linalg.norm(jv - q * x) / np.sqrt(vv)
            rl = np.linalg.norm(jv - lam * x) / np.sqrt(vv)
        else:
            jv = J(v)
            vv = v.inner(v)
            q = v.inner(jv) / vv
            rl = jv.copy().add_(v, -lam, 1.0).norm() / np.sqrt(vv)
            rho = jv.add_(v, -q, 1.0).norm() / np.sqrt(vv)
        d = abs(lam - SIGMA)
        probe(f"{name}:residual[{i}]", rl, 2.0 * d * (np.sqrt(45.0) * np.sqrt(1.0 + lm) * ETA + jn * TOL) + floor, d=d)
        # |q - lam| <= |J v - lam v| / |v| (q minimises the residual over the multiplier), plus the dot products' rounding
        probe(f"{name}:rayleigh_vs_value[{i}]", abs(q - lam), rl + floor)
        if exact is not None:
            # Kato-Temple: the exact eigenvalue nearest q is within rho^2 / gap of it, gap = distance of q to the rest of the spectrum:
            # inside the window the other listed values, outside it at least radius - |q - sigma|
            j = int(np.argmin(np.abs(exact - q)))
            gap = min(np.abs(np.delete(exact, j) - q).min(), radius - abs(q - SIGMA))
            assert gap > 0, (name, i, q, radius)
            kt = rho**2 / gap + floor
            probe(f"{name}:rayleigh_vs_exact[{i}]", abs(q - exact[j]), kt, rho=rho, gap=gap)
            # ... and that value is the i-th wanted one: vector i belongs to value i
            probe(f"{name}:rayleigh_vs_wanted[{i}]", abs(q - want[i]), bound[i] + kt)
    G = np.array([[a.inner(b) for b in V] for a in V])
    probe(f"{name}:orthonormality", np.abs(G - np.eye(len(V))).max(), 1e-10, tight=64 * 45 * EPS)


# (dims, box half-lengths, profile axis, profile seed, inner solvers).  Lengths are pairwise incommensurate, so transverse symbols
# do not coincide: the window holds no exact double eigenvalue.  Seeds were chosen for a clear gap after the 15th value; the
# reference side re-asserts it.
SEPARABLE = {
    "64^3-x": ((64, 64, 64), (9.7, 8.3, 7.1), 0, 53, ("minres",)),
    "64^3-y": ((64, 64, 64), (9.7, 8.3, 7.1), 1, 16, ("minres",)),
    "64^3-z": ((64, 64, 64), (9.7, 8.3, 7.1), 2, 27, ("minres",)),
    "128x64x64-x": ((128, 64, 64), (19.4, 8.3, 7.1), 0, 11, ("minres",)),
    "256x128x128-z": ((256, 128, 128), (12.1, 10.3, 8.9), 2, 0, ("minres",)),     # 2^22 points: the non-temporal kernels
}
_ORACLE_J = {}


def _oracle_J(dims, ls, u):
    key = (dims, ls)
    if key not in _ORACLE_J:
        _ORACLE_J.clear()
        _ORACLE_J[key] = operators.SwiftHohenberg(dims, ls)
    return _ORACLE_J[key].J(u, L0, NU)


@pytest.mark.parametrize("case", list(SEPARABLE))
def test_shift_invert_at_size_matches_the_separable_spectrum(ctx, case):
    """Config 5's eigensolve on a state that varies along one axis: the 15 values nearest sigma == the exact separable spectrum;
    converged; the returned pairs are eigenpairs of the oracle's J (the GPU stencil at 2^22 points).  (With GMRES(30) + Pl as the
    inner solver the same eigensolve does not report convergence at tol 1e-9 within maxiter 20 on 64^3: not covered here.)"""
    from bk_amd import hip
    dims, ls, axis, seed, kinds = SEPARABLE[case]
    prof = smooth_profile(dims[axis], seed)
    near, radius = S.spectrum_near(dims, ls, axis, prof, L0, NU, SIGMA, NEV)
    want, delta = reference_set(near)
    u = S.extend_profile(dims, axis, prof)
    big = int(np.prod(dims)) >= 1 << 22
    Jm = None if big else _oracle_J(dims, ls, u)
    prob = hip.SwiftHohenberg(ctx, dims, ls, l=L0, nu=NU)
    J = prob.jacobian(prob.vec(u), L0)
    P = hip.DCTPreconditioner(prob, 1.0)
    for kind in kinds:
        name = f"{case}:{kind}"
        vals, vecs, cv, nops = hip.ShiftInvert(SIGMA, inner_solver(hip, P, kind), tol=TOL, maxiter=20, hermitian=True)(J, NEV)
        assert cv, (name, nops)
        assert np.all(vals.imag == 0.0) and np.all(np.diff(vals.real) <= 0.0), (name, vals)
        bound, tight = eig_bound(kind, dims, ls, want, delta)
        err = np.abs(vals.real[:NEV] - want)
        for i in range(NEV):
            probe(f"{name}:eigenvalue[{i}]", err[i], bound[i], tight=tight[i], d=abs(want[i] - SIGMA))
        check_pairs(name, ctx, prob, J, vals, vecs, Jm=Jm, exact=near, radius=radius, want=want, bound=bound)
        del vecs


def test_shift_invert_2d_generic_state_matches_eigsh(ctx):
    """256 x 128 in 2-D at a generic state (guess() + noise, no separability): the reference is scipy's shift-invert eigsh on the
    assembled oracle J (a 2-D sparse LU is cheap)."""
    from bk_amd import hip
    dims, ls = (256, 128), (19.4, 9.1)
    sh = operators.SwiftHohenberg(dims, ls)
    u = sh.guess() + 0.1 * np.random.default_rng(3).standard_normal(sh.N)
    Jm = sh.J(u, L0, NU)
    ev = spla.eigsh(Jm.tocsc(), k=NEV + 9, sigma=SIGMA, which="LM", return_eigenvectors=False, tol=0)
    near = ev[np.argsort(np.abs(ev - SIGMA))]
    radius = float(np.abs(near[-1] - SIGMA))                         # eigsh's k values nearest sigma: complete within this radius
    want, delta = reference_set(near)
    prob = hip.SwiftHohenberg(ctx, dims, ls, l=L0, nu=NU)
    J = prob.jacobian(prob.vec(u), L0)
    P = hip.DCTPreconditioner(prob, 1.0)
    for kind in ("minres",):
        name = f"256x128-generic:{kind}"
        vals, vecs, cv, nops = hip.ShiftInvert(SIGMA, inner_solver(hip, P, kind), tol=TOL, maxiter=20, hermitian=True)(J, NEV)
        assert cv and np.all(np.diff(vals.real) <= 0.0), (name, nops, vals)
        bound, tight = eig_bound(kind, dims, ls, want, delta)
        err = np.abs(vals.real[:NEV] - want)
        for i in range(NEV):
            # (eigsh's own error: ARPACK to machine precision on the shift-inverted operator, ~ eps d_i^2 |(J - sigma)^-1|)
            probe(f"{name}:eigenvalue[{i}]", err[i], bound[i] + 1e-12, tight=tight[i] + 1e-12, d=abs(want[i] - SIGMA))
        check_pairs(name, ctx, prob, J, vals, vecs, Jm=Jm, exact=near, radius=radius, want=want, bound=bound + 1e-12)


def test_shift_invert_64cubed_generic_state_pairs(ctx):
    """64^3 at a generic state (guess() + noise): no exact spectrum, so the returned pairs are checked on their own -- converged,
    residuals against the oracle's J, Rayleigh quotients, orthonormality."""
    from bk_amd import hip
    dims, ls = (64, 64, 64), (9.7, 8.3, 7.1)
    sh = operators.SwiftHohenberg(dims, ls)
    u = sh.guess() + 0.05 * np.random.default_rng(4).standard_normal(sh.N)
    Jm = _oracle_J(dims, ls, u)
    prob = hip.SwiftHohenberg(ctx, dims, ls, l=L0, nu=NU)
    J = prob.jacobian(prob.vec(u), L0)
    P = hip.DCTPreconditioner(prob, 1.0)
    for kind in ("minres",):
        name = f"64^3-generic:{kind}"
        vals, vecs, cv, nops = hip.ShiftInvert(SIGMA, inner_solver(hip, P, kind), tol=TOL, maxiter=20, hermitian=True)(J, NEV)
        assert cv and np.all(np.diff(vals.real) <= 0.0), (name, nops, vals)
        check_pairs(name, ctx, prob, J, vals, vecs, Jm=Jm)


# --------------------------------------------------------------------------------------------- GMRES(30) + Pl inner solves
def test_gmres_inner_solve_of_the_shift_invert_at_64cubed_matches_the_oracle(ctx):
    """The stencil-free inner solver, GMRESKrylovKit(30, Pl), on the shift-invert's system (J - sigma) x = b at 64^3 (the 64^3-x
    state; csrc/eig.hip folds sigma into the operator).  Restarted GMRES(30) stagnates on this indefinite preconditioned system: the
    oracle's restatement (krylov.gmres_krylovkit) also ends 150 restarts without success, so the eigensolve with this inner solver
    cannot converge there and is not run.  What is checked is the first restart cycle from x = 0, which both sides take from the same
    Krylov space: its minimal preconditioned residual |Pl (b - (J - sigma) x)| (a well-conditioned quantity) agrees to 1e-8
    relative, and the iterates to 1e-6 relative (the 30 x 30 least-squares problem of a stagnating cycle amplifies rounding)."""
    import scipy.sparse as sp
    from bk_amd import hip
    dims, ls, axis, seed, _ = SEPARABLE["64^3-x"]
    u = S.extend_profile(dims, axis, smooth_profile(dims[axis], seed))
    b = np.random.default_rng(0).standard_normal(int(np.prod(dims)))
    b /= np.linalg.norm(b)
    Js = (_oracle_J(dims, ls, u) - SIGMA * sp.identity(b.size)).tocsr()
    Po = operators.dct_preconditioner(dims, ls, 1.0)
    xo, oko, ito, _ = krylov.gmres_krylovkit(Js, b, 0.0, 1.0, krylovdim=30, maxiter=1, rtol=ETA, atol=1e-14, Pl=Po)
    prob = hip.SwiftHohenberg(ctx, dims, ls, l=L0, nu=NU)
    # J - sigma = -L1 + diag(g - sigma) is the Jacobian at l - sigma (how csrc/eig.hip folds the shift in); passing a0 = -sigma to the
    # solver instead would solve the reference's (a0 I + Pl^-1 J) x = Pl^-1 b (src/LinearSolver.jl:268-277), a different system
    J = prob.jacobian(prob.vec(u), L0 - SIGMA)
    x, ok, it = hip.GMRESKrylovKit(dim=30, rtol=ETA, atol=1e-14, maxiter=1, Pl=hip.DCTPreconditioner(prob, 1.0))(J, prob.vec(b), 0.0, 1.0)
    assert not ok and not oko, (it, ito)
    xd = x.numpy()
    rd, ro = (np.linalg.norm(Po(b - Js @ y)) for y in (xd, xo))
    assert ro < np.linalg.norm(Po(b))                                 # the cycle made progress, it did not converge
    probe("gmres64:preconditioned_residual", abs(rd - ro) / ro, 1e-8, it=it, ito=ito)
    probe("gmres64:iterate", np.abs(xd - xo).max() / np.abs(xo).max(), 1e-6)


# --------------------------------------------------------------------------------------------- config-5-shaped branch
def roll_profile(n, length):
    """A 1-D roll state of the Neumann SH problem at l = 0.1, nu = 1.2: Newton (dense, exact) from 0.5 cos of the mode nearest the
    critical wavenumber 1 (k_m = pi m / 2 length)."""
    m = int(round(2.0 * length / np.pi))
    u = 0.5 * np.cos(np.pi * m * (np.arange(n) + 0.5) / n)
    D = operators.second_difference(n, length, operators.NEUMANN).toarray()
    A = np.eye(n) + D
    for _ in range(50):
        f = S.sh_profile_residual(n, length, u, L0, NU)
        if np.abs(f).max() < 1e-13:
            break
        u = u - np.linalg.solve(-(A @ A) + np.diag(L0 + 2 * NU * u - 3 * u**2), f)
    assert np.abs(S.sh_profile_residual(n, length, u, L0, NU)).max() < 1e-12 and np.abs(u).max() > 0.1
    return u


class _JacState:
    """What the oracle's prob.J returns on the small grid: applies J there, and carries (x, p) for the separable eigensolve."""

    def __init__(self, sh, x, p):
        self.sh, self.x, self.p = sh, x, p

    def __call__(self, dx):
        return self.sh.dF(self.x, self.p, NU, dx)


def oracle_branch(dims, ls, steps):
    """The oracle PALC with the settings of scripts/run_branch.py on (2, 2, n_z) -- the 3-D branch from a state constant along x
    and y is this one (DotTheta divides by N) -- with the eigenvalues of the FULL box from the separable spectrum."""
    nz, lz = dims[2], ls[2]
    small = (2, 2, nz)
    sh = operators.SwiftHohenberg(small, ls)
    u1 = roll_profile(nz, lz)
    Plo = operators.dct_preconditioner(small, ls, 1.0)
    # GMRES stops on max(atol, rtol |Pl b|): |.|_2 of an extended vector is sqrt(N / N_small) times that of the small one, so the
    # absolute floor is scaled the same way to take the same decisions as the device on the full box
    atol = 1e-12 * np.sqrt(len(u1) * 4 / np.prod(dims))
    ols = lambda Jx, r, a0=0.0, a1=1.0: krylov.gmres_krylovkit(Jx, r, a0, a1, krylovdim=30, maxiter=150, rtol=1e-9, atol=atol,
                                                                Pl=Plo)[:3]
    obls = lambda *a, **k: bordered.bordering_bls(ols, *a, check_precision=False, **k)
    spectra = []

    def eig(Jx, nev):
        prof = Jx.x.reshape(nz, 2, 2)[:, 0, 0]
        near, _ = S.spectrum_near(dims, ls, 2, prof, Jx.p, NU, SIGMA, nev)
        want, _ = reference_set(near) if nev == NEV else (np.sort(near[:nev])[::-1], None)
        # every positive eigenvalue must be among the nev computed: the largest eigenvalue of J is at most max g (-L1 <= 0)
        gmax = float((Jx.p + 2 * NU * prof - 3 * prof**2).max())
        allpos = S.sh_separable_spectrum(dims, ls, 2, prof, Jx.p, NU, window=(0.0, gmax + 1.0))
        assert np.all(np.isin(allpos[allpos > 1e-10], want)), ("a positive eigenvalue is not among the nev nearest sigma", allpos)
        spectra.append((want, near, Jx.x.copy()))
        return want, None, True, 0

    oprob = palc.Problem(lambda x, p: sh.F(x, p, NU), lambda x, p: _JacState(sh, x, p))
    cp = bifurcations.ContPar(ds=-0.001, dsmin=1e-4, dsmax=0.005, theta=0.5, p_min=-0.1, p_max=0.15, max_steps=steps, nev=NEV,
                              tol=1e-9, max_iterations=15, tangent="bordered")
    br = bifurcations.continuation(oprob, S.extend_profile(small, 2, u1), L0, ls=ols, bls=obls, eig=eig, cp=cp, normC=palc.norminf)
    return br, spectra, u1


def test_config5_shaped_branch_matches_the_separable_reference(ctx):
    """Two native bk_cont_step calls (PALC, Bordered tangent, BorderingBLS, GMRES(30) + Pl, Newton tol 1e-9, norminf, eigensolve
    with nev 15 and the MINRES inner solver every step) on 64^3 from a roll state along z, against the oracle branch on (2, 2, 64)
    and the exact spectrum of the full box at every oracle state."""
    from bk_amd import continuation as Cn
    from bk_amd import hip
    dims, ls, steps = (64, 64, 64), (7.15, 9.26, 7.1), 2
    br, spectra, u1 = oracle_branch(dims, ls, steps)
    assert not br["specialpoint"] and len(br["param"]) == steps + 1
    prob = hip.SwiftHohenberg(ctx, dims, ls, l=L0, nu=NU)
    P = hip.DCTPreconditioner(prob, 1.0)
    ls_ = hip.GMRESKrylovKit(dim=30, rtol=1e-9, atol=1e-12, maxiter=150, Pl=P)
    els = hip.KrylovLSSymmetric("minres", rtol=1e-9, atol=1e-12, itmax=4000, Pl=P)
    eig = hip.ShiftInvert(SIGMA, els, tol=1e-8, maxiter=20, hermitian=True, save_vectors=False)
    nopt = Cn.NewtonPar(tol=1e-9, max_iterations=15, linsolver=ls_, eigsolver=eig)
    cp = Cn.ContinuationPar(ds=-0.001, dsmin=1e-4, dsmax=0.005, p_min=-0.1, p_max=0.15, max_steps=steps, nev=NEV,
                            detect_bifurcation=3, newton_options=nopt)
    alg = Cn.PALC(tangent="bordered", theta=0.5, bls=hip.BorderingBLS(None, check_precision=False))
    bn = Cn.continuation_native(prob, prob.vec(S.extend_profile(dims, 2, u1)), L0, alg, cp, normC=Cn.norminf, save_sol=True)
    # (the oracle's loop runs one corrector past max_steps before `done` stops it: its spectra list holds one state more)
    assert len(bn.param) == len(br["param"]) == steps + 1 and len(spectra) >= steps + 1, (bn.param, br["param"])
    for k in range(len(bn.param)):
        probe(f"branch:p[{k}]", abs(bn.param[k] - br["param"][k]), 1e-9)
    # (the device branch records the ds each step used, the oracle the ds step-size control chose after it: shifted by one)
    assert np.allclose(bn.ds[1:], br["ds"][:-1], rtol=1e-12, atol=0), (bn.ds, br["ds"])
    assert list(bn.itnewton) == list(br["itnewton"]), (bn.itnewton, br["itnewton"])
    assert list(bn.n_unstable) == list(br["n_unstable"]), (bn.n_unstable, br["n_unstable"])
    lm = lmax(dims, ls)
    for k, (vals, (want, near, xo), sol) in enumerate(zip(bn.eig, spectra, bn.sol)):
        # the device eigensolve runs at the device state, the reference at the oracle's: Weyl moves every eigenvalue by at most
        # max |g_device - g_oracle| <= max |2 nu - 6 u| |du| + |dp|
        xg = sol.numpy()
        xo3 = S.extend_profile(dims, 2, xo.reshape(dims[2], 2, 2)[:, 0, 0])
        dg = float(np.abs((2 * NU - 3 * (xg + xo3)) * (xg - xo3)).max()) + abs(bn.param[k] - br["param"][k])
        delta = float(np.abs(near - SIGMA).min())
        tight = (1e-8 + np.sqrt(1.0 + lm) * 1e-9 / delta) * np.abs(want - SIGMA) * (np.abs(want - SIGMA) + CAP)
        err = np.abs(np.asarray(vals).real[:NEV] - want)
        for i in range(NEV):
            probe(f"branch:eig[{k}][{i}]", err[i], min(CAP, tight[i]) + dg, tight=tight[i] + dg, dg=dg)


# --------------------------------------------------------------------------------------------- lane-pair round trip (dct_rt_lanes)
def _choose_lt_wide_z(N, n0):
    """choose_lt (csrc/dct_fast.hip) for a wide axis-2 pass on a power-of-two N in [64, 512]: the lines per tile."""
    lt = 16
    if N < 512:
        lt = min(16 * (512 // N), 128)
        while lt > 16 and (n0 % lt != 0 or ((lt // 2) * (N + 1) + (N + 4)) * 16 > 76 * 1024):
            lt //= 2
    tw = N // 2 + N // 32                                             # dctc::tw_len (csrc/dct_core.h)
    while lt > 2 and ((lt // 2) * (N + 1) + tw) * 16 > 76 * 1024:
        lt -= 2
    return min(lt, (n0 + 1) & ~1)


LANE_SHAPES = [((16, 8, 512), (2.3, 1.7, 41.0)), ((128, 4, 64), (11.3, 0.9, 6.1)), ((256, 128, 128), (12.1, 10.3, 8.9))]


@pytest.mark.parametrize("dims,ls", LANE_SHAPES, ids=["16x8x512", "128x4x64", "256x128x128"])
def test_lane_pair_round_trip_matches_the_256_lane_kernel(ctx, dims, ls):
    """Option dct_rt_lanes = 512 takes the lane-pair instantiations of the z round trip when (LT/2)(N/8) == 512 (z = 512: LT = 16;
    z = 64 on x = 128: LT = 128; z = 128 on x = 256 at 2^22 points: LT = 64, the non-temporal pair).  Pl \\ v equals the 256-lane result
    and scipy's DCT to rounding, but NOT bitwise: the lane pairs round the merged middle in another order (about 0.1 eps max|v|).  That
    difference is also the device-side evidence that the lane-pair kernels ran: were both runs to take the 256-lane kernel, the two
    outputs would be bitwise equal.  A MINRES solve through the fused spectral dot gives the same iterates to rounding."""
    from bk_amd import hip
    lt = _choose_lt_wide_z(dims[2], dims[0])
    assert (lt // 2) * (dims[2] // 8) == 512 and dims[0] % lt == 0, lt
    prob = hip.SwiftHohenberg(ctx, dims, ls, l=L0, nu=NU)
    rng = np.random.default_rng(sum(dims))
    v = rng.standard_normal(prob.nglobal)
    u = S.extend_profile(dims, 2, smooth_profile(dims[2], 5)) + 0.05 * rng.standard_normal(prob.nglobal)
    J = prob.jacobian(prob.vec(u), L0)
    rhs = prob.vec(v)
    ref = operators.dct_preconditioner(dims, ls, 1.0)(v)
    out = {}
    try:
        ctx.set_option("solver_trace", 1)
        for lanes in (256, 512):
            ctx.set_option("dct_rt_lanes", lanes)
            P = hip.DCTPreconditioner(prob, 1.0)
            y = P.ldiv(rhs).numpy()
            ctx.solver_history(reset=True)
            x, ok, it = hip.KrylovLSSymmetric("minres", rtol=1e-10, atol=1e-14, itmax=4000, Pl=P)(J, rhs, -SIGMA, 1.0)
            out[lanes] = (y, x.numpy(), ok, it, ctx.solver_history(reset=True)[0])
    finally:
        ctx.set_option("dct_rt_lanes", 256)
        ctx.set_option("solver_trace", 0)
    (y0, x0, ok0, it0, h0), (y1, x1, ok1, it1, h1) = out[256], out[512]
    # three orthonormal DCT round trips of O(log N) butterflies each, against scipy's: a few hundred eps of max|v|
    probe(f"lanes{dims}:ldiv_vs_scipy", np.abs(y1 - ref).max(), 256 * EPS * np.abs(v).max())
    probe(f"lanes{dims}:ldiv_512_vs_256", np.abs(y1 - y0).max(), 256 * EPS * np.abs(v).max())
    assert not np.array_equal(y1, y0), "dct_rt_lanes = 512 gave the 256-lane kernel's bits: the lane-pair kernel did not run"
    assert ok0 and ok1 and it0 > 5
    # the spectral dot of the round trip is summed per tile in a lane order of its own: the residual estimates agree to the dot's
    # rounding (relative 1e-12) while the Lanczos recurrence has not amplified it, the count within 2, the solution to 1e-8 relative
    probe(f"lanes{dims}:history", max(abs(a - b) / b for a, b in zip(h0[:it0 // 2], h1[:it0 // 2])), 1e-10, tight=0.0)
    probe(f"lanes{dims}:iterations", abs(it1 - it0), 2, tight=0)
    probe(f"lanes{dims}:solution", np.abs(x1 - x0).max() / np.abs(x0).max(), 1e-8, tight=0.0)
