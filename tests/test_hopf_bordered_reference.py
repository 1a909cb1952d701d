"""CPU checks of the restatement tests/minaug_hopf_bordered_ref.py -- the complex bordered solve that stays regular at a Hopf point,
as ONE real GMRES on the real-equivalent (2N + 2) system left-preconditioned by diag(Pl, Pl, 1, 1) -- against dense complex
matrices, SciPy GMRES and the elimination path, and of the library boundary of the two new entries.  No device."""
import ctypes
import os
import re

import numpy as np
import pytest

import minaug_hopf_bordered_ref as H
from oracle import operators

EPS = np.finfo(float).eps
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["bk_cbordered_tail", "bk_bls_matrixfree_pl_cshift"]


def _small(seed=3):
    """6 x 5 grid, u != 0, every argument general: complex shift, c = dzp xip, kappa = xiu dotscale, complex n and R."""
    dims, ls = (6, 5), (np.pi, np.pi / 2)
    op = operators.CGL2d(dims, ls)
    rng = np.random.default_rng(seed)
    n = 2 * op.n
    cv = lambda: rng.standard_normal(n) + 1j * rng.standard_normal(n)
    u = 0.3 * rng.standard_normal(n)
    J = op.J(u, **dict(H.PARS, r=0.3, gamma=0.1))
    pl = operators.dst_block_preconditioner_cgl(dims, ls, 0.4, 0.9)
    dzp, xiu, xip, dotscale = 0.7 - 0.2j, 0.8, 1.25, 1.0 / n
    return dict(J=J, pl=pl, n=n, a=cv(), b=cv(), R=cv(), nn=0.6 + 0.3j, c=dzp * xip, kappa=xiu * dotscale, shift=0.37 - 1.1j)


def test_real_equivalent_operator_is_the_preconditioned_complex_matrix():
    """The (2N + 2) real operator, column by column, against [[Re C, -Im C], [Im C, Re C]] of C = diag(Pl^-1, 1) [shift + J, a;
    kappa b^H, c] in the ordering [xr; pr | xi; pi].  Bound: every entry is a sum of at most N + 1 products formed twice in another
    order, through the two products Pl^-1 (J .): 8 N eps of the sums of moduli."""
    s = _small()
    n = s["n"]
    M = H.PlCBordered(s["J"], s["a"], s["b"], s["c"], s["pl"], s["kappa"], s["shift"])
    A = M.dense()
    Pinv = np.column_stack([s["pl"](e) for e in np.eye(n)])
    D = np.block([[Pinv, np.zeros((n, 1))], [np.zeros((1, n)), np.ones((1, 1))]])
    Cm = H.complex_matrix(s["J"], s["a"], s["b"], s["c"], s["kappa"], s["shift"]).toarray()
    C = D @ Cm
    perm = np.concatenate([np.arange(n), [2 * n], np.arange(n, 2 * n), [2 * n + 1]])          # [xr; pr; xi; pi] in z's indices
    E = np.block([[C.real, -C.imag], [C.imag, C.real]])
    bound = 8 * n * EPS * (np.abs(D) @ np.abs(Cm)).max()
    assert np.abs(A[np.ix_(perm, perm)] - E).max() <= bound
    # ... and its right-hand side: (Pl^-1 R, n), the tail untouched
    rhs = M.rhs(s["R"], s["nn"])
    ref = np.append(Pinv @ s["R"], s["nn"])
    assert np.abs(rhs[perm] - np.concatenate([ref.real, ref.imag])).max() <= 8 * n * EPS * (np.abs(Pinv) @ np.abs(s["R"])).max()


def test_real_equivalent_solve_is_the_complex_bordered_solve():
    """Dense solve of the (2N + 2) real system against the sparse direct solve of the complex (N + 1) system.  Both are backward
    stable: each carries m eps cond |y| of its own matrix, m its size."""
    s = _small()
    n = s["n"]
    M = H.PlCBordered(s["J"], s["a"], s["b"], s["c"], s["pl"], s["kappa"], s["shift"])
    A = M.dense()
    z = np.linalg.solve(A, M.rhs(s["R"], s["nn"]))
    u, p = z[:n] + 1j * z[n:2 * n], complex(z[2 * n], z[2 * n + 1])
    ud, pd = H.direct_cbordered(s["J"], s["a"], s["b"], s["c"], s["R"], s["nn"], s["kappa"], s["shift"])
    Cm = H.complex_matrix(s["J"], s["a"], s["b"], s["c"], s["kappa"], s["shift"]).toarray()
    ny = np.linalg.norm(np.append(ud, pd))
    bound = ((2 * n + 2) * np.linalg.cond(A) + (n + 1) * np.linalg.cond(Cm)) * EPS * ny
    err = max(np.linalg.norm(u - ud), abs(p - pd))
    print("real-equivalent vs complex direct:", err, "bound", bound)
    assert err <= bound
    # the GMRES form of the same system lands there too, and its true residual is that of the complex system
    ug, pg, info, it, _ = H.cbordered_gmres(s["J"], s["a"], s["b"], s["c"], s["R"], s["nn"], s["pl"], kappa=s["kappa"],
                                            shift=s["shift"], restart=2 * n + 2, maxiter=4, rtol=1e-13)
    assert info == 0
    rhsn = np.linalg.norm(M.rhs(s["R"], s["nn"]))
    # |x - x*| <= |A^-1| |r| with |r| <= rtol |rhs| on the preconditioned system
    assert max(np.linalg.norm(ug - ud), abs(pg - pd)) <= np.linalg.norm(np.linalg.inv(A), 2) * 1e-13 * rhsn + bound
    assert H.cresidual(s["J"], s["a"], s["b"], s["c"], s["R"], s["nn"], ug, pg, s["kappa"], s["shift"]) <= \
        np.linalg.norm(Cm, 2) * (np.linalg.norm(np.linalg.inv(A), 2) * 1e-13 * rhsn + bound)


def test_spectral_solve_agrees_with_the_direct_solve_off_the_hopf_point():
    """The DST-basis solve of the u = 0 system (both the system and its adjoint) against the sparse direct solve at r* + 2e-2, where
    both are well conditioned: m eps cond |y| each."""
    op, rstar, a, b = H.trivial_case((16, 8))
    n = a.size
    nu = H.PARS["nu"]
    J = op.J(np.zeros(n), **dict(H.PARS, r=rstar + 2e-2))
    zero = np.zeros(n)
    for Jm, col, row, sh, adj in ((J, a, b, -1j * nu, False), (J.T.tocsr(), b, a, 1j * nu, True)):
        ud, pd = H.direct_cbordered(Jm, col, row, 0.0, zero, 1.0, shift=sh)
        us, ps = H.spectral_cbordered(op.dims, op.ls, rstar + 2e-2, nu, col, row, 0.0, zero, 1.0, shift=sh, adjoint=adj)
        cond = np.linalg.cond(H.complex_matrix(Jm, col, row, 0.0, 1.0, sh).toarray())
        bound = 2 * (n + 1) * EPS * cond * np.linalg.norm(np.append(ud, pd))
        assert max(np.linalg.norm(ud - us), abs(pd - ps)) <= bound, (adj, bound)


DISTANCES = [2e-2, 1e-5, 1e-9, 0.0]


@pytest.fixture(scope="module")
def table():
    """41 x 21, u = 0, a, b = Hopf mode + 0.05 noise, Pl = CGLBlockPreconditioner(r* + 0.02, 0.95 nu), SciPy GMRES(60), rtol 1e-13,
    at most 600 steps, on the real-equivalent systems."""
    op, rstar, a, b = H.trivial_case()
    nu = H.PARS["nu"]
    pl = operators.dst_block_preconditioner_cgl(op.dims, op.ls, rstar + 0.02, 0.95 * nu)
    n = a.size
    zero = np.zeros(n)
    rows = {}
    for d in DISTANCES:
        J = op.J(zero, **dict(H.PARS, r=rstar + d))
        Jt = J.T.tocsr()
        v, sg, info, it, na = H.cbordered_gmres(J, a, b, 0.0, zero, 1.0, pl, shift=-1j * nu)
        w, _, winfo, wit, wna = H.cbordered_gmres(Jt, b, a, 0.0, zero, 1.0, pl, shift=1j * nu)
        vd, sd = H.direct_cbordered(J, a, b, 0.0, zero, 1.0, shift=-1j * nu)
        wd, _ = H.direct_cbordered(Jt, b, a, 0.0, zero, 1.0, shift=1j * nu)
        _, einfo, eit, ena, erel = H.elimination_gmres(J, a, pl, shift=-1j * nu)
        rows[d] = dict(b_info=info, b_it=it, b_apply=na, w_info=winfo, w_it=wit, w_apply=wna, e_info=einfo, e_it=eit, e_apply=ena,
                       e_rel=erel, sigma=sg, v_err=np.linalg.norm(v - vd) / np.linalg.norm(vd),
                       w_err=np.linalg.norm(w - wd) / np.linalg.norm(wd), s_err=abs(sg - sd))
        print("r - r* =", d, rows[d])
    return rows


def test_bordered_gmres_converges_at_every_distance_with_one_count(table):
    for key in ("b", "w"):
        assert all(table[d][key + "_info"] == 0 for d in DISTANCES), key
        its = [table[d][key + "_it"] for d in DISTANCES]
        assert max(its) == min(its), (key, its)
    # within a restart length, and the adjoint system, preconditioned by the untransposed Pl, costs more than the system itself
    assert table[0.0]["b_it"] < table[0.0]["w_it"] < 60


def test_elimination_solve_is_unconverged_from_1e_5_inward(table):
    assert table[2e-2]["e_info"] == 0 and abs(table[2e-2]["e_it"] - table[2e-2]["b_it"]) <= 2, table[2e-2]
    for d in (1e-5, 1e-9, 0.0):
        assert table[d]["e_info"] != 0 and table[d]["e_it"] >= 500, table[d]
    assert table[1e-5]["e_rel"] < table[1e-9]["e_rel"] < table[0.0]["e_rel"]
    assert table[0.0]["e_rel"] > 0.1


def test_bordered_gmres_is_as_accurate_as_its_tolerance_at_every_distance(table):
    """rtol 1e-13 on the preconditioned system, whose inverse has norm <= 1e2 at every distance here (the bordered matrix is
    regular): relative 1e-11 in v, w, absolute in sigma."""
    for d in DISTANCES:
        assert table[d]["v_err"] <= 1e-11 and table[d]["w_err"] <= 1e-11 and table[d]["s_err"] <= 1e-11, (d, table[d])
    assert abs(table[0.0]["sigma"]) <= 1e-11


# ------------------------------------------------------------------------------------------ the boundary
def _declared():
    src = open(os.path.join(ROOT, "include", "bkhip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(bk_[a-z0-9_]+)\s*\(", src))


def test_header_library_and_binding_carry_the_two_new_entries():
    from bk_amd import _lib
    declared = _declared()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    # the argument list of bk_bls_bordering_cshift, with one itlinear
    assert _lib.SIGNATURES["bk_bls_matrixfree_pl_cshift"][1][:-1] == _lib.SIGNATURES["bk_bls_bordering_cshift"][1][:-1]
    bound = _lib.load()
    assert bound.bk_cbordered_tail.argtypes is not None and len(bound.bk_cbordered_tail.argtypes) == 12


def test_python_entries_take_bls():
    import inspect
    from bk_amd import codim2, hip
    assert "shift" in inspect.signature(hip.MatrixFreeBLS.solve_complex).parameters
    assert list(inspect.signature(hip.MatrixFreeBLS.solve_complex).parameters) == \
        list(inspect.signature(hip.BorderingBLS.solve_complex).parameters)
    for f in (codim2.hopf_terms, codim2.newton_hopf, codim2.newton_hopf_native, codim2.HopfProblem.__init__, codim2.continuation_hopf,
              codim2.bautin_normal_form, codim2.bautin_normal_form_native, codim2.hopf_start_vectors):
        assert inspect.signature(f).parameters["bls"].default is None, f
    ls = hip.GMRESKrylovKit(dim=10)
    with pytest.raises(TypeError, match="use_pl=True"):
        codim2._hopf_bordered_path(hip.MatrixFreeBLS(ls))
    assert codim2._hopf_bordered_path(hip.MatrixFreeBLS(ls, use_pl=True)) is True
    assert codim2._hopf_bordered_path(None) is False and codim2._hopf_bordered_path(hip.BorderingBLS(ls)) is False
